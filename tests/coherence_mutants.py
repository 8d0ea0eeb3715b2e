"""Mutants of the coherence reference (tests/coherence_ref.py), each one slip of one term of
coherence_kernel (csrc/dash_coherence.hip), for tests/test_coherence_adequacy.py: a corpus of states
is adequate for the kernel when every mutant gives at least 3 of its systems another record.

TEST INFRASTRUCTURE. check(nodes, num_procs, cache_size, m) is coherence_ref.check with slip m;
m = 0 is the reference itself (asserted on every corpus state and candidate the adequacy test sees).
The twin is written as the kernel accumulates -- one pass over the lines in the kernel's scan order
(node ascending, line ascending), a "first value" and the flags per address, then the bits per
address -- because several slips (17, 21) are about that order; it shares no code with the reference.

`pristine`: the nodes of the initial state, for callers whose states share untouched node objects
with it (coherence_states.py). A node that *is* its pristine object is skipped: its directory is
all U with an empty bitVector and its lines are all INVALID at 0xFF, and no single slip below makes
such a node contribute (slip 14 counts INVALID lines, but 0xFF is homed at node 15, past every
shape; slips 19 and 23 re-home foreign lines, but only valid ones). The adequacy test checks the
skipping path against the full one.
"""
import coherence_ref as cr

# number -> (the slip, the kernel expression it stands for)
MUTANTS = {
    0: ("the reference", ""),
    1: ("SWMR needs two owners", "own && n2"),
    2: ("SWMR without own", "own in own && n2"),
    3: ("DIR_U_HELD only at two copies", "n1 in d == 2u && n1"),
    4: ("DIR_EM accepts any own", "!n2 in !(n1 && !n2 && own)"),
    5: ("DIR_EM accepts any single copy", "own in !(n1 && !n2 && own)"),
    6: ("DIR_S without the 'no copy' arm", "!n1 in own || !n1"),
    7: ("DIR_S without the owner arm", "own in own || !n1"),
    8: ("LOST_SHARER also under U", "d != 2u && (mask & ~bv)"),
    9: ("STALE_SHARER also under U", "d != 2u && (bv & ~mask)"),
    10: ("bitVector masked to num_procs bits", "bv & ~mask"),
    11: ("STALE_VALUE for SHARED only", "(st == 1u) | (st == 2u)"),
    12: ("STALE_VALUE for MODIFIED too", "(st == 1u) | (st == 2u)"),
    13: ("a node's second line of an address is not a second value", "split"),
    14: ("INVALID lines count", "st != 3u"),
    15: ("directory value 3 read as U", "d == 2u, d != 2u"),
    16: ("copies counted by holder mask, not by line", "had << F_N2"),
    17: ("'a copy was seen' taken from a non-zero first value, not from F_N1", "had; x |= had ? 0u : val"),
    18: ("first_addr lowest within a home, homes in descending order", "the skey min over lanes"),
    19: ("a line homed at a node in [num_procs, P) counts at lane home - num_procs", "live; (addr >> 4) == t"),
    20: ("addrs counts set bits, not addresses", "addrs += bits ? 1u : 0u"),
    21: ("STALE_VALUE compared with the first copy's value, not memory", "the F_MEM field"),
    22: ("an EXCLUSIVE copy is not an owner", "st < 2u"),
    # found while reading the kernel
    23: ("a line homed at or past P counts at lane home & (P - 1)", "(addr >> 4) == t"),
    24: ("first_bits is the system's bits, not the first address's", "skey & 0xFFu"),
    25: ("the holder mask is indexed by line, not by node", "1u << (F_MASK + u)"),
    26: ("LOST_SHARER and STALE_SHARER swapped", "mask & ~bv, bv & ~mask"),
}
SLIPS = tuple(m for m in MUTANTS if m)


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def check(nodes, num_procs, cache_size, m=0, pristine=None):
    """(record dict with coherence_ref.FIELDS, per-address bits list [num_procs * 16]) under slip m."""
    N, CS, P = num_procs, cache_size, next_pow2(num_procs)
    touched = [t for t in range(N) if pristine is None or nodes[t] is not pristine[t]]
    # ---- the scan: one accumulator per address that a line is a copy of
    acc = {}
    for u in touched:
        s = nodes[u]
        for i in range(CS):
            addr, val, st = s.cache_addr[i], s.cache_value[i], s.cache_state[i]
            if st == cr.INVALID and m != 14:
                continue
            home = addr >> 4
            if home >= N:
                if m == 19 and home < P:
                    home -= N
                elif m == 23 and home >= P and (home & (P - 1)) < N:
                    home &= P - 1
                else:
                    continue
            a = home << 4 | (addr & 15)
            x = acc.setdefault(a, {"first": 0, "n1": False, "n2": False, "owners": 0, "mask": 0, "stale": False,
                                   "split": False, "lines": 0})
            had = (x["first"] != 0) if m == 17 else x["n1"]
            second = had and x["first"] != val
            if m == 13 and (x["mask"] >> u) & 1:
                second = False
            if not had:
                x["first"] |= val
            mem = x["first"] if m == 21 else nodes[home].memory[addr & 15]
            kinds = {0: (cr.SHARED, cr.EXCLUSIVE), 11: (cr.SHARED,), 12: (cr.SHARED, cr.EXCLUSIVE, cr.MODIFIED)}
            x["stale"] |= st in kinds.get(m, kinds[0]) and val != mem
            x["split"] |= second
            x["n2"] |= had
            x["n1"] = True
            x["owners"] += 1 if st == cr.MODIFIED or (st == cr.EXCLUSIVE and m != 22) else 0
            x["mask"] |= 1 << ((i & 7) if m == 25 else u)
            x["lines"] += 1
    # ---- the bits, address by address
    per = [0] * (N * 16)
    for t in range(N):
        if pristine is not None and nodes[t] is pristine[t] and not any((a >> 4) == t for a in acc):
            continue
        s = nodes[t]
        for b in range(16):
            a = t << 4 | b
            x = acc.get(a)
            d, bv = s.dir_state[b], s.dir_bitvector[b]
            if m == 15 and d == 3:
                d = cr.U
            if m == 10:
                bv &= (1 << N) - 1
            n1 = x is not None
            mask = x["mask"] if n1 else 0
            n2 = n1 and (bin(mask).count("1") >= 2 if m == 16 else x["n2"])
            own = n1 and x["owners"] >= 1
            bits = 0
            if (own or m == 2) and n2 and (m != 1 or x["owners"] >= 2):
                bits |= cr.SWMR
            if d == cr.U and (n2 if m == 3 else n1):
                bits |= cr.DIR_U_HELD
            if d == cr.EM and not (n1 and (not n2 or m == 4) and (own or m == 5)):
                bits |= cr.DIR_EM
            if d == cr.S and ((own and m != 7) or (not n1 and m != 6)):
                bits |= cr.DIR_S
            lost, stale_sharer = mask & ~bv, bv & ~mask
            if m == 26:
                lost, stale_sharer = stale_sharer, lost
            if (d != cr.U or m == 8) and lost:
                bits |= cr.LOST_SHARER
            if (d != cr.U or m == 9) and stale_sharer:
                bits |= cr.STALE_SHARER
            if n1 and x["stale"]:
                bits |= cr.STALE_VALUE
            if n1 and x["split"]:
                bits |= cr.VALUE_SPLIT
            per[a] = bits
    # ---- the record
    bad = [a for a, b in enumerate(per) if b]
    allbits = 0
    for b in per:
        allbits |= b
    if m == 18:
        first = min(bad, key=lambda a: (-(a >> 4), a & 15)) if bad else None
    else:
        first = bad[0] if bad else None
    addrs = sum(bin(per[a]).count("1") for a in bad) if m == 20 else len(bad)
    first_bits = 0 if first is None else (allbits if m == 24 else per[first])
    return {"bits": allbits, "addrs": addrs, "first_addr": cr.NONE if first is None else first,
            "first_bits": first_bits}, per
