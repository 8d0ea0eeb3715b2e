"""Plain-Python reference of the coherence invariants of a final state (include/dash.h, the
DASH_COH_* bits), written from the definitions alone: per address, collect the copies, then state
each bit as the header does. No shortcut shared with the C or the HIP implementation.

TEST INFRASTRUCTURE: used by tests/test_coherence_spec.py (CPU) and tests/test_gpu_coherence.py.
A node state is any object with the fields of dash_node_state (dash.NodeState, the oracle's
OrcNodeState): memory, dir_bitvector, dir_state, cache_addr, cache_value, cache_state.
"""
SWMR, DIR_U_HELD, DIR_EM, DIR_S, LOST_SHARER, STALE_SHARER, STALE_VALUE, VALUE_SPLIT = (1 << k for k in range(8))
MODIFIED, EXCLUSIVE, SHARED, INVALID = range(4)
EM, S, U = range(3)
NONE = 0xFFFFFFFF
FIELDS = ("bits", "addrs", "first_addr", "first_bits")


def address_bits(nodes, num_procs, cache_size, a):
    home, block = a >> 4, a & 15
    copies = [(t, nodes[t].cache_value[i], nodes[t].cache_state[i])
              for t in range(num_procs) for i in range(cache_size)
              if nodes[t].cache_addr[i] == a and nodes[t].cache_state[i] != INVALID]
    n = len(copies)
    own = sum(1 for _, _, st in copies if st in (MODIFIED, EXCLUSIVE))
    mask = 0
    for t, _, _ in copies:
        mask |= 1 << t
    d = nodes[home].dir_state[block]
    bv = nodes[home].dir_bitvector[block]
    mem = nodes[home].memory[block]
    bits = 0
    if own >= 1 and n >= 2:
        bits |= SWMR
    if d == U and n >= 1:
        bits |= DIR_U_HELD
    if d == EM and not (n == 1 and own == 1):
        bits |= DIR_EM
    if d == S and (own >= 1 or n == 0):
        bits |= DIR_S
    if d != U and (mask & ~bv) != 0:
        bits |= LOST_SHARER
    if d != U and (bv & ~mask) != 0:  # bits of bv at or above num_procs count
        bits |= STALE_SHARER
    if any(st in (SHARED, EXCLUSIVE) and v != mem for _, v, st in copies):
        bits |= STALE_VALUE
    if len({v for _, v, _ in copies}) >= 2:
        bits |= VALUE_SPLIT
    return bits


def check(nodes, num_procs, cache_size):
    """(record dict with FIELDS, per-address bits list [num_procs * 16]) of one system."""
    per = [address_bits(nodes, num_procs, cache_size, a) for a in range(num_procs * 16)]
    bad = [a for a, b in enumerate(per) if b]
    bits = 0
    for b in per:
        bits |= b
    return {"bits": bits, "addrs": len(bad), "first_addr": bad[0] if bad else NONE,
            "first_bits": per[bad[0]] if bad else 0}, per


def record(rec):
    """A structured-array element or dict as a plain dict of ints."""
    return {f: int(rec[f]) for f in FIELDS}
