"""GPU parity where both ring stores of a round are ranked in every lane.

Below the final tier the lockstep kernels of CACHE_SIZE 4, sim_kernel<P, 4, 16 | 32, 0>, read the
(arrival mask, tail) pair of the primary's and of the flush copy's receiver in every lane, lanes that
send nothing included, rank both slots and only then store, each store under its own lane mask
(DASH_FLAT_PLACE). Every case is bit-exact parity with the CPU oracle through
test_gpu_parity.check_batch -- final state of every node, digest, rounds, error bits and histogram of
every system, the run's drops and maximum depth -- on systems of at most 64 instructions per node in
batches of at most 16.

Each case first proves on the oracle's event log that it holds what it is about. Node 7 of every
hand-built system is a clock (test_gpu_hot_layout): one log line in every round, so a line's round is
the number of node-7 lines before it. A node's pops appear in its queue's order, so the order of
arrivals is read off the receiver's lines, and "the same round" off the lines of the senders' steps.
"""
import functools

import numpy as np
import pytest

import oracle_ctypes
from oracle_ctypes import LOG_INSTR, LOG_MSG, gen_system, pack, run_system
from test_gpu_hot_layout import CLOCK, D_OOB, batch, clock
from test_gpu_hot_layout import build as clocked_oob
from test_gpu_line_field import Sys, oob_system, quiet_system, shared_by
from test_gpu_parity import check_batch

pytestmark = pytest.mark.gpu

(T_RR, T_WRQ, T_RRD, T_RWR, T_RID, T_INV, T_UPG, T_WBINV, T_WBINT, T_FLUSH, T_FIA, T_ES,
 T_EMOD) = range(13)
D_EM, D_S, D_U = 0, 1, 2
L = 64
NSYS = [9, 16]  # one full wave and a wave of one system; two full waves


class Log:
    """The oracle's result of one clocked 8-node system and its log lines with their rounds:
    (round, node, sender, type, address), sender and type None for an issue."""

    def __init__(self, s):
        self.tr, self.lens = s.arrays()
        self.res, text = run_system(self.tr, self.lens, num_procs=8, cache_size=4, log=True, log_msgs=True)
        self.ev = []
        r = 0
        for x in text.splitlines():
            m = LOG_MSG.match(x)
            if m:
                self.ev.append((r, int(m[1]), int(m[2]), int(m[3]), int(m[4], 16)))
            else:
                i = LOG_INSTR.match(x)
                self.ev.append((r, int(i[1]), None, None, int(i[3], 16)))
            r += self.ev[-1][1] == CLOCK
        assert r == self.res.rounds == L + 2, "the clock missed a round"

    def pops(self, node):
        """The node's pops in queue order: (round, sender, type, address)."""
        return [(r, f, t, a) for r, n, f, t, a in self.ev if n == node and t is not None]

    def pop_round(self, node, typ, sender=None):
        (r,) = [r for r, f, t, _a in self.pops(node) if t == typ and sender in (None, f)]
        return r

    def issue_round(self, node, addr):
        (r,) = [r for r, n, _f, t, a in self.ev if n == node and t is None and a == addr]
        return r


def run(dash, nsys, placed, **kw):
    """`placed`: {system index: an object with .tr and .lens}; the other systems are quiet ones."""
    packed, lens = batch(nsys, placed)
    return check_batch(dash, packed, lens, 8, 4, **kw)


# ---- lanes that send nothing while their receiver index is no node's ----

def es_last_sharer():
    """Node 0 holds block 0 of node 3 EXCLUSIVE and replaces it: the home pops EVICT_SHARED from the
    entry's only sharer (es_bv == 0, es_own = ffbl(0)), the entry goes UNOWNED, nothing is sent."""
    a = 0x30
    lg = Log(clock(Sys()).rd(0, a).wait(0, 8).rd(0, a + 4))
    home = lg.res.node[3]
    assert lg.res.hist[T_ES] == 1 and lg.pop_round(3, T_ES, 0) > 0  # one notice: the home passed none on
    assert home.dir_state[0] == D_U and home.dir_bitvector[0] == 0
    return lg


def es_two_left():
    """Three sharers, one replaces the line: the home pops EVICT_SHARED, two sharers stay (es_pop == 2),
    nothing is sent."""
    a = 0x30
    lg = Log(shared_by(clock(Sys()), a, [0, 2, 5]).wait(0, 20).rd(0, a + 4))
    home = lg.res.node[3]
    assert lg.res.hist[T_ES] == 1 and lg.pop_round(3, T_ES, 0) > 0
    assert home.dir_state[0] == D_S and home.dir_bitvector[0] == (1 << 2) | (1 << 5)
    return lg


def request_at_em():
    """A READ_REQUEST popped at an EXCLUSIVE_MODIFIED entry: the home forwards it to own = ffbl(bv),
    the one lane state that uses that index (such a lane always sends)."""
    a = 0x30
    lg = Log(clock(Sys()).wr(0, a, 0x11).wait(4, 14).rd(4, a))
    assert lg.res.hist[T_WBINT] == 1 and lg.pop_round(0, T_WBINT, 3) > lg.pop_round(3, T_RR, 4)
    return lg


IDLE = {"es_last_sharer": es_last_sharer, "es_two_left": es_two_left, "request_at_em": request_at_em}


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("case", sorted(IDLE))
def test_idle_senders_in_the_first_and_the_last_segment(dash, case, nsys):
    """Systems 0 and 7 of the first wave (segments 0 and 7): in segment 0 an index of all ones would
    address the word below the arrival masks."""
    lg = IDLE[case]()
    assert lg.res.errors == 0
    stats = run(dash, nsys, {0: lg, 7: lg})
    assert stats["err_bits"] == 0 and stats["dropped"] == 0


# ---- the notice to node 15: a never-filled line (address 0xFF) evicted ----

@pytest.mark.parametrize("nsys", NSYS)
def test_never_filled_line_evicted_in_the_last_segment(dash, nsys):
    """N = 8: the notice's lane is in segment 7 of its wave; its receiver index is 15."""
    o = clocked_oob(d=D_OOB)
    assert o.res.errors == oracle_ctypes.ERR_OOB and o.res.dropped == 1 and o.oob > 0
    stats = run(dash, nsys, {7: o, nsys - 1: o})
    assert stats["err_bits"] == dash.ERR_OOB and stats["dropped"] == 2


@pytest.mark.parametrize("N", [3, 5, 6, 7])
def test_never_filled_line_evicted_in_the_last_segment_of_partial_systems(dash, N):
    """N < P: the lanes past the system read a slot too (their line is never filled: index 15). The
    notice's system is the last of the batch's last wave (16 systems: one wave at P = 4, two at 8)."""
    tr, lens = oob_system(N)
    alone, text = run_system(tr, lens, num_procs=N, cache_size=4, log=True, log_msgs=True)
    assert alone.errors == oracle_ctypes.ERR_OOB and alone.dropped == 1
    fia = [x for x in text.splitlines() if (m := LOG_MSG.match(x)) and int(m[1]) == 1 and int(m[3]) == T_FIA]
    assert len(fia) == 2  # home and requester: the first fill evicts the never-filled line
    gen = [gen_system(0x5EED, s, N, 16, kind=0) for s in range(15)]
    packed = np.stack(gen + [tr])
    plens = np.stack([np.full(N, 16, np.uint32)] * 15 + [lens])
    others = sum(run_system(g, np.full(N, 16, np.uint32), num_procs=N, cache_size=4).dropped for g in gen)
    stats = check_batch(dash, packed, plens, N, 4)
    assert stats["err_bits"] & dash.ERR_OOB and stats["dropped"] == 1 + others


# ---- five arrivals at one receiver in one round ----

H, X, Y, Z = 1, 0, 4, 5  # receiver (home and requester of the flushed block), owner, reader, writer
A_FL, A_RD, A_SH, A_OLD = 0x14, 0x13, 0x32, 0x16  # cache indices 0, 3, 2, 2


def crowd_system(wh, wy, wz, pre, ext):
    """Node 1 receives in one round, if the waits line up: both FLUSH_INVACKs of node 0 (it pops the
    WRITEBACK_INV of node 1's write to its own block 4, which node 0 holds: primary to the home, flush
    copy to the requester, the same node), node 4's READ_REQUEST for block 3 of node 1, and from node 5,
    which pops the REPLY_ID of its write to block 2 of node 3 (shared by nodes 1 and 2), an INV and the
    EVICT_SHARED of the line the fill replaces, block 6 of node 1. What moves the tail of node 1's
    ring beforehand: `pre` reads of node 1's own blocks of cache index 3 (each a miss: two messages,
    from the second on an eviction notice to itself too) and `ext` reads of node 1's blocks 9 and 10
    and then 8 and 12 by node 6 (one READ_REQUEST each, the last an eviction notice too)."""
    s = clock(Sys())
    s.ins[H] += [pack("R", (H << 4) | (7 + 4 * (i % 3)), 0) for i in range(pre)]
    s.ins[6] += [pack("R", (H << 4) | b, 0) for b in (9, 10, 8, 12)[:ext]]
    s.rd(X, A_FL)
    shared_by(s, A_SH, [H, 2])
    s.wait(H, wh).wr(H, A_FL, 0xA6)
    s.wait(Y, wy).rd(Y, A_RD)
    s.rd(Z, A_OLD).wait(Z, wz).wr(Z, A_SH, 0x77)
    return s


def aligned(pre, ext, wh=16):
    """The crowd system whose three senders step in one round: the waits of nodes 4 and 5 follow the
    round of node 0's WRITEBACK_INV until all three agree (the waits shift one another by a round or
    two, hence the iteration)."""
    wy = wz = 12
    for _ in range(12):
        try:
            lg = Log(crowd_system(wh, wy, wz, pre, ext))
            r = lg.pop_round(X, T_WBINV, H)
            dz, dy = r - lg.pop_round(Z, T_RID, 3), r - lg.issue_round(Y, A_RD)
        except (AssertionError, ValueError):
            return None
        if dz == 0 and dy == 0:
            return lg
        wz, wy = wz + dz, wy + dy
        if min(wz, wy) < 1 or max(wz, wy) > 60:
            return None
    return None


def crowd_round(lg):
    """The round of the five sends if they share one, else None."""
    try:
        r = lg.pop_round(X, T_WBINV, H)
        if lg.pop_round(Z, T_RID, 3) != r or lg.issue_round(Y, A_RD) != r:
            return None
    except ValueError:
        return None
    return r


WANT = [(X, T_FIA, A_FL), (X, T_FIA, A_FL), (Y, T_RR, A_RD), (Z, T_INV, A_SH), (Z, T_ES, A_OLD)]


def proven(lg):
    """The ring slot of the first of the five arrivals (the messages node 1 received before, mod 16)
    if the log shows the crowd, else None: the three senders step in one round, node 1 pops the five
    in the five rounds after it, in a row, lowest sender first, the INV before the notice."""
    r = crowd_round(lg)
    if r is None:
        return None
    pops = lg.pops(H)
    got = [(f, t, a) for _r, f, t, a in pops]
    k = next((i for i in range(len(got) - 4) if got[i:i + 5] == WANT), None)
    if k is None or [p[0] for p in pops[k:k + 5]] != list(range(r + 1, r + 6)):
        return None
    assert lg.res.errors == 0 and lg.res.max_depth >= 5
    return k % 16


@functools.lru_cache(maxsize=None)
def crowds():
    """{first slot: Log} of proven crowd systems: one whose five arrivals lie inside the ring, and one
    each that wraps after the third, second and first of them."""
    found = {}
    for pre in range(5):
        for ext in range(5):
            lg = aligned(pre, ext)
            k = proven(lg) if lg is not None else None
            if k is not None:
                found.setdefault(k, lg)
    assert {13, 14, 15} <= set(found) and min(found) <= 11, f"the search found first slots {sorted(found)} only"
    return found


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("first", [None, 13, 14, 15], ids=["inside", "wrap_after_3", "wrap_after_2", "wrap_after_1"])
def test_five_arrivals_at_one_receiver_in_one_round(dash, nsys, first):
    """Primary and flush copy of one sender, another sender's primary, a REPLY_ID's INV and its eviction
    notice, all at node 1 in one round; with `first` the five straddle the end of the 16-deep ring (the
    receiver's tail wraps in that round)."""
    found = crowds()
    lg = found[min(found) if first is None else first]
    assert first is not None or min(found) + 5 <= 16
    stats = run(dash, nsys, {1: lg, nsys - 1: lg})
    assert stats["err_bits"] == 0 and stats["max_depth"] >= 5 and stats["tier_systems"][1] == 0


# ---- queue depths at the ring's capacity ----

DEPTH = {15: (1, 127), 16: (1, 755), 17: (1, 1016)}  # generator seed and id of contention systems by maximum depth


def deep(d):
    tr = gen_system(DEPTH[d][0], DEPTH[d][1], 8, L, kind=1)
    lens = np.full(8, L, np.uint32)
    assert run_system(tr, lens, num_procs=8, cache_size=4).max_depth == d
    return tr, lens


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("depths", [(15,), (16,), (15, 16), (15, 16, 17)], ids=lambda d: "_".join(map(str, d)))
def test_queues_at_the_capacity_of_the_first_tier(dash, nsys, depths):
    """A queue of 15 and one that fills the 16-deep ring stay in the first tier; one of 17 hands its
    system to the 32-deep tier, which takes the same code."""
    packed, lens = batch(nsys, {})
    for i, d in enumerate(depths):
        packed[2 + 3 * i], lens[2 + 3 * i] = deep(d)
    stats = check_batch(dash, packed, lens, 8, 4)
    assert stats["max_depth"] == max(depths)
    assert stats["tier_systems"][0] == nsys and stats["tier_systems"][1] == (17 in depths)


# ---- rounds in which a store's lane mask is empty in the whole wave ----

def hits_only():
    """Every node reads one block of its own memory 64 times: an issue, its READ_REQUEST, its REPLY_RD,
    then hits. From round 3 on no lane sends anything."""
    s = Sys()
    for n in range(8):
        s.ins[n] = [pack("R", (n << 4) | 1, 0)] * L
    lg = Log(s)
    assert sum(lg.res.hist) == 16 and max(r for r, _n, _f, t, _a in lg.ev if t is not None) == 2
    assert {r for r, *_ in lg.ev} == set(range(L + 2))  # issues go on in every later round: hits
    return lg


@pytest.mark.parametrize("nsys", [8, 9])
def test_rounds_without_a_primary_in_the_wave(dash, nsys):
    """The first wave holds hit-only systems alone: 63 rounds in which no lane of it sends a primary
    (or a flush copy: only a lane with a reply sends one), both stores' masks empty."""
    lg = hits_only()
    packed = np.stack([lg.tr] * 8 + [quiet_system()[0]] * (nsys - 8))
    lens = np.stack([lg.lens] * 8 + [quiet_system()[1]] * (nsys - 8))
    stats = check_batch(dash, packed, lens, 8, 4)
    assert stats["hist"][T_RR] >= 64 and stats["err_bits"] == 0


@pytest.mark.parametrize("nsys", [8, 16])
def test_rounds_without_a_flush_copy_in_the_wave(dash, nsys):
    """Quiet systems alone: primaries in every round (requests, replies, eviction notices), never a
    write-back, so the flush copy's mask is empty in every round of every wave."""
    q = run_system(*quiet_system(), num_procs=8, cache_size=4)
    assert q.hist[T_WBINV] == q.hist[T_WBINT] == 0 and q.hist[T_RR] == 8 * L and q.hist[T_ES] > 0
    packed, lens = batch(nsys, {})
    stats = check_batch(dash, packed, lens, 8, 4)
    assert stats["hist"][T_WBINV] == stats["hist"][T_WBINT] == 0 and stats["hist"][T_RR] == nsys * 8 * L
