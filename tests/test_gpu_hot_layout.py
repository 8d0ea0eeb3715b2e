"""GPU parity where the round loop's cold blocks lie behind the loop.

The lockstep kernels of CACHE_SIZE 4, sim_kernel<P, 4, RING, 0>, reach their rare blocks -- the
accounting of an eviction notice to a node past the system (OOB), the REPLY_ID fan-out, the round
cap and the overflow stop -- through not-taken branches and come back into the round from behind
the loop. Every case is bit-exact parity with the CPU oracle through test_gpu_parity.check_batch
(final state of every node, digest, rounds, error bits, histogram of every system, the run's
totals), on 8-node systems of at most 64 instructions, in batches of 9 (one full wave and a wave
that holds one system) and 16 (two full waves) next to quiet read-only systems.

Each case first proves on the oracle alone that it exercises its path. The round of an event comes
from the oracle's log, whose lines are in (round, node) order: node 7 of every hand-built system
is a clock -- it reads one block of its own memory 64 times, which gives it exactly one log line in
every round from round 0 on (an issue, its own READ_REQUEST, its REPLY_RD, then 63 hits) -- so a
line's round is the number of node-7 lines before it; `ticks == rounds` shows the clock missed
no round. A trip is four rounds (k = round % 4); where a case is about a trip rather than a round
(overflow, round cap), runs capped at trip ends give the oracle's state trip by trip.
"""
import functools

import numpy as np
import pytest

import oracle_ctypes
from oracle_ctypes import LOG_INSTR, LOG_MSG, pack, run_system
from test_gpu_line_field import OOB_WAIT, Sys, quiet_system, shared_by
from test_gpu_parity import check_batch

pytestmark = pytest.mark.gpu

T_RID, T_INV, T_FIA = 4, 5, 10
L = 64
CLOCK = 7
A_FAN = 0x30  # the fan-out's block: home node 3, shared by nodes 2 and 4, written by node 5


def clock(s):
    s.ins[CLOCK] = [pack("R", (CLOCK << 4) | 1, 0)] * L
    return s


def fanout(s, w):
    """Nodes 2 and 4 share block 0 of node 3, node 5 writes it after `w` rounds of hits: one
    REPLY_ID pops at node 5, which fans two INVs out."""
    shared_by(s, A_FAN, [2, 4])
    return s.wait(5, w).wr(5, A_FAN, 0x77)


def oob(s, d):
    """test_gpu_line_field.oob_system on nodes 0 and 1, both delayed by `d` reads of block 2 of
    their own memory (another cache index): node 1's FLUSH_INVACK fill evicts a never-filled line,
    a notice to node 15."""
    s.ins[0] += [pack("R", 0x02, 0)] * d
    s.ins[1] += [pack("R", 0x12, 0)] * d
    s.rd(0, 0x14)
    s.ins[0] += [pack("R", 0x01, 0)] * OOB_WAIT[0]
    s.rd(0, 0x00)
    s.ins[1] += [pack("R", 0x11, 0)] * OOB_WAIT[1]
    return s.wr(1, 0x14, 0xA6)


class Rec:
    """The oracle's result of one clocked system and the round of each of its log lines."""

    def __init__(self, s, max_rounds=0):
        self.tr, self.lens = s.arrays()
        self.res, log = run_system(self.tr, self.lens, num_procs=8, cache_size=4, log=True, log_msgs=True,
                                   max_rounds=max_rounds)
        self.lines = []  # (round, node, message type or None for an issue)
        r = 0
        for x in log.splitlines():
            m = LOG_MSG.match(x)
            node = int(m[1]) if m else int(LOG_INSTR.match(x)[1])
            self.lines.append((r, node, int(m[3]) if m else None))
            r += node == CLOCK
        self.ticks = r

    def rounds_of(self, node, typ):
        return [r for r, n, t in self.lines if n == node and t == typ]

    @property
    def fan(self):  # the round in which node 5 pops its REPLY_ID
        (r,) = self.rounds_of(5, T_RID)
        return r

    @property
    def oob(self):
        """The round in which node 1 sends the notice to node 15. It is home and requester, so both
        FLUSH_INVACKs reach it in consecutive rounds: the first one's fill evicts the never-filled
        line, the second finds the block in the line and evicts nothing (one drop in all)."""
        r, r2 = self.rounds_of(1, T_FIA)
        assert r2 == r + 1
        return r


@functools.lru_cache(maxsize=None)
def build(w=None, d=None, max_rounds=0):
    """A clocked system with the fan-out (writer's wait `w`), the out-of-range notice (delay `d`) or
    both, and its oracle record; the record must show each event once, with its histogram rows and
    error bits, and a clock that ticked in every round."""
    s = clock(Sys())
    if w is not None:
        fanout(s, w)
    if d is not None:
        oob(s, d)
    rec = Rec(s, max_rounds)
    rec.w = w
    res = rec.res
    if not max_rounds:
        assert rec.ticks == res.rounds == L + 2, "the clock missed a round"
        assert res.hist[T_RID] == (w is not None) and res.hist[T_INV] == 2 * (w is not None)
        assert res.hist[T_FIA] == 2 * (d is not None)
        assert res.errors == (oracle_ctypes.ERR_OOB if d is not None else 0) and res.dropped == (d is not None)
    return rec


def fan_at(pred):
    """The fan-out system whose REPLY_ID pops in a round r with pred(r)."""
    for w in range(W_MIN, W_MAX):
        rec = build(w=w)
        if pred(rec.fan):
            return rec
    raise AssertionError("no writer's wait puts the fan-out there")


W_MIN, W_MAX = 18, 58  # the writer's waits: from where both readers hold the block SHARED, to a REPLY_ID in round 61
D_OOB = 20  # the notice's delay: the fan-out needs about 30 rounds before its REPLY_ID


def batch(nsys, placed):
    """`placed`: {system index: Rec}; every other system is a quiet one."""
    systems = [quiet_system() for _ in range(nsys)]
    for i, rec in placed.items():
        systems[i] = (rec.tr, rec.lens)
    return np.stack([x[0] for x in systems]), np.stack([x[1] for x in systems])


def run(dash, nsys, placed, **kw):
    packed, lens = batch(nsys, placed)
    stats = check_batch(dash, packed, lens, 8, 4, **kw)
    quiet = run_system(*quiet_system(), num_procs=8, cache_size=4)
    assert quiet.hist[T_RID] == 0 and quiet.errors == 0
    return stats


NSYS = [9, 16]


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("gap", [0, 1], ids=["A_same_round", "B_consecutive_rounds"])
def test_fanout_and_oob_in_two_systems_of_a_wave(dash, nsys, gap):
    """A, B: the fan-out in one system, the notice in another of the same wave, in the same round
    and one round later."""
    o = build(d=D_OOB)
    f = fan_at(lambda r: r + gap == o.oob)
    assert f.fan + gap == o.oob
    stats = run(dash, nsys, {2: f, 5: o})
    assert stats["hist"][T_RID] == 1 and stats["err_bits"] == dash.ERR_OOB and stats["dropped"] == 1


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("gap", [0, 1, -1], ids=["same_round", "oob_after", "oob_before"])
def test_fanout_and_oob_in_one_system(dash, nsys, gap):
    """C: both in the same system (disjoint nodes), in one round and in neighbouring rounds."""
    o = build(d=D_OOB)
    both = None
    for w in range(W_MIN, W_MAX):
        rec = build(w=w, d=D_OOB)
        if rec.fan + gap == rec.oob:
            both = rec
            break
    assert both is not None and both.oob == o.oob and both.fan + gap == both.oob
    stats = run(dash, nsys, {0: both, nsys - 1: both})
    assert stats["hist"][T_RID] == 2 and stats["err_bits"] == dash.ERR_OOB and stats["dropped"] == 2


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("where", [0, 7], ids=["first", "last"])
@pytest.mark.parametrize("what", ["fanout", "oob"])
def test_each_alone_at_the_ends_of_a_wave(dash, nsys, what, where):
    """D: each alone, as the first and as the last system of the (full) first wave."""
    rec = fan_at(lambda r: True) if what == "fanout" else build(d=D_OOB)
    stats = run(dash, nsys, {where: rec})
    if what == "fanout":
        assert stats["hist"][T_RID] == 1 and stats["hist"][T_INV] == 2 and stats["err_bits"] == 0
    else:
        assert stats["hist"][T_RID] == 0 and stats["err_bits"] == dash.ERR_OOB and stats["dropped"] == 1


@pytest.mark.parametrize("nsys", NSYS)
@pytest.mark.parametrize("k", range(4))
def test_fanout_in_every_round_of_a_trip(dash, nsys, k):
    """E: the fan-out falls in round k of a four-round trip."""
    f = fan_at(lambda r: r % 4 == k)
    assert f.fan % 4 == k
    stats = run(dash, nsys, {3: f, nsys - 1: f})
    assert stats["hist"][T_RID] == 2 and stats["hist"][T_INV] == 4


DEEP = (1, 21543)  # generator seed and system id of a 64-instruction contention system with a queue of 17


@functools.lru_cache(maxsize=None)
def deep_system():
    """(trace, lens, trip): a generated system one of whose queues exceeds 16 entries, and the trip in
    which it first does: the oracle's maximum depth of runs capped at each trip's end."""
    tr = oracle_ctypes.gen_system(DEEP[0], DEEP[1], 8, L, kind=1)
    lens = np.full(8, L, np.uint32)
    assert run_system(tr, lens, num_procs=8, cache_size=4).max_depth > 16
    trip = 0
    while run_system(tr, lens, num_procs=8, cache_size=4, max_rounds=4 * (trip + 1)).max_depth <= 16:
        trip += 1
    return tr, lens, trip


@pytest.mark.parametrize("nsys", NSYS)
def test_fanout_in_the_trip_of_an_overflow(dash, nsys):
    """F: a queue of the wave's system 1 passes 16 entries in trip K, the kernel's overflow stop runs
    at the start of trip K + 1 and the system goes to the 32-deep tier; fan-outs pop in the same wave
    in trip K (system 0) and in trip K + 1 (system 6)."""
    tr, lens, K = deep_system()
    f0 = fan_at(lambda r: r // 4 == K)
    f1 = fan_at(lambda r: r // 4 == K + 1)
    assert f0.fan // 4 == K and f1.fan // 4 == K + 1
    packed, plens = batch(nsys, {0: f0, 6: f1})
    packed[1], plens[1] = tr, lens
    stats = check_batch(dash, packed, plens, 8, 4)
    assert stats["tier_systems"][0] == nsys and stats["tier_systems"][1] == 1 and stats["max_depth"] > 16


@pytest.mark.parametrize("nsys", NSYS)
def test_fanout_in_the_trip_that_ends_at_the_round_cap(dash, nsys):
    """G: the REPLY_ID pops in the last trip before the round cap, which then stops every system of
    the batch (all are still active: ERR_ROUNDCAP in each)."""
    f = fan_at(lambda r: r % 4 == 2)
    cap = (f.fan // 4 + 1) * 4
    capped = build(w=f.w, max_rounds=cap)
    assert cap - 4 <= f.fan < cap and capped.res.hist[T_RID] == 1 and capped.res.rounds == cap
    assert capped.res.errors == oracle_ctypes.ERR_ROUNDCAP
    before = build(w=f.w, max_rounds=cap - 4)
    assert before.res.hist[T_RID] == 0
    quiet = run_system(*quiet_system(), num_procs=8, cache_size=4, max_rounds=cap)
    assert quiet.errors == oracle_ctypes.ERR_ROUNDCAP
    stats = run(dash, nsys, {0: f, 7: f}, max_rounds=cap)
    assert stats["hist"][T_RID] == 2 and stats["err_bits"] == dash.ERR_ROUNDCAP
