"""Delay words on the host (no GPU): dash_delay_count / dash_delay_word against itertools.combinations,
dash_delay_schedule against the definition (tests/delay_ref.py restates both without libdash), the
DASH_EINVAL cases, and the preconditions of tests/test_gpu_delays.py asserted on the CPU oracle: the sizes
and outcome counts of the test_3 / test_4 spaces, the fewest delays that reach each accepted run, and a
generated 8-node source whose space has more than one outcome."""
import ctypes
from math import comb

import numpy as np
import pytest

import delay_ref as dr

SPACES = [(3, 4, 2, 3), (2, 8, 1, 4), (5, 4, 3, 2)]  # (R, N, E, D)


@pytest.mark.parametrize("R,N,E,D", SPACES)
def test_delay_word_is_the_combinations_in_rank_order(dash, R, N, E, D):
    want = list(dr.words(R, N, E, D))
    K = dash.delay_count(R, E, D, N)
    assert K == len(want) == dr.count(R, N, E, D)
    got = [dash.delay_word(R, E, D, N, i) for i in range(K)]
    assert got == want
    assert got[0] == dr.LOCKSTEP == dash.DELAY_LOCKSTEP
    assert len(set(got)) == K  # bijective onto the cell sets
    delays = [dr.delay_count_of(w) for w in got]
    assert delays == sorted(delays) and delays[-1] == min(D, R * N * E)
    M, B = R * N * E, 0
    for d in range(D + 1):  # the block starts
        assert delays.index(d) == B and delays.count(d) == comb(M, d)
        B += comb(M, d)
    # within a word the slots hold descending cells from the top used slot down, the rest are empty
    for w in got:
        s = dash.delay_unpack(w)
        assert len(s) == dr.delay_count_of(w) and dash.delay_pack(s) == w


def test_delay_word_large_space_and_fast_twin():
    """The nested-loop order the oracle lists use is the sorted-combinations order."""
    want = list(dr.words(3, 4, 2, 3))
    assert list(dr.words_fast(3, 4, 2, 3)) == want
    assert [dr.word_at(3, 4, 2, 3, i) for i in range(len(want))] == want


def test_delay_word_at_the_largest_space(dash):
    """M = 1023 * 8 * 8 = 65,472 cells, D = 4: the last index is the four highest cells, and the
    arithmetic stays exact (C(M, 4) is about 7.7e17)."""
    R, N, E, D = 1023, 8, 8, 4
    M = R * N * E
    K = dash.delay_count(R, E, D, N)
    assert K == sum(comb(M, d) for d in range(5))
    assert dash.delay_word(R, E, D, N, K - 1) == dr.pack(dr.cell_slot(c, N, E) for c in range(M - 4, M))
    for d in range(1, 5):  # the first and last of every block
        B = sum(comb(M, k) for k in range(d))
        assert dash.delay_word(R, E, D, N, B) == dr.pack(dr.cell_slot(c, N, E) for c in range(d))
        assert dash.delay_word(R, E, D, N, B - 1) == dr.pack(dr.cell_slot(c, N, E) for c in range(M - d + 1, M))
    rng = np.random.default_rng(5)
    for _ in range(200):  # random cell sets: rank, then unrank
        d = int(rng.integers(1, 5))
        cells = sorted(int(c) for c in rng.choice(M, size=d, replace=False))
        idx = sum(comb(M, k) for k in range(d)) + sum(comb(c, k + 1) for k, c in enumerate(cells))
        assert dash.delay_word(R, E, D, N, idx) == dr.pack(dr.cell_slot(c, N, E) for c in cells)


WORDS = {
    "lockstep": dr.LOCKSTEP,
    "overlapping slots on one node": dr.pack([dr.slot(1, 2, 3), dr.slot(1, 3, 5)]),
    "a repeated slot": dr.pack([dr.slot(2, 1, 4), dr.slot(2, 1, 4)]),
    "a slot on node 5": dr.pack([dr.slot(5, 2, 1), dr.slot(0, 0, 2)]),
    "start 1022": dr.pack([dr.slot(0, 1, 1022)]),
    "e = 7": dr.pack([dr.slot(3, 7, 6)]),
    "four slots": dr.pack([dr.slot(0, 0, 0), dr.slot(1, 1, 1), dr.slot(2, 2, 2), dr.slot(3, 3, 3)]),
    "an empty slot between two": dr.pack([dr.slot(0, 2, 9), dr.EMPTY, dr.slot(3, 0, 1)]),
}


@pytest.mark.parametrize("name", WORDS)
@pytest.mark.parametrize("N", [1, 4, 5, 8])
def test_delay_schedule_is_the_definition(dash, name, N):
    word, rounds = WORDS[name], 1160
    got = dash.delay_schedule(word, N, rounds)
    assert np.array_equal(got, dr.schedule(word, N, rounds))
    sat = int((got == dash.SIT_OUT).sum())
    if name == "start 1022":
        assert sat == 2 and got[1022, 0] == got[1023, 0] == dash.SIT_OUT
    if name == "e = 7" and N > 3:
        assert sat == 128
    if name == "a slot on node 5" and N <= 5:
        assert sat == 1  # only node 0's round 2
    if name == "overlapping slots on one node" and N > 1:
        assert sat == 10  # rounds 3 .. 12 of node 1
    assert dash.delay_schedule(word, N, 0).shape == (0, N)


def test_pack_unpack_format(dash):
    w = dash.delay_pack([(1, 2, 64), (3, 1022, 1)])
    assert w == dr.pack([dr.slot(1, 6, 2), dr.slot(3, 0, 1022)])
    assert dash.delay_unpack(w) == [(1, 2, 64), (3, 1022, 1)]
    assert dash.delay_format(w) == "1@2+64,3@1022+1" and dash.delay_format(dash.DELAY_LOCKSTEP) == ""
    assert dash.delay_pack([]) == dash.DELAY_LOCKSTEP
    for bad in ([(8, 0, 1)], [(0, 1023, 1)], [(0, 0, 3)], [(0, 0, 256)], [(0, 0, 0)], [(0, 0, 1)] * 5):
        with pytest.raises(ValueError):
            dash.delay_pack(bad)


def test_einval(dash):
    def code(fn, *a):
        with pytest.raises(dash.DashError) as e:
            fn(*a)
        return e.value.code

    for R, E, D, N in [(0, 1, 1, 4), (1024, 1, 1, 4), (1, 0, 1, 4), (1, 9, 1, 4), (1, 1, 5, 4), (1, 1, 1, 0),
                       (1, 1, 1, 9), (1 << 32 - 1, 1, 1, 4)]:
        assert code(dash.delay_count, R, E, D, N) == dash.EINVAL
        assert code(dash.delay_word, R, E, D, N, 0) == dash.EINVAL
    K = dash.delay_count(3, 2, 2, 4)
    assert code(dash.delay_word, 3, 2, 2, 4, K) == dash.EINVAL
    assert code(dash.delay_word, 3, 2, 0, 4, 1) == dash.EINVAL and dash.delay_word(3, 2, 0, 4, 0) == dr.LOCKSTEP
    L, sp, out = dash.lib(), dash.DelaySpace(3, 2, 2, 0), ctypes.c_uint64()
    assert L.dash_delay_count(None, 4, ctypes.byref(out)) == dash.EINVAL
    assert L.dash_delay_count(ctypes.byref(sp), 4, None) == dash.EINVAL
    assert L.dash_delay_word(None, 4, 0, ctypes.byref(out)) == dash.EINVAL
    assert L.dash_delay_word(ctypes.byref(sp), 4, 0, None) == dash.EINVAL
    buf = np.zeros(8, np.uint8)
    assert L.dash_delay_schedule(dr.LOCKSTEP, 0, 1, buf.ctypes.data) == dash.EINVAL
    assert L.dash_delay_schedule(dr.LOCKSTEP, 9, 1, buf.ctypes.data) == dash.EINVAL
    assert L.dash_delay_schedule(dr.LOCKSTEP, 4, 1, None) == dash.EINVAL


# ---------------------------------------------------------------- preconditions of the GPU tests

@pytest.mark.parametrize("test,rounds,k1,k2,n1", [("test_3", 33, 925, 427_351, 19), ("test_4", 50, 1_401, 980_701, 7)])
def test_spaces_of_the_golden_tests(test, rounds, k1, k2, n1):
    assert dr.lockstep_rounds(test) == rounds
    assert (dr.count(rounds, 4, 7, 1), dr.count(rounds, 4, 7, 2)) == (k1, k2)
    one = dr.golden_list(test, 1)
    assert len(one) == n1 and sum(o["count"] for o in one) == k1 and one[0]["seed"] == 0
    two = dr.recorded(test)  # the D = 2 list, recorded (tests/golden/make_delay_outcomes.py)
    assert len(two) == (97 if test == "test_3" else 41) and sum(o["count"] for o in two) == k2
    assert [o["seed"] for o in two] == sorted(o["seed"] for o in two)
    # the D <= 1 block of the recorded list is the live list's witnesses
    assert [(o["digest"], o["errors"], o["seed"], o["rounds"]) for o in two if o["seed"] < k1] == \
           [(o["digest"], o["errors"], o["seed"], o["rounds"]) for o in one]


@pytest.mark.parametrize("test,run", dr.ACCEPTED)
def test_fewest_delays_of_the_accepted_runs(test, run):
    """The lowest index that reaches an accepted output lies in the block of its delay count."""
    R, want = dr.lockstep_rounds(test), dr.ACCEPTED[(test, run)]
    hit = [o for o in dr.recorded(test) if o["digest"] == dr.accepted_digest(test, run) and o["errors"] == 0]
    assert len(hit) == 1
    block = [dr.count(R, 4, 7, d - 1) if d else 0 for d in range(4)]
    assert block[want] <= hit[0]["seed"] < block[want + 1]
    # and the recorded witness reproduces it on the oracle
    word = dr.word_at(R, 4, 7, 2, hit[0]["seed"])
    assert dr.delay_count_of(word) == want
    assert dr.run_word(*dr.golden(test), word).digest == dr.accepted_digest(test, run)


def test_generated_source_has_outcomes_to_tell_apart():
    outs = dr.generated_list()
    assert len(outs) >= 2 and sum(o["count"] for o in outs) == dr.count(8, 8, 3, 2) == 18_529
