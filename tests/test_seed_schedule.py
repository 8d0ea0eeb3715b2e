"""dash_seed_schedule: a schedule seed written out as a dash_set_schedule table (CPU only).

The table must be the seeded schedule itself -- the oracle twins orc_arb_stall / orc_arb_prio
round by round and node by node -- and fed back through the oracle as an explicit schedule it
must reproduce the seeded run. Seed 0 is the lockstep schedule, as in dash_set_system_seeds.
"""
import ctypes

import numpy as np
import pytest

import oracle_ctypes as oc

ROUNDS = 128
# 16 seeds: the ones the racy tests' outcomes were found at, the extremes of the 64-bit range,
# and a fixed random draw
SEEDS = [87, 0xABCDEF, 1 << 63, (1 << 64) - 1, 1, 2, 413, 2316, 0x5EED5EED, 1 << 32, (1 << 32) - 1] + \
    [int(s) for s in np.random.default_rng(20).integers(1, 1 << 63, size=5, dtype=np.uint64)]
NODE_COUNTS = (1, 2, 3, 4, 8)


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


@pytest.fixture(scope="module")
def twins():
    L = oc.lib()
    L.orc_arb_stall.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    L.orc_arb_stall.restype = ctypes.c_int
    L.orc_arb_prio.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    L.orc_arb_prio.restype = ctypes.c_uint32
    return L


def test_seed_count():
    assert len(SEEDS) == len(set(SEEDS)) == 16 and 0 not in SEEDS


@pytest.mark.parametrize("N", NODE_COUNTS)
def test_table_is_the_oracle_twins(dash, twins, N):
    """Every round < 128, every node: sits out exactly when orc_arb_stall says so, else holds
    orc_arb_prio's position at P = next_pow2(N) (also for a non-power-of-two node count)."""
    P = next_pow2(N)
    for seed in SEEDS:
        sched = dash.seed_schedule(seed, N, ROUNDS)
        assert sched.shape == (ROUNDS, N) and sched.dtype == np.uint8
        exp = np.array([[dash.SIT_OUT if twins.orc_arb_stall(seed, r, t) else twins.orc_arb_prio(seed, r, t, P)
                         for t in range(N)] for r in range(ROUNDS)], dtype=np.uint8)
        assert np.array_equal(sched, exp), hex(seed)
        stepping = sched != dash.SIT_OUT
        assert (sched[stepping] < P).all()
        for r in range(ROUNDS):  # a valid dash_set_schedule row: distinct positions
            row = sched[r][stepping[r]]
            assert len(set(row.tolist())) == len(row)


@pytest.mark.parametrize("N", NODE_COUNTS)
def test_seed_zero_is_lockstep(dash, N):
    sched = dash.seed_schedule(0, N, 12)
    assert np.array_equal(sched, np.tile(np.arange(N, dtype=np.uint8), (12, 1)))


@pytest.mark.parametrize("test", ["test_3", "test_4"])
@pytest.mark.parametrize("seed", [87, 413, 2316])
def test_table_replays_the_seeded_run(dash, test, seed):
    """run_system(sched = the seed's table) is run_system(arb_seed = seed): 128 rounds cover the
    longest of these runs (94 rounds), and later rounds find the system quiescent."""
    tr, lens = oc.load_test_dir(oc.GOLDEN / test)
    want = oc.run_system(tr, lens, arb_seed=seed)
    assert want.rounds <= ROUNDS
    got = oc.run_system(tr, lens, sched=dash.seed_schedule(seed, 4, ROUNDS))
    assert (got.digest, got.rounds, list(got.hist)) == (want.digest, want.rounds, list(want.hist))
    assert got.errors == want.errors == 0
    # the rounds the run took are enough
    cut = oc.run_system(tr, lens, sched=dash.seed_schedule(seed, 4, int(want.rounds)))
    assert (cut.digest, cut.rounds, list(cut.hist)) == (want.digest, want.rounds, list(want.hist))


def test_argument_checks(dash):
    L = dash.lib()
    buf = np.zeros(9 * 4, dtype=np.uint8)
    assert L.dash_seed_schedule(87, 0, 4, buf.ctypes.data) == dash.EINVAL
    assert L.dash_seed_schedule(87, 9, 4, buf.ctypes.data) == dash.EINVAL
    assert L.dash_seed_schedule(87, 4, 4, None) == dash.EINVAL
    assert not buf.any()
    assert L.dash_seed_schedule(87, 4, 0, buf.ctypes.data) == dash.OK and not buf.any()  # nothing written
    guard = np.full(4 * 4 + 8, 0xEE, dtype=np.uint8)  # writes rounds x num_procs bytes, no more
    assert L.dash_seed_schedule(87, 4, 4, guard.ctypes.data) == dash.OK
    assert (guard[16:] == 0xEE).all() and np.array_equal(guard[:16].reshape(4, 4), dash.seed_schedule(87, 4, 4))
