"""Per-system schedule seeds, the trace broadcast and outcome exploration, on the GPU.

dash_set_system_seeds gives every system of a batch a seeded legal schedule of its own, hashed in
the kernel; every expectation is the CPU oracle's run of that system under that seed
(run_system(arb_seed=seeds[k])), the same twin the handle-wide seed is checked against. The
exploration results are compared as whole lists with what the oracle gives for the same seeds.
"""
import functools
import json
import shutil
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
from oracle_ctypes import GOLDEN, run_system
from test_gpu_parity import check_stats, random_batch, state_arrays

pytestmark = pytest.mark.gpu
SCHED_DIR = GOLDEN.parent / "schedules"


def cap_of(max_instr):
    return 1024 + 256 * max_instr


def oracle_per_system(packed, lens, N, CS, seeds):
    return [run_system(packed[s], lens[s], num_procs=N, cache_size=CS, ring_depth=256,
                       max_rounds=cap_of(packed.shape[2]), arb_seed=int(seeds[s])) for s in range(len(packed))]


def check_against(dash, eng, stats, results, N, CS):
    """State, histogram, rounds, error bits, digest of every system, and the run's statistics."""
    dig, rnd, err = eng.read_results()
    for s, res in enumerate(results):
        assert int(dig[s]) == res.digest, f"system {s} digest"
        assert int(rnd[s]) == res.rounds, f"system {s} rounds"
        assert int(err[s]) == res.errors, f"system {s} errors"
        assert eng.read_hist(s).tolist() == list(res.hist), f"system {s} hist"
        assert state_arrays(eng.read_state(s), N, CS) == state_arrays(res.node, N, CS), f"system {s} state"
    check_stats(stats, results)


# ---------------------------------------------------------------- 1. parity per system

# a wave split 8 / 16 / 32 ways, the generic (non-power-of-two CACHE_SIZE) kernel, and a
# non-power-of-two node count
SHAPES = [(8, 4), (4, 4), (8, 2), (3, 1), (8, 3), (2, 16)]


@pytest.mark.parametrize("N,CS", SHAPES)
def test_parity_per_system(dash, N, CS):
    rng = np.random.default_rng(3100 + 16 * N + CS)
    packed, lens = random_batch(rng, 96, N, 48, hot_frac=0.3)
    seeds = rng.integers(1, 1 << 64, size=96, dtype=np.uint64)
    seeds[0] = seeds[50] = 0  # the batch's own lockstep baseline
    results = oracle_per_system(packed, lens, N, CS, seeds)
    with dash.Engine(96, num_procs=N, cache_size=CS, max_instr=48, keep_state=True, schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_system_seeds(seeds)
        stats = eng.run()
        check_against(dash, eng, stats, results, N, CS)
        seeded = eng.read_results()
    # the schedules differ: the batch is not one schedule applied 96 times
    lock = oracle_per_system(packed, lens, N, CS, np.zeros(96, np.uint64))
    assert sum(a.rounds != b.rounds or a.digest != b.digest for a, b in zip(results, lock)) > 48
    # seed 0 is the lockstep engine (a handle created with schedule_seed = 0) on the same traces
    with dash.Engine(96, num_procs=N, cache_size=CS, max_instr=48) as eng:
        eng.load_traces(packed, lens)
        eng.run()
        dig, rnd, err = eng.read_results()
    for k in (0, 50):
        assert (int(dig[k]), int(rnd[k]), int(err[k])) == tuple(int(x[k]) for x in seeded)


# ---------------------------------------------------------------- 2. one seed everywhere

@pytest.mark.parametrize("S", [87, 0xABCDEF])
def test_same_seed_everywhere_is_the_handle_seed(dash, S):
    """The hashing path against the table path: identical results, statistics included."""
    rng = np.random.default_rng(3300)
    packed, lens = random_batch(rng, 96, 8, 48, hot_frac=0.3)
    out = []
    for per_system in (False, True):
        with dash.Engine(96, num_procs=8, cache_size=4, max_instr=48, keep_state=True,
                         schedule_seed=S if not per_system else 1) as eng:
            eng.load_traces(packed, lens)
            if per_system:
                eng.set_system_seeds([S] * 96)
            stats = eng.run()
            stats.pop("kernel_ms")
            out.append((stats, [a.tolist() for a in eng.read_results()],
                        [eng.read_hist(s).tolist() for s in range(96)],
                        [state_arrays(eng.read_state(s), 8, 4) for s in range(96)]))
    assert out[0] == out[1]
    assert out[0][0]["rounds_total"] > 0


# ---------------------------------------------------------------- 3. across a tier hand-off

@functools.lru_cache(maxsize=None)
def handoff_case(CS):
    """Hot lines at N = 8 (as tests/test_gpu_tiers.py builds them), with a seed per system."""
    rng = np.random.default_rng(4201)
    packed, lens = random_batch(rng, 96, 8, 48, block_span=4, hot_frac=0.9, fixed_len=True)
    seeds = rng.integers(1, 1 << 63, size=96, dtype=np.uint64)
    return packed, lens, seeds, oracle_per_system(packed, lens, 8, CS, seeds)


@pytest.mark.parametrize("CS", [1, 2])
def test_seeds_follow_systems_across_a_hand_off(dash, CS):
    """A system re-run at a deeper queue depth is reached through the hand-off list, where its
    position is not its id: it must still follow its own seed."""
    packed, lens, seeds, results = handoff_case(CS)
    depth = np.array([r.max_depth for r in results])
    assert (depth > 16).any() and (depth <= 16).any()  # the inputs put systems on both sides
    assert len(set(seeds.tolist())) == 96
    for flags in (0, dash.TIER_FROM_256):
        with dash.Engine(96, num_procs=8, cache_size=CS, max_instr=48, keep_state=True, flags=flags,
                         schedule_seed=1) as eng:
            eng.load_traces(packed, lens)
            eng.set_system_seeds(seeds)
            stats = eng.run()
            if flags == 0:
                assert stats["tier_systems"][1] + stats["tier_systems"][2] > 0
                assert stats["tier_systems"][1] == int((depth > 16).sum())
            check_against(dash, eng, stats, results, 8, CS)
            if flags == 0:  # again, now with the overflow hint of the first run (the side stream)
                stats = eng.run()
                check_against(dash, eng, stats, results, 8, CS)


# ---------------------------------------------------------------- 4. event log

def test_event_log_per_system(dash):
    rng = np.random.default_rng(3500)
    packed, lens = random_batch(rng, 8, 4, 40, hot_frac=0.3)
    seeds = rng.integers(1, 1 << 64, size=8, dtype=np.uint64)
    seeds[3] = 0
    with dash.Engine(8, num_procs=4, cache_size=4, max_instr=40, trace_events=256, schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_system_seeds(seeds)
        eng.run()
        for k in range(8):
            res, log = run_system(packed[k], lens[k], num_procs=4, cache_size=4, log=True, log_msgs=True,
                                  max_rounds=cap_of(40), arb_seed=int(seeds[k]))
            assert res.rounds <= 256 and log
            assert dash.format_events(eng.read_events(k)) == log, k


# ---------------------------------------------------------------- 5. selectors

def test_selectors(dash):
    rng = np.random.default_rng(3600)
    N, CS, n = 4, 4, 24
    packed, lens = random_batch(rng, n, N, 40, hot_frac=0.3)
    seeds = rng.integers(1, 1 << 64, size=n, dtype=np.uint64)
    sched = dash.seed_schedule(413, N, 64)

    def digests(eng):
        eng.run()
        return eng.read_results()[0].tolist()

    by_seeds = [r.digest for r in oracle_per_system(packed, lens, N, CS, seeds)]
    by_sched = [run_system(packed[s], lens[s], num_procs=N, cache_size=CS, sched=sched).digest for s in range(n)]
    by_handle = [r.digest for r in oracle_per_system(packed, lens, N, CS, [87] * n)]
    assert by_seeds != by_sched and by_seeds != by_handle and by_sched != by_handle
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=40, schedule_seed=87) as eng:
        eng.load_traces(packed, lens)
        assert digests(eng) == by_handle
        eng.set_schedule(sched)
        eng.set_system_seeds(seeds)  # the last call wins
        assert digests(eng) == by_seeds
        eng.set_schedule(sched)      # and the reverse
        assert digests(eng) == by_sched
        eng.set_system_seeds(seeds)
        assert digests(eng) == by_seeds
        eng.set_system_seeds(None)   # back to the handle's own seed, its table rebuilt
        assert digests(eng) == by_handle
        eng.set_system_seeds(seeds)
        eng.set_system_seeds(None)
        assert digests(eng) == by_handle
        for bad in (seeds[:-1], np.append(seeds, 5)):
            with pytest.raises(dash.DashError) as e:
                eng.set_system_seeds(bad)
            assert e.value.code == dash.EINVAL
        assert dash.lib().dash_set_system_seeds(eng.h, None, n) == dash.EINVAL
        assert digests(eng) == by_handle  # a refused call changes nothing
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=40) as eng:  # a lockstep handle
        with pytest.raises(dash.DashError) as e:
            eng.set_system_seeds(seeds)
        assert e.value.code == dash.ESTATE
        eng.load_traces(packed, lens)
        with pytest.raises(dash.DashError) as e:
            eng.explore(0, 0, n)
        assert e.value.code == dash.ESTATE
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=40, schedule_seed=87) as eng:
        acts = np.full((4, N), dash.SIT_OUT, dtype=np.uint8)
        acts[0, 0] = dash.MICRO_STEP
        eng.set_micro_schedule(acts)
        for arg in (seeds, None):
            with pytest.raises(dash.DashError) as e:
                eng.set_system_seeds(arg)
            assert e.value.code == dash.ESTATE


# ---------------------------------------------------------------- 6. broadcast

def test_broadcast(dash):
    rng = np.random.default_rng(3700)
    for N in (4, 3):  # the strided layout, and the padded one of a non-power-of-two node count
        packed, lens = random_batch(rng, 64, N, 33, hot_frac=0.3)
        with dash.Engine(64, num_procs=N, cache_size=4, max_instr=33) as eng:
            with pytest.raises(dash.DashError) as e:
                eng.broadcast_system(0)  # nothing loaded yet
            assert e.value.code == dash.ESTATE
            eng.load_traces(packed, lens)
            before = eng.read_traces()
            with pytest.raises(dash.DashError) as e:
                eng.broadcast_system(64)
            assert e.value.code == dash.EINVAL
            eng.broadcast_system(5)
            rows, ln = eng.read_traces()
            assert np.array_equal(ln, np.tile(before[1][5], (64, 1)))
            assert np.array_equal(rows, np.tile(before[0][5], (64, 1, 1)))
            assert ln[5].sum() > 0
            eng.run()
            dig, rnd, err = eng.read_results()
            want = run_system(packed[5], lens[5], num_procs=N, cache_size=4)
            assert dig.tolist() == [want.digest] * 64 and rnd.tolist() == [want.rounds] * 64


# ---------------------------------------------------------------- 7. exploration of test_4

EXPLORE_SEEDS = 4096


@functools.lru_cache(maxsize=None)
def golden_test_4():
    return oc.load_test_dir(GOLDEN / "test_4")


def oracle_outcomes(first, count):
    """dash_explore's contract from the oracle: distinct (digest, errors), their counts, the lowest
    seed reaching each and that run's rounds, ordered by that seed."""
    tr, lens = golden_test_4()
    found = {}
    for s in range(first, first + count):
        r = run_system(tr, lens, arb_seed=s)
        o = found.setdefault((r.digest, r.errors), dict(digest=r.digest, count=0, seed=s, rounds=r.rounds,
                                                        errors=r.errors))
        o["count"] += 1
    return sorted(found.values(), key=lambda o: o["seed"])


@functools.lru_cache(maxsize=None)
def expected_4096():
    return oracle_outcomes(0, EXPLORE_SEEDS)


def explorer(dash, nsys, **kw):
    tr, lens = golden_test_4()
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, **kw)
    packed = np.zeros((nsys, 4, tr.shape[1]), np.uint16)
    ln = np.zeros((nsys, 4), np.uint32)
    packed[0], ln[0] = tr, lens  # the other systems are empty until the broadcast
    eng.load_traces(packed, ln)
    return eng


def test_explore_test_4(dash, tmp_path):
    exp = expected_4096()
    assert len(exp) == 4 and all(o["errors"] == 0 for o in exp)
    assert sum(o["count"] for o in exp) == EXPLORE_SEEDS and exp[0]["seed"] == 0
    for run, o in (("run_1", exp[0]), ("run_2", exp[1])):
        rec = json.loads((SCHED_DIR / f"test_4_{run}.json").read_text())
        assert o["digest"] == int(rec["digest"], 16)
    assert exp[1]["seed"] == 87  # the CLI's documented example
    with explorer(dash, EXPLORE_SEEDS, keep_state=True) as eng:
        got = eng.explore(0, 0, EXPLORE_SEEDS)
        assert got == exp
        assert eng.explore_total == 4
        # the last pass stays readable: system k ran seed k
        dig = eng.read_results()[0]
        for o in exp:
            assert int(dig[o["seed"]]) == o["digest"]
        eng.dump_system(87, tmp_path)
        for n in range(4):
            assert (tmp_path / f"core_{n}_output.txt").read_bytes() == \
                (GOLDEN / "test_4" / "run_2" / f"core_{n}_output.txt").read_bytes()
        # cap below the total: the first two, and the total
        assert eng.explore(0, 0, EXPLORE_SEEDS, cap=2) == exp[:2]
        assert eng.explore_total == 4
        # a window that starts elsewhere
        assert eng.explore(0, 80, 16) == oracle_outcomes(80, 16)
    with explorer(dash, 1000) as eng:  # 5 passes, the last one padded with repeats
        assert eng.explore(0, 0, EXPLORE_SEEDS) == exp
    with explorer(dash, 64) as eng:
        packed, ln = eng.read_traces()
        assert ln[1:].sum() == 0
        got = eng.explore(0, 0, 0)  # no seeds: no outcomes, but the broadcast happened
        assert got == [] and eng.explore_total == 0
        assert np.array_equal(eng.read_traces()[1], np.tile(golden_test_4()[1], (64, 1)))


def test_witness_round_trip(dash, tmp_path):
    """A witness seed written out by seed_schedule and pinned with set_schedule reproduces its
    outcome: the bridge from an exploration's seed to a schedule file."""
    tr, lens = golden_test_4()
    for o in expected_4096():
        sched = dash.seed_schedule(o["seed"], 4, o["rounds"])
        with dash.Engine(1, num_procs=4, cache_size=4, max_instr=32, keep_state=True, schedule_seed=1) as eng:
            eng.set_schedule(sched)
            eng.load_traces(tr[None], lens[None])
            eng.run()
            dig, rnd, err = eng.read_results()
            assert (int(dig[0]), int(rnd[0]), int(err[0])) == (o["digest"], o["rounds"], 0), o["seed"]
            if o["seed"] == 87:
                eng.dump_system(0, tmp_path)
                for n in range(4):
                    assert (tmp_path / f"core_{n}_output.txt").read_bytes() == \
                        (GOLDEN / "test_4" / "run_2" / f"core_{n}_output.txt").read_bytes()


# ---------------------------------------------------------------- 8. CLI

def test_cli_explore_and_write_rounds(dash, tmp_path):
    exe = dash.PKG / "cache_simulator"
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / "test_4", tmp_path / "tests" / "test_4")
    p = subprocess.run([str(exe), "test_4", "--explore", "256"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    exp = oracle_outcomes(0, 256)
    assert [(o["seed"], o["count"]) for o in exp] == [(0, 252), (87, 4)]
    assert p.stdout.splitlines() == [f"{o['digest']:016x} {o['count']} {o['seed']} {o['rounds']} {o['errors']:x}"
                                     for o in exp]
    assert not list(tmp_path.glob("core_*_output.txt"))
    run_2 = [(GOLDEN / "test_4" / "run_2" / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    for d, args in (("a", ["--schedule", "87", "--write-rounds", str(tmp_path / "rounds.txt")]),
                    ("b", ["--rounds", str(tmp_path / "rounds.txt")])):
        (tmp_path / d).mkdir()
        p = subprocess.run([str(exe), "test_4", "-o", str(tmp_path / d)] + args, cwd=tmp_path, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert [(tmp_path / d / f"core_{n}_output.txt").read_bytes() for n in range(4)] == run_2, d
    rows = (tmp_path / "rounds.txt").read_text().splitlines()
    want = dash.seed_schedule(87, 4, exp[1]["rounds"])
    assert rows == ["".join("-" if v == dash.SIT_OUT else str(v) for v in row) for row in want]
