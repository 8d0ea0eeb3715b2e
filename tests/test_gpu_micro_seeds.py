"""Seeded micro-step schedules per system (dash_set_micro_seeds), on the GPU.

Every run is checked as an execution of the oracle's STRICT micro-step model: the acts the engine
recorded (read_micro_acts) and its event log give a witness that oc.replay_steps must accept step
by step and that must end terminal in the engine's final state. That the pick is the specified one
(dash_micro_pick over the enabled set) is checked against the CPU twin walk (tests/micro_twin.py)
on small systems, round for round.
"""
import ctypes
import functools
import json
import shutil
import subprocess

import numpy as np
import pytest

import micro_twin
import oracle_ctypes as oc
from micro_twin import ORC_ERR_OVERFLOW
from oracle_ctypes import GOLDEN
from test_gpu_parity import random_batch, state_arrays

pytestmark = pytest.mark.gpu
RECORDS = json.loads((GOLDEN.parent / "schedules" / "micro_seeds.json").read_text())["records"]
# the issue's weight vectors and the accepted run each is meant to reach
TABLE = {"test_4": [((4, 0, 31, 1), "run_3"), ((4, 1, 31, 31), "run_4"), ((4, 31, 31, 31), "run_2"), (None, "run_1")],
         "test_3": [((1, 1, 0, 1), "run_2"), (None, "run_1")]}


def pack_rows(dash, w):
    return np.array([dash.pack_weights(row) for row in w], dtype=np.uint64)


def random_weights(rng, nsys, N, zero_frac=0.25):
    """Weights 0..31 with zeros present; system 1 is all zeros (every round takes the flat rule)."""
    w = rng.integers(0, 32, size=(nsys, N))
    w[rng.random((nsys, N)) < zero_frac] = 0
    w[1 % nsys] = 0
    return w


def replay(tr, lens, steps, N, CS):
    """oc.replay_steps of a witness with the handled-message counts: (outcome, terminal), or None
    when a queue of the model overflowed (it holds 40 messages, the engine's 256: there the model,
    not the reference, drops a message, and a later step of the engine's run may find it missing)."""
    try:
        out, term = oc.replay_steps(tr, lens, steps, num_procs=N, cache_size=CS, count_msgs=True)
    except ValueError as e:
        words = str(e).split()
        if words[:2] != ["witness", "step"]:
            raise
        pre, _ = oc.replay_steps(tr, lens, steps[:int(words[2])], num_procs=N, cache_size=CS)
        if pre.errors & ORC_ERR_OVERFLOW:
            return None
        raise
    return None if out.errors & ORC_ERR_OVERFLOW else (out, term)


def check_legal(dash, eng, s, tr, lens, N, CS, dig, rnd, err):
    """System s of a finished micro-seeds run against the oracle; False = skipped (model overflow)."""
    acts, ev = eng.read_micro_acts(s), eng.read_events(s)
    steps = micro_twin.steps_of(acts, ev)
    assert int(rnd[s]) == len(steps) == len(acts), s
    assert sum(e.kind == dash.EV_INSTR for e in ev) == int(lens.sum()), s  # every instruction issued
    got = replay(tr, lens, steps, N, CS)
    if got is None:
        return False
    out, term = got
    hist = eng.read_hist(s).tolist()
    assert term, s
    assert hist == list(out.hist), s
    assert out.digest == oc.outcome_key(int(dig[s]), hist), s
    assert state_arrays(eng.read_state(s), N, CS) == state_arrays(out.node, N, CS), s
    assert int(err[s]) == out.errors, s
    return True


# ---------------------------------------------------------------- 1. legality per system

# a wave split 8 / 16 / 32 ways, the generic (non-power-of-two CACHE_SIZE) kernel, and a
# non-power-of-two node count
SHAPES = [(8, 4), (4, 4), (8, 2), (3, 1), (8, 3), (2, 16)]
MAXLEN = 24
LOG_ROUNDS = 8192  # above the default round cap, 1024 + 256 * 24 = 7168: no run outgrows the log


@functools.lru_cache(maxsize=None)
def shape_batch(N, CS):
    rng = np.random.default_rng(5100 + 16 * N + CS)
    packed, lens = random_batch(rng, 64, N, MAXLEN, hot_frac=0.3)
    lens[5] = 0          # an empty system
    lens[17, 0] = 0      # empty rows
    lens[33, N - 1] = 0
    packed = np.where(np.arange(MAXLEN)[None, None, :] < lens[:, :, None], packed, 0).astype(np.uint16)
    seeds = rng.integers(0, 1 << 64, size=64, dtype=np.uint64)
    return packed, lens, seeds, random_weights(rng, 64, N)


@pytest.mark.parametrize("N,CS", SHAPES)
def test_every_run_is_a_legal_execution(dash, N, CS):
    packed, lens, seeds, w = shape_batch(N, CS)
    assert (w == 0).any() and (w > 0).any()
    with dash.Engine(64, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True, trace_events=LOG_ROUNDS,
                     schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_micro_seeds(seeds, weights_per_system=pack_rows(dash, w))
        stats = eng.run()
        dig, rnd, err = eng.read_results()
        assert stats["tier_systems"] == [0, 0, 64] and stats["instructions"] == int(lens.sum())
        assert stats["rounds_total"] == int(rnd.sum()) and not stats["err_bits"] & dash.ERR_SCHEDULE
        assert int(rnd[5]) == 0
        checked = sum(check_legal(dash, eng, s, packed[s], lens[s], N, CS, dig, rnd, err) for s in range(64))
    print(f"N={N} CS={CS}: {checked} of 64 systems replayed, {64 - checked} skipped (model queue overflow)")
    assert checked >= 48, f"{64 - checked} of 64 systems overflowed the model's 40-entry queues"


# ---------------------------------------------------------------- 2. the pick is the specified one

@functools.lru_cache(maxsize=None)
def twin_case(N, CS, nsys, maxlen):
    """A small batch with its twin walks (computed once, shared by the tests below)."""
    rng = np.random.default_rng(5300 + N)
    packed, lens = random_batch(rng, nsys, N, maxlen, hot_frac=0.3)
    seeds = rng.integers(0, 1 << 64, size=nsys, dtype=np.uint64)
    w = random_weights(rng, nsys, N)
    walks = [micro_twin.walk(packed[s], lens[s], int(seeds[s]), w[s].tolist(), N, CS, count_msgs=True)
             for s in range(nsys)]
    return packed, lens, seeds, w, walks


TWIN_CASES = [(4, 4, 8, 8), (8, 2, 4, 6)]


def run_twin_case(dash, N, CS, nsys, maxlen):
    packed, lens, seeds, w, walks = twin_case(N, CS, nsys, maxlen)
    eng = dash.Engine(nsys, num_procs=N, cache_size=CS, max_instr=maxlen, keep_state=True, trace_events=4096,
                      schedule_seed=1)
    eng.load_traces(packed, lens)
    eng.set_micro_seeds(seeds, weights_per_system=pack_rows(dash, w))
    eng.run()
    return eng, walks


@pytest.mark.parametrize("N,CS,nsys,maxlen", TWIN_CASES)
def test_acts_are_the_twin_walk(dash, N, CS, nsys, maxlen):
    eng, walks = run_twin_case(dash, N, CS, nsys, maxlen)
    with eng:
        dig, rnd, err = eng.read_results()
        for s, (steps, out, term) in enumerate(walks):
            assert term and not out.errors & ORC_ERR_OVERFLOW, s  # small systems: the model holds them
            acts = eng.read_micro_acts(s)
            assert np.array_equal(acts, micro_twin.acts_of(steps, N)), s
            assert micro_twin.steps_of(acts, eng.read_events(s)) == steps, s
            assert out.digest == oc.outcome_key(int(dig[s]), eng.read_hist(s).tolist()), s
            assert (int(rnd[s]), int(err[s])) == (len(steps), out.errors), s
    assert len({len(st) for st, _, _ in walks}) > 1


# ---------------------------------------------------------------- 3. replay through the table path

def test_acts_replay_through_set_micro_schedule(dash):
    N, CS, nsys, maxlen = TWIN_CASES[0]
    packed, lens = twin_case(N, CS, nsys, maxlen)[:2]
    eng, _ = run_twin_case(dash, N, CS, nsys, maxlen)
    with eng:
        dig = eng.read_results()[0]
        want = [(int(dig[s]), eng.read_micro_acts(s), [(e.round, e.node, e.kind, e.word) for e in eng.read_events(s)])
                for s in range(4)]
    for s, (d, acts, events) in enumerate(want):
        assert len(acts) > 0
        with dash.Engine(1, num_procs=N, cache_size=CS, max_instr=maxlen, trace_events=4096, schedule_seed=1) as one:
            one.set_micro_schedule(acts)
            one.load_traces(packed[s:s + 1], lens[s:s + 1])
            st = one.run()
            assert int(one.read_results()[0][0]) == d and st["err_bits"] == 0, s
            assert [(e.round, e.node, e.kind, e.word) for e in one.read_events(0)] == events, s


def test_replay_of_a_run_that_holds_a_notice_to_a_missing_node(dash):
    """test_4 under weights (4, 1, 31, 31), seed 17: node 0's line 0, still at its initial address
    0xFF, is made EXCLUSIVE by an EVICT_SHARED at its home (no address check) and evicted by the next
    fill; its notice goes to node 15 (DASH_ERR_OOB). The seeded run holds the notice and drops it at
    its delivery, mid-run; the table-driven replay drops it at the step and that delivery act finds
    an empty outbox: the same digest, error bits, event log and, the delivery not being the last
    act, rounds."""
    def results(eng):
        d, r, e = eng.read_results()
        return int(d[0]), int(r[0]), int(e[0]), [(x.round, x.node, x.kind, x.word) for x in eng.read_events(0)]

    eng, tr, lens = explorer(dash, "test_4", 1, trace_events=1024)
    with eng:
        eng.set_micro_seeds([17], (4, 1, 31, 31))
        eng.run()
        want, acts = results(eng), eng.read_micro_acts(0)
        assert want[2] == dash.ERR_OOB and want[1] == len(acts)
        steps = micro_twin.steps_of(acts, eng.read_events(0))
        out, term = oc.replay_steps(tr, lens, steps)  # the oracle holds the notice too
        assert term and (out.digest, out.errors) == (want[0], dash.ERR_OOB)
        assert acts[-1].tolist().count(dash.MICRO_SEND) == 0  # the last act is a step
        eng.set_micro_schedule(acts)
        eng.run()
        assert results(eng) == want


# ---------------------------------------------------------------- 4. determinism and independence

def test_deterministic_and_read_by_system_id(dash):
    N, CS = 4, 4
    rng = np.random.default_rng(5400)
    packed, lens = random_batch(rng, 96, N, 16, hot_frac=0.3)
    seeds = rng.integers(0, 1 << 64, size=96, dtype=np.uint64)
    w = pack_rows(dash, random_weights(rng, 96, N))

    def run(order):
        with dash.Engine(96, num_procs=N, cache_size=CS, max_instr=16, schedule_seed=1) as eng:
            eng.load_traces(packed[order], lens[order])
            eng.set_micro_seeds(seeds[order], weights_per_system=w[order])
            out = []
            for _ in range(2):
                eng.run()
                out.append([a.tolist() for a in eng.read_results()])
            assert out[0] == out[1]
            return [np.array(a) for a in out[0]]

    base = run(np.arange(96))
    perm = np.random.default_rng(1).permutation(96)
    moved = run(perm)  # system perm[k] sits in slot k, on another lane of another wave
    for a, b in zip(base, moved):
        assert np.array_equal(a[perm], b)
    assert len(set(base[0].tolist())) > 48 and len(set(base[1].tolist())) > 8
    # the seed matters, and so do the weights: not one schedule applied 96 times
    with dash.Engine(96, num_procs=N, cache_size=CS, max_instr=16, schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_micro_seeds(seeds + np.uint64(1), weights_per_system=w)
        eng.run()
        assert (eng.read_results()[0] != base[0]).sum() > 8


# ---------------------------------------------------------------- 5. exploration

EXPLORE_SEEDS, EXPLORE_SYSTEMS = 250, 64


def explorer(dash, test, nsys, **kw):
    tr, lens = oc.load_test_dir(GOLDEN / test)
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, **kw)
    packed = np.zeros((nsys, 4, tr.shape[1]), np.uint16)
    ln = np.zeros((nsys, 4), np.uint32)
    packed[0], ln[0] = tr, lens  # the other systems are empty until the broadcast
    eng.load_traces(packed, ln)
    return eng, tr, lens


def run_digest(test, run):
    return oc.dumps_digest([(GOLDEN / test / run / f"core_{n}_output.txt").read_text() for n in range(4)])


@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_explore_micro(dash, test):
    eng, tr, lens = explorer(dash, test, EXPLORE_SYSTEMS, keep_state=True, trace_events=1024)
    one, _, _ = explorer(dash, test, 1, trace_events=1024)
    with eng, one:
        for weights, run in TABLE[test]:
            got = eng.explore_micro(0, 1, EXPLORE_SEEDS, weights)  # 4 passes, the last one padded
            assert eng.explore_total == len(got) >= 1
            assert sum(o["count"] for o in got) == EXPLORE_SEEDS
            assert [o["seed"] for o in got] == sorted(o["seed"] for o in got) and got[0]["seed"] == 1
            assert len({(o["digest"], o["errors"]) for o in got}) == len(got)
            assert run_digest(test, run) in [o["digest"] for o in got], (weights, run)
            # the handle holds the last pass: slot k ran seed 1 + 192 + k % 58 (6 slots pad)
            dig = eng.read_results()[0]
            assert dig[58:].tolist() == dig[:6].tolist()
            for o in got:  # the witness seed alone reaches the outcome, by a legal execution
                one.set_micro_seeds([o["seed"]], weights)
                one.run()
                d, r, e = one.read_results()
                assert (int(d[0]), int(r[0]), int(e[0])) == (o["digest"], o["rounds"], o["errors"]), o
                steps = micro_twin.steps_of(one.read_micro_acts(0), one.read_events(0))
                out, term = oc.replay_steps(tr, lens, steps)
                assert term and (out.digest, out.errors) == (o["digest"], o["errors"]), o
        assert eng.explore_micro(0, 1, 0) == [] and eng.explore_total == 0
        uni = eng.explore_micro(0, 1, EXPLORE_SEEDS)
        assert eng.explore_micro(0, 1, EXPLORE_SEEDS, cap=1) == uni[:1] and eng.explore_total == len(uni)


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: f"{r['test']}-{r['run']}")
def test_committed_witness_dumps_the_accepted_run(dash, rec, tmp_path):
    eng, _, _ = explorer(dash, rec["test"], 1, keep_state=True)
    with eng:
        eng.set_micro_seeds([rec["seed"]], rec["weights"])
        eng.run()
        d, r, e = eng.read_results()
        assert (f"{int(d[0]):016x}", int(r[0]), int(e[0])) == (rec["digest"], rec["rounds"], 0)
        eng.dump_system(0, tmp_path)
    for n in range(4):
        assert (tmp_path / f"core_{n}_output.txt").read_bytes() == \
            (GOLDEN / rec["test"] / rec["run"] / f"core_{n}_output.txt").read_bytes()


# ---------------------------------------------------------------- 6. boundary

def test_boundary(dash):
    N, CS, n = 4, 4, 12
    rng = np.random.default_rng(5600)
    packed, lens = random_batch(rng, n, N, 12, hot_frac=0.3)
    seeds = rng.integers(1, 1 << 64, size=n, dtype=np.uint64)
    L = dash.lib()
    rounds = ctypes.c_uint32(77)

    def code(fn, *a):
        with pytest.raises(dash.DashError) as e:
            fn(*a)
        return e.value.code

    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=12) as eng:  # a lockstep handle
        assert code(eng.set_micro_seeds, seeds) == dash.ESTATE
        assert code(eng.set_micro_seeds, None) == dash.ESTATE
        eng.load_traces(packed, lens)
        assert code(eng.explore_micro, 0, 1, 4) == dash.ESTATE
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=12, schedule_seed=87) as eng:  # no event log
        eng.load_traces(packed, lens)
        assert code(eng.set_micro_seeds, seeds[:-1]) == dash.EINVAL
        assert code(eng.set_micro_seeds, np.append(seeds, 5)) == dash.EINVAL
        assert L.dash_set_micro_seeds(eng.h, None, None, n) == dash.EINVAL
        assert code(eng.set_micro_seeds, seeds, [1, 2, 32, 1]) == dash.EINVAL
        bad = np.full(n, dash.MICRO_UNIFORM, dtype=np.uint64)
        bad[n - 1] |= np.uint64(0x20 << 56)  # a node past num_procs counts too
        assert code(eng.set_micro_seeds, seeds, None, bad) == dash.EINVAL
        with pytest.raises(ValueError):
            eng.set_micro_seeds(seeds, [1, 1, 1, 1], bad)
        assert code(eng.explore_micro, 0, 1, 4, [1, 1, 1, 40]) == dash.EINVAL
        assert code(eng.read_micro_acts, 0) == dash.ESTATE  # no micro seeds
        eng.set_micro_seeds(seeds)
        assert code(eng.read_micro_acts, 0) == dash.ESTATE  # no log
        eng.run()
        assert code(eng.read_micro_acts, 0) == dash.ESTATE
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=12, schedule_seed=87, trace_events=8) as eng:
        eng.load_traces(packed, lens)
        eng.set_micro_seeds(seeds)
        assert code(eng.read_micro_acts, 0) == dash.ESTATE  # before a run
        eng.run()
        assert int(eng.read_results()[1][0]) > 8
        assert L.dash_read_micro_acts(eng.h, 0, None, 0, rounds) == dash.ETRUNC  # longer than the log
        assert rounds.value == int(eng.read_results()[1][0])
        with pytest.raises(dash.DashError) as e:
            eng.read_events(0)
        assert e.value.code == dash.ETRUNC
        assert L.dash_read_micro_acts(eng.h, n, None, 0, rounds) == dash.EINVAL and rounds.value == 0
    by_handle = [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS, arb_seed=87).digest for s in range(n)]
    by_seeds = [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS, arb_seed=int(seeds[s])).digest
                for s in range(n)]
    sched = dash.seed_schedule(413, N, 64)
    by_sched = [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS, sched=sched).digest for s in range(n)]
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=12, schedule_seed=87, trace_events=2048,
                     flags=dash.TEST_SHORT_ARB) as eng:
        # a handle whose round table is too short for dash_set_micro_schedule still takes micro seeds
        acts = np.full((4, N), dash.SIT_OUT, dtype=np.uint8)
        assert code(eng.set_micro_schedule, acts) == dash.EINVAL
        eng.load_traces(packed, lens)
        eng.set_micro_seeds(seeds)
        eng.run()
        assert len(eng.read_micro_acts(0)) == int(eng.read_results()[1][0])

    def digests(eng):
        eng.run()
        return eng.read_results()[0].tolist()

    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=12, schedule_seed=87, trace_events=2048) as eng:
        eng.load_traces(packed, lens)
        assert digests(eng) == by_handle
        eng.set_micro_seeds(seeds)
        by_micro = digests(eng)
        assert by_micro not in (by_handle, by_seeds, by_sched)
        # a delivery's marker never comes back as an event: one event per pop and per issue
        acts, ev = eng.read_micro_acts(0), eng.read_events(0)
        assert (acts == dash.MICRO_SEND).sum() > 0
        assert len(ev) == (acts == dash.MICRO_STEP).sum()
        assert all(e.kind in (dash.EV_MSG, dash.EV_INSTR) and e.word >> 27 == 0 for e in ev)
        assert sum(e.kind == dash.EV_INSTR for e in ev) == int(lens[0].sum())
        assert L.dash_read_micro_acts(eng.h, 0, None, 0, rounds) == dash.EINVAL and rounds.value == len(acts)
        small = np.zeros((len(acts) - 1, N), np.uint8)
        assert L.dash_read_micro_acts(eng.h, 0, small.ctypes.data, len(small), rounds) == dash.EINVAL
        assert rounds.value == len(acts) and not small.any()
        # the last call wins, in the four orders
        eng.set_schedule(sched)
        eng.set_micro_seeds(seeds)
        assert digests(eng) == by_micro
        eng.set_schedule(sched)
        assert digests(eng) == by_sched
        eng.set_micro_seeds(seeds)
        eng.set_system_seeds(seeds)
        assert digests(eng) == by_seeds
        assert code(eng.read_micro_acts, 0) == dash.ESTATE
        eng.set_micro_seeds(seeds)
        assert digests(eng) == by_micro
        one = eng.read_micro_acts(3)
        eng.set_micro_schedule(one)          # every system follows system 3's acts
        by_table = digests(eng)
        assert by_table[3] == by_micro[3] and by_table != by_micro
        eng.set_micro_seeds(seeds)           # replaces the micro-step table
        assert digests(eng) == by_micro
        eng.set_micro_schedule(one)          # and is replaced by one
        assert digests(eng) == by_table
        for arg in (seeds, None):            # the refusals on a micro-step handle stay
            assert code(eng.set_system_seeds, arg) == dash.ESTATE
        assert code(eng.explore, 0, 0, n) == dash.ESTATE
        # NULL, NULL, 0: back to the handle's own seed and table, whatever was set
        eng.set_micro_seeds(None)
        assert digests(eng) == by_handle
        eng.set_micro_seeds(seeds)
        eng.set_micro_seeds(None)
        assert digests(eng) == by_handle
        eng.set_system_seeds(seeds)
        eng.set_micro_seeds(None)
        assert digests(eng) == by_handle
        eng.set_micro_seeds(seeds, None)     # weights NULL is the uniform vector
        assert digests(eng) == by_micro
        eng.set_micro_seeds(seeds, [1, 1, 1, 1])
        assert digests(eng) == by_micro
        # dash_set_system_seeds takes a handle on micro seeds, whether or not a micro-step table was
        # set before them; its NULL rebuilds the handle seed's table, which that table overwrote
        eng.set_micro_schedule(one)
        eng.set_micro_seeds(seeds)
        eng.set_system_seeds(None)
        assert digests(eng) == by_handle
        eng.set_micro_schedule(one)
        eng.set_micro_seeds(seeds)
        eng.set_system_seeds(seeds)
        assert digests(eng) == by_seeds
        eng.set_system_seeds(None)
        assert digests(eng) == by_handle


# ---------------------------------------------------------------- 7. CLI

def test_cli(dash, tmp_path):
    exe = dash.PKG / "cache_simulator"
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / "test_4", tmp_path / "tests" / "test_4")

    def cli(*args):
        p = subprocess.run([str(exe), "test_4", *map(str, args)], cwd=tmp_path, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()

    lines = cli("--explore-micro", 250, "--weights", "4,0,31,1")
    assert lines and all(len(ln.split()) == 5 for ln in lines)
    assert f"{run_digest('test_4', 'run_3'):016x}" in [ln.split()[0] for ln in lines]
    assert sum(int(ln.split()[1]) for ln in lines) == 250
    assert not list(tmp_path.glob("core_*_output.txt"))
    (rec,) = [r for r in RECORDS if (r["test"], r["run"]) == ("test_4", "run_3")]
    run_3 = [(GOLDEN / "test_4" / "run_3" / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    micro = tmp_path / "micro.txt"
    for d, args in (("a", ["--micro-seed", rec["seed"], "--weights", ",".join(map(str, rec["weights"])),
                           "--write-micro", micro]),
                    ("b", ["--micro", micro])):
        (tmp_path / d).mkdir()
        cli("-o", tmp_path / d, *args)
        assert [(tmp_path / d / f"core_{n}_output.txt").read_bytes() for n in range(4)] == run_3, d
    toks = micro.read_text().split()
    assert len(toks) == rec["rounds"] and {t[0] for t in toks} == {"P", "I", "D"}
    tr, lens = oc.load_test_dir(GOLDEN / "test_4")
    steps, _, _ = micro_twin.walk(tr, lens, rec["seed"], rec["weights"], 4, 4)
    assert toks == [("D" if s >> 8 == micro_twin.XK_SEND else "PI"[s >> 8]) + str(s & 15) for s in steps]
