"""dash_check_coherence / dash_read_coherence / dash_check_outcomes (csrc/dash_coherence.hip) on the
GPU: every system's record against tests/coherence_ref.py applied to Engine.read_state of that
system (itself pinned on the oracle by the parity tests), the totals against the records, and the
CLI's --coherence against both. tests/test_coherence_spec.py keeps the inputs' preconditions true on
the CPU (clean and violating systems in every batch, all eight bits among them).

The shapes are the smallest at which the kernel can go wrong: the four 13-system batches of
tests/test_gpu_metrics.py (a partial last wave at every lane-segment width, dead lanes at 3 and 5
nodes, an empty system, a span whose length is no multiple of 16 B at (5, 1)), (8, 16) with the
largest staged span, and (2, 4) with 70 systems: 32 systems per wave and a partial third wave."""
import functools
import shutil
import subprocess

import numpy as np
import pytest

import coherence_ref as cr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN
from test_gpu_metrics import MAXLEN, NSYS, SHAPES, batch
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
EXTRA = {(8, 16): (13, 31), (2, 4): (70, 32)}  # (num_procs, cache_size) -> systems, rng seed


@functools.lru_cache(maxsize=None)
def extra_batch(N, CS):
    nsys, seed = EXTRA[N, CS]
    packed, lens = random_batch(np.random.default_rng(seed), nsys, N, MAXLEN, block_span=4, hot_frac=0.3)
    lens[0] = 0
    return packed, lens


def reference(eng):
    """The reference's records and per-address bits over the states the engine holds."""
    checked = [cr.check(eng.read_state(s), eng.num_procs, eng.cache_size) for s in range(eng.num_systems)]
    return [c[0] for c in checked], [c[1] for c in checked]


def check_all(eng, tot):
    """Every record against the reference, and the totals against the records (bit_addrs: against the
    reference's per-address bits). Returns the records."""
    rec = eng.read_coherence()
    want, per = reference(eng)
    assert rec.dtype.names == cr.FIELDS and rec.shape == (eng.num_systems,)
    for s in range(eng.num_systems):
        assert cr.record(rec[s]) == want[s], s
    errors = eng.read_results()[2]
    bad = rec["bits"] != 0
    assert tot == {"systems": eng.num_systems, "violating_systems": int(bad.sum()),
                   "violating_clean_systems": int((bad & (errors == 0)).sum()), "addrs": int(rec["addrs"].sum()),
                   "bit_systems": [int(((rec["bits"] >> k) & 1).sum()) for k in range(8)],
                   "bit_addrs": [sum((b >> k) & 1 for p in per for b in p) for k in range(8)]}
    return rec


def run_and_check(eng, packed, lens):
    eng.load_traces(packed, lens)
    stats = eng.run()
    tot = eng.check_coherence()
    return stats, tot, check_all(eng, tot)


@pytest.mark.parametrize("N,CS", list(SHAPES) + list(EXTRA))
def test_shapes(dash, N, CS):
    packed, lens = batch(N, CS) if (N, CS) in SHAPES else extra_batch(N, CS)
    nsys = len(lens)
    with dash.Engine(nsys, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True) as eng:
        stats, tot, rec = run_and_check(eng, packed, lens)
        assert cr.record(rec[0]) == {"bits": 0, "addrs": 0, "first_addr": cr.NONE, "first_bits": 0}  # no instruction
        if (N, CS) in SHAPES:  # the CPU test's preconditions, seen here
            assert stats["err_bits"] == 0 and 0 < tot["violating_clean_systems"] == tot["violating_systems"] < nsys
        assert np.array_equal(eng.read_coherence(5, 3), rec[5:8])  # a window of the batch


def test_walk_of_several_trips(dash):
    """100 systems of 8 nodes are 13 waves, four workgroups of work; with DASH_TEST_ONE_GROUP one
    workgroup walks them in four trips (the next span loaded during the scan, the totals carried in
    registers), the last with one live wave, and gives what the device-sized grid gives."""
    N, CS = 8, 4
    packed, lens = random_batch(np.random.default_rng(77), 100, N, MAXLEN, block_span=4, hot_frac=0.3)
    with dash.Engine(100, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True,
                     flags=dash.TEST_ONE_GROUP) as eng:
        _, tot, rec = run_and_check(eng, packed, lens)
        assert 0 < tot["violating_systems"] < 100 and tot["addrs"] > tot["violating_systems"]
    with dash.Engine(100, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True) as eng:
        eng.load_traces(packed, lens)
        eng.run()
        assert eng.check_coherence() == tot and np.array_equal(eng.read_coherence(), rec)


def test_systems_rerun_at_a_deeper_queue_tier(dash):
    """The contention batch of the metrics test: the systems handed to the 32-deep tier are simulated
    again from scratch, and the state (so the records) is the final tier's."""
    N, CS = 8, 2
    packed, lens = random_batch(np.random.default_rng(9000 + 16 * N + CS), 16, N, 100, block_span=4, hot_frac=0.9,
                                fixed_len=True)
    with dash.Engine(16, num_procs=N, cache_size=CS, max_instr=100, keep_state=True) as eng:
        stats, tot, rec = run_and_check(eng, packed, lens)
        assert stats["tier_systems"][0] == 16 and 0 < stats["tier_systems"][1] < 16 and stats["err_bits"] == 0
    # cut mid-flight: every system stops at the round cap, and its state is checked as it is
    with dash.Engine(16, num_procs=N, cache_size=CS, max_instr=100, keep_state=True, max_rounds=8) as eng:
        stats, tot, rec = run_and_check(eng, packed, lens)
        assert (eng.read_results()[2] & dash.ERR_ROUNDCAP).all()
        assert tot["violating_clean_systems"] == 0 and tot["systems"] == 16


def test_stale_records_of_an_earlier_run(dash):
    N, CS = 8, 2
    long_tr, long_lens = batch(N, CS)
    short_lens = np.minimum(long_lens, np.arange(NSYS, dtype=np.uint32)[:, None] % 5)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True) as eng:
        _, long_tot, long_rec = run_and_check(eng, long_tr, long_lens)
        eng.load_traces(long_tr, short_lens)
        eng.run()
        with pytest.raises(dash.DashError) as e:
            eng.read_coherence()
        assert e.value.code == dash.ESTATE  # the records are the long run's
        tot = eng.check_coherence()
        rec = check_all(eng, tot)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True) as fresh:
        _, tot2, rec2 = run_and_check(fresh, long_tr, short_lens)
    assert np.array_equal(rec, rec2) and tot == tot2
    assert not np.array_equal(rec, long_rec)


def test_call_order_and_range_errors(dash):
    N, CS = 4, 4
    packed, lens = batch(N, CS)

    def code(fn, *args):
        with pytest.raises(dash.DashError) as e:
            fn(*args)
        return e.value.code

    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, keep_state=True) as eng:
        eng.load_traces(packed, lens)
        assert code(eng.check_coherence) == dash.ESTATE  # before a run
        eng.run()
        assert code(eng.read_coherence) == dash.ESTATE   # not checked yet
        eng.check_coherence()
        rec = eng.read_coherence()
        assert code(eng.read_coherence, NSYS, 1) == dash.EINVAL
        assert code(eng.read_coherence, 0, NSYS + 1) == dash.EINVAL
        assert code(eng.read_coherence, NSYS - 1, 2) == dash.EINVAL
        assert eng.read_coherence(NSYS, 0).shape == (0,)  # the empty window at the end is inside
        eng.run()
        assert code(eng.read_coherence) == dash.ESTATE   # the second run invalidated the records
        eng.check_coherence()
        assert np.array_equal(eng.read_coherence(), rec)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN) as eng:  # no DASH_KEEP_STATE
        eng.load_traces(packed, lens)
        eng.run()
        assert code(eng.check_coherence) == dash.ESTATE
        assert code(eng.read_coherence) == dash.ESTATE
        assert code(eng.check_outcomes, 0, []) == dash.ESTATE


# ---------------------------------------------------------------- explore

def explorer(dash, test, nsys, **kw):
    tr, lens = oc.load_test_dir(GOLDEN / test)
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True, **kw)
    packed = np.zeros((nsys, 4, tr.shape[1]), np.uint16)
    ln = np.zeros((nsys, 4), np.uint32)
    packed[0], ln[0] = tr, lens  # the other systems are empty until the broadcast
    eng.load_traces(packed, ln)
    return eng, tr, lens


@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_check_outcomes_of_an_explore(dash, test):
    """300 seeded round schedules on a 64-system handle: five passes, and the witness pass padded.
    Every outcome's record is the reference's on the oracle's run of its witness seed."""
    eng, tr, lens = explorer(dash, test, 64)
    with eng:
        outs = eng.explore(0, 0, 300)
        rec = eng.check_outcomes(0, outs)
        assert len(rec) == len(outs) == eng.explore_total and 0 < len(outs) < 64
        for o, r in zip(outs, rec):
            run = oc.run_system(tr, lens, arb_seed=o["seed"])
            assert (run.digest, run.errors) == (o["digest"], o["errors"])
            assert cr.record(r) == cr.check(run.node, 4, 4)[0], o
        if test == "test_3":  # outcomes no DASH_ERR_* bit warns of
            assert any(r["bits"] != 0 and o["errors"] == 0 for o, r in zip(outs, rec))
        else:
            assert not rec["bits"].any() and not rec["addrs"].any()
        # afterwards the handle holds the last pass: the witnesses, padded with repeats
        dig = eng.read_results()[0]
        assert dig[:len(outs)].tolist() == [o["digest"] for o in outs]
        assert dig[len(outs):2 * len(outs)].tolist() == dig[:len(outs)].tolist()[:64 - len(outs)]
        # an outcome the witness does not reproduce
        forged = [dict(o) for o in outs]
        forged[-1]["digest"] ^= 1
        with pytest.raises(dash.DashError) as e:
            eng.check_outcomes(0, forged)
        assert e.value.code == dash.ESTATE and f"outcome {len(outs) - 1}" in str(e.value)


@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_check_outcomes_of_a_micro_explore(dash, test):
    """250 seeded micro-step schedules under uniform weights: every outcome's record is the
    reference's on the state read back after running that witness alone."""
    eng, tr, lens = explorer(dash, test, 64)
    one, _, _ = explorer(dash, test, 1)
    with eng, one:
        outs = eng.explore_micro(0, 0, 250)
        rec = eng.check_outcomes(0, outs, weights=dash.MICRO_UNIFORM)
        assert len(rec) == len(outs) >= 1
        for o, r in zip(outs, rec):
            one.set_micro_seeds([o["seed"]])
            one.run()
            d, _, e = one.read_results()
            assert (int(d[0]), int(e[0])) == (o["digest"], o["errors"]), o
            assert cr.record(r) == cr.check(one.read_state(0), 4, 4)[0], o


# ---------------------------------------------------------------- CLI

def cli_dir(dash, tmp_path, test):
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / test, tmp_path / "tests" / test)
    exe = dash.PKG / "cache_simulator"
    return lambda *args: subprocess.run([str(exe), test, *args], cwd=tmp_path, capture_output=True, text=True,
                                        timeout=120)


def test_cli_coherence_line(dash, tmp_path):
    """`cache_simulator sample --coherence`: the plain run's dumps and lines, byte for byte, and one
    line more."""
    cli = cli_dir(dash, tmp_path, "sample")
    plain = cli()
    assert plain.returncode == 0, plain.stderr
    dumps = [(tmp_path / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    for n in range(4):
        (tmp_path / f"core_{n}_output.txt").unlink()
    p = cli("--coherence")
    assert p.returncode == 0, p.stderr
    assert [(tmp_path / f"core_{n}_output.txt").read_bytes() for n in range(4)] == dumps
    assert dumps == [(GOLDEN / "sample" / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    lines = p.stdout.splitlines()
    assert lines[:4] == plain.stdout.splitlines() == [f"Processor {n} initialized" for n in range(4)]
    assert lines[4:] == ["coherence addrs=0 bits=0x0"]


def test_cli_coherence_column_of_an_explore(dash, tmp_path):
    """`test_3 --explore 300 --coherence`: the lines of the run without the flag, each with a sixth
    column, the outcome's bits as check_outcomes gives them."""
    cli = cli_dir(dash, tmp_path, "test_3")
    plain, flagged = cli("--explore", "300"), cli("--explore", "300", "--coherence")
    assert plain.returncode == 0 and flagged.returncode == 0, plain.stderr + flagged.stderr
    rows = [ln.split() for ln in flagged.stdout.splitlines()]
    assert [" ".join(r[:5]) for r in rows] == plain.stdout.splitlines() and all(len(r) == 6 for r in rows)
    eng, _, _ = explorer(dash, "test_3", 64)
    with eng:
        outs = eng.explore(0, 0, 300)
        rec = eng.check_outcomes(0, outs)
    assert [r[0] for r in rows] == [f"{o['digest']:016x}" for o in outs]
    assert [r[5] for r in rows] == [f"{int(b):x}" for b in rec["bits"]]
    assert any(r[5] != "0" and r[4] == "0" for r in rows)
    # a violating witness as a directory run: the line names the first address and its bits
    k = next(i for i, r in enumerate(rec) if r["bits"])
    p = cli("--schedule", str(outs[k]["seed"]), "--coherence")
    assert p.returncode in (0, 2), p.stderr
    assert p.stdout.splitlines()[-1] == (f"coherence addrs={rec[k]['addrs']} bits=0x{int(rec[k]['bits']):X} "
                                         f"first=0x{int(rec[k]['first_addr']):02X} "
                                         f"first_bits=0x{int(rec[k]['first_bits']):X}")
