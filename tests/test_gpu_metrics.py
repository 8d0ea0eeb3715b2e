"""dash_compute_metrics / dash_read_metrics (csrc/dash_metrics.hip) on the GPU: every field of every
node's record against tests/metrics_ref.py applied to the host path's events (Engine.read_events,
itself pinned on the oracle), the count fields against the oracle's own text log, the totals
against the records, and the message histogram of dash_run against both.

The shapes are the smallest at which the kernel can go wrong: 13 systems (a partial last wave at
every lane-segment width), 3 and 5 nodes (dead lanes in each segment), random lengths 0..40 with
an all-empty system, and round counts of every residue mod 4 (the last 4-round row is partly
stale)."""
import functools
import json
import shutil
import subprocess

import numpy as np
import pytest

import metrics_ref as mr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
NSYS, MAXLEN = 13, 40
# (num_procs, cache_size) -> the rng seed of its batch, chosen on the CPU with the oracle so that the
# batch holds systems of every rounds % 4 (asserted below)
SHAPES = {(4, 4): 5, (8, 2): 4, (3, 4): 1, (5, 1): 1}


@functools.lru_cache(maxsize=None)
def batch(N, CS):
    """13 systems: random lengths 0..40; system 0 has no instruction at all (rounds == 0), system 1
    is short next to long neighbours of the same wave."""
    packed, lens = random_batch(np.random.default_rng(SHAPES[N, CS]), NSYS, N, MAXLEN, block_span=4, hot_frac=0.3)
    lens[0] = 0
    lens[1] = np.minimum(lens[1], 2)
    return packed, lens


@functools.lru_cache(maxsize=None)
def oracle_runs(N, CS, seed=0):
    packed, lens = batch(N, CS)
    return [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS, log=True, log_msgs=True, arb_seed=seed)
            for s in range(NSYS)]


def as_dicts(rec_sys):
    return [{f: int(node[f]) for f in mr.FIELDS} for node in rec_sys]


def events_of(eng, s):
    return [(e.round, e.node, e.kind, e.word) for e in eng.read_events(s)]


def check_records(eng, rec, rounds, deliveries=None):
    """All 16 fields of every node of every system against the Python reference over the host path's
    events of rounds [0, rounds[s])."""
    for s in range(eng.num_systems):
        want = mr.metrics_from_events(events_of(eng, s), int(rounds[s]), eng.num_procs,
                                      deliveries(s) if deliveries else ())
        assert as_dicts(rec[s]) == want, s


def check_totals(tot, rec, cut):
    for f in mr.FIELDS:
        col = rec[f].astype(np.uint64)
        assert tot[f] == int(col.max() if f == "wait_max" and col.size else col.sum()), f
    assert tot["systems"] == len(cut) and tot["truncated_systems"] == int(cut.sum())


def check_hist(rec, hist):
    """The identities of an untruncated, error-free batch against a per-type message histogram."""
    total = {f: int(rec[f].astype(np.uint64).sum()) for f in mr.FIELDS}
    assert total["read_misses"] == hist[mr.READ_REQUEST]
    assert total["write_misses"] == hist[mr.WRITE_REQUEST]
    assert total["upgrades"] == hist[mr.UPGRADE]
    assert total["invalidations"] == hist[mr.INV]
    assert total["interventions"] == hist[mr.WRITEBACK_INV] + hist[mr.WRITEBACK_INT]
    assert total["msgs"] == sum(hist)


def check_oracle_counts(rec, runs, N):
    """The count fields against those parsed from the oracle's own text log of the same traces."""
    for s, (_, log) in enumerate(runs):
        ev = mr.events_from_text(log)
        want = mr.metrics_from_events(ev, len(ev), N)
        got = as_dicts(rec[s])
        for t in range(N):
            assert {f: got[t][f] for f in mr.COUNT_FIELDS} == {f: want[t][f] for f in mr.COUNT_FIELDS}, (s, t)


def run_and_measure(eng, packed, lens):
    eng.load_traces(packed, lens)
    stats = eng.run()
    tot = eng.compute_metrics()
    rec, cut = eng.read_metrics()
    return stats, tot, rec, cut


@pytest.mark.parametrize("N,CS", list(SHAPES))
def test_lockstep_shapes(dash, N, CS):
    packed, lens = batch(N, CS)
    runs = oracle_runs(N, CS)
    want_rounds = np.array([res.rounds for res, _ in runs])
    assert {int(r) % 4 for r in want_rounds} == {0, 1, 2, 3}  # every cut of the last 4-round row
    assert want_rounds[0] == 0 and want_rounds.max() > 4 * want_rounds[1] > 0  # empty, short, long
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as eng:
        stats, tot, rec, cut = run_and_measure(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert np.array_equal(rounds, want_rounds) and stats["err_bits"] == 0
        assert rec.shape == (NSYS, N) and rec.dtype.names == mr.FIELDS and not cut.any()
        assert as_dicts(rec[0]) == [dict.fromkeys(mr.FIELDS, 0)] * N  # rounds == 0: an all-zero record
        check_records(eng, rec, rounds)
        check_oracle_counts(rec, runs, N)
        check_totals(tot, rec, cut)
        check_hist(rec, stats["hist"])
        assert int(rec["reads"].sum() + rec["writes"].sum()) == stats["instructions"] == int(lens.sum())
        # a window of the batch
        part, part_cut = eng.read_metrics(5, 3)
        assert np.array_equal(part, rec[5:8]) and len(part_cut) == 3


def test_stale_rows_of_an_earlier_run_are_not_read(dash):
    """The log is never cleared: after long traces, short ones on the same handle leave the long
    run's words in the rows past each system's last round, and inside its last 4-round row."""
    N, CS = 8, 2
    long_tr, long_lens = batch(N, CS)
    short_lens = np.minimum(long_lens, np.arange(NSYS, dtype=np.uint32)[:, None] % 5)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as eng:
        eng.load_traces(long_tr, long_lens)
        eng.run()
        _, tot, rec, cut = run_and_measure(eng, long_tr, short_lens)
        rounds = eng.read_results()[1]
        check_records(eng, rec, rounds)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as fresh:
        _, tot2, rec2, cut2 = run_and_measure(fresh, long_tr, short_lens)
    assert np.array_equal(rec, rec2) and tot == tot2 and np.array_equal(cut, cut2)
    assert {int(r) % 4 for r in rounds} == {0, 1, 2, 3}


def test_truncated_log(dash):
    """trace_events = half the longest run: the flags are set exactly for the systems that ran
    longer, whose records are the reference over [0, ev_rounds); the others are unaffected."""
    N, CS = 8, 2
    packed, lens = batch(N, CS)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as full:
        _, _, full_rec, _ = run_and_measure(full, packed, lens)
        rounds = full.read_results()[1]
        events = [events_of(full, s) for s in range(NSYS)]
    half = int(rounds.max()) // 2
    ev_rounds = (half + 3) & ~3
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=half) as eng:
        stats, tot, rec, cut = run_and_measure(eng, packed, lens)
        assert np.array_equal(eng.read_results()[1], rounds)
    assert np.array_equal(cut, (rounds > ev_rounds).astype(np.uint8))
    assert 0 < cut.sum() < NSYS and tot["truncated_systems"] == int(cut.sum())
    for s in range(NSYS):
        assert as_dicts(rec[s]) == mr.metrics_from_events(events[s], min(int(rounds[s]), ev_rounds), N), s
        if not cut[s]:
            assert np.array_equal(rec[s], full_rec[s]), s
    check_totals(tot, rec, cut)


def test_seeded_schedule(dash):
    N, CS, seed = 4, 4, 5
    packed, lens = batch(N, CS)
    runs = oracle_runs(N, CS, seed)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096,
                     schedule_seed=seed) as eng:
        stats, tot, rec, cut = run_and_measure(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert np.array_equal(rounds, [res.rounds for res, _ in runs]) and stats["err_bits"] == 0
        check_records(eng, rec, rounds)
    check_oracle_counts(rec, runs, N)
    check_totals(tot, rec, cut)
    check_hist(rec, stats["hist"])


def test_explicit_round_schedule(dash):
    """The five reference fixtures as one batch under the committed schedule of test_4's run_3."""
    record = json.loads((GOLDEN.parent / "schedules" / "test_4_run_3.json").read_text())
    sched = np.array([[0xFF if c == "-" else int(c) for c in row] for row in record["rounds"]], np.uint8)
    loaded = [oc.load_test_dir(GOLDEN / d) for d in ("sample", "test_1", "test_2", "test_3", "test_4")]
    width = max(tr.shape[1] for tr, _ in loaded)
    packed = np.zeros((5, 4, width), np.uint16)
    for k, (tr, _) in enumerate(loaded):
        packed[k, :, :tr.shape[1]] = tr
    lens = np.stack([ln for _, ln in loaded])
    with dash.Engine(5, num_procs=4, cache_size=4, max_instr=32, trace_events=1024, schedule_seed=1) as eng:
        eng.set_schedule(sched)
        stats, tot, rec, cut = run_and_measure(eng, packed, lens)
        rounds = eng.read_results()[1]
        check_records(eng, rec, rounds)
    runs = [oc.run_system(packed[k], lens[k], log=True, log_msgs=True, sched=sched) for k in range(5)]
    check_oracle_counts(rec, runs, 4)
    check_totals(tot, rec, cut)
    check_hist(rec, stats["hist"])


def test_micro_seeds_count_deliveries(dash):
    """test_4 broadcast to 16 systems, each under its own seeded micro-step schedule: the delivery
    markers of the log are the DASH_MICRO_SEND acts, and every round of a node is an event, a
    delivery or idle."""
    tr, lens = oc.load_test_dir(GOLDEN / "test_4")
    packed = np.zeros((16, 4, tr.shape[1]), np.uint16)
    packed[0] = tr
    all_lens = np.zeros((16, 4), np.uint32)
    all_lens[0] = lens
    with dash.Engine(16, num_procs=4, cache_size=4, max_instr=32, trace_events=1024, schedule_seed=1) as eng:
        eng.load_traces(packed, all_lens)
        eng.broadcast_system(0)
        eng.set_micro_seeds(np.arange(100, 116, dtype=np.uint64))
        stats = eng.run()
        tot = eng.compute_metrics()
        rec, cut = eng.read_metrics()
        rounds = eng.read_results()[1]
        acts = [eng.read_micro_acts(s) for s in range(16)]
        check_records(eng, rec, rounds,
                      lambda s: [(int(r), int(t)) for r, t in zip(*np.nonzero(acts[s] == dash.MICRO_SEND))])
    assert len({a.tobytes() for a in acts}) > 1  # distinct schedules
    for s in range(16):
        assert np.array_equal(rec[s]["deliveries"], (acts[s] == dash.MICRO_SEND).sum(axis=0)), s
        assert rec[s]["deliveries"].sum() > 0
        busy = rec[s]["reads"] + rec[s]["writes"] + rec[s]["msgs"] + rec[s]["deliveries"]
        assert np.array_equal(rec[s]["idle_rounds"] + busy, np.full(4, rounds[s])), s
    check_totals(tot, rec, cut)
    assert tot["deliveries"] > 0


def test_after_explore_the_metrics_are_the_last_pass(dash):
    tr, lens = oc.load_test_dir(GOLDEN / "test_4")
    packed = np.zeros((8, 4, tr.shape[1]), np.uint16)
    packed[0] = tr
    all_lens = np.zeros((8, 4), np.uint32)
    all_lens[0] = lens
    with dash.Engine(8, num_procs=4, cache_size=4, max_instr=32, trace_events=1024, schedule_seed=1) as eng:
        eng.load_traces(packed, all_lens)
        assert eng.explore(0, 0, 16)
        tot = eng.compute_metrics()
        rec, cut = eng.read_metrics()
        check_records(eng, rec, eng.read_results()[1])
    check_totals(tot, rec, cut)
    assert tot["reads"] + tot["writes"] == 8 * int(lens.sum())


def test_systems_rerun_at_a_deeper_queue_tier(dash):
    """A contention batch: the systems handed to the 32-deep tier are simulated again from scratch,
    and the log (so the metrics) is the final tier's."""
    N, CS = 8, 2
    packed, lens = random_batch(np.random.default_rng(9000 + 16 * N + CS), 16, N, 100, block_span=4, hot_frac=0.9,
                                fixed_len=True)
    with dash.Engine(16, num_procs=N, cache_size=CS, max_instr=100, trace_events=2048) as eng:
        stats, tot, rec, cut = run_and_measure(eng, packed, lens)
        # precondition: some systems were handed on and simulated again, others were not
        assert stats["tier_systems"][0] == 16 and 0 < stats["tier_systems"][1] < 16
        assert stats["err_bits"] == 0 and not cut.any()
        check_records(eng, rec, eng.read_results()[1])
    check_totals(tot, rec, cut)
    check_hist(rec, stats["hist"])


def test_call_order_and_range_errors(dash):
    N, CS = 4, 4
    packed, lens = batch(N, CS)

    def code(fn, *args):
        with pytest.raises(dash.DashError) as e:
            fn(*args)
        return e.value.code

    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=64) as eng:
        eng.load_traces(packed, lens)
        assert code(eng.compute_metrics) == dash.ESTATE  # before a run
        eng.run()
        assert code(eng.read_metrics) == dash.ESTATE     # not computed yet
        eng.compute_metrics()
        rec, _ = eng.read_metrics()
        assert code(eng.read_metrics, NSYS, 1) == dash.EINVAL
        assert code(eng.read_metrics, 0, NSYS + 1) == dash.EINVAL
        assert code(eng.read_metrics, NSYS - 1, 2) == dash.EINVAL
        assert eng.read_metrics(NSYS, 0)[0].shape == (0, N)  # the empty window at the end is inside
        eng.run()
        assert code(eng.read_metrics) == dash.ESTATE     # the second run invalidated the records
        eng.compute_metrics()
        assert np.array_equal(eng.read_metrics()[0], rec)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN) as eng:  # no event log
        eng.load_traces(packed, lens)
        eng.run()
        assert code(eng.compute_metrics) == dash.ESTATE
        assert code(eng.read_metrics) == dash.ESTATE


def test_cli_metrics(dash, tmp_path):
    """`cache_simulator sample --metrics`: one line per node that equals the Python reference on
    the fixture, after dumps that are byte-identical to a run without the flag."""
    exe = dash.PKG / "cache_simulator"
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / "sample", tmp_path / "tests" / "sample")
    plain = subprocess.run([str(exe), "sample"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    dumps = [(tmp_path / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    for n in range(4):
        (tmp_path / f"core_{n}_output.txt").unlink()
    p = subprocess.run([str(exe), "sample", "--metrics"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert [(tmp_path / f"core_{n}_output.txt").read_bytes() for n in range(4)] == dumps
    assert dumps == [(GOLDEN / "sample" / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    lines = p.stdout.splitlines()
    assert lines[:4] == plain.stdout.splitlines() == [f"Processor {n} initialized" for n in range(4)]
    tr, lens = oc.load_test_dir(GOLDEN / "sample")
    with dash.Engine(1, num_procs=4, cache_size=4, max_instr=32, trace_events=1024) as eng:
        eng.load_traces(tr[None], lens[None])
        eng.run()
        rounds = int(eng.read_results()[1][0])
        want = mr.metrics_from_events(events_of(eng, 0), rounds, 4)
    assert len(lines) == 8
    for t, line in enumerate(lines[4:]):
        words = line.split()
        assert words[:2] == ["metrics", f"node={t}"]
        got = dict(w.split("=") for w in words[2:])
        w = want[t]
        expect = {"instructions": w["reads"] + w["writes"], "evictions": w["evict_shared"] + w["evict_modified"],
                  **{f: w[f] for f in ("reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations",
                                       "interventions", "evict_shared", "evict_modified", "home_requests", "waits",
                                       "wait_max", "idle_rounds")}}
        mean = got.pop("wait_mean")
        assert {k: int(v) for k, v in got.items()} == expect, t
        assert mean == (f"{w['wait_rounds'] / w['waits']:.2f}" if w["waits"] else "0.00")
