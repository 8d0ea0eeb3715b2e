"""dash_compute_addr_metrics / dash_read_addr_metrics (csrc/dash_addr.hip) on the GPU: every field of
every address's record against tests/addr_metrics_ref.py applied to the host path's events
(Engine.read_events, itself pinned on the oracle) and against the library's host function, the totals
and class counts against the records, and the sums over addresses against the per-node metrics and
the message histogram of the same run.

The shapes are the smallest at which the kernel can go wrong. The kernel gives one wave to a system,
four systems to a workgroup, and loads 64 / P log rows (4 rounds each) per step, P = next_pow2(nodes),
four steps at a time: 13 systems (a partial last workgroup whose last wave stands alone), 3 and 5 nodes
(dead lanes at both P), random lengths 0..40 with an all-empty system, round counts of every residue
mod 4 (the last row is partly stale), runs shorter than one step and longer than two, and, in a test of
their own, runs long enough for two trips of the loop that needs no masks."""

import numpy as np
import pytest

import addr_metrics_ref as ar
import metrics_ref as mr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN
from test_gpu_metrics import MAXLEN, NSYS, SHAPES, batch, oracle_runs
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
SHARED = ("reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations", "interventions",
          "evict_shared", "evict_modified", "msgs")  # fields dash_node_metrics has too


def step_rounds(N):
    """Rounds one load step of a wave covers."""
    return 4 * 64 // (1 << (N - 1).bit_length())


def as_dicts(rec_sys):
    return [{f: int(m[f]) for f in ar.FIELDS} for m in rec_sys]


def events_of(eng, s):
    return [(e.round, e.node, e.kind, e.word) for e in eng.read_events(s)]


def check_records(dash, rec, events, kept, N):
    """All 12 fields of every address of every system against the Python reference and the host function
    over the events of rounds [0, kept[s])."""
    for s, ev in enumerate(events):
        want, foreign = ar.addr_metrics_from_events(ev, int(kept[s]), N)
        assert as_dicts(rec[s]) == want and foreign == 0, s
        host, host_foreign = dash.addr_metrics_from_events(ev, N, int(kept[s]))
        assert np.array_equal(host, rec[s]) and host_foreign == 0, s


def check_totals(dash, tot, rec, cut):
    want = ar.totals_from_records([as_dicts(r) for r in rec])
    assert {k: tot[k] for k in want} == want
    classes = [dash.addr_class(m) for r in rec for m in r]
    assert tot["class_addrs"] == [classes.count(c) for c in range(5)] and sum(tot["class_addrs"]) == rec.size
    assert tot["foreign_events"] == 0
    assert tot["systems"] == len(cut) and tot["truncated_systems"] == int(cut.sum())


def check_node_metrics(eng, rec):
    """The other axis of the same log: sums over addresses == sums over nodes, system by system."""
    eng.compute_metrics()
    nodes, _ = eng.read_metrics()
    for f in SHARED:
        assert np.array_equal(rec[f].astype(np.uint64).sum(axis=1), nodes[f].astype(np.uint64).sum(axis=1)), f


def check_hist(rec, hist):
    total = {f: int(rec[f].astype(np.uint64).sum()) for f in ar.SUM_FIELDS}
    assert total["read_misses"] == hist[mr.READ_REQUEST]
    assert total["write_misses"] == hist[mr.WRITE_REQUEST]
    assert total["upgrades"] == hist[mr.UPGRADE]
    assert total["invalidations"] == hist[mr.INV]
    assert total["interventions"] == hist[mr.WRITEBACK_INV] + hist[mr.WRITEBACK_INT]
    assert total["flushes"] == hist[mr.FLUSH] + hist[mr.FLUSH_INVACK]
    assert total["msgs"] == sum(hist)


def trace_classes(packed, lens, N):
    """The class of every address of every system from the traces alone: who reads it, who writes it."""
    out = []
    for tr, ln in zip(packed, lens):
        r, w = [0] * (N * 16), [0] * (N * 16)
        for t in range(N):
            for word in tr[t][:ln[t]]:
                (w if word & 0x8000 else r)[(int(word) >> 8) & 0x7F] |= 1 << t
        out.append([ar.addr_class({"reads": bin(r[a]).count("1"), "writes": bin(w[a]).count("1"),
                                   "nodes": r[a] | w[a] << 8}) for a in range(N * 16)])
    return out


def run_and_profile(eng, packed, lens):
    eng.load_traces(packed, lens)
    stats = eng.run()
    tot = eng.compute_addr_metrics()
    rec, cut = eng.read_addr_metrics()
    return stats, tot, rec, cut


@pytest.mark.parametrize("N,CS", list(SHAPES))
def test_lockstep_shapes(dash, N, CS):
    packed, lens = batch(N, CS)
    want_rounds = np.array([res.rounds for res, _ in oracle_runs(N, CS)])
    # preconditions, chosen on the CPU with the oracle
    assert {int(r) % 4 for r in want_rounds} == {0, 1, 2, 3}      # every cut of the last 4-round row
    assert want_rounds[0] == 0 and 0 < want_rounds[1] < step_rounds(N)  # empty; shorter than one load step
    assert want_rounds.max() > 2 * step_rounds(N)                  # longer than two
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as eng:
        stats, tot, rec, cut = run_and_profile(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert np.array_equal(rounds, want_rounds) and stats["err_bits"] == 0
        assert rec.shape == (NSYS, N * 16) and rec.dtype.names == ar.FIELDS and not cut.any()
        assert not rec[0].view(np.uint32).any()                    # rounds == 0: all-zero records
        assert all(dash.addr_class(m) == dash.ADDR_UNTOUCHED for m in rec[0])
        check_records(dash, rec, [events_of(eng, s) for s in range(NSYS)], rounds, N)
        check_totals(dash, tot, rec, cut)
        # an error-free run issues every instruction: the classes follow from the traces alone
        assert [[dash.addr_class(m) for m in r] for r in rec] == trace_classes(packed, lens, N)
        assert tot["class_addrs"][dash.ADDR_UNTOUCHED] >= N * 16 and tot["class_addrs"][dash.ADDR_MULTI_WRITER] > 0
        check_node_metrics(eng, rec)
        check_hist(rec, stats["hist"])
        assert int(rec["reads"].sum() + rec["writes"].sum()) == stats["instructions"] == int(lens.sum())
        part, part_cut = eng.read_addr_metrics(5, 3)  # a window of the batch
        assert np.array_equal(part, rec[5:8]) and len(part_cut) == 3


@pytest.mark.parametrize("N,CS", list(SHAPES))
def test_long_runs_take_the_unmasked_loop(dash, N, CS):
    """Five systems of 120 instructions per node: every run is longer than two trips of the loop over
    whole steps (4 steps of 64 / P rows of 4 rounds), which the 40-instruction batches never enter at
    P = 4."""
    packed, lens = random_batch(np.random.default_rng(9000 + 16 * N + CS), 5, N, 120, block_span=4, hot_frac=0.5,
                                fixed_len=True)
    with dash.Engine(5, num_procs=N, cache_size=CS, max_instr=120, trace_events=2048) as eng:
        stats, tot, rec, cut = run_and_profile(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert rounds.min() >= 2 * 4 * step_rounds(N) and rounds.max() <= 2048 and not cut.any()
        check_records(dash, rec, [events_of(eng, s) for s in range(5)], rounds, N)
        check_totals(dash, tot, rec, cut)
        check_node_metrics(eng, rec)
        check_hist(rec, stats["hist"])


def test_every_lane_on_one_address_and_every_address_once(dash):
    """(8, 2). System 0: all 8 nodes issue 40 instructions on one address, alternating RD and WR, so every
    lane of the wave updates the same table words. System 1: each of the 128 addresses is touched exactly
    once, by a node that is not its home, so every table slot is used."""
    N, CS, L = 8, 2, 40
    hot = 0x35
    packed = np.zeros((2, N, L), np.uint16)
    lens = np.zeros((2, N), np.uint32)
    k = np.arange(L)
    packed[0] = ((k % 2) << 15 | hot << 8 | np.where(k % 2, k + 1, 0))[None, :]
    lens[0] = L
    for t in range(N):  # node t takes the 16 blocks homed on node (t + 3) % 8, every second one a write
        b = np.arange(16)
        packed[1, t, :16] = (b % 2) << 15 | (((t + 3) % 8) << 4 | b) << 8 | np.where(b % 2, 100 + b, 0)
    lens[1] = 16
    with dash.Engine(2, num_procs=N, cache_size=CS, max_instr=L, trace_events=4096) as eng:
        stats, tot, rec, cut = run_and_profile(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert stats["err_bits"] == 0 and not cut.any()
        check_records(dash, rec, [events_of(eng, s) for s in range(2)], rounds, N)
        check_totals(dash, tot, rec, cut)
        check_node_metrics(eng, rec)
        check_hist(rec, stats["hist"])
    one = rec[0][hot]
    assert (one["reads"], one["writes"], one["nodes"] & 0xFFFF) == (N * L // 2, N * L // 2, 0xFFFF)
    assert dash.addr_class(one) == dash.ADDR_MULTI_WRITER and one["invalidations"] > 0
    others = np.delete(rec[0], hot)
    assert not others.view(np.uint32).any()
    assert tot["msgs_max"] == int(one["msgs"]) == int(rec["msgs"].max())
    assert np.array_equal(rec[1]["reads"] + rec[1]["writes"], np.ones(128, np.uint32))
    assert all(dash.addr_class(m) == dash.ADDR_PRIVATE for m in rec[1])
    for a in range(128):
        t = (a // 16 - 3) % 8
        assert rec[1][a]["nodes"] & 0xFFFF == (1 << t) << (8 if a % 2 else 0), a


@pytest.mark.parametrize("trace_events", [8, 36])
def test_truncated_log_after_a_longer_run(dash, trace_events):
    """A log of 8 and of 36 rounds, shorter than most runs: the flags are set exactly for the systems that
    ran longer, and their records are the reference over [0, the log's rounds). The long batch runs first
    and a short one second on the same handle, so the short one's last kept row and the rows behind it
    hold the long run's words."""
    N, CS = 8, 2
    packed, long_lens = batch(N, CS)
    short_lens = np.minimum(long_lens, np.arange(NSYS, dtype=np.uint32)[:, None] % 5)
    full = {}
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096) as eng:
        for name, lens in (("long", long_lens), ("short", short_lens)):
            eng.load_traces(packed, lens)
            eng.run()
            full[name] = (eng.read_results()[1], [events_of(eng, s) for s in range(NSYS)])
    ev_rounds = (trace_events + 3) & ~3
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=trace_events) as eng:
        for name, lens in (("long", long_lens), ("short", short_lens)):
            rounds, events = full[name]
            stats, tot, rec, cut = run_and_profile(eng, packed, lens)
            assert np.array_equal(eng.read_results()[1], rounds)
            assert np.array_equal(cut, (rounds > ev_rounds).astype(np.uint8))
            check_records(dash, rec, events, np.minimum(rounds, ev_rounds), N)
            check_totals(dash, tot, rec, cut)
            check_node_metrics(eng, rec)
            if name == "long":
                assert 0 < cut.sum() < NSYS  # some systems are cut, some are not
    rounds = full["short"][0]
    if trace_events == 8:
        assert 0 < cut.sum() < NSYS
    else:  # the short runs all fit: every cut of a last row whose other rounds are the long run's
        assert not cut.any() and {int(r) % 4 for r in rounds} == {0, 1, 2, 3}


def test_system_seeds(dash):
    """Distinct seeded round schedules per system, one of them seed 0 (lockstep)."""
    N, CS = 4, 4
    packed, lens = batch(N, CS)
    seeds = np.arange(40, 40 + NSYS, dtype=np.uint64)
    seeds[3] = 0
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=4096, schedule_seed=1) as eng:
        eng.set_system_seeds(seeds)
        stats, tot, rec, cut = run_and_profile(eng, packed, lens)
        rounds = eng.read_results()[1]
        assert stats["err_bits"] == 0 and not cut.any()
        assert rounds[3] == oracle_runs(N, CS)[3][0].rounds
        check_records(dash, rec, [events_of(eng, s) for s in range(NSYS)], rounds, N)
        check_totals(dash, tot, rec, cut)
        check_node_metrics(eng, rec)
        check_hist(rec, stats["hist"])


def test_micro_seeds_delivery_markers_count_nowhere(dash):
    """test_4 broadcast to 16 systems, each under its own seeded micro-step schedule: the log holds
    delivery markers between the events, and no record counts them."""
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
        tot = eng.compute_addr_metrics()
        rec, cut = eng.read_addr_metrics()
        rounds = eng.read_results()[1]
        assert rounds.max() <= 1024 and not cut.any()  # the log holds every run
        events = [events_of(eng, s) for s in range(16)]
        check_records(dash, rec, events, rounds, 4)
        check_totals(dash, tot, rec, cut)
        check_node_metrics(eng, rec)
        assert eng.compute_metrics()["deliveries"] > 0  # the markers are there
    check_hist(rec, stats["hist"])
    assert len({r.tobytes() for r in rec}) > 1  # distinct schedules, distinct profiles
    for s in range(16):
        assert int(rec[s]["reads"].sum() + rec[s]["writes"].sum() + rec[s]["msgs"].sum()) == len(events[s])


def test_call_order_and_range_errors(dash):
    N, CS = 4, 4
    packed, lens = batch(N, CS)

    def code(fn, *args):
        with pytest.raises(dash.DashError) as e:
            fn(*args)
        return e.value.code

    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN, trace_events=64) as eng:
        eng.load_traces(packed, lens)
        assert code(eng.compute_addr_metrics) == dash.ESTATE  # before a run
        eng.run()
        assert code(eng.read_addr_metrics) == dash.ESTATE     # not computed yet
        eng.compute_metrics()
        assert code(eng.read_addr_metrics) == dash.ESTATE     # the node metrics' validity is their own
        eng.compute_addr_metrics()
        rec, _ = eng.read_addr_metrics()
        nodes, _ = eng.read_metrics()                         # still readable
        assert code(eng.read_addr_metrics, NSYS, 1) == dash.EINVAL
        assert code(eng.read_addr_metrics, 0, NSYS + 1) == dash.EINVAL
        assert code(eng.read_addr_metrics, NSYS - 1, 2) == dash.EINVAL
        assert eng.read_addr_metrics(NSYS, 0)[0].shape == (0, N * 16)  # the empty window at the end is inside
        eng.run()
        assert code(eng.read_addr_metrics) == dash.ESTATE     # the second run invalidated the records
        assert code(eng.read_metrics) == dash.ESTATE
        eng.compute_addr_metrics()                            # the other order
        assert code(eng.read_metrics) == dash.ESTATE
        eng.compute_metrics()
        assert np.array_equal(eng.read_addr_metrics()[0], rec)
        assert np.array_equal(eng.read_metrics()[0], nodes)
    with dash.Engine(NSYS, num_procs=N, cache_size=CS, max_instr=MAXLEN) as eng:  # no event log
        eng.load_traces(packed, lens)
        eng.run()
        assert code(eng.compute_addr_metrics) == dash.ESTATE
        assert code(eng.read_addr_metrics) == dash.ESTATE
