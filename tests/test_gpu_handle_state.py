"""The handle's state rules, call by call: after every call that loads traces, changes the schedule,
runs, computes or searches, which reads work and which refuse (DashError with ESTATE), what
read_traces returns, and that the next run() follows the schedule source the call left behind. The
testing-only write_states is in the table too: it voids the coherence records alone.

One table per handle shape: 50 systems (a partial last wave) of 4 nodes, and of 3 (lanes per system !=
nodes: the staged load and read-back path), cache_size 4, max_instr 32, keep_state, an event log of 64
rounds, schedule_seed 1. The traces come from the on-device generator; system 0 is a racy source (the
test_4 fixture at 4 nodes, a contended random system at 3, where the fixture's node 3 does not exist) and
system 1 a system that the CPU oracle finds incoherent, for shrink. Expected digests come from the CPU
oracle under the same seeds and tables, or from the outcomes the call itself reported.

test_overflow_hint_is_dropped: a handle whose earlier runs left an overflow hint (a few systems deeper
than the 16-deep first tier, as in tests/test_gpu_tiers.py), then one of the calls, then a run: digests
and tier_systems are those of a fresh handle with the same traces and seeds. A hint that outlived the
call would start its systems one tier deeper and show in tier_systems[1]."""
import collections

import numpy as np
import pytest

import oracle_ctypes as oc
import shrink_ref as sr
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
S, CS, M = 50, 4, 32
ALL = frozenset(("read_results", "read_coherence", "read_metrics", "read_state"))
RAN = frozenset(("read_results", "read_state"))
CHECKED = RAN | {"read_coherence"}
NONE = frozenset()


def engine(dash, N, seeded=True):
    return dash.Engine(S, num_procs=N, cache_size=CS, max_instr=M, keep_state=True, trace_events=64,
                       schedule_seed=1 if seeded else 0)


def reads(dash, eng):
    """The reads that work; every other one must refuse with ESTATE."""
    calls = {"read_results": eng.read_results, "read_coherence": eng.read_coherence,
             "read_metrics": eng.read_metrics, "read_state": lambda: eng.read_state(eng.num_systems - 1)}
    ok = set()
    for name, call in calls.items():
        try:
            call()
            ok.add(name)
        except dash.DashError as e:
            assert e.code == dash.ESTATE, (name, e)
    return frozenset(ok)


def fill(dash, eng):
    """Run, check and compute: every read works, so that a refusal afterwards is the call's doing."""
    eng.run()
    assert reads(dash, eng) == RAN
    eng.check_coherence()
    assert reads(dash, eng) == CHECKED
    eng.compute_metrics()
    assert reads(dash, eng) == ALL
    return eng.read_results()[0]


def state_bytes(dash, nodes):
    return [bytes(getattr(s, f)) for s in nodes for f, _ in dash.NodeState._fields_]


def loaded_form(tr):
    """Traces as the device keeps them: a read carries value 0."""
    return np.where(tr & 0x8000, tr, tr & 0xFF00).astype(np.uint16)


def sources(N):
    """(racy system, incoherent system) as ([N, M] words, [N] lengths) each."""
    packed, lens = random_batch(np.random.default_rng(40 + N), 8, N, M, block_span=4, hot_frac=0.5)
    if N == 4:
        tr, ln = oc.load_test_dir(oc.GOLDEN / "test_4")
        racy = np.zeros((N, M), np.uint16)
        racy[:, :tr.shape[1]] = tr
        return (racy, ln), (packed[2], lens[2])
    return (packed[0], lens[0]), (packed[2], lens[2])


def oracle_digests(tr, ln, N, seeds):
    return [oc.run_system(tr[k], ln[k], num_procs=N, cache_size=CS, arb_seed=int(seeds[k])).digest
            for k in range(len(seeds))]


def same_traces(eng, tr, ln):
    got_tr, got_ln = eng.read_traces()
    assert np.array_equal(got_ln, ln) and np.array_equal(got_tr, tr)


@pytest.mark.parametrize("N", [4, 3])
def test_state_after_every_call(dash, N, tmp_path):
    (racy_tr, racy_ln), (bad_tr, bad_ln) = sources(N)
    assert len({oc.run_system(racy_tr, racy_ln, num_procs=N, cache_size=CS, arb_seed=s).digest
                for s in range(100, 100 + S)}) > 1, "the racy source has one outcome"
    with engine(dash, N) as eng:
        assert reads(dash, eng) == NONE

        # ---- generate, run, the two compute calls, a second run
        eng.generate(0x5EED, M)
        assert reads(dash, eng) == NONE
        G, G_ln = eng.read_traces()
        assert (G_ln == M).all()
        eng.run()
        assert reads(dash, eng) == RAN
        eng.check_coherence()
        assert reads(dash, eng) == CHECKED
        eng.run()
        assert reads(dash, eng) == RAN
        eng.compute_metrics()
        assert reads(dash, eng) == RAN | {"read_metrics"}
        eng.run()
        assert reads(dash, eng) == RAN
        fill(dash, eng)

        # ---- write_states (testing only): voids the coherence records alone, and read_state returns
        # what was written; the next run puts the run's state back
        ran_state = eng.read_state(S - 1)
        st = eng.read_state(S - 1)
        st[N - 1].cache_addr[CS - 1], st[N - 1].cache_value[CS - 1], st[N - 1].cache_state[CS - 1] = 0x05, 9, 2
        st[0].dir_state[5], st[0].dir_bitvector[5] = 3, 0x81
        results = [a.copy() for a in eng.read_results()]
        eng.write_states(S - 1, [st])
        assert reads(dash, eng) == ALL - {"read_coherence"}
        assert state_bytes(dash, eng.read_state(S - 1)) == state_bytes(dash, st) != state_bytes(dash, ran_state)
        assert all(np.array_equal(a, b) for a, b in zip(results, eng.read_results()))
        eng.check_coherence()
        assert reads(dash, eng) == ALL
        eng.run()
        assert reads(dash, eng) == RAN
        assert state_bytes(dash, eng.read_state(S - 1)) == state_bytes(dash, ran_state)
        fill(dash, eng)

        eng.generate(0x5EED, M)
        assert reads(dash, eng) == NONE
        with pytest.raises(dash.DashError) as refused:
            eng.write_states(0, [st])
        assert refused.value.code == dash.ESTATE
        same_traces(eng, G, G_ln)

        # ---- the loads
        T, T_ln = G.copy(), G_ln.copy()
        T[0], T_ln[0] = racy_tr, racy_ln
        T[1], T_ln[1] = bad_tr, bad_ln
        T = loaded_form(T)
        for k in range(S):
            for t in range(N):
                T[k, t, T_ln[k, t]:] = 0
        fill(dash, eng)
        eng.load_traces(T, T_ln)
        assert reads(dash, eng) == NONE
        same_traces(eng, T, T_ln)
        own = fill(dash, eng)
        assert own.tolist() == oracle_digests(T, T_ln, N, [1] * S)

        blobs = []
        for k in (0, 1):
            dash.write_dir(T[k], T_ln[k], tmp_path / f"s{k}")
            blobs.append([(tmp_path / f"s{k}" / f"core_{t}.txt").read_bytes() for t in range(N)])
        eng.load_text([blobs[k % 2] for k in range(S)])
        assert reads(dash, eng) == NONE
        same_traces(eng, T[np.arange(S) % 2], T_ln[np.arange(S) % 2])
        assert fill(dash, eng).tolist() == [int(own[k % 2]) for k in range(S)]

        eng.load_traces(T, T_ln)
        fill(dash, eng)
        eng.broadcast_system(1)
        assert reads(dash, eng) == NONE
        same_traces(eng, T[[1] * S], T_ln[[1] * S])
        assert fill(dash, eng).tolist() == [int(own[1])] * S

        # ---- the schedule calls: each voids the results, and the next run follows what it set
        eng.load_traces(T, T_ln)
        v = np.arange(100, 100 + S, dtype=np.uint64)
        v[3] = 0  # lockstep
        sched = dash.seed_schedule(7, N, 64)
        by_table = [oc.run_system(T[k], T_ln[k], num_procs=N, cache_size=CS, sched=sched).digest for k in range(S)]
        micro = {}

        def after_system_seeds(dig):
            assert dig.tolist() == oracle_digests(T, T_ln, N, v)

        def after_table(dig):
            assert dig.tolist() == by_table

        def after_micro_seeds(dig):
            micro["dig"] = dig.copy()  # compared with explore_micro's outcomes below

        def after_micro_table(dig):
            assert len(set(dig.tolist())) == 1  # nobody acts: every system keeps its initial state

        def back_to_own(dig):
            assert dig.tolist() == own.tolist()

        SCHEDULE_CALLS = [
            ("set_system_seeds", lambda: eng.set_system_seeds(v), after_system_seeds),
            ("set_system_seeds(None)", lambda: eng.set_system_seeds(None), back_to_own),
            ("set_micro_seeds", lambda: eng.set_micro_seeds(v), after_micro_seeds),
            ("set_micro_seeds(None)", lambda: eng.set_micro_seeds(None), back_to_own),
            ("set_schedule", lambda: eng.set_schedule(sched), after_table),
            ("set_system_seeds(None) after a table", lambda: eng.set_system_seeds(None), back_to_own),
            ("set_micro_schedule", lambda: eng.set_micro_schedule(np.full((4, N), dash.SIT_OUT, np.uint8)),
             after_micro_table),
            ("set_micro_seeds(None) after a micro table", lambda: eng.set_micro_seeds(None), back_to_own),
        ]
        for name, call, follow_up in SCHEDULE_CALLS:
            fill(dash, eng)
            call()
            assert reads(dash, eng) == NONE, name
            same_traces(eng, T, T_ln)
            eng.run()
            assert reads(dash, eng) == RAN, name
            follow_up(eng.read_results()[0])

        # ---- the searches over seeds: the handle is left run, every system a copy of src, following
        # the seeds of the last pass
        def counts(outs):
            return {o["digest"]: o["count"] for o in outs}

        for K in (S, S + 20, 0):
            eng.load_traces(T, T_ln)
            fill(dash, eng)
            outs = eng.explore(0, 100, K)
            assert reads(dash, eng) == (RAN if K else NONE), K
            same_traces(eng, T[[0] * S], T_ln[[0] * S])
            eng.run()
            dig = eng.read_results()[0]
            if K == 0:
                assert outs == []
                continue
            fresh, base = (S, 0) if K == S else (20, S)
            seeds = [100 + base + i % fresh for i in range(S)]
            assert dig.tolist() == oracle_digests(T[[0] * S], T_ln[[0] * S], N, seeds)
            assert set(dig.tolist()) <= set(counts(outs))
            if K == S:
                assert collections.Counter(dig.tolist()) == counts(outs) and len(outs) > 1
        explored = eng.explore(0, 100, S)

        eng.load_traces(T, T_ln)
        fill(dash, eng)
        rec = eng.check_outcomes(0, explored)
        assert reads(dash, eng) == CHECKED
        same_traces(eng, T[[0] * S], T_ln[[0] * S])
        assert np.array_equal(eng.read_coherence()[:len(explored)], rec)
        eng.run()
        assert reads(dash, eng) == RAN
        assert eng.read_results()[0].tolist() == [explored[i % len(explored)]["digest"] for i in range(S)]

        eng.load_traces(T, T_ln)
        fill(dash, eng)
        outs = eng.explore_micro(0, 100, S)
        assert reads(dash, eng) == RAN
        same_traces(eng, T[[0] * S], T_ln[[0] * S])
        eng.run()
        dig = eng.read_results()[0]
        assert collections.Counter(dig.tolist()) == counts(outs)
        assert int(dig[0]) == int(micro["dig"][0])  # system 0 under micro seed 100, as set_micro_seeds ran it
        eng.set_micro_seeds(None)

        # ---- explore_sources: run and checked, the sources replicated per explore_assign
        Gs, K = 3, 40
        passes = -(-K // (S // Gs))
        assign = [dash.explore_assign(S, Gs, K, 100, passes - 1, k) for k in range(S)]
        src_of = [a[0] for a in assign]
        eng.load_traces(T, T_ln)
        fill(dash, eng)
        outs, _per, totals = eng.explore_sources(Gs, 100, K)
        assert totals["passes"] == passes > 1 and totals["schedules"] == Gs * K
        assert reads(dash, eng) == CHECKED
        same_traces(eng, T[src_of], T_ln[src_of])
        eng.run()
        assert reads(dash, eng) == RAN
        dig = eng.read_results()[0]
        assert dig.tolist() == oracle_digests(T[src_of], T_ln[src_of], N, [a[1] for a in assign])
        found = {(int(o["source"]), int(o["digest"])) for o in outs}
        assert all((src_of[k], int(dig[k])) in found for k in range(S) if assign[k][2])

        eng.load_traces(T, T_ln)
        fill(dash, eng)
        outs, _per, totals = eng.explore_sources(Gs, 100, 0)
        assert len(outs) == 0 and totals["passes"] == 0
        assert reads(dash, eng) == NONE
        same_traces(eng, T[src_of], T_ln[src_of])
        eng.set_system_seeds(None)

    # ---- shrink: run and checked, every system the minimal set; without a schedule seed the handle
    # still runs its plain lockstep kernel
    for seeded, seed in ((True, 3), (False, 0)):
        bits = sr.outcome(T[1], T_ln[1], N, CS, seed)[0]
        assert bits, "the source is coherent under the seed"
        with engine(dash, N, seeded) as eng:
            eng.load_traces(T, T_ln)
            fill(dash, eng)
            out = eng.shrink(1, bits & -bits, seed=seed)
            assert reads(dash, eng) == CHECKED
            assert 0 < int(out["lens"].sum()) < int(T_ln[1].sum())
            same_traces(eng, out["trace"][None].repeat(S, 0), out["lens"][None].repeat(S, 0))
            assert (eng.read_coherence()["bits"] & (bits & -bits)).all()
            want = oc.run_system(out["trace"], out["lens"], num_procs=N, cache_size=CS, arb_seed=seed).digest
            assert eng.read_results()[0].tolist() == [want] * S
            eng.run()
            assert reads(dash, eng) == RAN
            assert eng.read_results()[0].tolist() == [want] * S


# ---------------------------------------------------------------- the overflow hint

HS, HN, HCS, HL = 256, 8, 1, 200
DEEP = (2, 67, 130, 255)


def hint_traces():
    """256 systems of 8 nodes: four full-length contention systems, deeper than the first tier's 16; a
    racy 4-node source in system 0 and an incoherent one in system 1; the rest four instructions long."""
    tr, ln = random_batch(np.random.default_rng(801), HS, HN, HL, block_span=4, hot_frac=0.9, fixed_len=True)
    ln[:] = 4
    tr[:, :, 4:] = 0
    deep, deep_ln = random_batch(np.random.default_rng(802), len(DEEP), HN, HL, block_span=4, hot_frac=0.9,
                                 fixed_len=True)
    for slot, d, dl in zip(DEEP, deep, deep_ln):
        tr[slot], ln[slot] = d, dl
    for k, (s_tr, s_ln) in enumerate(sources(4)):
        tr[k], ln[k] = 0, 0
        tr[k, :4, :M], ln[k, :4] = s_tr, s_ln
    return tr, ln


def hinted(dash, tr, ln):
    """A handle with an overflow hint: two runs of the traces, the second of which used it."""
    eng = dash.Engine(HS, num_procs=HN, cache_size=HCS, max_instr=HL, keep_state=True, schedule_seed=1)
    eng.load_traces(tr, ln)
    for _ in range(2):
        tiers = eng.run()["tier_systems"]
        assert tiers[0] == HS and 1 <= tiers[1] <= HS // 32, tiers  # the first tier stays the 16-deep one
    return eng


def hint_calls(dash, tr, ln):
    """(name, the call on the hinted handle, the same schedule on a fresh handle with the traces it left)."""
    v = np.arange(500, 500 + HS, dtype=np.uint64)
    nothing = lambda e, r: None
    blobs = {}
    bits = sr.outcome(tr[1], ln[1], HN, HCS, 3)[0]
    assert bits, "the shrink source is coherent under seed 3"

    def load_text(e):
        import pathlib
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            for k in (0, 1, 2):
                dash.write_dir(tr[k], ln[k], pathlib.Path(td, str(k)))
                blobs[k] = [pathlib.Path(td, str(k), f"core_{t}.txt").read_bytes() for t in range(HN)]
        e.load_text([blobs[2 if k in DEEP else k % 2] for k in range(HS)])

    def check_outcomes(e):
        outs = e.explore(0, 500, HS)
        e.load_traces(tr, ln)  # the hint again, for check_outcomes to drop
        for _ in range(2):
            assert e.run()["tier_systems"][1] >= 1
        e.check_outcomes(0, outs)
        return outs

    def witness_seeds(e, outs):
        e.set_system_seeds([outs[i % len(outs)]["seed"] for i in range(HS)])

    def explore_sources(e):
        return e.explore_sources(2, 500, 200)

    def sources_seeds(e, r):
        passes = r[2]["passes"]
        e.set_system_seeds([dash.explore_assign(HS, 2, 200, 500, passes - 1, k)[1] for k in range(HS)])

    return [
        ("load_traces", lambda e: e.load_traces(tr, ln), nothing),
        ("generate", lambda e: e.generate(0x5EED, 8), nothing),
        ("broadcast_system", lambda e: e.broadcast_system(0), nothing),
        ("load_text", load_text, nothing),
        ("set_system_seeds", lambda e: e.set_system_seeds(v), lambda e, r: e.set_system_seeds(v)),
        ("set_micro_seeds", lambda e: e.set_micro_seeds(v), lambda e, r: e.set_micro_seeds(v)),
        ("explore", lambda e: e.explore(0, 500, HS), lambda e, r: e.set_system_seeds(v)),
        ("explore_micro", lambda e: e.explore_micro(0, 500, HS), lambda e, r: e.set_micro_seeds(v)),
        ("check_outcomes", check_outcomes, witness_seeds),
        ("explore_sources", explore_sources, sources_seeds),
        ("shrink", lambda e: e.shrink(1, bits & -bits, seed=3), lambda e, r: e.set_system_seeds([3] * HS)),
    ]


def test_overflow_hint_is_dropped(dash):
    tr, ln = hint_traces()
    for slot in DEEP:
        assert oc.run_system(tr[slot], ln[slot], num_procs=HN, cache_size=HCS, ring_depth=256, arb_seed=1,
                             max_rounds=1024 + 256 * HL).max_depth > 16, slot
    for name, call, same_schedule in hint_calls(dash, tr, ln):
        with hinted(dash, tr, ln) as eng:
            result = call(eng)
            left, left_ln = eng.read_traces()
            stats = eng.run()
            dig = eng.read_results()[0]
        with dash.Engine(HS, num_procs=HN, cache_size=HCS, max_instr=HL, keep_state=True, schedule_seed=1) as fresh:
            fresh.load_traces(left, left_ln)
            same_schedule(fresh, result)
            fresh_stats = fresh.run()
            assert dig.tolist() == fresh.read_results()[0].tolist(), name
            assert stats["tier_systems"] == fresh_stats["tier_systems"], name
