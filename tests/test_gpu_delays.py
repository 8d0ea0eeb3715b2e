"""Delay words on the GPU: dash_set_system_delays (the third schedule source of sim_kernel's seeded modes)
and dash_explore_delays (the enumeration of a delay space on the device).

A word's yardstick is the CPU oracle under the word's explicit round table, which tests/delay_ref.py
builds from the definition without libdash, and the engine itself under dash_set_schedule of
dash_delay_schedule's table. An exploration's yardstick is the Python enumeration of the space over the
oracle: live for the D = 1 spaces and the generated source, recorded (tests/golden/delay_outcomes.json)
for D = 2."""
import functools

import numpy as np
import pytest

import coherence_ref as cr
import delay_ref as dr
import oracle_ctypes as oc
from oracle_ctypes import run_system
from test_gpu_parity import check_stats, random_batch, state_arrays

pytestmark = pytest.mark.gpu
S = dr.slot


def cap_of(max_instr):
    return 1024 + 256 * max_instr


def special_words(N):
    """The shapes a word can take; t < N throughout, so every slot acts."""
    hi = N - 1
    return [
        dr.LOCKSTEP,
        dr.pack([S(1, 2, 3)]),                                      # rounds 3..6: across the trip boundary at 4
        dr.pack([S(0, 0, 5)]),                                      # length 1
        dr.pack([S(hi, 7, 2)]),                                     # length 128
        dr.pack([S(0, 1, 1022)]),                                   # start 1022 (past these runs: no effect)
        dr.pack([S(0, 1, 1), S(1, 3, 2), S(2, 0, 7), S(hi, 4, 9)]),  # all four slots
        dr.pack([S(2, 2, 6), S(2, 3, 8)]),                          # two slots on one node that overlap
        dr.pack([S(0, 2, 8), S(1, 2, 8), S(2, 2, 8), S(3, 2, 8)]),  # N = 4: every node sits out trip 8..11
        dr.pack([S(3, 5, 0), dr.EMPTY, S(1, 6, 4)]),                # an empty slot between two
    ]


def words_for(rng, n, N):
    """n words: the special ones first (so neighbouring systems of a wave differ), then random ones with
    1..4 slots, starts within the runs and every length."""
    out = special_words(N)
    while len(out) < n:
        k = int(rng.integers(1, 5))
        out.append(dr.pack(S(int(rng.integers(0, N)), int(rng.integers(0, 8)), int(rng.integers(0, 60)))
                           for _ in range(k)))
    return np.array(out[:n], np.uint64)


def oracle_under(packed, lens, N, CS, words, **kw):
    return [dr.run_word(packed[s], lens[s], int(words[s]), N, CS, ring_depth=256, max_rounds=cap_of(packed.shape[2]),
                        **kw) for s in range(len(words))]


def check_against(eng, stats, results, N, CS):
    dig, rnd, err = eng.read_results()
    for s, res in enumerate(results):
        assert int(dig[s]) == res.digest, f"system {s} digest"
        assert int(rnd[s]) == res.rounds, f"system {s} rounds"
        assert int(err[s]) == res.errors, f"system {s} errors"
        assert state_arrays(eng.read_state(s), N, CS) == state_arrays(res.node, N, CS), f"system {s} state"
    check_stats(stats, results)


# ---------------------------------------------------------------- word parity

@pytest.mark.parametrize("CS", [1, 2, 4, 8, 16, 3])
@pytest.mark.parametrize("N", [4, 8])
def test_word_parity(dash, N, CS):
    """Handles of 1, 7 and 130 systems (a lone system, a partial wave, full waves and a partial one) on the
    first systems of one batch, every system under a word of its own."""
    rng = np.random.default_rng(7100 + 16 * N + CS)
    packed, lens = random_batch(rng, 130, N, 24, hot_frac=0.3)
    words = words_for(rng, 130, N)
    results = oracle_under(packed, lens, N, CS, words)
    lock = oracle_under(packed, lens, N, CS, [dr.LOCKSTEP] * 130)
    # the words act: most systems differ from their lockstep run, and the all-sit-out trip lengthens its own
    assert sum(a.digest != b.digest or a.rounds != b.rounds for a, b in zip(results, lock)) > 65
    if N == 4:
        assert results[7].rounds != lock[7].rounds or results[7].digest != lock[7].digest
    for n in (1, 7, 130):
        with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=24, keep_state=True, schedule_seed=1) as eng:
            eng.load_traces(packed[:n], lens[:n])
            eng.set_system_delays(words[:n])
            stats = eng.run()
            check_against(eng, stats, results[:n], N, CS)
            by_words = [a.tolist() for a in eng.read_results()]
            if n == 7:
                # the engine under dash_set_schedule of every word's own table: system k is the one to compare
                for k in range(7):
                    tab = dash.delay_schedule(int(words[k]), N, max(dr.last_round(int(words[k])), 1))
                    assert np.array_equal(tab, dr.schedule(int(words[k]), N, len(tab)))
                    eng.set_schedule(tab)
                    eng.run()
                    assert [int(a[k]) for a in eng.read_results()] == [a[k] for a in by_words], k
                    assert state_arrays(eng.read_state(k), N, CS) == state_arrays(results[k].node, N, CS)
            if n == 130:
                # the all-ones word next to seed 0 of dash_set_system_seeds: both are lockstep
                eng.set_system_delays(np.full(n, dr.LOCKSTEP, np.uint64))
                eng.run()
                ones = [a.tolist() for a in eng.read_results()]
                eng.set_system_seeds(np.zeros(n, np.uint64))
                eng.run()
                assert ones == [a.tolist() for a in eng.read_results()]
                assert ones[0] == [r.digest for r in lock] and ones[1] == [r.rounds for r in lock]
                eng.set_system_delays(words)  # and back: the last call wins
                eng.run()
                assert [a.tolist() for a in eng.read_results()] == by_words


def test_start_1022_in_a_run_that_reaches_it(dash):
    """Long hot traces run past round 1022, so a delay that starts there acts."""
    rng = np.random.default_rng(7300)
    packed, lens = random_batch(rng, 7, 4, 400, block_span=4, hot_frac=0.9, fixed_len=True)
    words = np.array([dr.pack([S(k % 4, 1 + k % 7, 1022)]) for k in range(7)], np.uint64)
    words[6] = dr.pack([S(0, 7, 1022), S(1, 7, 1022), S(2, 6, 1000), S(3, 0, 1022)])
    results = oracle_under(packed, lens, 4, 4, words)
    lock = oracle_under(packed, lens, 4, 4, [dr.LOCKSTEP] * 7)
    assert min(r.rounds for r in lock) > 1030
    assert sum(a.digest != b.digest or a.rounds != b.rounds for a, b in zip(results, lock)) >= 4
    with dash.Engine(7, num_procs=4, cache_size=4, max_instr=400, keep_state=True, schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_system_delays(words)
        check_against(eng, eng.run(), results, 4, 4)
        tab = dash.delay_schedule(int(words[6]), 4, 1150)
        eng.set_schedule(tab)
        eng.run()
        assert int(eng.read_results()[0][6]) == results[6].digest


def test_selectors_and_errors(dash):
    rng = np.random.default_rng(7400)
    packed, lens = random_batch(rng, 24, 4, 24, hot_frac=0.3)
    words = words_for(rng, 24, 4)
    with dash.Engine(24, num_procs=4, cache_size=4, max_instr=24, schedule_seed=87) as eng:
        eng.load_traces(packed, lens)
        eng.run()
        by_handle = eng.read_results()[0].tolist()
        assert by_handle == [run_system(packed[s], lens[s], arb_seed=87).digest for s in range(24)]
        eng.set_system_delays(words)
        eng.set_system_delays(None)  # back to the handle's own seed and table
        eng.run()
        assert eng.read_results()[0].tolist() == by_handle
        for bad in (words[:-1], np.append(words, words[0])):
            with pytest.raises(dash.DashError) as e:
                eng.set_system_delays(bad)
            assert e.value.code == dash.EINVAL
        assert dash.lib().dash_set_system_delays(eng.h, None, 24) == dash.EINVAL
        acts = np.full((4, 4), dash.SIT_OUT, dtype=np.uint8)
        eng.set_micro_schedule(acts)
        with pytest.raises(dash.DashError) as e:
            eng.set_system_delays(words)
        assert e.value.code == dash.ESTATE
    with dash.Engine(24, num_procs=4, cache_size=4, max_instr=24) as eng:  # a lockstep handle
        with pytest.raises(dash.DashError) as e:
            eng.set_system_delays(words)
        assert e.value.code == dash.ESTATE
        eng.load_traces(packed, lens)
        with pytest.raises(dash.DashError) as e:
            eng.explore_delays(1, 4, 2, 1)
        assert e.value.code == dash.ESTATE
    with dash.Engine(24, num_procs=4, cache_size=4, max_instr=24, schedule_seed=1, keep_state=True) as eng:
        eng.load_traces(packed, lens)
        for space in ((0, 1, 1), (1024, 1, 1), (4, 0, 1), (4, 9, 1), (4, 2, 5)):
            with pytest.raises(dash.DashError) as e:
                eng.explore_delays(1, *space)
            assert e.value.code == dash.EINVAL
        with pytest.raises(dash.DashError) as e:
            eng.explore_delays(25, 4, 2, 1)
        assert e.value.code == dash.EINVAL


# ---------------------------------------------------------------- tiers and the event log

@functools.lru_cache(maxsize=None)
def contention_case():
    """Hot lines at N = 8 (as tests/test_gpu_tiers.py builds them), a word per system."""
    rng = np.random.default_rng(7500)
    packed, lens = random_batch(rng, 96, 8, 48, block_span=4, hot_frac=0.9, fixed_len=True)
    words = words_for(rng, 96, 8)
    return packed, lens, words, oracle_under(packed, lens, 8, 2, words)


@pytest.mark.parametrize("flags", ["TIER_FROM_32", "default", "TIER_FROM_256"])
def test_words_follow_systems_through_the_tiers(dash, flags):
    packed, lens, words, results = contention_case()
    depth = np.array([r.max_depth for r in results])
    assert (depth > 16).any() and (depth <= 16).any()  # the inputs put systems on both sides of depth 16
    with dash.Engine(96, num_procs=8, cache_size=2, max_instr=48, keep_state=True, schedule_seed=1,
                     flags=0 if flags == "default" else getattr(dash, flags)) as eng:
        eng.load_traces(packed, lens)
        eng.set_system_delays(words)
        stats = eng.run()
        if flags == "default":
            assert stats["tier_systems"][0] == 96 and stats["tier_systems"][1] == int((depth > 16).sum())
        if flags == "TIER_FROM_32":
            assert stats["tier_systems"][0] == 0 and stats["tier_systems"][1] == 96
            assert stats["tier_systems"][2] == int((depth > 32).sum())
        check_against(eng, stats, results, 8, 2)
        if flags == "default":  # again, now with the overflow hint of the first run
            check_against(eng, eng.run(), results, 8, 2)


def test_event_log_under_words(dash):
    """MODE 3: the log of every system is the oracle's under the word's table."""
    rng = np.random.default_rng(7600)
    packed, lens = random_batch(rng, 9, 4, 24, hot_frac=0.3)
    words = words_for(rng, 9, 4)
    with dash.Engine(9, num_procs=4, cache_size=4, max_instr=24, trace_events=512, schedule_seed=1) as eng:
        eng.load_traces(packed, lens)
        eng.set_system_delays(words)
        eng.run()
        for k in range(9):
            res, log = dr.run_word(packed[k], lens[k], int(words[k]), 4, 4, log=True, log_msgs=True,
                                   max_rounds=cap_of(24))
            assert res.rounds <= 512 and log
            assert dash.format_events(eng.read_events(k)) == log, k


# ---------------------------------------------------------------- dash_explore_delays

def rows(outs, source=None):
    keep = outs if source is None else outs[outs["source"] == source]
    return [{f: int(o[f]) for f in dr.OUT_FIELDS + cr.FIELDS} for o in keep]


def golden_engine(dash, tests, nsys):
    """A handle whose systems 0 .. len(tests) - 1 hold golden trace sets; the others are empty."""
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True)
    sets = [oc.load_test_dir(oc.GOLDEN / t) for t in tests]
    width = max(tr.shape[1] for tr, _ in sets)
    packed, ln = np.zeros((nsys, 4, width), np.uint16), np.zeros((nsys, 4), np.uint32)
    for s, (tr, lens) in enumerate(sets):
        packed[s, :, :tr.shape[1]], ln[s] = tr, lens
    eng.load_traces(packed, ln)
    return eng


def check_totals(result, K, G=1):
    outs, per, tot = result
    assert tot["schedules"] == G * K and tot["unplaced"] == 0 and tot["outcomes"] == len(outs)
    assert int(outs["count"].sum()) == G * K and per["schedules"].tolist() == [K] * G
    assert [(int(o["source"]), int(o["seed"])) for o in outs] == sorted((int(o["source"]), int(o["seed"])) for o in outs)


@pytest.mark.parametrize("nsys", [2048, 100])
@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_explore_one_delay(dash, test, nsys):
    """D = 1 at R = the lockstep rounds, E = 7: 925 and 1,401 schedules, on a handle that holds them all
    (the rest is padding) and on one of 100 systems (10 and 15 passes, the last one padded)."""
    R, want = dr.lockstep_rounds(test), dr.golden_list(test, 1)
    K = dr.count(R, 4, 7, 1)
    with golden_engine(dash, [test], nsys) as eng:
        result = outs, per, tot = eng.explore_delays(1, R, 7, 1)
        assert rows(outs) == want
        assert eng.explore_total == len(want) and tot["passes"] == -(-K // nsys)
        check_totals(result, K)
        # every witness is the stated word, and it reproduces the outcome on the oracle
        for o in outs:
            w = dash.delay_word(R, 7, 1, 4, int(o["seed"]))
            assert w == dr.word_at(R, 4, 7, 1, int(o["seed"]))
        # afterwards the handle holds the last pass: its words stay set
        base = (tot["passes"] - 1) * nsys
        fresh = K - base
        dig = eng.read_results()[0]
        for k in (0, 1, nsys // 2, nsys - 1):
            word = dr.word_at(R, 4, 7, 1, base + k % fresh)
            assert int(dig[k]) == dr.run_word(*dr.golden(test), word).digest, k
        eng.run()  # and a plain run follows them again
        assert np.array_equal(eng.read_results()[0], dig)


@pytest.mark.parametrize("nsys", [32768, 100])
def test_explore_generated_8_nodes(dash, nsys):
    """An 8-node x 6-instruction source at (R, E, D) = (8, 3, 2): 18,529 schedules."""
    tr, lens = dr.generated()
    want = dr.generated_list()
    with dash.Engine(nsys, num_procs=8, cache_size=4, max_instr=8, schedule_seed=1, keep_state=True) as eng:
        packed, ln = np.zeros((nsys, 8, tr.shape[1]), np.uint16), np.zeros((nsys, 8), np.uint32)
        packed[0], ln[0] = tr, lens
        eng.load_traces(packed, ln)
        result = outs, per, tot = eng.explore_delays(1, *dr.GEN_SPACE)
        assert rows(outs) == want and len(want) >= 2
        check_totals(result, 18_529)
        assert tot["passes"] == -(-18_529 // nsys)


@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_explore_two_delays(dash, test):
    """D = 2 on a 2^17-system handle (4 and 8 passes) against the recorded oracle list, and the accepted
    outputs of the reference at their fewest delays."""
    R, want = dr.lockstep_rounds(test), dr.recorded(test)
    K = dr.count(R, 4, 7, 2)
    with golden_engine(dash, [test], 1 << 17) as eng:
        result = outs, per, tot = eng.explore_delays(1, R, 7, 2)
        assert rows(outs) == want
        check_totals(result, K)
        assert tot["passes"] == -(-K // (1 << 17))
    blocks = [0, 1, dr.count(R, 4, 7, 1), K]
    by_digest = {(int(o["digest"]), int(o["errors"])): int(o["seed"]) for o in outs}
    for (t, run), d in dr.ACCEPTED.items():
        if t == test:
            seed = by_digest[(dr.accepted_digest(t, run), 0)]
            assert blocks[d] <= seed < blocks[d + 1], run
            assert len(dash.delay_unpack(dash.delay_word(R, 7, 2, 4, seed))) == d


def test_explore_several_sources(dash):
    """test_3, test_4 and sample in one call: three passes of 333 schedules per source on 1000 systems."""
    tests, (R, E, D) = ["test_3", "test_4", "sample"], (33, 7, 1)
    want = [dr.oracle_list(*oc.load_test_dir(oc.GOLDEN / t), R, E, D) for t in tests]
    assert want[0] == dr.golden_list("test_3", 1)
    with golden_engine(dash, tests, 1000) as eng:
        result = outs, per, tot = eng.explore_delays(3, R, E, D)
        for g in range(3):
            assert rows(outs, g) == want[g], tests[g]
        check_totals(result, 925, G=3)
        assert tot["passes"] == 3
        assert per["outcomes"].tolist() == [len(w) for w in want]
        assert per["incoherent_schedules"].tolist() == [sum(o["count"] for o in w if o["bits"]) for w in want]
        assert per["top_count"].tolist() == [max(o["count"] for o in w) for w in want]
    for g, t in enumerate(tests):  # and each source alone gives its own list
        with golden_engine(dash, [t], 1000) as eng:
            assert rows(eng.explore_delays(1, R, E, D)[0]) == want[g]


def test_full_table(dash):
    """97 outcomes do not fit 64 slots: DASH_ETRUNC, and what is listed is exact."""
    R = dr.lockstep_rounds("test_3")
    K, want = dr.count(R, 4, 7, 2), {(o["digest"], o["errors"]): o for o in dr.recorded("test_3")}
    with golden_engine(dash, ["test_3"], 1 << 17) as eng:
        with pytest.raises(dash.DashError) as e:
            eng.explore_delays(1, R, 7, 2, table_slots=64)
        assert e.value.code == dash.ETRUNC
        outs, per, tot = eng.explore_sources_result
        assert len(outs) == 64 and tot["table_slots"] == 64 and tot["unplaced"] > 0
        assert int(outs["count"].sum()) + tot["unplaced"] == tot["schedules"] == K
        for o in rows(outs):
            assert o == want[(o["digest"], o["errors"])]
