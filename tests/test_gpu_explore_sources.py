"""dash_explore_sources (csrc/dash_outcomes.hip, csrc/dash_outcomes.cpp) on the GPU: many trace sets
explored in one call, their outcomes merged in a device hash table and classified from the passes'
own final states.

With one source the yardstick is the existing route on a twin handle (explore / explore_micro, then
check_outcomes); with several, the CPU oracle's run of every (source, seed) and tests/coherence_ref.py
on its final state. Which system runs which seed is never restated here: the handle sizes are chosen
so that dash_explore_assign (tests/test_explore_assign.py) takes every branch -- a last pass with fewer
fresh seeds than rows, a padding system, R = 1 -- and the expectations only depend on the set of
(source, seed) pairs.

Shapes: 64- and 70-system handles (one wave of 4-node systems and a partial second one), 256 systems
for the one-outcome case (four waves of one key each), a 64-slot table at load 59 / 64 and an 8-slot
table that 9 keys overfill."""
import functools
import shutil
import subprocess

import numpy as np
import pytest

import coherence_ref as cr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN
from test_gpu_coherence import explorer
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
OUT_FIELDS = ("digest", "count", "seed", "rounds", "errors")


@functools.lru_cache(maxsize=None)
def golden(test):
    return oc.load_test_dir(GOLDEN / test)


def oracle_list(tr, lens, first, count, N=4, CS=4, max_rounds=0):
    """What the oracle gives for seeds first .. first + count - 1 of one trace set: the distinct
    (digest, errors) outcomes in witness order, each with its count, the rounds of its witness and the
    reference's coherence record of its final state."""
    found = {}
    for s in range(first, first + count):
        r = oc.run_system(tr, lens, num_procs=N, cache_size=CS, max_rounds=max_rounds, arb_seed=s)
        o = found.setdefault((r.digest, r.errors), dict(digest=r.digest, count=0, seed=s, rounds=r.rounds,
                                                        errors=r.errors, **cr.check(r.node, N, CS)[0]))
        o["count"] += 1
    return list(found.values())


@functools.lru_cache(maxsize=None)
def golden_list(test, first, count):
    return oracle_list(*golden(test), first, count)


def rows(outs, source=None):
    """The outcomes (of one source) as dicts of the oracle's fields."""
    keep = outs if source is None else outs[outs["source"] == source]
    return [{f: int(o[f]) for f in OUT_FIELDS + cr.FIELDS} for o in keep]


def sums_of(dash, outs, G, unplaced=0):
    """per_source and the totals' counts as sums over the list."""
    per = np.zeros(G, dash.SOURCE_SUMMARY_DTYPE)
    for o in outs:
        p, bad = per[o["source"]], o["bits"] != 0
        p["schedules"] += o["count"]
        p["outcomes"] += 1
        p["top_count"] = max(p["top_count"], o["count"])
        p["coh_bits"] |= o["bits"]
        p["err_bits"] |= o["errors"]
        p["incoherent_outcomes"] += bad
        p["incoherent_schedules"] += o["count"] * bad
    bad = outs["bits"] != 0
    tot = {"schedules": int(outs["count"].sum()) + unplaced, "outcomes": len(outs), "unplaced": unplaced,
           "incoherent_outcomes": int(bad.sum()), "incoherent_schedules": int(outs["count"][bad].sum()),
           "incoherent_clean_schedules": int(outs["count"][bad & (outs["errors"] == 0)].sum()),
           "bit_schedules": [int(outs["count"][(outs["bits"] >> k) & 1 == 1].sum()) for k in range(8)]}
    return per, tot


def check_sums(dash, result, G, unplaced=0):
    outs, per, tot = result
    want_per, want_tot = sums_of(dash, outs, G, unplaced)
    assert np.array_equal(per, want_per)
    assert {k: tot[k] for k in want_tot} == want_tot
    assert tot["sim_ms"] > 0 and tot["merge_ms"] > 0
    # ordered by (source, witness seed)
    assert [(int(o["source"]), int(o["seed"])) for o in outs] == sorted((int(o["source"]), int(o["seed"])) for o in outs)
    assert not outs["_reserved"].any()


def load_sources(dash, tests, nsys, **kw):
    """A handle whose systems 0 .. len(tests) - 1 hold the golden trace sets; the others are empty."""
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True, **kw)
    width = max(golden(t)[0].shape[1] for t in tests)
    packed, ln = np.zeros((nsys, 4, width), np.uint16), np.zeros((nsys, 4), np.uint32)
    for s, t in enumerate(tests):
        tr, lens = golden(t)
        packed[s, :, :tr.shape[1]], ln[s] = tr, lens
    eng.load_traces(packed, ln)
    return eng


# ---------------------------------------------------------------- one source: the existing route

@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_one_source_equals_explore(dash, test):
    """300 round seeds on a 64-system handle: five passes, the last with 44 fresh."""
    eng, tr, lens = explorer(dash, test, 64)
    twin, _, _ = explorer(dash, test, 64)
    with eng, twin:
        outs, per, tot = result = eng.explore_sources(1, 0, 300)
        old = twin.explore(0, 0, 300)
        rec = twin.check_outcomes(0, old)
        assert [{f: int(o[f]) for f in OUT_FIELDS} for o in outs] == old
        assert [cr.record(o) for o in outs] == [cr.record(r) for r in rec]
        assert not outs["source"].any() and eng.explore_total == len(old)
        assert (tot["passes"], tot["table_slots"], tot["schedules"], tot["unplaced"]) == (5, 1024, 300, 0)
        check_sums(dash, result, 1)
        # the oracle's list, checked on the CPU when this test was written
        assert rows(outs) == golden_list(test, 0, 300)
        counts = sorted((int(c) for c in outs["count"]), reverse=True)
        assert counts[:6] == ([254, 28, 7, 4, 2, 2] if test == "test_3" else [295, 5])
        assert len(outs) == (9 if test == "test_3" else 2)
        # afterwards the handle holds the last pass: seeds 256 .. 299, then repeats of them
        dig = eng.read_results()[0]
        want = [oc.run_system(tr, lens, arb_seed=256 + k % 44).digest for k in range(64)]
        assert dig.tolist() == want
        assert eng.read_coherence().shape == (64,)  # and its records are readable


@pytest.mark.parametrize("test", ["test_3", "test_4"])
def test_one_source_equals_explore_micro(dash, test):
    """250 micro seeds under uniform weights: four passes, the last with 58 fresh."""
    eng, _, _ = explorer(dash, test, 64)
    twin, _, _ = explorer(dash, test, 64)
    with eng, twin:
        outs, per, tot = result = eng.explore_sources(1, 0, 250, weights=dash.MICRO_UNIFORM)
        old = twin.explore_micro(0, 0, 250)
        rec = twin.check_outcomes(0, old, weights=dash.MICRO_UNIFORM)
        assert [{f: int(o[f]) for f in OUT_FIELDS} for o in outs] == old
        assert [cr.record(o) for o in outs] == [cr.record(r) for r in rec]
        assert tot["passes"] == 4 and int(per[0]["schedules"]) == 250
        check_sums(dash, result, 1)
        # another weight vector is another walk: the call passes it on
        skew = eng.explore_sources(1, 0, 250, weights=[4, 0, 31, 1])[0]
        assert [{f: int(o[f]) for f in OUT_FIELDS} for o in skew] == twin.explore_micro(0, 0, 250, weights=[4, 0, 31, 1])


# ---------------------------------------------------------------- several sources: the oracle

THREE = ("test_3", "test_4", "sample")


@pytest.mark.parametrize("nsys", [64, 70])
def test_three_sources(dash, nsys):
    """R = 21 (64 systems: one padding system) or 23 (70: one, and a partial second wave): 50 seeds each
    in passes of 21, 21, 8 or 23, 23, 4."""
    with load_sources(dash, THREE, nsys) as eng:
        outs, per, tot = result = eng.explore_sources(3, 0, 50)
        for s, t in enumerate(THREE):
            assert rows(outs, s) == golden_list(t, 0, 50), t
        assert [sorted(map(int, outs["count"][outs["source"] == s]), reverse=True) for s in range(3)] == \
            [[43, 4, 2, 1], [50], [50]]
        assert tot["passes"] == 3 and tot["schedules"] == 150 and per["schedules"].tolist() == [50, 50, 50]
        check_sums(dash, result, 3)
        # a first seed other than 0, and a cap: the first entries, the whole count
        outs7, _, tot7 = eng.explore_sources(3, 7, 30, cap=2)
        want = [o for t in THREE for o in golden_list(t, 7, 30)]
        assert eng.explore_total == tot7["outcomes"] == len(want) and rows(outs7) == want[:2]


def test_keys_are_compared_in_full(dash):
    """The same traces as sources 0 and 1: two equal lists, no doubled counts."""
    with load_sources(dash, ("test_3", "test_3"), 64) as eng:
        outs, per, tot = result = eng.explore_sources(2, 0, 64)
        want = golden_list("test_3", 0, 64)
        assert rows(outs, 0) == rows(outs, 1) == want and len(outs) == 2 * len(want) > 2
        assert per["schedules"].tolist() == [64, 64] and tot["schedules"] == 128
        check_sums(dash, result, 2)


WAVE_N, WAVE_CS, WAVE_LEN, WAVE_SOURCES, WAVE_SEEDS, WAVE_RNG = 8, 4, 2, 40, 6, 5


@functools.lru_cache(maxsize=None)
def wave_case():
    packed, lens = random_batch(np.random.default_rng(WAVE_RNG), WAVE_SOURCES, WAVE_N, WAVE_LEN, block_span=4)
    want = [oracle_list(packed[s], lens[s], 0, WAVE_SEEDS, N=WAVE_N, CS=WAVE_CS, max_rounds=1024 + 256 * WAVE_LEN)
            for s in range(WAVE_SOURCES)]
    return packed, lens, want


@pytest.mark.parametrize("flag", ["", "TEST_INSERT_PER_LANE", "TEST_INSERT_GROUPS"])
def test_a_wave_of_distinct_keys_in_a_loaded_table(dash, flag):
    """40 racy 8-node sources on a 64-system handle: R = 1, so the 40 counted lanes of the one wave hold
    40 distinct keys in every pass, and the 64-slot table ends at a load of 59 / 64, with probe runs that
    wrap its end. The default insert (a few groups, then every lane for itself), the per-lane
    one and the all-groups one give the same list."""
    packed, lens, want = wave_case()
    keys = sum(len(w) for w in want)
    # fixed by a CPU run of the oracle: two instructions per node at most keep the 240 schedules on 59 keys
    assert keys == 59 and sum(len(w) > 1 for w in want) == 14
    full = np.zeros((64, WAVE_N, WAVE_LEN), np.uint16), np.zeros((64, WAVE_N), np.uint32)
    full[0][:WAVE_SOURCES], full[1][:WAVE_SOURCES] = packed, lens
    with dash.Engine(64, num_procs=WAVE_N, cache_size=WAVE_CS, max_instr=WAVE_LEN, schedule_seed=1, keep_state=True,
                     flags=getattr(dash, flag) if flag else 0) as eng:
        eng.load_traces(*full)
        outs, per, tot = result = eng.explore_sources(WAVE_SOURCES, 0, WAVE_SEEDS, table_slots=64)
        assert tot["table_slots"] == 64 and tot["passes"] == WAVE_SEEDS and tot["unplaced"] == 0
        for s in range(WAVE_SOURCES):
            assert rows(outs, s) == want[s], s
        check_sums(dash, result, WAVE_SOURCES)


@pytest.mark.parametrize("flag", ["", "TEST_INSERT_PER_LANE"])
def test_one_outcome_many_schedules(dash, flag):
    """test_1 has one outcome: 1,024 seeds on a 256-system handle are four passes of four waves whose 64
    lanes all hold one key -- one group per wave."""
    eng, tr, lens = explorer(dash, "test_1", 256, flags=getattr(dash, flag) if flag else 0)
    with eng:
        outs, per, tot = eng.explore_sources(1, 5, 1024)
        run = oc.run_system(tr, lens, arb_seed=5)
        assert rows(outs) == [dict(digest=run.digest, count=1024, seed=5, rounds=run.rounds, errors=run.errors,
                                   **cr.check(run.node, 4, 4)[0])]
        assert tot["passes"] == 4 and int(per[0]["top_count"]) == 1024


def test_a_table_that_fills(dash):
    """test_3's nine outcomes for eight slots."""
    eng, _, _ = explorer(dash, "test_3", 64)
    with eng:
        with pytest.raises(dash.DashError) as e:
            eng.explore_sources(1, 0, 300, table_slots=8)
        assert e.value.code == dash.ETRUNC
        outs, per, tot = result = eng.explore_sources_result  # stored before the raise
        want = golden_list("test_3", 0, 300)
        assert len(want) == 9 and tot["table_slots"] == 8 and len(outs) == 8
        assert tot["unplaced"] > 0 and int(outs["count"].sum()) + tot["unplaced"] == 300 == tot["schedules"]
        for o in rows(outs):  # exact for the keys it lists
            assert o in want
        check_sums(dash, result, 1, unplaced=tot["unplaced"])
        # the table is cleared by the next call
        assert rows(eng.explore_sources(1, 0, 300)[0]) == want


def test_call_errors(dash):
    def code(eng, *args, **kw):
        with pytest.raises(dash.DashError) as e:
            eng.explore_sources(*args, **kw)
        return e.value.code

    tr, lens = golden("test_3")
    packed, ln = np.zeros((8, 4, tr.shape[1]), np.uint16), np.zeros((8, 4), np.uint32)
    packed[0], ln[0] = tr, lens
    with dash.Engine(8, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1) as eng:  # no DASH_KEEP_STATE
        eng.load_traces(packed, ln)
        assert code(eng, 1, 0, 8) == dash.ESTATE
    with dash.Engine(8, num_procs=4, cache_size=4, max_instr=32, keep_state=True) as eng:  # schedule_seed == 0
        eng.load_traces(packed, ln)
        assert code(eng, 1, 0, 8) == dash.ESTATE
    with dash.Engine(8, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True) as eng:
        assert code(eng, 1, 0, 8) == dash.ESTATE  # nothing loaded
        eng.load_traces(packed, ln)
        assert code(eng, 0, 0, 8) == dash.EINVAL and code(eng, 9, 0, 8) == dash.EINVAL
        assert code(eng, 1, 0, 8, weights=[1, 32, 1, 1]) == dash.EINVAL
        assert code(eng, 1, (1 << 64) - 8, 8) == dash.EINVAL  # first_seed + seeds_per_source wraps
        n = dash.ctypes.c_uint64(7)
        assert dash.lib().dash_explore_sources(eng.h, 1, 0, 8, None, 0, None, 4, dash.ctypes.byref(n), None,
                                               None) == dash.EINVAL  # out == NULL with cap != 0
        assert dash.lib().dash_explore_sources(eng.h, 1, 0, 8, None, 0, None, 0, dash.ctypes.byref(n), None,
                                               None) == dash.OK  # count only
        assert n.value == len(golden_list("test_3", 0, 8))
        outs, _, tot = eng.explore_sources(8, 0, 0)  # no seeds: no pass, no outcome
        assert len(outs) == 0 and tot["passes"] == 0 and tot["schedules"] == 0
        eng.set_micro_schedule(np.full((4, 4), dash.SIT_OUT, np.uint8))
        assert code(eng, 1, 0, 8) == dash.ESTATE  # round seeds on a handle that follows a micro-step table


# ---------------------------------------------------------------- CLI

def test_cli_sources(dash, tmp_path):
    """`test_3 --explore 300 --sources FILE` with test_4 in FILE: each directory's own --explore lines behind
    a source column, then one summary line per directory."""
    (tmp_path / "tests").mkdir()
    for t in ("test_3", "test_4"):
        shutil.copytree(GOLDEN / t, tmp_path / "tests" / t)
    (tmp_path / "more.txt").write_text("test_4\n")
    exe = dash.PKG / "cache_simulator"

    def cli(*args):
        p = subprocess.run([str(exe), *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()

    for flags in ([], ["--coherence"]):
        own = {t: cli(t, "--explore", "300", *flags) for t in ("test_3", "test_4")}
        both = cli("test_3", "--explore", "300", "--sources", "more.txt", *flags)
        bad = [sum(o["count"] for o in golden_list(t, 0, 300) if o["bits"]) for t in ("test_3", "test_4")]
        assert both == [f"0 {ln}" for ln in own["test_3"]] + [f"1 {ln}" for ln in own["test_4"]] + \
            [f"source 0 test_3 outcomes=9 schedules=300 incoherent={bad[0]}",
             f"source 1 test_4 outcomes=2 schedules=300 incoherent={bad[1]}"]
        assert bad[0] > 0 and bad[1] == 0
    micro = cli("test_4", "--explore-micro", "250", "--sources", "more.txt")
    own = cli("test_4", "--explore-micro", "250")
    assert micro[:-2] == [f"0 {ln}" for ln in own] + [f"1 {ln}" for ln in own]
    p = subprocess.run([str(exe), "test_3", "--sources", "more.txt"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode != 0 and "--sources goes with" in p.stderr
