"""dash_shrink_many (csrc/dash_shrink.hip, csrc/dash_shrink.cpp) on the GPU: many jobs (source
system, seed, goal) shrunk side by side in lock-step rounds, the handle's systems dealt out over the
candidates of all jobs that are still shrinking.

The yardstick is the twin of tests/shrink_ref.py applied job by job (tests/shrink_many_ref.py): statuses,
steps, final traces and counts must be equal, and so must dash_shrink on a handle of its own. The inputs
(shrink_many_ref.SHAPES: ten jobs per shape, the same traces under two seeds with different fates, jobs that
stop in different rounds, UNMET jobs of both kinds) and what they exercise are checked on the CPU in
tests/test_shrink_many_spec.py.

Handle sizes: 50 systems (many sub-passes per round, a last one that is not full) and 600 (several
sub-passes early, then one with padding, and in the late rounds several jobs within one wave)."""
import ctypes
import subprocess

import numpy as np
import pytest

import coherence_ref as cr
import oracle_ctypes as oc
import shrink_many_ref as smr
import shrink_ref as sr

pytestmark = pytest.mark.gpu
M = smr.M


def engine(dash, N, CS, S, seeded=True, **kw):
    return dash.Engine(S, num_procs=N, cache_size=CS, max_instr=M, keep_state=True,
                       schedule_seed=1 if seeded else 0, **kw)


def load_batch(eng, N, r):
    """The shape's batch of 8 systems in systems 0..7 of the handle; the others are empty."""
    packed, lens = smr.batch(N, r)
    S = eng.num_systems
    tr, ln = np.zeros((S, N, M), np.uint16), np.zeros((S, N), np.uint32)
    tr[:8], ln[:8] = packed, lens
    eng.load_traces(tr, ln)


def as_steps(steps):
    return [tuple(int(x) for x in s) for s in steps]


def check_against_twin(eng, out, jobs, twin, N, CS, systems=None):
    """The call's results and the handle's state afterwards against the twin's results, job by job."""
    J, S = len(jobs), eng.num_systems
    res, rep = out["results"], out["report"]
    assert res["status"].tolist() == [t["status"] for t in twin]
    for i, t in enumerate(twin):
        assert as_steps(out["steps"][i]) == t["steps"], i
        assert out["lens"][i].tolist() == t["lens"].tolist() and np.array_equal(out["trace"][i][:, :M], t["trace"]), i
        assert (int(res["rounds"][i]), int(res["variants"][i]), int(res["instr_before"][i]), int(res["instr_after"][i])) == \
            (len(t["steps"]), t["variants"], t["before"], int(t["lens"].sum())), i
        assert (int(res["src_coh_bits"][i]), int(res["src_errors"][i])) == (t["bits"], t["errors"]), i
    minimal = sum(t["status"] == smr.MINIMAL for t in twin)
    assert (rep["jobs"], rep["minimal"], rep["unmet"]) == (J, minimal, J - minimal)
    assert rep["variants"] == sum(t["variants"] for t in twin) == int(res["variants"].sum())
    assert rep["instr_before"] == sum(t["before"] for t in twin) and rep["instr_after"] == int(out["lens"].sum())
    rounds = smr.round_cands(twin)
    assert rep["rounds"] == len(rounds) and rep["passes"] == smr.passes_run(twin, S)
    assert rep["sim_ms"] > 0 and rep["gen_ms"] > 0 and rep["select_ms"] > 0
    # the handle: system k holds the final set of job k % J, run under that job's seed and checked
    got_tr, got_ln = eng.read_traces()
    dig, rnd, err = eng.read_results()
    rec = eng.read_coherence()
    want = [oc.run_system(t["trace"], t["lens"], num_procs=N, cache_size=CS, arb_seed=jobs[i][1]) for i, t in enumerate(twin)]
    for k in systems if systems is not None else [k for k in range(S) if k < 2 * J] + [S - 1]:
        i = k % J
        assert got_ln[k].tolist() == twin[i]["lens"].tolist() and np.array_equal(got_tr[k][:, :M], twin[i]["trace"]), k
        assert (int(dig[k]), int(rnd[k]), int(err[k])) == (want[i].digest, want[i].rounds, want[i].errors), k
        assert cr.record(rec[k]) == cr.check(want[i].node, N, CS)[0], k


CASES = [(shape, S) for shape in smr.SHAPES for S in (50, 600)]


@pytest.mark.parametrize("shape,S", CASES, ids=["N%d-cs%d-r%d-s%d" % (*c[0], c[1]) for c in CASES])
def test_shrink_many_equals_twin(dash, shape, S):
    N, CS, r = shape
    jobs, twin = smr.jobs(*shape), smr.twin(*shape)
    with engine(dash, N, CS, S) as eng:
        load_batch(eng, N, r)
        out = eng.shrink_many(jobs)
        check_against_twin(eng, out, jobs, twin, N, CS)
        # a fixed point: system i holds job i's final set; shrinking those again takes no step for a MINIMAL
        # job (its last round's candidates run once more), leaves an UNMET one UNMET, and every row alone
        again = eng.shrink_many([(i,) + j[1:] for i, j in enumerate(jobs)])
        assert again["results"]["status"].tolist() == out["results"]["status"].tolist()
        assert not again["results"]["rounds"].any() and all(len(s) == 0 for s in again["steps"])
        assert np.array_equal(again["trace"], out["trace"]) and np.array_equal(again["lens"], out["lens"])
        assert again["results"]["variants"].tolist() == [
            len(sr.candidates(t["lens"])) if t["status"] == smr.MINIMAL else 0 for t in twin]


@pytest.mark.parametrize("shape", smr.SHAPES, ids=["N%d-cs%d-r%d" % s for s in smr.SHAPES])
def test_shrink_many_equals_shrink(dash, shape):
    """dash_shrink, the one-job case of the same engine, on a handle of its own, job by job: the same steps
    and traces for a MINIMAL job, a refusal for an UNMET one. A job's result does not depend on which other
    jobs share the call (both sides are pinned on the CPU twin elsewhere)."""
    N, CS, r = shape
    jobs = smr.jobs(*shape)
    with engine(dash, N, CS, 600) as eng:
        load_batch(eng, N, r)
        out = eng.shrink_many(jobs)
    with engine(dash, N, CS, 600) as eng:
        for i, (src, seed, coh_all, err_all, err_none) in enumerate(jobs):
            load_batch(eng, N, r)
            if out["results"]["status"][i] == dash.SHRINK_UNMET:
                with pytest.raises(dash.DashError) as e:
                    eng.shrink(src, coh_all, err_all=err_all, err_none=err_none, seed=seed)
                assert e.value.code == dash.EINVAL and "does not meet the goal" in str(e.value)
                continue
            alone = eng.shrink(src, coh_all, err_all=err_all, err_none=err_none, seed=seed)
            assert as_steps(alone["steps"]) == as_steps(out["steps"][i]), i
            assert np.array_equal(alone["trace"], out["trace"][i]) and np.array_equal(alone["lens"], out["lens"][i]), i
            rep, res = alone["report"], out["results"][i]
            assert (rep["rounds"], rep["variants"], rep["instr_before"], rep["instr_after"]) == \
                (int(res["rounds"]), int(res["variants"]), int(res["instr_before"]), int(res["instr_after"])), i


def test_lockstep_jobs_on_an_unseeded_handle(dash):
    """The lockstep jobs of (4,4,12) on a handle created without a schedule seed (the plain lockstep kernel);
    a non-zero seed there is refused."""
    shape = smr.SHAPES[0]
    N, CS, r = shape
    pick = [i for i, j in enumerate(smr.jobs(*shape)) if j[1] == 0]
    jobs, twin = [smr.jobs(*shape)[i] for i in pick], [smr.twin(*shape)[i] for i in pick]
    assert len(jobs) >= 4 and {t["status"] for t in twin} == {smr.MINIMAL, smr.UNMET}
    with engine(dash, N, CS, 50, seeded=False) as eng:
        load_batch(eng, N, r)
        with pytest.raises(dash.DashError) as e:
            eng.shrink_many(jobs[:1] + [(1, 7, 1, 0, 0)])
        assert e.value.code == dash.ESTATE
        check_against_twin(eng, eng.shrink_many(jobs), jobs, twin, N, CS)


def test_as_many_jobs_as_systems(dash):
    """J == S: the 8 jobs (k, SEEDS[k]) on a handle of 8 systems; every sub-pass is full of candidates or
    padded by one base per job."""
    shape = smr.SHAPES[1]
    N, CS, r = shape
    jobs, twin = smr.jobs(*shape)[:8], smr.twin(*shape)[:8]
    with engine(dash, N, CS, 8) as eng:
        load_batch(eng, N, r)
        check_against_twin(eng, eng.shrink_many(jobs), jobs, twin, N, CS)


def test_one_job_alone_equals_shrink(dash):
    row = sr.ROWS[0]  # (8, 4, 11, 7): tests/test_gpu_shrink.py's first row
    N, CS, r, seed = row
    k, _tr, lens, bits = sr.row_source(*row)
    tr, ln, steps = sr.row_twin(*row)
    with engine(dash, N, CS, 50) as eng:
        load_batch(eng, N, r)
        out = eng.shrink_many([(k, seed, bits & -bits, 0, 0xFFFFFFFF)])
        assert as_steps(out["steps"][0]) == steps and out["lens"][0].tolist() == ln.tolist()
        assert np.array_equal(out["trace"][0], tr)
        rep = out["report"]
        assert rep["variants"] == sr.variants_run(lens, steps) and rep["rounds"] == len(steps) + 1
        Cs = [c for _, _, _, c in steps] + [len(sr.candidates(ln))]
        assert rep["passes"] == 2 + sum(-(-c // 50) for c in Cs)  # dash_shrink's own count


def test_more_systems_than_a_grid_dimension(dash):
    """66,000 systems x 4 nodes: a launch over systems takes a second trip of a 65,535 grid cap; the systems
    past it must hold their jobs' final sets like the others."""
    shape = smr.SHAPES[0]
    N, CS, r = shape
    jobs, twin = smr.jobs(*shape), smr.twin(*shape)
    S = 66000
    with engine(dash, N, CS, S) as eng:
        load_batch(eng, N, r)
        out = eng.shrink_many(jobs)
        check_against_twin(eng, out, jobs, twin, N, CS, systems=list(range(20)) + list(range(65530, 65560)) + [S - 1])


def test_step_cap_and_optional_outputs(dash):
    shape = smr.SHAPES[0]
    N, CS, r = shape
    jobs, twin = smr.jobs(*shape), smr.twin(*shape)
    with engine(dash, N, CS, 600) as eng:
        load_batch(eng, N, r)
        out = eng.shrink_many(jobs, cap=3)  # the first 3 winners of every job; rounds says how many there were
        for i, t in enumerate(twin):
            assert as_steps(out["steps"][i]) == t["steps"][:3] and int(out["results"]["rounds"][i]) == len(t["steps"])
            assert out["lens"][i].tolist() == t["lens"].tolist()
        assert max(len(t["steps"]) for t in twin) > 3
        # every output NULL
        load_batch(eng, N, r)
        rec = np.zeros(len(jobs), dash.SHRINK_JOB_DTYPE)
        for i, j in enumerate(jobs):
            rec[i] = j + (0,)
        assert dash.lib().dash_shrink_many(eng.h, rec.ctypes.data, len(jobs), None, 0, None, None, 0, None, None) == dash.OK
        got_tr, got_ln = eng.read_traces()
        for i, t in enumerate(twin):
            assert got_ln[i].tolist() == t["lens"].tolist() and np.array_equal(got_tr[i][:, :M], t["trace"])


def test_refusals(dash):
    shape = smr.SHAPES[0]
    N, CS, r = shape
    jobs, twin = smr.jobs(*shape), smr.twin(*shape)
    lib = dash.lib()

    def code(fn):
        with pytest.raises(dash.DashError) as e:
            fn()
        return e.value.code

    def raw(eng, rows, packed=None, stride=0, steps=None, step_cap=0, count=None):
        rec = np.zeros(max(len(rows), 1), dash.SHRINK_JOB_DTYPE)
        for i, j in enumerate(rows):
            rec[i] = tuple(j) + (0,)
        return lib.dash_shrink_many(eng.h, rec.ctypes.data, len(rows) if count is None else count,
                                    packed.ctypes.data if packed is not None else None, stride, None,
                                    steps.ctypes.data if steps is not None else None, step_cap, None, None)

    with engine(dash, N, CS, 50) as eng:
        assert code(lambda: eng.shrink_many(jobs)) == dash.ESTATE  # no traces loaded
        load_batch(eng, N, r)
        assert lib.dash_shrink_many(eng.h, None, 1, None, 0, None, None, 0, None, None) == dash.EINVAL  # jobs == NULL
        assert raw(eng, jobs, count=0) == dash.EINVAL
        assert raw(eng, [jobs[0]] * 51) == dash.EINVAL  # more jobs than systems
        assert raw(eng, jobs, count=dash.SHRINK_MAX_JOBS + 1) == dash.EINVAL
        assert code(lambda: eng.shrink_many(jobs[:2] + [(50, 0, 1, 0, 0)])) == dash.EINVAL  # a src out of range
        with pytest.raises(dash.DashError) as e:
            eng.shrink_many(jobs[:2] + [(1, 0, 0, 0, 0)])  # an empty goal
        assert e.value.code == dash.EINVAL and "job 2" in str(e.value)
        longest = int(smr.batch(N, r)[1].max())
        small = np.zeros((len(jobs), N, longest - 1), np.uint16)
        assert raw(eng, jobs, packed=small, stride=longest - 1) == dash.EINVAL and b"stride" in lib.dash_last_error(eng.h)
        assert raw(eng, jobs, step_cap=4) == dash.EINVAL  # steps == NULL with step_cap != 0
        # after the refusals the handle still works
        check_against_twin(eng, eng.shrink_many(jobs), jobs, twin, N, CS)
        eng.set_micro_schedule(np.full((4, N), dash.SIT_OUT, np.uint8))  # a micro-step table
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink_many(jobs)) == dash.ESTATE
    with dash.Engine(50, num_procs=N, cache_size=CS, max_instr=M, schedule_seed=1) as eng:  # no KEEP_STATE
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink_many(jobs)) == dash.ESTATE


# ---------------------------------------------------------------- the CLI

def cli(dash, *args, cwd):
    return subprocess.run([str(dash.PKG / "cache_simulator"), *map(str, args)], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def distinct_sets(results):
    return len({(tuple(t["lens"].tolist()), t["trace"].tobytes()) for t in results if t["status"] == smr.MINIMAL})


def job_lines(i, t, goal_bit, seed=None):
    tag = "source=%d" % i + ("" if seed is None else " seed=%d" % seed)
    return ["shrink %s node=%d start=%d count=%d candidates=%d" % ((tag,) + s) for s in t["steps"]] + \
        ["shrunk %s instr=%d->%d rounds=%d variants=%d bits=0x%X" % (tag, t["before"], int(t["lens"].sum()),
                                                                   len(t["steps"]), t["variants"], goal_bit)]


def check_dir(path, t, N):
    got_tr, got_ln = oc.load_test_dir(path, N, M)
    assert got_ln.tolist() == t["lens"].tolist() and np.array_equal(got_tr, t["trace"][:, :got_tr.shape[1]])


def test_cli_shrinks_many_directories(dash, tmp_path):
    """--shrink OUTDIR --sources LIST under lockstep: the 8 systems of (4,4,12) as directories; the coherent
    ones give no job. The single-directory form prints what it printed before."""
    N, CS, r = smr.SHAPES[0]
    packed, lens = smr.batch(N, r)
    for k in range(8):
        dash.write_dir(packed[k], lens[k], tmp_path / f"src{k}")
    (tmp_path / "list.txt").write_text("".join(f"{tmp_path}/src{k}\n" for k in range(1, 8)))
    twin = [smr.one(packed[k], lens[k], N, CS, (k, 0, (sr.outcome(packed[k], lens[k], N, CS, 0)[0] & -sr.outcome(
        packed[k], lens[k], N, CS, 0)[0]) or 1, 0, 0xFFFFFFFF)) for k in range(8)]
    p = cli(dash, tmp_path / "src0", "-m", M, "--shrink", tmp_path / "min", "--sources", tmp_path / "list.txt", cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    want, coherent = [], 0
    for k, t in enumerate(twin):
        if not t["bits"]:
            want.append("source %d: nothing to shrink (coherent)" % k)
            coherent += 1
    shrunk = [k for k, t in enumerate(twin) if t["bits"]]
    assert len(shrunk) >= 2 and coherent >= 1 and all(not twin[k]["errors"] for k in shrunk)
    for k in shrunk:
        want += job_lines(k, twin[k], twin[k]["bits"] & -twin[k]["bits"])
        check_dir(tmp_path / "min" / str(k), twin[k], N)
    want.append("shrunk sources=8 minimal=%d coherent=%d distinct=%d" % (
        len(shrunk), coherent, distinct_sets([twin[k] for k in shrunk])))
    assert p.stdout.splitlines() == want
    assert sorted(d.name for d in (tmp_path / "min").iterdir()) == sorted(str(k) for k in shrunk)
    # the single-directory form: its lines as before this call existed
    k = shrunk[0]
    q = cli(dash, tmp_path / f"src{k}", "-m", M, "--shrink", tmp_path / "one", cwd=tmp_path)
    assert q.returncode == 0, q.stderr
    t = twin[k]
    assert q.stdout.splitlines() == ["shrink node=%d start=%d count=%d candidates=%d" % s for s in t["steps"]] + [
        "shrunk instr=%d->%d rounds=%d variants=%d bits=0x%X" % (t["before"], int(t["lens"].sum()), len(t["steps"]),
                                                                t["variants"], t["bits"] & -t["bits"])]
    check_dir(tmp_path / "one", t, N)


def test_cli_shrinks_the_outcomes_of_an_explore(dash, tmp_path):
    """--explore K --coherence --shrink OUTDIR: one job per incoherent outcome, under its witness seed."""
    N, CS, r = smr.SHAPES[0]
    packed, lens = smr.batch(N, r)
    tr, ln = packed[3], lens[3]  # coherent under lockstep, incoherent under seed 5
    dash.write_dir(tr, ln, tmp_path / "src")
    K = 12
    p = cli(dash, tmp_path / "src", "-m", M, "--explore", K, "--coherence", "--shrink", tmp_path / "min", cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    plain = cli(dash, tmp_path / "src", "-m", M, "--explore", K, "--coherence", cwd=tmp_path)
    assert plain.returncode == 0 and lines[:len(plain.stdout.splitlines())] == plain.stdout.splitlines()
    outcomes = [ln_.split() for ln_ in plain.stdout.splitlines()]
    want, results = [], []
    for i, o in enumerate(outcomes):
        seed, errors, bits = int(o[2]), int(o[4], 16), int(o[5], 16)
        assert sr.outcome(tr, ln, N, CS, seed) == (bits, errors)
        if not bits:
            continue
        t = smr.one(tr, ln, N, CS, (0, seed, bits & -bits, 0, ~errors & 0xFFFFFFFF))
        assert t["status"] == smr.MINIMAL
        want += job_lines(i, t, bits & -bits, seed)
        check_dir(tmp_path / "min" / str(i), t, N)
        results.append(t)
    assert len(results) >= 2 and len(results) < len(outcomes)  # some outcome is coherent (lockstep, seed 0)
    want.append("shrunk sources=%d minimal=%d coherent=%d distinct=%d" % (
        len(outcomes), len(results), len(outcomes) - len(results), distinct_sets(results)))
    assert lines[len(outcomes):] == want
