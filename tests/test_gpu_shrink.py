"""dash_shrink (csrc/dash_shrink.hip, csrc/dash_shrink.cpp) on the GPU: one incoherent system cut down to
a 1-minimal trace set, every variant written, simulated, checked and ranked on the device.

The yardstick is the twin of tests/shrink_ref.py (the rule of include/dash.h over the CPU oracle and
tests/coherence_ref.py): steps, final traces and counts must be equal, not merely as small. The inputs
(shrink_ref.ROWS) and what they must exercise -- at least 8 rounds, winners of more than one instruction,
blocks that span a chunk boundary, start inside a chunk or make the kernel join two base chunks -- are
checked on the CPU in tests/test_shrink_spec.py.

Handle sizes: 50 systems (several sub-passes per round, a last sub-pass that is not full, a partial last
wave) and 600 (one sub-pass, more systems than candidates: the padding must not count); the lockstep rows
also on a handle created without a schedule seed, which runs the plain lockstep kernel."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import coherence_ref as cr
import oracle_ctypes as oc
import shrink_ref as sr
from oracle_ctypes import GOLDEN

pytestmark = pytest.mark.gpu
M = 40  # max_instr of the rows' batches


def engine(dash, N, CS, S, seeded=True, **kw):
    return dash.Engine(S, num_procs=N, cache_size=CS, max_instr=M, keep_state=True,
                       schedule_seed=1 if seeded else 0, **kw)


def load_batch(eng, N, r):
    """The row's batch of 8 systems in systems 0..7 of the handle; the others are empty."""
    from test_gpu_parity import random_batch
    packed, lens = random_batch(np.random.default_rng(r), 8, N, M, block_span=4, hot_frac=0.3)
    S = eng.num_systems
    tr, ln = np.zeros((S, N, M), np.uint16), np.zeros((S, N), np.uint32)
    tr[:8], ln[:8] = packed, lens
    eng.load_traces(tr, ln)


def check_against_twin(eng, out, twin, lens_before, N, CS, seed):
    """The call's results and the handle's state afterwards against the twin's (trace, lens, steps)."""
    tr, ln, steps = twin
    assert [tuple(int(x) for x in s) for s in out["steps"]] == steps
    assert out["lens"].tolist() == ln.tolist() and np.array_equal(out["trace"][:, :tr.shape[1]], tr)
    assert not out["trace"][:, tr.shape[1]:].any()
    rep = out["report"]
    assert (rep["rounds"], rep["instr_before"], rep["instr_after"]) == (len(steps), int(lens_before.sum()), int(ln.sum()))
    assert rep["variants"] == sr.variants_run(lens_before, steps)
    assert rep["passes"] >= rep["rounds"] + 3 and rep["sim_ms"] > 0 and rep["gen_ms"] > 0 and rep["select_ms"] > 0
    # the handle: the minimal set in its first and its last system, run and checked
    want = oc.run_system(tr, ln, num_procs=N, cache_size=CS, arb_seed=seed)
    got_tr, got_ln = eng.read_traces()
    dig, rnd, err = eng.read_results()
    rec = eng.read_coherence()
    for k in (0, eng.num_systems - 1):
        assert got_ln[k].tolist() == ln.tolist() and np.array_equal(got_tr[k][:, :tr.shape[1]], tr), k
        assert (int(dig[k]), int(rnd[k]), int(err[k])) == (want.digest, want.rounds, want.errors), k
        assert cr.record(rec[k]) == cr.check(want.node, N, CS)[0], k
    assert int(eng.read_results()[0][0]) == want.digest


# every row on a seeded handle of 50 and of 600 systems; the lockstep rows also on one without a seed
CASES = [(row, S, True) for row in sr.ROWS for S in (50, 600)] + [(row, 50, False) for row in sr.ROWS if row[3] == 0]


@pytest.mark.parametrize("row,S,seeded", CASES,
                         ids=["N%d-cs%d-r%d-seed%d-s%d%s" % (*c[0], c[1], "" if c[2] else "-unseeded") for c in CASES])
def test_shrink_equals_twin(dash, row, S, seeded):
    N, CS, r, seed = row
    k, _tr, lens, bits = sr.row_source(*row)
    with engine(dash, N, CS, S, seeded) as eng:
        load_batch(eng, N, r)
        out = eng.shrink(k, bits & -bits, seed=seed)
        check_against_twin(eng, out, sr.row_twin(*row), lens, N, CS, seed)
        # sub-passes: ceil(C / S) per round, plus the check of the source and the final run
        Cs = [c for _, _, _, c in sr.row_twin(*row)[2]] + [len(sr.candidates(out["lens"]))]
        assert out["report"]["passes"] == 2 + sum(-(-c // S) for c in Cs)
        # the result is a fixed point: shrinking it again takes no step and leaves it alone
        again = eng.shrink(eng.num_systems - 1, bits & -bits, seed=seed)
        assert len(again["steps"]) == 0 and np.array_equal(again["trace"], out["trace"])
        assert again["report"]["variants"] == Cs[-1] and again["report"]["instr_after"] == int(out["lens"].sum())


def test_goal_on_an_error_bit(dash):
    """err_all: a system that ends with DASH_ERR_OOB under seed 3, shrunk to the twin's result with the
    goal 'still DASH_ERR_OOB', whatever its coherence bits."""
    N, CS, r, seed = sr.OOB_ROW
    k, _tr, lens = sr.oob_source()
    with engine(dash, N, CS, 50) as eng:
        load_batch(eng, N, r)
        out = eng.shrink(k, 0, err_all=dash.ERR_OOB, err_none=0, seed=seed)
        check_against_twin(eng, out, sr.oob_twin(), lens, N, CS, seed)
        assert int(eng.read_results()[2][0]) & dash.ERR_OOB


def test_err_none_decides(dash):
    """The same source and bit with err_none = 0 may keep variants that pick up an error bit; with the
    default err_none it may not: both equal the twin under their own goal."""
    row = sr.ROWS[1]
    N, CS, r, seed = row
    k, tr, lens, bits = sr.row_source(*row)
    with engine(dash, N, CS, 50) as eng:
        load_batch(eng, N, r)
        out = eng.shrink(k, bits & -bits, err_none=0, seed=seed)
        check_against_twin(eng, out, sr.shrink(tr, lens, N, CS, seed, (bits & -bits, 0, 0)), lens, N, CS, seed)


def test_error_paths(dash):
    row = sr.ROWS[1]
    N, CS, r, seed = row
    k, _tr, lens, bits = sr.row_source(*row)
    bit = bits & -bits

    def code(fn):
        with pytest.raises(dash.DashError) as e:
            fn()
        return e.value.code

    with engine(dash, N, CS, 50) as eng:
        assert code(lambda: eng.shrink(k, bit)) == dash.ESTATE  # no traces loaded
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink(50, bit)) == dash.EINVAL  # src out of range
        assert code(lambda: eng.shrink(k, 0, err_all=0)) == dash.EINVAL  # an empty goal
        lib, goal = dash.lib(), dash.ShrinkGoal(bit, 0, 0xFFFFFFFF, 0)
        small = np.zeros((N, 8), np.uint16)
        assert int(lens.max()) > 8
        rc = lib.dash_shrink(eng.h, k, 0, goal, small.ctypes.data, 8, None, None, 0, None, None)
        assert rc == dash.EINVAL and b"stride" in lib.dash_last_error(eng.h)
        steps = np.zeros(4, dash.SHRINK_STEP_DTYPE)
        assert lib.dash_shrink(eng.h, k, 0, goal, None, 0, None, steps.ctypes.data, 4, None, None) == dash.EINVAL
        assert lib.dash_shrink(eng.h, k, 0, None, None, 0, None, None, 0, None, None) == dash.EINVAL
        # a source that does not meet the goal: a bit its record does not have, or an error bit it lacks
        missing = next(1 << b for b in range(8) if not bits >> b & 1)
        with pytest.raises(dash.DashError) as e:
            eng.shrink(k, missing)
        assert e.value.code == dash.EINVAL and "does not meet the goal" in str(e.value)
        # what include/dash.h promises of the refusal: the batch holds copies of the source, run and checked
        src = np.where(np.arange(M)[None, :] < lens[:, None], _tr, 0)  # zero past its lengths
        want = oc.run_system(_tr, lens, num_procs=N, cache_size=CS, arb_seed=seed)
        got_tr, got_ln = eng.read_traces()
        dig, rnd, err = eng.read_results()
        rec = eng.read_coherence()
        for s in (0, 49):
            assert got_ln[s].tolist() == lens.tolist() and np.array_equal(got_tr[s], src), s
            assert (int(dig[s]), int(rnd[s]), int(err[s])) == (want.digest, want.rounds, want.errors), s
            assert cr.record(rec[s]) == cr.check(want.node, N, CS)[0], s
        assert code(lambda: eng.shrink(k, bit, err_all=dash.ERR_OOB)) == dash.EINVAL
        # after the refusals the handle still shrinks (the refused calls left copies of the source behind)
        # cap smaller than the rounds: the first steps, and *n says how many there were
        twin = sr.row_twin(*row)
        out = eng.shrink(0, bit, cap=3)
        assert [tuple(int(x) for x in s) for s in out["steps"]] == twin[2][:3]
        assert out["report"]["rounds"] == len(twin[2]) > 3 and out["lens"].tolist() == twin[1].tolist()
        # all outputs optional
        load_batch(eng, N, r)
        n = ctypes.c_uint32()
        assert lib.dash_shrink(eng.h, k, 0, goal, None, 0, None, None, 0, ctypes.byref(n), None) == dash.OK
        assert n.value == len(twin[2])
        # a micro-step table
        eng.set_micro_schedule(np.full((4, N), dash.SIT_OUT, np.uint8))
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink(k, bit)) == dash.ESTATE
    with dash.Engine(50, num_procs=N, cache_size=CS, max_instr=M, schedule_seed=1) as eng:  # no KEEP_STATE
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink(k, bit)) == dash.ESTATE
    with engine(dash, N, CS, 50, seeded=False) as eng:
        load_batch(eng, N, r)
        assert code(lambda: eng.shrink(k, bit, seed=5)) == dash.ESTATE  # a seed on an unseeded handle


# ---------------------------------------------------------------- the CLI

def cli(dash, *args, cwd):
    return subprocess.run([str(dash.PKG / "cache_simulator"), *map(str, args)], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def test_cli_shrinks_a_directory(dash, tmp_path):
    row = sr.ROWS[1]  # (4, 4, 12, 0): the CLI's default node count and cache size, lockstep
    N, CS, _r, seed = row
    _k, tr, lens, bits = sr.row_source(*row)
    twin_tr, twin_ln, steps = sr.row_twin(*row)
    dash.write_dir(tr, lens, tmp_path / "src")
    p = cli(dash, tmp_path / "src", "-m", M, "--shrink", tmp_path / "min", cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert lines[:-1] == ["shrink node=%d start=%d count=%d candidates=%d" % s for s in steps]
    assert lines[-1] == "shrunk instr=%d->%d rounds=%d variants=%d bits=0x%X" % (
        lens.sum(), twin_ln.sum(), len(steps), sr.variants_run(lens, steps), bits & -bits)
    got_tr, got_ln = oc.load_test_dir(tmp_path / "min", N, M)
    assert got_ln.tolist() == twin_ln.tolist() and np.array_equal(got_tr, twin_tr[:, :got_tr.shape[1]])
    assert not list(tmp_path.glob("core_*_output.txt"))
    # the minimal directory still shows the bit
    q = cli(dash, tmp_path / "min", "-m", M, "--coherence", "-o", tmp_path, cwd=tmp_path)
    assert q.returncode == 0, q.stderr
    shown = int(re.search(r"coherence addrs=\d+ bits=0x([0-9A-F]+)", q.stdout)[1], 16)
    assert shown & bits & -bits
    # --shrink-bits: a bit the source does not have is refused, with the library's reason
    missing = next(1 << b for b in range(8) if not bits >> b & 1)
    bad = cli(dash, tmp_path / "src", "-m", M, "--shrink", tmp_path / "no", "--shrink-bits", hex(missing), cwd=tmp_path)
    assert bad.returncode != 0 and "does not meet the goal" in bad.stderr and not (tmp_path / "no").exists()
    # a coherent fixture
    ok = cli(dash, GOLDEN / "test_1", "--shrink", tmp_path / "none", cwd=tmp_path)
    assert ok.returncode == 0 and ok.stdout.splitlines()[-1] == "shrink: nothing to shrink (coherent)"
    assert not (tmp_path / "none").exists()
