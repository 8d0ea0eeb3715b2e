"""dash_shrink_many's rule on the CPU: dash_shrink_assign (the library's host form of the assignment)
against the twin of tests/shrink_many_ref.py, its refusals, the arithmetic the kernels share with the host
against a plain loop (tools/shrink_many_host_check.cpp, under the host sanitizers), and the inputs of
tests/test_gpu_shrink_many.py: they have the properties that file relies on. No device call is made here."""
import itertools
import os
import pathlib
import subprocess

import numpy as np
import pytest

import shrink_many_ref as smr

ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "ue22cs343bb1-openmp-assignment_amd"


# ---------------------------------------------------------------- the assignment

def test_assign_equals_twin_on_every_small_case(dash):
    """J <= 3 jobs with 0..5 candidates each, S <= 4 systems (S >= J), every sub-pass and system."""
    for J in (1, 2, 3):
        for cands in itertools.product(range(6), repeat=J):
            for S in range(J, 5):
                passes = -(-sum(cands) // S)
                for p in range(passes):
                    for k in range(S):
                        assert dash.shrink_assign(cands, S, p, k) == smr.assign(cands, S, p, k), (cands, S, p, k)
                counted = sum(dash.shrink_assign(cands, S, p, k)[2] for p in range(passes) for k in range(S))
                assert counted == sum(cands)
                with pytest.raises(dash.DashError):  # one sub-pass past the last
                    dash.shrink_assign(cands, S, passes, 0)


def test_assign_equals_twin_on_large_vectors(dash):
    """Random vectors of up to 5,000 jobs, most of them stopped in some, on handles up to 65,536 systems."""
    rng = np.random.default_rng(4)
    for it in range(10):
        J = int(rng.integers(1, 5001))
        cands = rng.integers(0, 70000, size=J)
        if it % 2:
            cands[rng.random(J) < 0.9] = 0
        cands[int(rng.integers(0, J))] = 65535
        S = int(rng.integers(J, 65537))
        passes = -(-int(cands.sum()) // S)
        for p in [0, passes - 1] + rng.integers(0, passes, size=6).tolist():
            for k in [0, S - 1] + rng.integers(0, S, size=12).tolist():
                assert dash.shrink_assign(cands, S, p, k) == smr.assign(cands, S, p, k), (it, p, k)


def test_assign_refusals(dash):
    lib = dash.lib()
    c = np.array([3, 0, 2], np.uint64)
    assert lib.dash_shrink_assign(c.ctypes.data, 3, 4, 0, 0, None, None, None) == dash.OK  # outputs are optional
    assert lib.dash_shrink_assign(None, 3, 4, 0, 0, None, None, None) == dash.EINVAL
    assert lib.dash_shrink_assign(c.ctypes.data, 0, 4, 0, 0, None, None, None) == dash.EINVAL
    assert lib.dash_shrink_assign(c.ctypes.data, 3, 2, 0, 0, None, None, None) == dash.EINVAL  # J above S
    assert lib.dash_shrink_assign(c.ctypes.data, 3, 4, 0, 4, None, None, None) == dash.EINVAL  # k >= S
    assert lib.dash_shrink_assign(c.ctypes.data, 3, 4, 2, 0, None, None, None) == dash.EINVAL  # ceil(5 / 4) == 2 sub-passes
    assert lib.dash_shrink_assign(c.ctypes.data, 3, 4, 1, 3, None, None, None) == dash.OK
    zero = np.zeros(3, np.uint64)
    assert lib.dash_shrink_assign(zero.ctypes.data, 3, 4, 0, 0, None, None, None) == dash.EINVAL  # T == 0: no sub-pass
    big = np.array([1 << 32], np.uint64)
    assert lib.dash_shrink_assign(big.ctypes.data, 1, 4, 0, 0, None, None, None) == dash.EINVAL
    many = np.ones(dash.SHRINK_MAX_JOBS + 1, np.uint64)
    assert lib.dash_shrink_assign(many.ctypes.data, len(many), 1 << 20, 0, 0, None, None, None) == dash.EINVAL
    assert dash.shrink_assign(many[:-1], 1 << 20, 0, 65535) == (65535, 0, True)
    assert dash.shrink_assign(many[:-1], 1 << 20, 0, 65536) == (0, 0, False)
    assert dash.shrink_assign([3, 0, 2], 4, 1, 2) == (2, 0, False) and dash.shrink_assign([3, 0, 2], 4, 1, 0) == (2, 1, True)


def test_assign_arithmetic_under_host_sanitizers(tmp_path):
    """csrc/dash_shrink.h's many_find_job and many_assign, compiled for the host into a stand-alone
    program with AddressSanitizer and UBSan, against a plain loop over the jobs."""
    rocm = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"  # hip_runtime.h, for uint2
    exe = tmp_path / "shrink_many_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", f"-I{rocm}", f"-I{PKG / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tools" / "shrink_many_host_check.cpp")], check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("shrink many host check ok"), p.stdout + p.stderr


# ---------------------------------------------------------------- the GPU tests' inputs

# per shape: MINIMAL jobs, UNMET coherent, UNMET with an error bit, the MINIMAL jobs' rounds, T of round 0, T of the last round
EXPECTED = {
    (4, 4, 12): (4, 6, 0, [12, 10, 8, 26], 705, 6),
    (8, 4, 11): (8, 0, 2, [17, 16, 18, 19, 15, 17, 17, 20], 2941, 14),
    (3, 1, 13): (7, 3, 0, [12, 9, 7, 10, 13, 15, 14], 1201, 6),
    (5, 16, 14): (5, 3, 2, [14, 15, 15, 12, 21], 1211, 35),
}


def shared_waves(row):
    """The waves of a sub-pass (64 consecutive global indices) that hold candidates of more than one job."""
    owner = [i for i, c in enumerate(row) for _ in range(c)]
    return [w for w in range(0, len(owner), 64) if len(set(owner[w:w + 64])) > 1]


@pytest.mark.parametrize("shape", smr.SHAPES)
def test_gpu_inputs_have_their_preconditions(shape):
    """What tests/test_gpu_shrink_many.py relies on, on the oracle: the statuses, the jobs' rounds and the
    rounds' totals of every shape; jobs that stop in different rounds; a round with T > 600 and a later round
    of one sub-pass on 600 systems in which some wave (64 consecutive systems) carries candidates of two or
    more jobs. (T < 64 with two or more active jobs, the plainest form of that, is asserted over the shapes
    below: (5,16,14) goes from T = 89 with three jobs to one job alone.)"""
    N, CS, r = shape
    res = smr.twin(N, CS, r)
    jobs = smr.jobs(N, CS, r)
    minimal = [x for x in res if x["status"] == smr.MINIMAL]
    unmet = [x for x in res if x["status"] == smr.UNMET]
    rounds = smr.round_cands(res)
    T = [sum(row) for row in rounds]
    got = (len(minimal), sum(1 for x in unmet if not x["bits"]), sum(1 for x in unmet if x["errors"]),
           [len(x["steps"]) for x in minimal], T[0], T[-1])
    assert got == EXPECTED[shape]
    for x, j in zip(res, jobs):  # an UNMET job is coherent (its goal is bit 1) or has an error bit, never both kinds of miss
        assert (x["status"] == smr.UNMET) == (not x["bits"] or bool(x["errors"]))
        assert j[2] == ((x["bits"] & -x["bits"]) or 1)
    assert len({len(x["steps"]) for x in minimal}) >= 2
    assert len(rounds) == max(len(x["steps"]) for x in minimal) + 1
    assert any(t > 600 for t in T)
    late = [i for i, row in enumerate(rounds) if sum(row) <= 600 and shared_waves(row)]
    assert late and max(late) > min(i for i, t in enumerate(T) if t > 600)


def test_the_same_traces_under_two_seeds():
    """(4,4,12): system 3 is coherent under lockstep and shrinks under seed 5; system 0 is a job twice."""
    N, CS, r = smr.SHAPES[0]
    jobs, res = smr.jobs(N, CS, r), smr.twin(N, CS, r)
    assert jobs[3][:2] == (3, 5) and jobs[9][:2] == (3, 0)
    assert res[3]["status"] == smr.MINIMAL and res[3]["steps"] and res[9]["status"] == smr.UNMET and not res[9]["bits"]
    assert jobs[0][:2] == (0, 0) and jobs[8][:2] == (0, 5)
    small = [s for s in smr.SHAPES
             if any(sum(row) < 64 and sum(1 for c in row if c) >= 2 for row in smr.round_cands(smr.twin(*s)))]
    assert len(small) >= 3  # a round with T < 64 and two or more jobs still active
    over_shapes = [x["status"] for s in smr.SHAPES for x in smr.twin(*s)]
    assert smr.MINIMAL in over_shapes and smr.UNMET in over_shapes
