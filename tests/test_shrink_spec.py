"""dash_shrink's rule on the CPU: dash_shrink_candidate (the library's host form of the enumeration)
against the twin of tests/shrink_ref.py, dash_write_dir against dash_parse_core_file, the chunk arithmetic
of the variant kernel against a plain deletion (tools/shrink_host_check.cpp, under the host sanitizers),
and the twin itself: its results are 1-minimal on the oracle, and the inputs of tests/test_gpu_shrink.py
have the properties that file relies on. No device call is made here."""
import itertools
import os
import pathlib
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
import shrink_ref as sr

ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "ue22cs343bb1-openmp-assignment_amd"


def library_candidates(dash, lens):
    C = dash.shrink_candidate(lens, 0)[0]
    return [dash.shrink_candidate(lens, c)[1:] for c in range(C)], C


# ---------------------------------------------------------------- the enumeration

def test_candidate_equals_twin_on_every_small_base(dash):
    """Every lens vector of 1..3 nodes with lengths 0..9."""
    for n in (1, 2, 3):
        for lens in itertools.product(range(10), repeat=n):
            got, C = library_candidates(dash, lens)
            want = sr.candidates(lens)
            assert C == len(want) and got == want, lens


def test_candidate_equals_twin_on_large_bases(dash):
    """Random vectors up to 8 x 4,096: the count, and 200 random indices with the first and the last."""
    rng = np.random.default_rng(1)
    for _ in range(12):
        lens = rng.integers(0, 4097, size=int(rng.integers(1, 9)))
        lens[int(rng.integers(0, len(lens)))] = 4096
        want = sr.candidates(lens)
        for c in [0, len(want) - 1] + rng.integers(0, len(want), size=200).tolist():
            assert dash.shrink_candidate(lens, c) == (len(want),) + want[c], (lens.tolist(), c)


def test_candidate_counts_and_refusals(dash):
    lib = dash.lib()
    assert dash.shrink_candidate([0, 0, 0], 0) == (0, None, None, None)
    assert dash.shrink_candidate([0], 17)[0] == 0  # C == 0 whatever c is
    # one node of length L: sum over j <= J of ceil(L / 2^j); 5 -> 1 + 2 + 3 + 5
    assert dash.shrink_candidate([5], 0)[0] == 11 and dash.shrink_candidate([1], 0) == (1, 0, 0, 1)
    assert dash.shrink_candidate([4096] * 8, 0)[0] == 8 * 8191  # 4096 + 2048 + ... + 1 per node
    for lens in ([5], [3, 0, 9], [4096] * 8):
        C = dash.shrink_candidate(lens, 0)[0]
        assert dash.shrink_candidate(lens, C - 1)[0] == C
        for c in (C, C + 1, 1 << 40):
            with pytest.raises(dash.DashError) as e:
                dash.shrink_candidate(lens, c)
            assert e.value.code == dash.EINVAL
    arr = np.array([3, 3], np.uint32)
    assert lib.dash_shrink_candidate(None, 2, 0, None, None, None) == dash.EINVAL
    assert lib.dash_shrink_candidate(arr.ctypes.data, 0, 0, None, None, None) == dash.EINVAL
    assert lib.dash_shrink_candidate(arr.ctypes.data, 9, 0, None, None, None) == dash.EINVAL
    assert lib.dash_shrink_candidate(arr.ctypes.data, 2, 0, None, None, None) == 12  # outputs are optional
    big = np.array([(1 << 24) + 1], np.uint32)
    assert lib.dash_shrink_candidate(big.ctypes.data, 1, 0, None, None, None) == dash.EINVAL


def test_every_single_deletion_once_at_level_0(dash):
    rng = np.random.default_rng(2)
    for lens in [[1], [2], [7, 0, 8], [9, 16, 17]] + [rng.integers(0, 40, size=5).tolist() for _ in range(6)]:
        got, _ = library_candidates(dash, lens)
        # level 0 is the last lens[t] candidates of node t: every single deletion, once, in order (a
        # clipped last block of a higher level may delete one instruction too: that is another candidate)
        for t, L in enumerate(lens):
            mine = [(s, n) for tt, s, n in got if tt == t]
            assert mine[len(mine) - L:] == [(s, 1) for s in range(L)]
            J = max(L - 1, 0).bit_length()
            assert len(mine) == sum(-(-L // 2 ** j) for j in range(J + 1)) * (L > 0)


# ---------------------------------------------------------------- dash_write_dir

def test_write_dir_round_trips_through_the_parser(dash, tmp_path):
    """Random words, a node of length 0 and a node of max_instr lines; an RD's value bits are not written."""
    rng = np.random.default_rng(3)
    M = 32
    tr = rng.integers(0, 1 << 16, size=(4, M)).astype(np.uint16) & np.uint16(0xBFFF)  # homes 0..3
    lens = np.array([M, 0, 17, 1], np.uint32)
    dash.write_dir(tr, lens, tmp_path / "out")
    want = np.where(tr & 0x8000, tr, tr & 0xFF00).astype(np.uint16)
    for t in range(4):
        got = dash.parse_core_file(tmp_path / "out" / f"core_{t}.txt", 4, M)
        assert got.tolist() == want[t, :lens[t]].tolist(), t
    assert (tmp_path / "out" / "core_1.txt").read_bytes() == b""
    # the fixtures' spelling, and a second write into the existing directory
    one = np.array([[oc.pack("R", 0x3C, 0), oc.pack("W", 0x00, 110)]], np.uint16)
    dash.write_dir(one, [2], tmp_path / "out")
    assert (tmp_path / "out" / "core_0.txt").read_text() == "RD 0x3C\nWR 0x00 110\n"
    # a golden directory written back byte for byte
    gtr, glens = oc.load_test_dir(oc.GOLDEN / "test_3")
    dash.write_dir(gtr, glens, tmp_path / "g")
    for t in range(4):
        assert (tmp_path / "g" / f"core_{t}.txt").read_bytes() == (oc.GOLDEN / "test_3" / f"core_{t}.txt").read_bytes()
    with pytest.raises(dash.DashError) as e:
        dash.write_dir(one, [3], tmp_path / "out")  # a length above the stride
    assert e.value.code == dash.EINVAL
    with pytest.raises(dash.DashError) as e:
        dash.write_dir(one, [2], tmp_path / "missing" / "out")
    assert e.value.code == dash.EIO


# ---------------------------------------------------------------- the kernel's chunk arithmetic

def test_chunk_arithmetic_under_host_sanitizers(tmp_path):
    """csrc/dash_shrink.h's shrink_decode and variant_chunk, compiled for the host into a stand-alone
    program with AddressSanitizer and UBSan, against a plain deletion."""
    rocm = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"  # hip_runtime.h, for uint2
    exe = tmp_path / "shrink_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", f"-I{rocm}", f"-I{PKG / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tools" / "shrink_host_check.cpp")], check=True, capture_output=True, text=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("shrink host check ok"), p.stdout + p.stderr


# ---------------------------------------------------------------- the twin, and the GPU tests' inputs

@pytest.mark.parametrize("row", sr.ROWS + (sr.OOB_ROW,))
def test_twin_result_is_one_minimal(row):
    """The source meets the goal, the result meets it, and every single deletion from the result breaks it:
    each re-run on the oracle."""
    N, CS, r, seed = row
    if row == sr.OOB_ROW:
        (_k, tr0, ln0), goal = sr.oob_source(), sr.ERR_OOB_GOAL
    else:
        _k, tr0, ln0, bits = sr.row_source(*row)
        goal = (bits & -bits, 0, 0xFFFFFFFF)
    tr, ln, steps = sr.shrink(tr0, ln0, N, CS, seed, goal)
    assert sr.passes(*sr.outcome(tr0, ln0, N, CS, seed), goal) and sr.passes(*sr.outcome(tr, ln, N, CS, seed), goal)
    assert int(ln.sum()) == int(ln0.sum()) - sum(s[2] for s in steps) and int(ln.sum()) > 0
    for t in range(N):
        assert not tr[t, int(ln[t]):].any()
        for s in range(int(ln[t])):
            assert not sr.passes(*sr.outcome(*sr.delete(tr, ln, t, s, 1), N, CS, seed), goal), (t, s)


def test_gpu_inputs_have_their_preconditions():
    """What tests/test_gpu_shrink.py relies on: per row the source is incoherent with errors == 0, the twin
    takes at least 8 rounds and some winner deletes more than one instruction; over the rows some winning
    block spans a chunk boundary (four instructions per chunk), one is not aligned to 4 instructions, one
    makes the kernel join two base chunks and one starts inside a chunk."""
    spans = unaligned = joins = cuts = 0
    for row in sr.ROWS:
        N, CS, _r, seed = row
        _k, tr, ln, bits = sr.row_source(*row)
        assert bits and sr.outcome(tr, ln, N, CS, seed) == (bits, 0)
        _t, _l, steps = sr.row_twin(*row)
        assert len(steps) >= 8 and any(n > 1 for _, _, n, _ in steps)
        left = [int(x) for x in ln]
        for t, s, n, _ in steps:
            after = left[t] - (s + n)  # instructions that move down
            spans += s // 4 != (s + n - 1) // 4
            unaligned += bool(s % 4 or n % 4)
            joins += n % 4 != 0 and after >= 4  # a later chunk is joined from two base chunks
            cuts += s % 4 != 0 and after > 0    # the block starts inside a chunk that keeps its low words
            left[t] -= n
    assert spans and unaligned and joins and cuts
    assert sr.outcome(*sr.oob_source()[1:], *sr.OOB_ROW[:2], sr.OOB_ROW[3])[1] & oc.ERR_OOB
    assert len(sr.oob_twin()[2]) >= 8
