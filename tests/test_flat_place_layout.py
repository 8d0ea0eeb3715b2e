"""The ring stores of the built headline kernel carry no skip branch (CPU only).

tools/hot_layout.py reads the disassembly of sim_kernel<8, 4, 16, 0> in the built library. Below the
final tier the kernel reads and ranks both receivers' slots in every lane (DASH_FLAT_PLACE), so each
ring store's exec-masked region holds the LDS write alone and needs no s_cbranch_execz over it: the
one skip left in the hot span is the trace refill's. The out-of-line tests (two rare tests per round,
round cap, overflow stop, refill threshold) stay, the latch stays, nothing loops inside the span.
"""
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import hot_layout  # noqa: E402
import isa_table  # noqa: E402

LIB = ROOT / "ue22cs343bb1-openmp-assignment_amd" / "libdash.so"


@pytest.fixture(scope="module")
def built(dash):
    return hot_layout.report(str(LIB), isa_table.SYM)


def test_one_skip_branch_in_the_hot_span(built):
    skips = [b for b in built["branches"] if b["kind"] == "skip"]
    assert len(skips) == 1 and skips[0]["op"] == "s_cbranch_execz"  # the refill's
    assert built["conditional_by_kind"]["skip"] == 1


def test_at_most_twelve_conditional_branches_besides_the_latch(built):
    kinds = built["conditional_by_kind"]
    assert kinds["latch"] == 1
    assert built["conditional_branches"] - kinds["latch"] <= 12


def test_no_inner_loop(built):
    assert built["inner_loops"] == [] and built["conditional_by_kind"]["inner"] == 0


def test_delivery_operations_per_trip(built):
    mem, r = built["memory_ops"], built["rounds_per_trip"]
    assert r == 4
    assert mem["ds_or_b32"] == 2 * r          # primary and flush-copy arrival bits
    assert mem["ds_wrxchg_rtn_b32"] == r      # the arrival exchange
    # (mask, tail) of the primary's and of the flush copy's receiver, every round, in the span
    assert mem["ds_read2_b32"] >= 2 * r
