"""The round loop of the built headline kernel keeps its cold blocks out of line (CPU only).

tools/hot_layout.py reads the disassembly of sim_kernel<8, 4, 16, 0> in the built library. The hot
span -- loop header to latch, what a wave fetches on the common path of a trip -- must hold no
inner loop (the REPLY_ID fan-out's two waterfall loops lie behind the latch) and no more
conditional branches than the committed report of this tree (profiles/r09/hot_layout_tree.json);
what is common stays inline: per round both arrival ORs, both ring-store regions and the arrival
exchange, per trip the trace refill's load.
"""
import json
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import hot_layout  # noqa: E402
import isa_table  # noqa: E402

LIB = ROOT / "ue22cs343bb1-openmp-assignment_amd" / "libdash.so"
R09 = ROOT / "profiles" / "r09"


@pytest.fixture(scope="module")
def built(dash):
    return hot_layout.report(str(LIB), isa_table.SYM)


@pytest.fixture(scope="module")
def committed():
    return json.loads((R09 / "hot_layout_tree.json").read_text())


def test_hot_span_holds_no_inner_loop(built):
    assert built["inner_loops"] == []
    assert built["conditional_by_kind"]["inner"] == 0


def test_no_more_conditional_branches_than_the_committed_report(built, committed):
    assert built["conditional_branches"] <= committed["conditional_branches"]
    assert built["hot_span"]["instructions"] <= committed["hot_span"]["instructions"]


def test_common_regions_stay_inline(built):
    mem = built["memory_ops"]
    r = built["rounds_per_trip"]
    assert mem["ds_or_b32"] == 2 * r        # primary and flush-copy arrival bits, every round
    assert mem["ds_wrxchg_rtn_b32"] == r    # the arrival exchange
    assert mem["global_load_dwordx2"] == 1  # the trace refill's next chunk
    # the skip branches that remain guard the exec-masked regions of the round (place, refill)
    skips = [b for b in built["branches"] if b["kind"] == "skip"]
    assert skips and all(b["op"] == "s_cbranch_execz" for b in skips)


def test_committed_reports_are_of_parent_and_tree(built, committed):
    parent = json.loads((R09 / "hot_layout_parent.json").read_text())
    assert committed["kernel_fingerprint"] == built["kernel_fingerprint"]
    assert parent["kernel_fingerprint"] != committed["kernel_fingerprint"]
    assert len(parent["inner_loops"]) == 2 * parent["rounds_per_trip"]
    assert parent["hot_span"]["instructions"] > committed["hot_span"]["instructions"]
