"""The coherence invariants of final states on the CPU: the definitions of include/dash.h pinned on
hand-built states (tests/coherence_ref.py, the plain-Python reference, and dash_check_states, the
library's host statement, against the expected bits), the committed reference dumps, the
preconditions the GPU tests of tests/test_gpu_coherence.py rely on, and dash_check_states against
the reference on oracle states and on random ones. No device call is made here."""
import functools

import numpy as np
import pytest

import coherence_ref as cr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN
from test_gpu_metrics import NSYS, SHAPES, batch

DUMPS = ["sample", "test_1", "test_2", "test_3/run_1", "test_3/run_2", "test_4/run_1", "test_4/run_2",
         "test_4/run_3", "test_4/run_4"]
SEEDS = 300
CLEAN = {"bits": 0, "addrs": 0, "first_addr": cr.NONE, "first_bits": 0}


# ---------------------------------------------------------------- the inputs of the GPU tests

@functools.lru_cache(maxsize=None)
def shape_runs(N, CS):
    """The oracle's lockstep runs of the 13 systems of a SHAPES batch."""
    packed, lens = batch(N, CS)
    return [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS) for s in range(NSYS)]


@functools.lru_cache(maxsize=None)
def seeded_runs(test):
    """The oracle's runs of a reference fixture under the seeded schedules 0 .. SEEDS - 1."""
    tr, lens = oc.load_test_dir(GOLDEN / test)
    return [oc.run_system(tr, lens, arb_seed=seed) for seed in range(SEEDS)]


def ref_record(res, N, CS):
    return cr.check(res.node, N, CS)[0]


# ---------------------------------------------------------------- hand-built states

def fresh(dash, N=4, CS=4):
    return [dash.init_node_state(t, CS) for t in range(N)]


def line(node, i, addr, value, state):
    node.cache_addr[i], node.cache_value[i], node.cache_state[i] = addr, value, state


def entry(nodes, addr, d, bv, mem=None):
    home, block = addr >> 4, addr & 15
    nodes[home].dir_state[block], nodes[home].dir_bitvector[block] = d, bv
    if mem is not None:
        nodes[home].memory[block] = mem


def both(dash, nodes, N=4, CS=4):
    """The record and per-address bits of the reference, after checking that dash_check_states
    gives the same."""
    want, per = cr.check(nodes, N, CS)
    got, got_per = dash.check_states(nodes, N, CS)
    assert got == want and got_per.tolist() == per
    return want, per


A = 0x25  # home 2, block 5: initial memory 20 * 2 + 5 = 45


def test_initial_state_is_clean(dash):
    for N, CS in ((4, 4), (8, 16), (1, 1), (5, 3)):
        rec, per = both(dash, fresh(dash, N, CS), N, CS)
        assert rec == CLEAN and per == [0] * (N * 16)


def single_bit_states(dash):
    """bit -> a minimal state that sets it (on address A)."""
    out = {}
    # a MODIFIED and a SHARED copy. Under EM, S or U the directory's own bit would come with it
    # (n >= 2 breaks EM, an owner breaks S, any copy breaks U), so the entry holds the fourth value
    # of its two bits, which is none of them; d != U, so the holders must match
    s = fresh(dash)
    line(s[0], 0, A, 7, cr.MODIFIED)
    line(s[1], 0, A, 7, cr.SHARED)
    entry(s, A, 3, 0b0011, mem=7)
    out[cr.SWMR] = s
    s = fresh(dash)
    line(s[1], 2, A, 45, cr.SHARED)
    out[cr.DIR_U_HELD] = s
    s = fresh(dash)
    entry(s, A, cr.EM, 0)
    out[cr.DIR_EM] = s
    s = fresh(dash)
    entry(s, A, cr.S, 0)
    out[cr.DIR_S] = s
    s = fresh(dash)
    line(s[1], 0, A, 45, cr.SHARED)
    line(s[2], 3, A, 45, cr.SHARED)
    entry(s, A, cr.S, 0b0010)
    out[cr.LOST_SHARER] = s
    s = fresh(dash)
    line(s[1], 0, A, 45, cr.SHARED)
    entry(s, A, cr.S, 0b0110)
    out[cr.STALE_SHARER] = s
    s = fresh(dash)
    line(s[1], 0, A, 46, cr.SHARED)
    entry(s, A, cr.S, 0b0010)
    out[cr.STALE_VALUE] = s
    return out


@pytest.mark.parametrize("bit", [cr.SWMR, cr.DIR_U_HELD, cr.DIR_EM, cr.DIR_S, cr.LOST_SHARER, cr.STALE_SHARER,
                                 cr.STALE_VALUE])
def test_each_bit_alone(dash, bit):
    rec, per = both(dash, single_bit_states(dash)[bit])
    assert rec == {"bits": bit, "addrs": 1, "first_addr": A, "first_bits": bit}
    assert per[A] == bit and sum(1 for b in per if b) == 1


def test_value_split_and_its_smallest_companions(dash):
    """VALUE_SPLIT cannot stand alone: copies that differ without STALE_VALUE hold at most one SHARED
    or EXCLUSIVE value (the memory's), so one of them is MODIFIED, and an owner among n >= 2 copies is
    SWMR. Its two minimal states: with SWMR alone, and with STALE_VALUE alone."""
    s = fresh(dash)
    line(s[0], 0, A, 8, cr.MODIFIED)
    line(s[1], 0, A, 7, cr.SHARED)
    entry(s, A, 3, 0b0011, mem=7)
    assert both(dash, s)[0] == {"bits": cr.SWMR | cr.VALUE_SPLIT, "addrs": 1, "first_addr": A,
                                "first_bits": cr.SWMR | cr.VALUE_SPLIT}
    s = fresh(dash)
    line(s[0], 0, A, 45, cr.SHARED)
    line(s[1], 0, A, 44, cr.SHARED)
    entry(s, A, cr.S, 0b0011)
    assert both(dash, s)[0]["bits"] == cr.STALE_VALUE | cr.VALUE_SPLIT
    # the same two lines with equal values: nothing
    line(s[1], 0, A, 45, cr.SHARED)
    assert both(dash, s)[0] == CLEAN


def test_invalid_and_foreign_lines_never_count(dash):
    s = fresh(dash)
    line(s[1], 0, A, 99, cr.INVALID)    # would be DIR_U_HELD and STALE_VALUE if it counted
    line(s[2], 1, 0xFF, 3, cr.MODIFIED)  # the initial address with a valid state
    line(s[3], 1, 0x45, 3, cr.MODIFIED)  # homed on node 4 of a 4-node system
    assert both(dash, s)[0] == CLEAN
    s = fresh(dash, 8, 2)
    line(s[7], 1, 0xFF, 3, cr.EXCLUSIVE)
    line(s[0], 0, 0x80, 3, cr.EXCLUSIVE)
    assert both(dash, s, 8, 2)[0] == CLEAN
    # a line past cache_size is not a line
    s = fresh(dash, 4, 2)
    line(s[1], 2, A, 99, cr.SHARED)
    assert both(dash, s, 4, 2)[0] == CLEAN


def test_bitvector_bit_at_or_above_num_procs_is_a_stale_sharer(dash):
    s = fresh(dash)
    line(s[1], 0, A, 45, cr.SHARED)
    entry(s, A, cr.S, 0b0010)
    assert both(dash, s)[0] == CLEAN
    entry(s, A, cr.S, 0b100010)  # node 5 of a 4-node system
    assert both(dash, s)[0]["bits"] == cr.STALE_SHARER


def test_two_lines_of_one_node_are_two_copies(dash):
    s = fresh(dash)
    line(s[1], 0, A, 9, cr.EXCLUSIVE)
    entry(s, A, cr.EM, 0b0010, mem=9)
    assert both(dash, s)[0] == CLEAN
    line(s[1], 3, A, 9, cr.EXCLUSIVE)  # the same address again, elsewhere in the same cache
    assert both(dash, s)[0]["bits"] == cr.SWMR | cr.DIR_EM


def test_first_addr_is_the_lowest_address(dash):
    s = fresh(dash)
    line(s[0], 0, 0x25, 45, cr.SHARED)  # node 0 holds the higher address: DIR_U_HELD at 0x25
    line(s[3], 0, 0x13, 0, cr.SHARED)   # node 3 the lower one: DIR_U_HELD and STALE_VALUE at 0x13
    rec, per = both(dash, s)
    assert rec == {"bits": cr.DIR_U_HELD | cr.STALE_VALUE, "addrs": 2, "first_addr": 0x13,
                   "first_bits": cr.DIR_U_HELD | cr.STALE_VALUE}
    assert per[0x25] == cr.DIR_U_HELD


# ---------------------------------------------------------------- committed dumps, corpus

@pytest.mark.parametrize("run", DUMPS)
def test_committed_reference_dumps_are_clean(dash, run):
    nodes = [oc.parse_dump((GOLDEN / run / f"core_{n}_output.txt").read_text(), n) for n in range(4)]
    assert both(dash, nodes)[0] == CLEAN


def test_shapes_batches_hold_clean_and_violating_systems():
    """What tests/test_gpu_coherence.py::test_shapes relies on: under lockstep every batch has clean
    and violating systems, none with an error bit, and together they show all eight bits."""
    union = 0
    for N, CS in SHAPES:
        runs = shape_runs(N, CS)
        bits = [ref_record(r, N, CS)["bits"] for r in runs]
        assert any(bits) and not all(bits), (N, CS)
        assert all(r.errors == 0 for r in runs), (N, CS)
        assert bits[0] == 0  # the system without instructions
        for b in bits:
            union |= b
    assert union == 0xFF


def test_seeded_fixtures_hold_what_the_explore_test_needs():
    bad = [r for r in seeded_runs("test_3") if ref_record(r, 4, 4)["bits"]]
    assert any(r.errors == 0 for r in bad)
    assert not any(ref_record(r, 4, 4)["bits"] for r in seeded_runs("test_4"))


# ---------------------------------------------------------------- dash_check_states

def test_check_states_equals_the_reference_on_oracle_states(dash):
    for N, CS in SHAPES:
        for r in shape_runs(N, CS):
            both(dash, list(r.node[:N]), N, CS)
    for test in ("test_3", "test_4"):
        for r in seeded_runs(test):
            both(dash, list(r.node[:4]))


def test_check_states_equals_the_reference_on_random_states(dash):
    """2,000 states of uniform random bytes in every field, the two state fields masked to their two
    bits, at random shapes: directory values and addresses no run produces included."""
    rng = np.random.default_rng(20)
    union = 0
    for _ in range(2000):
        N, CS = int(rng.integers(1, 9)), int(rng.integers(1, 17))
        nodes = []
        for t in range(N):
            s = dash.NodeState()
            for name, _ in dash.NodeState._fields_:
                arr = getattr(s, name)
                raw = rng.integers(0, 256, len(arr), dtype=np.uint8)
                if name in ("dir_state", "cache_state"):
                    raw &= 3
                arr[:] = raw.tolist()
            nodes.append(s)
        union |= both(dash, nodes, N, CS)[0]["bits"]
    assert union == 0xFF


@pytest.mark.parametrize("N,CS", [(0, 4), (9, 4), (4, 0), (4, 17)])
def test_check_states_refuses_shapes_outside_the_contract(dash, N, CS):
    with pytest.raises(dash.DashError) as e:
        dash.check_states([dash.init_node_state(t, 4) for t in range(8)], N, CS)
    assert e.value.code == dash.EINVAL
