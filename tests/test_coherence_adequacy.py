"""The corpus of hand-built states (tests/coherence_states.py) that tests/test_gpu_coherence_states.py
gives to coherence_kernel is adequate: at every shape, every single-term slip of
tests/coherence_mutants.py changes the record (bits, addrs, first_addr, first_bits) of at least 3
corpus systems. 3 is a condition, not a measurement: one coincidence must not carry a term. A
(slip, shape) cell is exempt only with a stated proof (coherence_states.EXEMPT), and then no
candidate of a budget of 20,000 per shape tells it apart. No device call is made here.

The module also audits, without asserting, the inputs the GPU tests of coherence_kernel had before
this corpus: the final states of runs (test_audit_of_the_run_inputs prints the table that DESIGN.md
§5.2 holds). This shows that the corpus would catch these slips at each shape. It does not show that
no other slip exists."""
import pytest

import coherence_mutants as cm
import coherence_ref as cr
import coherence_states as cs


def kill_counts(states, N, CS, pristine=False):
    cnt = {m: 0 for m in cm.SLIPS}
    for nodes in states:
        init = cs.initial(N, CS) if pristine else None
        base = cm.check(nodes, N, CS, 0, pristine=init)[0]
        for m in cm.SLIPS:
            cnt[m] += cm.check(nodes, N, CS, m, pristine=init)[0] != base
    return cnt


def test_mutant_table_is_whole():
    assert sorted(cm.MUTANTS) == list(range(len(cm.MUTANTS))) and len(cm.SLIPS) >= 22
    assert all(m in cm.MUTANTS and shape in cs.SHAPES and why for (m, shape), why in cs.EXEMPT.items())


@pytest.mark.parametrize("N,CS", cs.SHAPES)
def test_every_slip_changes_three_records(N, CS):
    corpus = cs.corpus(N, CS)
    assert len(corpus) < 64
    cnt = kill_counts(corpus, N, CS)
    short = {m: cnt[m] for m in cm.SLIPS if (m, (N, CS)) not in cs.EXEMPT and cnt[m] < cs.NEED}
    assert not short, f"slips that change fewer than {cs.NEED} records at {(N, CS)}: {short}"
    assert not any(cnt[m] for m in cm.SLIPS if (m, (N, CS)) in cs.EXEMPT)
    # the hand-built states at every home lane are candidates of the cover, and the GPU test writes them too
    assert all(any(nodes[t] is not cs.initial(N, CS)[t] for nodes in cs.hand_built(N, CS)) for t in range(N))


@pytest.mark.parametrize("N,CS", cs.SHAPES)
def test_exempt_cells_within_a_budget(N, CS):
    """No candidate of the budget (other seeds than the pool's) gives an exempt slip another record."""
    exempt = tuple(m for m in cm.SLIPS if (m, (N, CS)) in cs.EXEMPT)
    if not exempt:
        assert N in (3, 5) and CS > 1  # the shapes with dead lanes and more than one line per node
        return
    told = set()
    for nodes in cs.candidates(N, CS, cs.BUDGET, seed=1) + cs.pool(N, CS):
        told |= cs.kills(nodes, N, CS, exempt)
    assert not told, f"exempt slips told apart at {(N, CS)}: {sorted(told)}"


@pytest.mark.parametrize("N,CS", cs.SHAPES)
def test_reference_twin_and_host_statement_agree(dash, N, CS):
    """Mutant 0 = coherence_ref = dash_check_states on every corpus state and hand-built state, and on
    the pool for the two Python statements; the twin's shortcut over untouched nodes changes nothing
    under any slip; the initial state is dash_init_node_state's."""
    init = cs.initial(N, CS)
    for t in range(N):
        want = dash.init_node_state(t, CS)
        assert all(list(getattr(want, f)) == getattr(init[t], f) for f in cs.Node.__slots__)
    for nodes in cs.pool(N, CS):
        assert cm.check(nodes, N, CS, 0, pristine=init) == cr.check(nodes, N, CS)
    for nodes in cs.corpus(N, CS) + cs.hand_built(N, CS):
        want, per = cr.check(nodes, N, CS)
        got, got_per = dash.check_states(nodes, N, CS)
        assert got == want and got_per.tolist() == per
        assert cm.check(nodes, N, CS, 0) == (want, per)
        for m in cm.SLIPS:
            assert cm.check(nodes, N, CS, m) == cm.check(nodes, N, CS, m, pristine=init), m


@pytest.mark.parametrize("N,CS", cs.SHAPES)
def test_corpus_states_survive_packing(N, CS):
    """dash_test_write_states keeps two bits of the state fields and a byte of the others: every
    corpus state is what dash_read_state gives back."""
    for nodes in cs.corpus(N, CS) + cs.hand_built(N, CS):
        assert len(nodes) == N
        for s in nodes:
            assert all(0 <= v <= 3 for v in s.dir_state + s.cache_state)
            assert all(0 <= v <= 255 for v in s.memory + s.dir_bitvector + s.cache_addr + s.cache_value)


def test_corpus_is_deterministic():
    """No fixture is committed: the corpus is generated where it is used, and twice the same."""
    N, CS = 5, 3
    first = [cs.state_key(n) for n in cs.corpus(N, CS)]
    cs.pool.cache_clear()
    cs.corpus.cache_clear()
    assert [cs.state_key(n) for n in cs.corpus(N, CS)] == first


# ---------------------------------------------------------------- audit of the inputs of runs

def audit():
    """{input set: (systems, {slip: records changed})} for the final states that
    tests/test_gpu_coherence.py and tests/test_gpu_launch_edges.py classify today, from the oracle."""
    import oracle_ctypes as oc
    import test_coherence_spec as spec
    from test_gpu_coherence import EXTRA, extra_batch
    from test_gpu_metrics import SHAPES

    out = {}
    for N, CS in SHAPES:
        out[f"SHAPES ({N}, {CS})"] = (N, CS, [list(r.node[:N]) for r in spec.shape_runs(N, CS)])
    for N, CS in EXTRA:
        packed, lens = extra_batch(N, CS)
        runs = [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS) for s in range(len(lens))]
        out[f"EXTRA ({N}, {CS})"] = (N, CS, [list(r.node[:N]) for r in runs])
    for test in ("test_3", "test_4"):
        out[f"{test}, 300 seeds"] = (4, 4, [list(r.node[:4]) for r in spec.seeded_runs(test)])
    return {name: (len(states), kill_counts(states, N, CS)) for name, (N, CS, states) in out.items()}


def test_audit_of_the_run_inputs():
    """Not an assertion about the kernel: which slips fewer than 3 systems of each present input set
    tell apart (run with -s to see the table)."""
    table = audit()
    print()
    for name, (n, cnt) in table.items():
        weak = {m: c for m, c in cnt.items() if c < cs.NEED}
        print(f"{name}: {n} systems; slips with fewer than {cs.NEED} records changed: "
              + (", ".join(f"{m} ({c})" for m, c in weak.items()) or "none"))
    assert set(table) and all(set(cnt) == set(cm.SLIPS) for _, cnt in table.values())
