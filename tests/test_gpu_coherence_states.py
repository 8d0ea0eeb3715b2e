"""coherence_kernel (csrc/dash_coherence.hip) on states it is given, not on the states runs leave:
the corpus of tests/coherence_states.py -- every slip of tests/coherence_mutants.py changes at least 3
of its records at every shape (tests/test_coherence_adequacy.py) -- and the hand-built states of
tests/test_coherence_spec.py at every home lane, written with dash_test_write_states. Every record is
compared with tests/coherence_ref.py on the state written, the totals with the records, and
read_state with the state.

The handles are a few systems larger than the states (the padding keeps the states of the run, and is
checked against read_state): at least two waves, the last one partial. A third of the systems have no
instruction; the others stop at a round cap of 4 with DASH_ERR_ROUNDCAP, so violating_clean_systems
differs from violating_systems."""
import functools

import numpy as np
import pytest

import coherence_mutants as cm
import coherence_ref as cr
import coherence_states as cs
from test_gpu_parity import random_batch

pytestmark = pytest.mark.gpu
LEN = 8


@functools.lru_cache(maxsize=None)
def states_of(N, CS):
    return cs.corpus(N, CS) + cs.hand_built(N, CS)


@functools.lru_cache(maxsize=None)
def expected(N, CS):
    """The reference on every state of the shape: computed once, shared by the cases."""
    return [cr.check(nodes, N, CS) for nodes in states_of(N, CS)]


def batch_size(N, count, pad=2):
    """count + pad or more systems: at least two waves, the last one partial."""
    spw = 64 // cm.next_pow2(N)
    nsys = max(count + pad, spw + 1)
    return nsys + 1 if nsys % spw == 0 else nsys


def ran_engine(dash, nsys, N, CS, **kw):
    """A handle that has run: every third system empty (clean), the others cut at the round cap."""
    packed, lens = random_batch(np.random.default_rng(100 * N + CS), nsys, N, LEN, block_span=4, hot_frac=0.3,
                                fixed_len=True)
    lens[::3] = 0
    packed[::3] = 0
    eng = dash.Engine(nsys, num_procs=N, cache_size=CS, max_instr=LEN, keep_state=True, max_rounds=4, **kw)
    eng.load_traces(packed, lens)
    eng.run()
    errors = eng.read_results()[2]
    assert (errors[::3] == 0).all() and (np.delete(errors, np.s_[::3]) & dash.ERR_ROUNDCAP).all()
    return eng


def same_state(got, want, CS):
    return all(list(getattr(g, f)) == list(getattr(w, f)) for g, w in zip(got, want) for f in cs.Node.__slots__)


def check_batch(eng, want):
    """check_coherence on the handle: every record against want[s] = (record, per-address bits), the
    totals against the records and the run's error words. Returns (totals, records)."""
    tot = eng.check_coherence()
    rec = eng.read_coherence()
    for s in range(eng.num_systems):
        assert cr.record(rec[s]) == want[s][0], (s, cr.record(rec[s]), want[s][0])
    errors = eng.read_results()[2]
    bad = rec["bits"] != 0
    assert tot == {"systems": eng.num_systems, "violating_systems": int(bad.sum()),
                   "violating_clean_systems": int((bad & (errors == 0)).sum()), "addrs": int(rec["addrs"].sum()),
                   "bit_systems": [int(((rec["bits"] >> k) & 1).sum()) for k in range(8)],
                   "bit_addrs": [sum((b >> k) & 1 for _, per in want for b in per) for k in range(8)]}
    return tot, rec


def written(eng, first, states, want_states):
    """write_states, and what the whole batch should now hold: (record, per) per system."""
    N, CS = eng.num_procs, eng.cache_size
    eng.write_states(first, states)
    for k, nodes in enumerate(states):
        assert same_state(eng.read_state(first + k), nodes, CS), first + k
    return [want_states[s - first] if first <= s < first + len(states)
            else cr.check(eng.read_state(s), N, CS) for s in range(eng.num_systems)]


@pytest.mark.parametrize("N,CS", cs.SHAPES)
def test_corpus(dash, N, CS):
    """The states at systems 0 .., then rotated by one system: every state meets another lane segment
    of its wave, and the neighbours of every state change."""
    states, want_states = states_of(N, CS), expected(N, CS)
    nsys = batch_size(N, len(states))
    with ran_engine(dash, nsys, N, CS) as eng:
        want = written(eng, 0, states, want_states)
        tot, rec = check_batch(eng, want)
        assert 0 < tot["violating_clean_systems"] < tot["violating_systems"] < nsys
        assert sum(1 for k in range(8) if tot["bit_systems"][k]) == 8 or N * CS == 1
        want = written(eng, 1, states, want_states)
        tot1, rec1 = check_batch(eng, want)
        assert np.array_equal(rec1[1:len(states) + 1], rec[:len(states)])


def test_walk_of_several_trips(dash):
    """(8, 4) under DASH_TEST_ONE_GROUP: one workgroup walks the states in several trips of 32 systems
    and gives the records and totals of the device-sized grid."""
    N, CS = 8, 4
    states, want_states = states_of(N, CS), expected(N, CS)
    nsys = batch_size(N, len(states))
    assert nsys > 3 * 32
    got = []
    for flags in (dash.TEST_ONE_GROUP, 0):
        with ran_engine(dash, nsys, N, CS, flags=flags) as eng:
            got.append(check_batch(eng, written(eng, 0, states, want_states)))
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("nsys", [21, 22, 23])
def test_tail_chunk_carries_a_verdict(dash, nsys):
    """(5, 1): a system is 85 words, so the buffer ends 1, 2 or 3 words into a 16-B chunk, which the
    last wave loads word by word. The last word is the last system's last node's line: that line alone
    makes the system violate."""
    N, CS = 5, 1
    assert nsys * N * (16 + CS) % 4 == nsys % 4 != 0
    b = cs.Builder(N, CS)
    b.line(N - 1, 0, 0x25, 45, cr.SHARED)  # a SHARED copy of an uncached block, with the memory's value
    want_last = cr.check(b.nodes, N, CS)
    assert want_last[0] == {"bits": cr.DIR_U_HELD, "addrs": 1, "first_addr": 0x25, "first_bits": cr.DIR_U_HELD}
    with ran_engine(dash, nsys, N, CS) as eng:
        clean = [list(cs.initial(N, CS))] * (nsys - 1)
        want = written(eng, 0, clean + [b.nodes], [cr.check(clean[0], N, CS)] * (nsys - 1) + [want_last])
        tot, rec = check_batch(eng, want)
        assert tot["violating_systems"] == 1 and cr.record(rec[nsys - 1]) == want_last[0]
        # the same line with another value: the verdict follows the last word
        b.line(N - 1, 0, 0x25, 44, cr.SHARED)
        want[nsys - 1] = cr.check(b.nodes, N, CS)
        eng.write_states(nsys - 1, [b.nodes])
        tot, rec = check_batch(eng, want)
        assert int(rec[nsys - 1]["bits"]) == cr.DIR_U_HELD | cr.STALE_VALUE


def test_states_over_part_of_the_batch(dash):
    """The systems outside the window keep the run's states and records."""
    N, CS = 4, 4
    states, want_states = states_of(N, CS), expected(N, CS)
    nsys = batch_size(N, len(states), pad=20)
    with ran_engine(dash, nsys, N, CS) as eng:
        before = [cr.check(eng.read_state(s), N, CS) for s in range(nsys)]
        tot0, rec0 = check_batch(eng, before)
        assert tot0["violating_systems"] > 0  # the cut runs left something to keep
        results = [a.copy() for a in eng.read_results()]
        first = 9
        want = written(eng, first, states, want_states)
        with pytest.raises(dash.DashError) as e:
            eng.read_coherence()
        assert e.value.code == dash.ESTATE  # the records are of the states that were
        assert all(np.array_equal(a, b) for a, b in zip(results, eng.read_results()))  # the run's, untouched
        assert want[:first] == before[:first] and want[first + len(states):] == before[first + len(states):]
        tot, rec = check_batch(eng, want)
        assert np.array_equal(rec[:first], rec0[:first])
        assert np.array_equal(rec[first + len(states):], rec0[first + len(states):])
        assert not np.array_equal(rec[first:first + len(states)], rec0[first:first + len(states)])


def test_refusals(dash):
    N, CS, nsys = 4, 4, 20
    one = [list(cs.initial(N, CS))]

    def code(fn, *args):
        with pytest.raises(dash.DashError) as e:
            fn(*args)
        return e.value.code

    packed, lens = random_batch(np.random.default_rng(3), nsys, N, LEN, block_span=4)
    with dash.Engine(nsys, num_procs=N, cache_size=CS, max_instr=LEN, keep_state=True) as eng:
        eng.load_traces(packed, lens)
        assert code(eng.write_states, 0, one) == dash.ESTATE  # before a run
        eng.run()
        eng.check_coherence()
        assert code(eng.write_states, nsys, one) == dash.EINVAL
        assert code(eng.write_states, nsys - 1, one * 2) == dash.EINVAL
        assert code(eng.write_states, 0, one * (nsys + 1)) == dash.EINVAL
        assert code(eng.write_states, 2 ** 64 - 1, one * 2) == dash.EINVAL  # first + count wraps
        eng.read_coherence()  # a refused call changed nothing
        eng.write_states(nsys, [])  # the empty window at the end is inside
        eng.write_states(0, one * nsys)
        assert code(eng.read_coherence) == dash.ESTATE
        tot = eng.check_coherence()
        assert tot["violating_systems"] == 0 and tot["systems"] == nsys
        eng.load_traces(packed, lens)
        assert code(eng.write_states, 0, one) == dash.ESTATE  # loaded again, not run
    with dash.Engine(nsys, num_procs=N, cache_size=CS, max_instr=LEN) as eng:  # no DASH_KEEP_STATE
        eng.load_traces(packed, lens)
        eng.run()
        assert code(eng.write_states, 0, one) == dash.ESTATE
