"""Plain-Python twin of dash_shrink, written from the text of include/dash.h alone: the candidate
enumeration, the deletion, the goal over the CPU oracle's run plus tests/coherence_ref.py, and the greedy
loop. No arithmetic shared with csrc/dash_shrink.h.

TEST INFRASTRUCTURE: used by tests/test_shrink_spec.py (CPU) and tests/test_gpu_shrink.py.
"""
import functools

import numpy as np

import coherence_ref as cr
import oracle_ctypes as oc


def candidates(lens):
    """[(node, start, count)] in index order: node ascending; levels J .. 0 with J the least integer with
    2^J >= lens[t]; block starts 0, 2^j, 2 * 2^j, ... below lens[t]."""
    out = []
    for t, L in enumerate(int(x) for x in lens):
        if L == 0:
            continue
        J = 0
        while 2 ** J < L:
            J += 1
        for j in range(J, -1, -1):
            for s in range(0, L, 2 ** j):
                out.append((t, s, min(s + 2 ** j, L) - s))
    return out


def delete(trace, lens, node, start, count):
    """The trace set without instructions [start, start + count) of `node`: later instructions move down,
    words at or past the new length are 0."""
    tr, ln = np.array(trace, dtype=np.uint16), np.array(lens, dtype=np.uint32)
    L = int(ln[node])
    assert 0 < count and start + count <= L
    row = list(tr[node, :start]) + list(tr[node, start + count:L])
    tr[node] = 0
    tr[node, :len(row)] = row
    ln[node] = L - count
    return tr, ln


def outcome(trace, lens, N, CS, seed):
    """(coherence bits, error bits) of the final state under the schedule of `seed` (0 = lockstep)."""
    r = oc.run_system(trace, lens, num_procs=N, cache_size=CS, arb_seed=seed)
    return cr.check(r.node, N, CS)[0]["bits"], r.errors


def passes(bits, errors, goal):
    coh_all, err_all, err_none = goal
    return (bits & coh_all) == coh_all and (errors & err_all) == err_all and (errors & err_none) == 0


def shrink(trace, lens, N, CS, seed, goal):
    """The greedy loop: per round the passing candidate that deletes the most, the lowest index among
    equals, becomes the base, until none passes. goal = (coh_all, err_all, err_none). Returns (trace,
    lens, steps) with steps = [(node, start, count, candidates of that round's base)]."""
    tr, ln = np.array(trace, dtype=np.uint16), np.array(lens, dtype=np.uint32)
    for t in range(N):
        tr[t, int(ln[t]):] = 0
    assert passes(*outcome(tr, ln, N, CS, seed), goal), "the source does not meet the goal"
    steps = []
    while True:
        cands = candidates(ln)
        best = None
        for c, (t, s, n) in enumerate(cands):
            if best is not None and n <= cands[best][2]:
                continue  # could not beat the winner so far: more deleted wins, then the lower index
            if passes(*outcome(*delete(tr, ln, t, s, n), N, CS, seed), goal):
                best = c
        if best is None:
            return tr, ln, steps
        t, s, n = cands[best]
        steps.append((t, s, n, len(cands)))
        tr, ln = delete(tr, ln, t, s, n)


def variants_run(lens_before, steps):
    """The candidates a call evaluates: every round's, the last round's (none passed) included."""
    ln = [int(x) for x in lens_before]
    total = 0
    for t, _s, n, C in steps:
        total += C
        ln[t] -= n
    return total + len(candidates(ln))


# ---------------------------------------------------------------- the inputs both test files use

ROWS = ((8, 4, 11, 7), (4, 4, 12, 0), (3, 1, 13, 5), (5, 16, 14, 0), (2, 8, 15, 9))  # (N, CS, r, seed)


@functools.lru_cache(maxsize=None)
def row_source(N, CS, r, seed):
    """(index, trace, lens, coherence bits) of the first system of
    random_batch(default_rng(r), 8, N, 40, block_span=4, hot_frac=0.3) that is incoherent with no error
    bit under the seed."""
    from test_gpu_parity import random_batch
    packed, lens = random_batch(np.random.default_rng(r), 8, N, 40, block_span=4, hot_frac=0.3)
    for k in range(8):
        bits, err = outcome(packed[k], lens[k], N, CS, seed)
        if bits and not err:
            return k, packed[k], lens[k], bits
    raise AssertionError("no incoherent clean system in the batch")


OOB_ROW = (4, 4, 29, 3)  # a batch with a system that ends with DASH_ERR_OOB under the seed, found on the oracle
ERR_OOB_GOAL = (0, oc.ERR_OOB, 0)


@functools.lru_cache(maxsize=None)
def oob_source():
    """(index, trace, lens) of the first system of OOB_ROW's batch with DASH_ERR_OOB."""
    from test_gpu_parity import random_batch
    N, CS, r, seed = OOB_ROW
    packed, lens = random_batch(np.random.default_rng(r), 8, N, 40, block_span=4, hot_frac=0.3)
    k = next(k for k in range(8) if outcome(packed[k], lens[k], N, CS, seed)[1] & oc.ERR_OOB)
    return k, packed[k], lens[k]


@functools.lru_cache(maxsize=None)
def oob_twin():
    _k, tr, ln = oob_source()
    N, CS, _r, seed = OOB_ROW
    return shrink(tr, ln, N, CS, seed, ERR_OOB_GOAL)


@functools.lru_cache(maxsize=None)
def row_twin(N, CS, r, seed):
    """The twin's result for a row, with the goal the tests use: the lowest bit of the source's record and
    no error bit allowed."""
    _k, tr, ln, bits = row_source(N, CS, r, seed)
    return shrink(tr, ln, N, CS, seed, (bits & -bits, 0, 0xFFFFFFFF))
