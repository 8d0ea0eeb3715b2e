"""Plain-Python twin of dash_shrink_many, written from the text of include/dash.h alone: every job is the
twin of dash_shrink (tests/shrink_ref.py) on its own, or UNMET when its source does not pass its goal; the
lock-step rounds' candidate counts follow from the jobs' steps; assign() is the header's rule for what a
system of a sub-pass holds. No arithmetic shared with csrc/dash_shrink.h.

TEST INFRASTRUCTURE: used by tests/test_shrink_many_spec.py (CPU) and tests/test_gpu_shrink_many.py.
"""
import functools

import numpy as np

import shrink_ref as sr

MINIMAL, UNMET = 0, 1
M = 40  # max_instr of the batches


def assign(cands, S, pass_, k):
    """(job, cand, counted) of system k in sub-pass pass_: with P_i the candidates of the jobs before i and
    T their total, g = pass_ * S + k; g < T: candidate g - P_i of the job with P_i <= g < P_(i+1), counted;
    otherwise the unchanged base of job k % J, not counted."""
    g = pass_ * S + k
    before = 0
    for i, C in enumerate(int(c) for c in cands):
        if before <= g < before + C:
            return i, g - before, True
        before += C
    return k % len(cands), 0, False


# ---------------------------------------------------------------- the inputs both test files use

SHAPES = ((4, 4, 12), (8, 4, 11), (3, 1, 13), (5, 16, 14))  # (N, CS, r)
SEEDS = (0, 7, 0, 5, 9, 0, 3, 11)


@functools.lru_cache(maxsize=None)
def batch(N, r):
    from test_gpu_parity import random_batch
    return random_batch(np.random.default_rng(r), 8, N, M, block_span=4, hot_frac=0.3)


def job_list(N, CS, r):
    """[(src, seed)]: every system of the batch under its seed of SEEDS, then system 0 under seed 5 and system
    3 under lockstep."""
    return [(k, SEEDS[k]) for k in range(8)] + [(0, 5), (3, 0)]


@functools.lru_cache(maxsize=None)
def jobs(N, CS, r):
    """[(src, seed, coh_all, err_all, err_none)]: the goal is the lowest bit of the source's own record under
    the job's seed (1 if it has none) and no error bit."""
    packed, lens = batch(N, r)
    out = []
    for src, seed in job_list(N, CS, r):
        bits, _err = sr.outcome(packed[src], lens[src], N, CS, seed)
        out.append((src, seed, (bits & -bits) or 1, 0, 0xFFFFFFFF))
    return out


def one(trace, lens, N, CS, job):
    """The twin's result for one job on a source: dash_shrink's twin, or the source as it is when UNMET."""
    _src, seed, *goal = job
    tr, ln = np.array(trace, dtype=np.uint16), np.array(lens, dtype=np.uint32)
    for t in range(N):
        tr[t, int(ln[t]):] = 0
    bits, errors = sr.outcome(tr, ln, N, CS, seed)
    res = {"status": MINIMAL, "trace": tr, "lens": ln, "steps": [], "variants": 0, "bits": bits, "errors": errors,
           "before": int(ln.sum())}
    if not sr.passes(bits, errors, tuple(goal)):
        res["status"] = UNMET
        return res
    res["trace"], res["lens"], res["steps"] = sr.shrink(tr, ln, N, CS, seed, tuple(goal))
    res["variants"] = sr.variants_run(ln, res["steps"])
    return res


@functools.lru_cache(maxsize=None)
def twin(N, CS, r):
    packed, lens = batch(N, r)
    return [one(packed[j[0]], lens[j[0]], N, CS, j) for j in jobs(N, CS, r)]


def round_cands(results):
    """[[C_i per job] per lock-step round], up to and without the first round with T == 0: a MINIMAL job has
    the C of each of its steps, then the candidates of its final set, then 0; an UNMET job 0 throughout."""
    per_job = []
    for res in results:
        if res["status"] == UNMET:
            per_job.append([])
        else:
            per_job.append([C for _t, _s, _n, C in res["steps"]] + [len(sr.candidates(res["lens"]))])
    rounds = []
    for rnd in range(max(len(c) for c in per_job)):
        row = [c[rnd] if rnd < len(c) else 0 for c in per_job]
        if sum(row) == 0:
            break
        rounds.append(row)
    return rounds


def passes_run(results, S):
    """dash_run calls of a call: the check of the sources, every round's sub-passes, the final run."""
    return 2 + sum(-(-sum(row) // S) for row in round_cands(results))
