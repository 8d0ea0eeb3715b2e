"""The adequacy corpus through every sim_kernel class on the GPU.

tests/test_adequacy_corpus.py shows on the CPU that the corpus of tests/golden/adequacy/ tells
every oracle mutant apart -- at every CACHE_SIZE class, all-lockstep and under its own schedule
seeds, and in its micro-step walks. Here the same systems go through the C-ABI at every node
count of the fixture (and the generated one-node batch), every CACHE_SIZE class and every first
queue tier (RING 16, 32, 256), on a plain handle (MODE 0), with the event log (MODE 2), under
per-system schedule seeds (MODE 1) and both (MODE 3); the walks drive one-system handles through
dash_set_micro_schedule (MODE 4). Every system's node state, histogram, rounds, error bits and
digest are the oracle's, all systems stay in the forced tier, and every logged run's formatted
events are the oracle's DEBUG log. A kernel with one of the mutants' deviations in one of these
classes fails here.
"""
import functools

import numpy as np
import pytest

import adequacy as ad
from micro_fuzz import XK_ISSUE, XK_POP, acts_of
from oracle_ctypes import run_system
from test_gpu_system_seeds import check_against
from test_gpu_tiers import depth_of, first_tier_flag, tier_counts

pytestmark = pytest.mark.gpu
CASES = [(N, CS) for N in (1,) + ad.NODE_COUNTS for CS in ad.CACHE_SIZES]


@functools.lru_cache(maxsize=None)
def corpus(N):
    if N == 1:
        return ad.n1_batch()
    fx = ad.load_fixture(N)
    return fx["packed"], fx["lens"], fx["seeds"]


@functools.lru_cache(maxsize=2)
def oracle(N, CS, seeded):
    """(results, DEBUG logs) of the N corpus, all-lockstep or each system under its own seed."""
    packed, lens, seeds = corpus(N)
    runs = [run_system(packed[s], lens[s], num_procs=N, cache_size=CS, ring_depth=256, max_rounds=ad.ROUND_CAP,
                       log=True, log_msgs=True, arb_seed=int(seeds[s]) if seeded else 0) for s in range(len(packed))]
    return [r for r, _ in runs], [log for _, log in runs]


@pytest.mark.parametrize("N,CS", CASES)
def test_corpus_bit_exact_in_every_kernel_class(dash, N, CS):
    packed, lens, seeds = corpus(N)
    n = len(packed)
    for seeded in (False, True):
        results, logs = oracle(N, CS, seeded)
        depth = depth_of(results)
        assert depth.max() <= 16  # no hand-off: every system stays in the tier the run starts at
        rounds = max(r.rounds for r in results)
        for first in (0, 1, 2):
            for logged in (False, True):
                with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=ad.MAX_LEN, keep_state=True,
                                 flags=first_tier_flag(dash, first), trace_events=rounds + 8 if logged else 0,
                                 schedule_seed=1 if seeded else 0) as eng:
                    eng.load_traces(packed, lens)
                    if seeded:
                        eng.set_system_seeds(seeds)
                    stats = eng.run()
                    check_against(dash, eng, stats, results, N, CS)
                    assert stats["tier_systems"] == tier_counts(depth, first), (seeded, first, logged)
                    assert stats["tier_systems"][first] == n and sum(stats["tier_systems"]) == n
                    if logged:
                        for s in range(n):
                            assert dash.format_events(eng.read_events(s)) == logs[s], (seeded, first, s)


@pytest.mark.parametrize("CS", ad.MICRO_CS)
@pytest.mark.parametrize("N", ad.NODE_COUNTS)
def test_micro_walks_bit_exact(dash, N, CS):
    """Each system of the micro-step section: its walk of the STRICT model, re-enacted send by send
    (tests/micro_fuzz.py does the same for random systems). Digest, instructions issued and every
    node's order of pops and issues are the walk's."""
    for k, (tr, lens, wseed, weights) in enumerate(ad.load_fixture(N)["micro"]):
        out, steps = ad.walk(tr, lens, N, CS, wseed, weights)
        with dash.Engine(1, num_procs=N, cache_size=CS, max_instr=ad.MAX_LEN, trace_events=len(steps) + 8,
                         schedule_seed=1, max_rounds=len(steps) + 64) as eng:
            eng.set_micro_schedule(acts_of(steps, N))
            eng.load_traces(tr[None], lens[None])
            stats = eng.run()
            dig = int(eng.read_results()[0][0])
            ev = eng.read_events(0)
        want = [[(x >> 8) == XK_ISSUE for x in steps if (x & 15) == t and (x >> 8) in (XK_POP, XK_ISSUE)]
                for t in range(N)]
        got = [[e.kind == dash.EV_INSTR for e in ev if e.node == t] for t in range(N)]
        assert dig == out.digest, k
        assert stats["instructions"] == int(lens.sum()), k
        assert not stats["err_bits"] & (dash.ERR_ROUNDCAP | dash.ERR_DEADLOCK | dash.ERR_SCHEDULE), k
        assert got == want, k
