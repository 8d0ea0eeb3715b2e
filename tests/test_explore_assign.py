"""dash_explore_assign (csrc/dash_host.c): which source and seed a system of a dash_explore_sources pass
runs, and whether it is counted -- against a restatement of include/dash.h's rule, over random
arguments and the edges of the rule, and as a whole: over all passes and systems every (source, seed
index) is counted exactly once (CPU only)."""
import collections
import random

import pytest

U64 = 1 << 64


def restated(S, G, K, F, p, k):
    """The rule of include/dash.h, or None where the call is refused."""
    if not (1 <= G <= S) or F + K >= U64 or k >= S:
        return None
    R = S // G
    if p >= -(-K // R):
        return None
    fresh = min(R, K - p * R)
    j = p * R + k // G
    counted = k < G * R and j < K
    if not counted:
        j = p * R + (k // G) % fresh
    return k % G, F + j, counted


def got(dash, S, G, K, F, p, k):
    try:
        return dash.explore_assign(S, G, K, F, p, k)
    except dash.DashError as e:
        assert e.code == dash.EINVAL
        return None


def test_random_arguments(dash):
    rng = random.Random(343)
    refused = 0
    for _ in range(4000):
        S = rng.choice([1, 2, 63, 64, 70, 256, 65536, 1 << 20, rng.randrange(1, 1 << 32)])
        G = rng.choice([1, S, rng.randrange(0, S + 2), rng.randrange(1, S + 1)])
        K = rng.choice([0, 1, rng.randrange(1, 5000), rng.randrange(1, 1 << 40)])
        F = rng.choice([0, 1, rng.randrange(U64), U64 - K - 1, (U64 - K) % U64])
        R = max(S // max(G, 1), 1)
        p = rng.choice([0, rng.randrange(0, K // R + 2), K // R, max(-(-K // R) - 1, 0)])
        k = rng.choice([0, S - 1, S, rng.randrange(0, S + 1)])
        want = restated(S, G, K, F, p, k)
        refused += want is None
        assert got(dash, S, G, K, F, p, k) == want, (S, G, K, F, p, k)
    assert 200 < refused < 3800


EDGES = [
    (64, 64, 6, 10),        # G = S: one seed of every source per pass
    (64, 1, 300, 0),        # G = 1: dash_explore's passes, the last with 44 fresh
    (64, 3, 50, 7),         # S not a multiple of G: one padding system per pass
    (70, 3, 50, 0),         # the same, S not a multiple of 64
    (256, 4, 10, 5),        # K < R: one pass, mostly repeats
    (64, 40, 6, 0),         # R = 1 with 24 padding systems
    (8, 3, 5, U64 - 6),     # the highest seeds that do not wrap
    (5, 5, 0, 0),           # no seeds: no pass
]


@pytest.mark.parametrize("S,G,K,F", EDGES)
def test_edges_and_coverage(dash, S, G, K, F):
    R = S // G
    passes = -(-K // R)
    seen = collections.Counter()
    for p in range(passes):
        fresh = min(R, K - p * R)
        for k in range(S):
            src, seed, counted = dash.explore_assign(S, G, K, F, p, k)
            assert (src, seed, counted) == restated(S, G, K, F, p, k)
            assert src == k % G and p * R <= seed - F < p * R + fresh  # a repeat is a seed of its own pass
            if counted:
                seen[src, seed - F] += 1
            assert counted or k >= G * R or k // G >= fresh
    assert seen == {(s, j): 1 for s in range(G) for j in range(K)}
    assert got(dash, S, G, K, F, passes, 0) is None and got(dash, S, G, K, F, 0, S) is None


def test_refusals(dash):
    assert got(dash, 64, 0, 10, 0, 0, 0) is None and got(dash, 64, 65, 10, 0, 0, 0) is None
    assert got(dash, 0, 0, 10, 0, 0, 0) is None
    # the wrap: first_seed + seeds_per_source must stay below 2^64
    assert got(dash, 64, 1, 10, U64 - 10, 0, 0) is None and got(dash, 64, 1, 1, U64 - 1, 0, 0) is None
    assert got(dash, 64, 1, 10, U64 - 11, 0, 9) == (0, U64 - 2, True)
    assert got(dash, 64, 1, 10, 0, 1, 0) is None  # one pass only
    # optional outputs may be null
    assert dash.lib().dash_explore_assign(64, 3, 50, 0, 2, 5, None, None, None) == dash.OK
