"""Queue-depth tiers across shapes and run modes: sim_kernel<P, CS, RING, MODE> at RING 32 and
256, the hand-offs between the tiers (16 -> 32 -> 256), the overflow hint and the adaptive first
tier, in lockstep, seeded and event-log runs.

Every expectation comes from the CPU oracle at queue capacity 256 under the same schedule seed:
per-system state, histogram, rounds, error bits and digest, every statistic of the run
(check_stats), the event log, and -- from the oracle's max_depth -- exactly which systems each
tier hands to the next. The depth bands each case needs (systems on both sides of a hand-off,
queues that peak at exactly 16 and 32) are asserted from the oracle inside the tests, so a drift
of the inputs fails instead of passing without reaching the deeper tiers.

All tests but the oracle-only guard need the GPU (marked one by one, so that the guard runs in
the CPU suite).
"""
import functools

import numpy as np
import pytest

from oracle_ctypes import GOLDEN, run_system
from test_gpu_parity import check_batch, check_stats, random_batch

gpu = pytest.mark.gpu
TIERS = (16, 32, 256)
SEEDS = (0, 87, 0x5EED5EED)


def oracle_batch(packed, lens, N, CS, seed=0):
    return [run_system(packed[s], lens[s], num_procs=N, cache_size=CS, ring_depth=256,
                       max_rounds=1024 + 256 * packed.shape[2], arb_seed=seed) for s in range(len(packed))]


def oracle_log(tr, lens, N, CS, seed=0, max_rounds=0):
    return run_system(tr, lens, num_procs=N, cache_size=CS, ring_depth=256, log=True, log_msgs=True,
                      max_rounds=max_rounds or 1024 + 256 * tr.shape[1], arb_seed=seed, log_bytes=1 << 24)[1]


def depth_of(results):
    return np.array([r.max_depth for r in results])


def tier_counts(depth, first=0):
    """dash_stats.tier_systems of a run that starts every system at tier `first`: a system is
    handed on exactly when its unbounded queue depth exceeds the tier's (maxd > RING)."""
    out = [0, 0, 0]
    out[first] = len(depth)
    for k in range(first + 1, 3):
        out[k] = int((depth > TIERS[k - 1]).sum())
    return out


def first_tier_flag(dash, first):
    return {0: 0, 1: dash.TIER_FROM_32, 2: dash.TIER_FROM_256}[first]


def check_results(eng, stats, results):
    """Digests, rounds, error bits and every statistic of a run against the oracle's results."""
    dig, rnd, err = eng.read_results()
    assert dig.tolist() == [r.digest for r in results]
    assert rnd.tolist() == [r.rounds for r in results]
    assert err.tolist() == [r.errors for r in results]
    check_stats(stats, results)


# ---------------------------------------------------------------- inputs, made once

@functools.lru_cache(maxsize=None)
def organic(N, CS):
    """Ragged contention traces: some systems of each wave overflow the 16-deep rings."""
    return random_batch(np.random.default_rng(9000 + 16 * N + CS), 256, N, 300, block_span=4, hot_frac=0.9)


@functools.lru_cache(maxsize=None)
def contended(N, CS, L):
    """Full-length contention traces: deep enough for a second hand-off (32 -> 256)."""
    return random_batch(np.random.default_rng(100 * N + CS), 256, N, L, block_span=4, hot_frac=0.9,
                        fixed_len=True)


@functools.lru_cache(maxsize=None)
def organic_oracle(N, CS, seed):
    return oracle_batch(*organic(N, CS), N, CS, seed)


@functools.lru_cache(maxsize=None)
def contended_oracle(N, CS, L, seed):
    return oracle_batch(*contended(N, CS, L), N, CS, seed)


# ---------------------------------------------------------------- 1. forced deeper tiers

SHAPES = [(1, 4), (2, 8), (2, 1), (3, 16), (4, 2), (4, 16), (4, 5), (5, 1), (6, 8), (7, 3), (8, 16), (8, 11)]
LOG_SHAPES = [(2, 8), (4, 2), (5, 1), (8, 16)]


def forced_batches(N, CS):
    rng = np.random.default_rng(7000 + 16 * N + CS)
    return [random_batch(rng, 64, N, 40), random_batch(rng, 64, N, 40, block_span=4, hot_frac=0.5)]


@gpu
@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("N,CS", SHAPES)
def test_forced_tier_shape_matrix(dash, N, CS, first):
    """RING 32 / 256 at every node-count class (P 1, 2, 4, 8), every CACHE_SIZE class (1, 2, 4,
    8, 16, generic) and non-power-of-two node counts, lockstep and seeded (MODE 0, 1): all 64
    systems start in the forced tier and come out bit-exact, statistics included."""
    for packed, lens in forced_batches(N, CS):
        for seed in SEEDS[:2]:
            stats = check_batch(dash, packed, lens, N, CS, flags=first_tier_flag(dash, first), seed=seed)
            depth = depth_of(oracle_batch(packed, lens, N, CS, seed))
            assert stats["tier_systems"] == tier_counts(depth, first)
            assert stats["tier_systems"][first] == 64 and sum(stats["tier_systems"][:first]) == 0


@gpu
@pytest.mark.parametrize("first", [1, 2])
@pytest.mark.parametrize("N,CS", LOG_SHAPES)
def test_forced_tier_event_log(dash, N, CS, first):
    """The event log at RING 32 / 256 (MODE 2, 3): every system's formatted log is the oracle's."""
    for packed, lens in forced_batches(N, CS):
        for seed in SEEDS[:2]:
            with dash.Engine(64, num_procs=N, cache_size=CS, max_instr=40, trace_events=4096,
                             flags=first_tier_flag(dash, first), schedule_seed=seed) as eng:
                eng.load_traces(packed, lens)
                stats = eng.run()
                assert stats["tier_systems"][first] == 64 and sum(stats["tier_systems"][:first]) == 0
                for s in range(64):
                    assert dash.format_events(eng.read_events(s)) == oracle_log(packed[s], lens[s], N, CS, seed), \
                        (seed, s)


# ---------------------------------------------------------------- 2. organic hand-offs

ORGANIC = [(N, CS, seed) for N, CS in [(8, 1), (8, 2), (8, 3), (7, 1), (7, 2), (6, 1), (8, 16)]
           for seed in SEEDS[:2] if (N, CS, seed) != (8, 16, 87)]  # (8,16) seed 87: none deep


@gpu
@pytest.mark.parametrize("N,CS,seed", ORGANIC)
def test_organic_hand_off_inside_mixed_waves(dash, N, CS, seed):
    """Waves in which some systems overflow the 16-deep rings and are re-run from scratch at 32
    while their neighbours finish: both kinds bit-exact, lockstep and seeded, and the systems
    handed on are exactly those whose oracle depth exceeds 16."""
    packed, lens = organic(N, CS)
    depth = depth_of(organic_oracle(N, CS, seed))
    handed = int((depth > 16).sum())
    least = 32 if (N, CS) in ((8, 1), (8, 2)) else 1
    assert handed >= least and 256 - handed >= least  # both sides of the hand-off are present
    stats = check_batch(dash, packed, lens, N, CS, seed=seed)
    assert stats["tier_systems"] == tier_counts(depth)


# ---------------------------------------------------------------- 3. second hand-off, exact capacity

SECOND = [(8, 1, 200, 0), (8, 1, 200, 87), (8, 1, 200, 0x5EED5EED), (8, 2, 400, 0), (7, 1, 400, 0)]


@gpu
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("N,CS,L,seed", SECOND)
def test_second_hand_off(dash, N, CS, L, seed, first):
    """Systems that overflow the 32-deep rings too (16 -> 32 -> 256, or 32 -> 256 when the run
    starts at 32), next to systems that stay: bit-exact, with exactly the oracle's hand-offs."""
    packed, lens = contended(N, CS, L)
    depth = depth_of(contended_oracle(N, CS, L, seed))
    assert 0 < (depth > 32).sum() < 256  # the 32-deep tier hands on some systems and keeps others
    stats = check_batch(dash, packed, lens, N, CS, flags=first_tier_flag(dash, first), seed=seed)
    assert stats["tier_systems"] == tier_counts(depth, first)


def exact_capacity_cases():
    """(input, oracle results) of every case of the two tests above."""
    for N, CS, seed in ORGANIC:
        yield organic(N, CS), organic_oracle(N, CS, seed), N, CS, seed
    for N, CS, L, seed in SECOND:
        yield contended(N, CS, L), contended_oracle(N, CS, L, seed), N, CS, seed


@gpu
def test_exact_capacity_stays_in_its_tier(dash):
    """A queue that reaches exactly 16 (32) entries fits the 16-deep (32-deep) ring: the hand-off
    test is depth > RING. Of the inputs above, the first that holds such systems is run again
    with only them and their nearest deeper and shallower neighbours: bit-exact, and
    tier_systems counts none of the exact-capacity systems as handed on."""
    for edge in (16, 32):
        found = [(c, depth_of(c[1])) for c in exact_capacity_cases()]
        found = [(c, d) for c, d in found if (d == edge).any()]
        assert found, f"no input holds a queue that peaks at exactly {edge}"
        ((packed, lens), _, N, CS, seed), depth = found[0]
        pick = np.flatnonzero((depth >= edge - 1) & (depth <= edge + 1))
        assert (depth[pick] == edge).any()
        stats = check_batch(dash, packed[pick], lens[pick], N, CS, seed=seed)
        assert stats["tier_systems"] == tier_counts(depth[pick])
        k = TIERS.index(edge)
        assert len(pick) - stats["tier_systems"][k + 1] >= int((depth[pick] == edge).sum())


def test_oracle_tells_queue_capacities_apart():
    """CPU guard against a vacuous parity check: on the (8, 1, 200) input the oracle run with
    queue capacity 32 differs (digest or error bits) from capacity 256 on every system deeper
    than 32, and capacity 16 differs on every system deeper than 16 -- so a tier that computed
    with the wrong capacity could not pass. A queue that peaks at exactly 32 sticks at capacity
    32 (full means stuck, as in the reference), so final-tier semantics applied one tier early
    differ as well."""
    packed, lens = contended(8, 1, 200)
    ref = contended_oracle(8, 1, 200, 0)
    depth = depth_of(ref)
    assert (depth > 32).sum() >= 1 and (depth == 32).sum() >= 1 and (depth > 16).sum() >= 32
    for cap in (16, 32):
        for s in np.flatnonzero(depth >= cap):
            r = run_system(packed[s], lens[s], num_procs=8, cache_size=1, ring_depth=cap,
                           max_rounds=1024 + 256 * 200)
            assert (r.digest, r.errors) != (ref[s].digest, ref[s].errors), (cap, int(s), int(depth[s]))


# ---------------------------------------------------------------- 4. event log through hand-offs

@gpu
@pytest.mark.parametrize("seed", SEEDS[:2])
def test_event_log_through_hand_offs(dash, seed):
    """The event log of systems re-run at 32 and 256 after a hand-off, lockstep and seeded (MODE
    2, 3): the log of each of 32 systems (every system outside the 17..32 band, then the first
    of the rest) is the oracle's, with nothing left from the abandoned shallower run, and the
    digests of all 256 equal the oracle's and those of the same run without the log."""
    N, CS, L = 8, 1, 120
    packed, lens = contended(N, CS, L)
    ref = contended_oracle(N, CS, L, seed)
    depth = depth_of(ref)
    band = (depth > 16) & (depth <= 32)
    assert (depth <= 16).any() and band.sum() >= 32 and max(r.rounds for r in ref) <= 4096
    if seed == 0:
        assert (depth > 32).any()
    pick = np.flatnonzero(~band).tolist()
    pick += np.flatnonzero(band)[:32 - len(pick)].tolist()
    assert len(pick) == 32
    with dash.Engine(256, num_procs=N, cache_size=CS, max_instr=L, trace_events=4096, schedule_seed=seed) as eng:
        eng.load_traces(packed, lens)
        stats = eng.run()
        check_results(eng, stats, ref)
        assert stats["tier_systems"] == tier_counts(depth)
        dig_log = eng.read_results()[0]
        for s in pick:
            assert dash.format_events(eng.read_events(s)) == oracle_log(packed[s], lens[s], N, CS, seed), s
    with dash.Engine(256, num_procs=N, cache_size=CS, max_instr=L, schedule_seed=seed) as eng:
        eng.load_traces(packed, lens)
        eng.run()
        assert np.array_equal(eng.read_results()[0], dig_log)


@gpu
def test_event_log_of_the_deepest_systems(dash):
    """The three deepest systems of the (8, 1, 200) input (handed on twice, 16 -> 32 -> 256):
    their event logs are the oracle's."""
    N, CS, L = 8, 1, 200
    packed, lens = contended(N, CS, L)
    ref = contended_oracle(N, CS, L, 0)
    depth = depth_of(ref)
    deepest = np.argsort(-depth, kind="stable")[:3]
    assert (depth[deepest] > 32).all() and max(r.rounds for r in ref) <= 8192
    with dash.Engine(256, num_procs=N, cache_size=CS, max_instr=L, trace_events=8192) as eng:
        eng.load_traces(packed, lens)
        stats = eng.run()
        check_results(eng, stats, ref)
        assert stats["tier_systems"] == tier_counts(depth)
        for s in deepest:
            assert dash.format_events(eng.read_events(s)) == oracle_log(packed[s], lens[s], N, CS), int(s)


# ---------------------------------------------------------------- 5. overflow hint, adaptive tier

HINT_NSYS = 1024
# where the deep systems go: the first and the last system, two of one wave (8 systems of 8
# lanes: 0 and 3), the rest scattered over other waves
HINT_SLOTS = [0, 3, 1023] + [37 * k + 11 for k in range(1, 27)] + [1016]


def hint_batch(N, CS, L, seed):
    """1,024 systems of which few are deep: every system with oracle depth > 32 of the source
    input and ten with 17..32 sit at HINT_SLOTS; all others run the first four instructions
    of a source system."""
    src, src_lens = contended(N, CS, L)
    depth = depth_of(contended_oracle(N, CS, L, seed))
    deep = np.flatnonzero(depth > 32).tolist()
    mid = np.flatnonzero((depth > 16) & (depth <= 32))[:10].tolist()
    chosen = deep + mid
    assert len(deep) >= 1 and len(mid) == 10 and len(chosen) <= len(HINT_SLOTS)
    assert len(set(HINT_SLOTS)) == len(HINT_SLOTS) and max(HINT_SLOTS) == HINT_NSYS - 1
    packed = src[np.arange(HINT_NSYS) % 256].copy()
    lens = np.full((HINT_NSYS, N), 4, np.uint32)
    slots = HINT_SLOTS[:len(chosen)]  # those that overflow twice first: systems 0 and 3 share a wave
    for slot, s in zip(slots, chosen):
        packed[slot] = src[s]
        lens[slot] = src_lens[s]
    return packed, lens, sorted(slots[:len(deep)])


@gpu
@pytest.mark.parametrize("N,L,seed,events", [(8, 200, 0, 0), (8, 200, 87, 0), (8, 200, 0, 8192), (7, 400, 0, 0)])
def test_overflow_hint_against_the_oracle(dash, N, L, seed, events):
    """Repeated runs of the same traces: from the second run on, the systems that overflowed the
    16-deep rings start at 32 on the side stream while the first tier skips them, and those that
    overflow again (32 -> 256) join the main stream's hand-off list. Every run's digests,
    rounds, error bits and statistics are the oracle's and tier_systems stays [1024, deeper
    than 16, deeper than 32]; the deep systems' event logs after the third run are the
    oracle's; new traces drop the hint."""
    CS = 1
    packed, lens, deep_slots = hint_batch(N, CS, L, seed)
    ref = oracle_batch(packed, lens, N, CS, seed)
    depth = depth_of(ref)
    expect = tier_counts(depth)
    assert expect[2] >= 1 and expect[1] > expect[2] and expect[1] * 32 < HINT_NSYS  # first tier stays 16
    assert np.flatnonzero(depth > 32).tolist() == deep_slots
    fresh, fresh_lens = random_batch(np.random.default_rng(5000 + N), HINT_NSYS, N, L, block_span=4, hot_frac=0.5)
    fresh_ref = oracle_batch(fresh, fresh_lens, N, CS, seed)
    with dash.Engine(HINT_NSYS, num_procs=N, cache_size=CS, max_instr=L, trace_events=events,
                     schedule_seed=seed) as eng:
        eng.load_traces(packed, lens)
        for run in range(3):
            stats = eng.run()
            check_results(eng, stats, ref)
            assert stats["tier_systems"] == expect, run
        if events:
            assert max(r.rounds for r in ref) <= events
            for s in deep_slots:
                assert dash.format_events(eng.read_events(s)) == oracle_log(packed[s], lens[s], N, CS, seed), s
        eng.load_traces(fresh, fresh_lens)
        stats = eng.run()
        check_results(eng, stats, fresh_ref)
        assert stats["tier_systems"] == tier_counts(depth_of(fresh_ref))


@gpu
def test_adaptive_tier_escalates_twice(dash):
    """Without a TIER flag the first tier follows the overflow share: > 1/32 of the systems
    overflow 16, then > 1/32 overflow 32, so the second run starts at 32 and the third at 256.
    Every run gives the oracle's results and statistics. The first tier is never lowered again:
    shallow traces loaded afterwards still run at 256, with the oracle's results."""
    N, CS, L = 8, 1, 400
    packed, lens = contended(N, CS, L)
    ref = contended_oracle(N, CS, L, 0)
    depth = depth_of(ref)
    d16, d32 = int((depth > 16).sum()), int((depth > 32).sum())
    assert d16 * 32 > 256 and d32 * 32 > 256 and d32 < 256
    shallow_lens = np.minimum(lens, 4).astype(np.uint32)
    shallow_ref = oracle_batch(packed, shallow_lens, N, CS)
    assert depth_of(shallow_ref).max() <= 16
    with dash.Engine(256, num_procs=N, cache_size=CS, max_instr=L) as eng:
        eng.load_traces(packed, lens)
        for expect in ([256, d16, d32], [0, 256, d32], [0, 0, 256]):
            stats = eng.run()
            check_results(eng, stats, ref)
            assert stats["tier_systems"] == expect
        eng.load_traces(packed, shallow_lens)
        stats = eng.run()
        check_results(eng, stats, shallow_ref)
        assert stats["tier_systems"] == [0, 0, 256]


# ---------------------------------------------------------------- 6. final-tier drops

def stuck_input():
    tr = np.load(GOLDEN.parent / "stuck_queue.npy")
    return tr[None, :, :].astype(np.uint16), np.full((1, 8), tr.shape[1], dtype=np.uint32)


@gpu
def test_final_tier_drops_with_the_event_log(dash):
    """The trace that fills a queue to the reference's capacity (256: stuck for good, later
    sends dropped) with the event log on (MODE 2 at RING 256, clamp and drop path): the
    formatted log is the oracle's, digest and error bits equal the run without the log and the
    oracle, and the four dropped sends are counted."""
    packed, lens = stuck_input()
    cap = 1024 + 256 * packed.shape[2]
    res, log = run_system(packed[0], lens[0], num_procs=8, cache_size=1, ring_depth=256, max_rounds=cap,
                          log=True, log_msgs=True, log_bytes=1 << 24)
    assert (res.errors, res.max_depth, res.dropped, res.rounds) == (0x29, 256, 4, 34616)
    assert len(log.splitlines()) == 113245
    with dash.Engine(1, num_procs=8, cache_size=1, max_instr=packed.shape[2], max_rounds=cap) as eng:
        eng.load_traces(packed, lens)
        eng.run()
        plain = [x.tolist() for x in eng.read_results()]
    with dash.Engine(1, num_procs=8, cache_size=1, max_instr=packed.shape[2], max_rounds=cap,
                     trace_events=34616) as eng:
        eng.load_traces(packed, lens)
        stats = eng.run()
        check_results(eng, stats, [res])
        assert [x.tolist() for x in eng.read_results()] == plain
        assert stats["dropped"] == 4 and stats["tier_systems"] == [1, 1, 1]
        assert dash.format_events(eng.read_events(0)) == log


@gpu
def test_stuck_trace_under_a_seeded_schedule(dash):
    """The same trace under seeded schedule 87 no longer sticks but still needs the 256-deep
    rings (MODE 1 at RING 256 after two hand-offs)."""
    packed, lens = stuck_input()
    res = oracle_batch(packed, lens, 8, 1, 87)[0]
    assert 32 < res.max_depth < 256 and res.errors == 0
    stats = check_batch(dash, packed, lens, 8, 1, seed=87)
    assert stats["tier_systems"] == [1, 1, 1]
