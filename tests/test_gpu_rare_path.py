"""GPU parity of the lean CACHE_SIZE 4 lockstep round.

The kernels sim_kernel<P, 4, RING, 0> leave work out of the round that the result does not need.
Every case here is bit-exact parity with the CPU oracle through test_gpu_parity.check_batch: final
state of every node, digest, rounds, error bits, per-type histogram of every system, and the run's
totals (maximum queue depth, drops, longest run). The shapes are the smallest at which such a round
can go wrong: a full wave plus a one-system wave, padded lanes (N = 5), REPLY_ID / INV / UPGRADE
pops confined to lane 0, lane 63 or one system of a wave, systems that go quiet in each round of a
trip, and a batch that hands systems to the 32-deep tier.
"""
import numpy as np
import pytest

import oracle_ctypes
from oracle_ctypes import pack, run_system
from test_gpu_parity import DEEP_SYSTEMS, check_batch

pytestmark = pytest.mark.gpu

T_RID, T_INV, T_UPG = 4, 5, 6  # transactionType ordinals of REPLY_ID, INV, UPGRADE


@pytest.mark.parametrize("kind", [0, 1], ids=["uniform", "contention"])
@pytest.mark.parametrize("N", [8, 5])
@pytest.mark.parametrize("nsys", [9, 16])
def test_generated_traces(dash, nsys, N, kind):
    """64 generated instructions per node: 9 systems of 8 lanes are one full wave and a wave that
    holds one system, 16 are two full waves; N = 5 leaves three padded lanes per system."""
    L = 64
    packed = np.stack([oracle_ctypes.gen_system(0x5EED, s, N, L, kind=kind) for s in range(nsys)])
    lens = np.full((nsys, N), L, np.uint32)
    stats = check_batch(dash, packed, lens, N, 4)
    if kind == 0:  # the uniform batches pop each of the three types (contention: mostly forwards)
        assert all(stats["hist"][T_RID:T_UPG + 1])


def upgrade_system(home, req, sharer, L):
    """One write hit on a SHARED line: `req` and `sharer` read block 0 of `home`, `req` re-reads it
    (hits, one round each) until both fills have settled, then writes it: one UPGRADE pops at
    `home`, one REPLY_ID at `req`, one INV at `sharer`, each in a round of its own."""
    a = (home << 4) | 0
    tr = np.zeros((8, L), np.uint16)
    lens = np.zeros(8, np.uint32)
    tr[req, :L - 1] = pack("R", a, 0)
    tr[req, L - 1] = pack("W", a, 0x5A)
    lens[req] = L
    tr[sharer, 0] = pack("R", a, 0)
    lens[sharer] = 1
    return tr, lens


def quiet_system(L):
    """Every node reads blocks of its own memory, round robin over eight of them: requests, replies
    and eviction notices, no write, so no REPLY_ID, INV or UPGRADE; active for longer than an
    upgrade_system of the same length."""
    tr = np.zeros((8, L), np.uint16)
    for n in range(8):
        tr[n] = [pack("R", (n << 4) | (i % 8), 0) for i in range(L)]
    return tr, np.full(8, L, np.uint32)


# (system of the wave, home, requester, sharer): lane 0 = node 0 of system 0 and lane 63 = node 7
# of system 7 in each of the three roles, and a system in the middle of the wave
PLACEMENTS = [(0, 0, 1, 2), (0, 1, 0, 2), (0, 1, 2, 0), (7, 7, 5, 6), (7, 5, 7, 6), (7, 5, 6, 7), (3, 2, 4, 6)]


@pytest.mark.parametrize("where,home,req,sharer", PLACEMENTS)
def test_rare_pops_in_one_lane(dash, where, home, req, sharer):
    """One wave of eight systems of which one alone ever pops REPLY_ID, INV or UPGRADE, one lane at
    a time: the wave-uniform test must see that lane wherever it sits, and the other 56 lanes'
    results (checked system by system) must not notice."""
    L = 16
    systems = [quiet_system(L) for _ in range(8)]
    systems[where] = upgrade_system(home, req, sharer, L)
    packed = np.stack([s[0] for s in systems])
    lens = np.stack([s[1] for s in systems])
    alone = run_system(packed[where], lens[where], num_procs=8, cache_size=4)
    assert [alone.hist[k] for k in (T_RID, T_INV, T_UPG)] == [1, 1, 1]
    stats = check_batch(dash, packed, lens, 8, 4)
    assert stats["hist"][T_RID:T_UPG + 1] == [1, 1, 1]


def test_quiescence_in_every_round_of_a_trip(dash):
    """`rounds` is exact wherever in a four-round trip a system goes quiet: node 0 alone runs 1..8
    instructions (reads of one block of its own, then hits), so consecutive systems end one round
    apart; all eight in one wave, then each in a wave of its own."""
    packed = np.zeros((8, 8, 8), np.uint16)
    lens = np.zeros((8, 8), np.uint32)
    for s in range(8):
        packed[s, 0, :s + 1] = pack("R", 0x03, 0)
        lens[s, 0] = s + 1
    rounds = [run_system(packed[s], lens[s], num_procs=8, cache_size=4).rounds for s in range(8)]
    assert {r % 4 for r in rounds} == {0, 1, 2, 3}
    check_batch(dash, packed, lens, 8, 4)
    for s in range(8):
        check_batch(dash, packed[s:s + 1], lens[s:s + 1], 8, 4)


def test_deep_queues_reach_the_second_tier(dash):
    """Maximum depth and the hand-off: two contention systems whose queues exceed 16 entries are
    re-run by the 32-deep kernel, next to one that stays shallow (the traces of
    test_queue_depth_tiers)."""
    ids = DEEP_SYSTEMS[:2] + [0]
    L = 4096
    packed = np.stack([oracle_ctypes.gen_system(0x5EED, s, 8, L, kind=1) for s in ids])
    lens = np.full((len(ids), 8), L, np.uint32)
    stats = check_batch(dash, packed, lens, 8, 4)
    assert stats["tier_systems"][0] == 3 and stats["tier_systems"][1] == 2
    assert stats["max_depth"] > 16
