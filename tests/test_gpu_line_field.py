"""GPU parity where a line's new state rides in the message word.

The lockstep kernels of CACHE_SIZE 4, sim_kernel<P, 4, RING, 0>, take the state a cache line
changes to from two bits of the popped word, which the sender fills from its constant tables.
Every case is bit-exact parity with the CPU oracle through test_gpu_parity.check_batch: final
state of every node, digest, rounds, error bits, per-type histogram of every system, and the
run's totals.

* One hand-built 8-node system per line transition, as the first and the last system of a batch
  of 9 (one full wave and a wave that holds one system) and of 16 (two full waves); the other
  systems are quiet read-only ones. Each builder's `want` is checked on the oracle's result of
  the system alone first -- the histogram row of the type the case is about, and the line states
  the transition must leave -- so no case passes without its transition.
* Partial systems (N < P lanes used), generated traces, at every queue-depth tier, and one
  hand-built system per N whose eviction notice goes to a node >= N (DASH_ERR_OOB, one drop).
* N == P at every P.
"""
import numpy as np
import pytest

import oracle_ctypes
from oracle_ctypes import pack, run_system
from test_gpu_parity import check_batch

pytestmark = pytest.mark.gpu

(T_RR, T_WRQ, T_RRD, T_RWR, T_RID, T_INV, T_UPG, T_WBINV, T_WBINT, T_FLUSH, T_FIA, T_ES,
 T_EMOD) = range(13)
M, E, S, I = 0, 1, 2, 3  # cacheLineState
L = 64


def line(res, node, idx=0):
    s = res.node[node]
    return s.cache_addr[idx], s.cache_state[idx]


class Sys:
    """A system under construction: per-node instruction lists. `wait(n, k)` keeps node n busy for
    a while with reads of block 1 of its own memory (cache index 1: a miss, then k - 1 hits of one
    round each), so the accesses to the block under test (cache index 0) happen in a set order."""

    def __init__(self):
        self.ins = [[] for _ in range(8)]

    def rd(self, n, a):
        self.ins[n].append(pack("R", a, 0))
        return self

    def wr(self, n, a, v):
        self.ins[n].append(pack("W", a, v))
        return self

    def wait(self, n, k):
        self.ins[n] += [pack("R", (n << 4) | 1, 0)] * k
        return self

    def arrays(self):
        tr = np.zeros((8, L), np.uint16)
        lens = np.zeros(8, np.uint32)
        for n, w in enumerate(self.ins):
            assert len(w) <= L
            tr[n, :len(w)] = w
            lens[n] = len(w)
        return tr, lens


def shared_by(s, a, readers):
    """Block `a` ends SHARED in every reader's cache: the first read makes it EXCLUSIVE, the second
    is forwarded (WRITEBACK_INT, FLUSH), any later one gets REPLY_RD from a SHARED entry."""
    for k, n in enumerate(readers):
        s.wait(n, 1 + 12 * k).rd(n, a)
    return s


# every builder returns (Sys, want) with want(res) asserting on the oracle's result of the system
def reply_rd_exclusive():
    a = 0x30
    return Sys().rd(0, a), lambda r: (r.hist[T_RRD] == 1 and line(r, 0) == (a, E))


def reply_rd_shared():
    a = 0x30
    s = shared_by(Sys(), a, [0, 7, 5])
    # node 0's read and node 5's get a REPLY_RD (the three waits' too), node 5's from a SHARED entry;
    # node 7's is forwarded: a FLUSH to the home and one to node 7
    return s, lambda r: (r.hist[T_RRD] == 2 + 3 and r.hist[T_FLUSH] == 2
                         and [line(r, n) for n in (0, 7, 5)] == [(a, S)] * 3)


def reply_wr():
    a = 0x30
    return Sys().wr(7, a, 0x5A), lambda r: (r.hist[T_RWR] == 1 and line(r, 7) == (a, M))


def reply_id_inv_matching():
    a = 0x30
    s = shared_by(Sys(), a, [0, 7, 5]).wait(2, 40).wr(2, a, 0x77)
    return s, lambda r: (r.hist[T_RID] == 1 and r.hist[T_INV] == 3 and line(r, 2) == (a, M)
                         and [line(r, n) for n in (0, 7, 5)] == [(a, I)] * 3)


def inv_not_matching():
    """Node 7 shares block a, then reads another block of the same cache index while node 2's
    write is under way: the home lists node 7 when the write arrives, the INV finds the other
    block in the line and leaves it alone (`want` reads the order off the oracle's log)."""
    a, b = 0x30, 0x44
    s = shared_by(Sys(), a, [0, 7]).wait(2, 30).wr(2, a, 0x77)
    s.wait(7, INV_RACE_WAIT).rd(7, b)
    return s, lambda r: (r.hist[T_INV] == 2 and line(r, 0) == (a, I) and line(r, 7) == (b, E)
                         and inv_after_refill(s, 7, a, b))


INV_RACE_WAIT = 12  # node 7's second wait: its refill lands between the home's REPLY_ID and the INV (11..13 do)


def inv_after_refill(s, node, a, b):
    tr, lens = s.arrays()
    _res, log = run_system(tr, lens, num_procs=8, cache_size=4, log=True, log_msgs=True)
    mine = [x for x in log.splitlines() if x.startswith(f"Processor {node} msg")]
    fill = next(i for i, x in enumerate(mine) if f"type: {T_RRD}, address: 0x{b:02X}" in x)
    inv = next(i for i, x in enumerate(mine) if f"type: {T_INV}, address: 0x{a:02X}" in x)
    return fill < inv


def flush_invack(requester):
    """WRITEBACK_INV -> FLUSH_INVACK: node 0 owns the block MODIFIED, `requester` writes it. The
    owner's reply copies byte 3 of the forward (secondReceiver and the forward's own field, I)."""
    a = 0x30

    def build():
        s = Sys().wr(0, a, 0x11).wait(requester, 14).wr(requester, a, 0x22)
        return s, lambda r: (r.hist[T_WBINV] == 1 and r.hist[T_FIA] == 2
                             and line(r, requester) == (a, M) and line(r, 0) == (a, I))
    return build


def flush(requester):
    """WRITEBACK_INT -> FLUSH: node 0 owns the block MODIFIED, `requester` reads it (one FLUSH when
    the requester is the home, else one to each)."""
    a = 0x30

    def build():
        s = Sys().wr(0, a, 0x11).wait(requester, 14).rd(requester, a)
        return s, lambda r: (r.hist[T_WBINT] == 1 and r.hist[T_FLUSH] == (1 if requester == 3 else 2)
                             and line(r, requester) == (a, S) and line(r, 0) == (a, S))
    return build


def evict_shared_sharer_elsewhere():
    a, b = 0x30, 0x44
    s = shared_by(Sys(), a, [0, 7]).wait(0, 20).rd(0, b)  # node 0 replaces the line: node 7 is left
    return s, lambda r: (r.hist[T_ES] == 2 and line(r, 7) == (a, E) and line(r, 0) == (b, E))


def evict_shared_home_last():
    a, b = 0x30, 0x44
    s = shared_by(Sys(), a, [3, 0]).wait(0, 20).rd(0, b)  # the home itself is the sharer left
    return s, lambda r: (r.hist[T_ES] == 1 and line(r, 3) == (a, E) and line(r, 0) == (b, E))


def wr_hit_exclusive():
    a = 0x30
    return Sys().rd(7, a).wr(7, a, 0x33), lambda r: (r.hist[T_RRD] == 1 and r.hist[T_WRQ] == 0
                                                    and r.hist[T_UPG] == 0 and line(r, 7) == (a, M))


def wr_hit_modified():
    a = 0x30
    return Sys().wr(7, a, 0x33).wr(7, a, 0x34), lambda r: (r.hist[T_RWR] == 1 and r.hist[T_WRQ] == 1
                                                          and r.hist[T_UPG] == 0 and line(r, 7) == (a, M)
                                                          and r.node[7].cache_value[0] == 0x34)


def wr_hit_shared():
    a = 0x30
    s = shared_by(Sys(), a, [0, 7]).wait(7, 20).wr(7, a, 0x35)
    return s, lambda r: (r.hist[T_UPG] == 1 and r.hist[T_RID] == 1 and r.hist[T_INV] == 1
                         and line(r, 7) == (a, M) and line(r, 0) == (a, I))


CASES = {
    "reply_rd_E": reply_rd_exclusive, "reply_rd_S": reply_rd_shared, "reply_wr": reply_wr,
    "reply_id_inv": reply_id_inv_matching, "inv_other_block": inv_not_matching,
    "flush_invack": flush_invack(7), "flush_invack_home": flush_invack(3),
    "flush": flush(7), "flush_home": flush(3),
    "evict_shared_elsewhere": evict_shared_sharer_elsewhere, "evict_shared_home": evict_shared_home_last,
    "wr_hit_E": wr_hit_exclusive, "wr_hit_M": wr_hit_modified, "wr_hit_S": wr_hit_shared,
}


# the type a case is about (for a WR hit: the fill that made the line it hits); the run's histogram
# must hold the case's pops twice, next to what the quiet systems pop of that type
ABOUT = {
    "reply_rd_E": T_RRD, "reply_rd_S": T_FLUSH, "reply_wr": T_RWR, "reply_id_inv": T_RID, "inv_other_block": T_INV,
    "flush_invack": T_FIA, "flush_invack_home": T_FIA, "flush": T_FLUSH, "flush_home": T_FLUSH,
    "evict_shared_elsewhere": T_ES, "evict_shared_home": T_ES, "wr_hit_E": T_RRD, "wr_hit_M": T_RWR,
    "wr_hit_S": T_UPG,
}


def quiet_system():
    """Every node reads eight blocks of its own memory, round robin: requests, replies and eviction
    notices for the whole length of the batch, no sharing."""
    tr = np.zeros((8, L), np.uint16)
    for n in range(8):
        tr[n] = [pack("R", (n << 4) | (i % 8), 0) for i in range(L)]
    return tr, np.full(8, L, np.uint32)


@pytest.mark.parametrize("nsys", [9, 16])
@pytest.mark.parametrize("case", sorted(CASES))
def test_line_transition(dash, case, nsys):
    s, want = CASES[case]()
    tr, lens = s.arrays()
    alone = run_system(tr, lens, num_procs=8, cache_size=4)
    assert alone.errors == 0 and want(alone), f"{case}: the oracle's run lacks the transition"
    systems = [quiet_system() for _ in range(nsys)]
    systems[0] = systems[-1] = (tr, lens)
    packed = np.stack([x[0] for x in systems])
    lens = np.stack([x[1] for x in systems])
    stats = check_batch(dash, packed, lens, 8, 4)
    quiet = run_system(*quiet_system(), num_procs=8, cache_size=4)
    k = ABOUT[case]
    assert alone.hist[k] > 0 and stats["hist"][k] == 2 * alone.hist[k] + (nsys - 2) * quiet.hist[k]


TIER_FLAGS = {"tier16": 0, "tier32": 2, "tier256": 4}  # DASH_TIER_FROM_32 = 2, DASH_TIER_FROM_256 = 4


@pytest.mark.parametrize("tier", sorted(TIER_FLAGS))
@pytest.mark.parametrize("kind", [0, 1], ids=["uniform", "contention"])
@pytest.mark.parametrize("N", [3, 5, 6, 7])
def test_partial_systems(dash, N, kind, tier):
    packed = np.stack([oracle_ctypes.gen_system(0x5EED, s, N, L, kind=kind) for s in range(16)])
    lens = np.full((16, N), L, np.uint32)
    check_batch(dash, packed, lens, N, 4, flags=TIER_FLAGS[tier])


def oob_system(N):
    """An eviction notice to a node >= N (the reference's messageBuffers[15]): node 0 holds block
    0x14 EXCLUSIVE and replaces it while the home, node 1, writes it. The home's own request makes
    it the entry's one sharer, so node 0's EVICT_SHARED turns the home's line of that index -- never
    filled, address 0xFF -- EXCLUSIVE, and the FLUSH_INVACK's fill evicts it: a notice to node 15."""
    tr = np.zeros((N, 16), np.uint16)
    lens = np.zeros(N, np.uint32)
    w0 = [pack("R", 0x14, 0)] + [pack("R", 0x01, 0)] * OOB_WAIT[0] + [pack("R", 0x00, 0)]
    w1 = [pack("R", 0x11, 0)] * OOB_WAIT[1] + [pack("W", 0x14, 0xA6)]
    tr[0, :len(w0)], tr[1, :len(w1)] = w0, w1
    lens[0], lens[1] = len(w0), len(w1)
    return tr, lens


OOB_WAIT = (4, 6)  # hits before node 0's replacement and node 1's write: the notice passes the forward


@pytest.mark.parametrize("N", [3, 5, 6, 7])
def test_eviction_notice_to_a_node_past_the_system(dash, N):
    tr, lens = oob_system(N)
    alone = run_system(tr, lens, num_procs=N, cache_size=4)
    assert alone.errors == oracle_ctypes.ERR_OOB and alone.dropped == 1
    # next to generated systems, first and last of the batch
    gen = [oracle_ctypes.gen_system(0x5EED, s, N, 16, kind=0) for s in range(14)]
    packed = np.stack([tr] + gen + [tr])
    lens = np.stack([lens] + [np.full(N, 16, np.uint32)] * 14 + [lens])
    stats = check_batch(dash, packed, lens, N, 4)
    assert stats["err_bits"] & dash.ERR_OOB and stats["dropped"] >= 2


@pytest.mark.parametrize("kind", [0, 1], ids=["uniform", "contention"])
@pytest.mark.parametrize("N", [1, 2, 4, 8])
def test_full_systems_at_every_segment_width(dash, N, kind):
    packed = np.stack([oracle_ctypes.gen_system(0x5EED, s, N, L, kind=kind) for s in range(16)])
    lens = np.full((16, N), L, np.uint32)
    check_batch(dash, packed, lens, N, 4)
