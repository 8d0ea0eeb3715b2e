"""The states that tests/test_gpu_coherence_states.py writes into a handle (dash_test_write_states)
for coherence_kernel to classify, chosen so that every slip of tests/coherence_mutants.py decides at
least 3 records per shape (tests/test_coherence_adequacy.py asserts it).

TEST INFRASTRUCTURE, CPU only, no library call: corpus(N, CS) is generated at import time of the
tests that use it, deterministically (random.Random with a seed per shape), in well under a second
per shape, so no fixture is committed.

Candidates are *sparse*: the initial state with one or two perturbed directory entries and up to
four perturbed lines (candidates()), plus the hand-built states of tests/test_coherence_spec.py moved
to every home lane of the shape (hand_built()). On a uniformly random state nearly every address
already carries DIR_EM or a sharer bit, and the record -- OR of bits, count of addresses, lowest
address -- saturates, so a slipped term changes nothing (DESIGN.md §5.2 has the measurement).

A state is a list of Node; untouched nodes are the shape's initial Node objects themselves (the
mutants' `pristine` shortcut relies on that identity).
"""
import functools
import random

import coherence_mutants as cm
import coherence_ref as cr

SHAPES = ((1, 1), (2, 4), (3, 2), (4, 4), (5, 1), (5, 3), (8, 4), (8, 12), (8, 16))
NEED = 3      # systems of the corpus that every slip must change
POOL = 700    # generated candidates the cover chooses from, per shape
BUDGET = 20000  # candidates that must not tell an exempt cell apart, per shape
VALUES = (0, 7, 8)


class Node:
    """dash_node_state as plain lists (all 16 lines; those at or past cache_size are zero, as
    dash_init_node_state leaves them)."""
    __slots__ = ("memory", "dir_bitvector", "dir_state", "cache_addr", "cache_value", "cache_state")

    def __init__(self, t, CS):
        self.memory = [(20 * t + b) & 0xFF for b in range(16)]
        self.dir_bitvector = [0] * 16
        self.dir_state = [cr.U] * 16
        self.cache_addr = [0xFF if i < CS else 0 for i in range(16)]
        self.cache_value = [0] * 16
        self.cache_state = [cr.INVALID if i < CS else 0 for i in range(16)]

    def copy(self):
        c = Node.__new__(Node)
        for f in Node.__slots__:
            setattr(c, f, list(getattr(self, f)))
        return c

    def key(self):
        return tuple(tuple(getattr(self, f)) for f in Node.__slots__)


@functools.lru_cache(maxsize=None)
def initial(N, CS):
    return tuple(Node(t, CS) for t in range(N))


class Builder:
    """Copy-on-write edits of the initial state."""

    def __init__(self, N, CS):
        self.N, self.CS, self.nodes = N, CS, list(initial(N, CS))

    def own(self, t):
        if self.nodes[t] is initial(self.N, self.CS)[t]:
            self.nodes[t] = self.nodes[t].copy()
        return self.nodes[t]

    def entry(self, a, d, bv, mem=None):
        s = self.own(a >> 4)
        s.dir_state[a & 15], s.dir_bitvector[a & 15] = d, bv
        if mem is not None:
            s.memory[a & 15] = mem

    def line(self, u, i, addr, value, state):
        s = self.own(u)
        s.cache_addr[i], s.cache_value[i], s.cache_state[i] = addr, value, state

    def mem(self, a):
        return self.nodes[a >> 4].memory[a & 15]


# ---------------------------------------------------------------- candidates

def candidate(rng, N, CS):
    b = Builder(N, CS)
    blocks = (0, 5, 15, rng.randrange(16))
    addrs = [rng.randrange(N) << 4 | rng.choice(blocks) for _ in range(rng.choice((1, 1, 2)))]
    for a in addrs:
        d = rng.choice((cr.EM, cr.S, cr.U, 3))
        kind = rng.randrange(6)
        if kind == 0:
            bv = 0
        elif kind == 1:
            bv = 1 << rng.randrange(N)
        elif kind == 2:
            bv = 1 << rng.randrange(N) | 1 << rng.randrange(N)
        elif kind == 3:
            bv = (1 << N) - 1
        elif kind == 4:  # a byte with bits at or above N (at N = 8 there is none: a full byte)
            bv = ((1 << rng.randrange(N)) | (1 << rng.randrange(N, 8))) if N < 8 else 0xFF
        else:
            bv = rng.randrange(256)
        b.entry(a, d, bv, rng.choice((None, None, 0, 7)))
    last = None
    for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 4))):
        u, i = rng.randrange(N), rng.randrange(CS)
        r = rng.random()
        if last is not None and CS >= 2 and r < 0.2:  # the same address again in the same cache
            u, addr = last
            i = rng.randrange(CS)
        elif r < 0.75:
            addr = rng.choice(addrs)
        elif r < 0.9:  # homed at or past N, 0xFF among them
            addr = rng.choice((0xFF, rng.randrange(N, 16) << 4 | rng.choice(blocks)))
        else:
            addr = rng.randrange(N * 16)
        home = addr >> 4
        mem = b.mem(addr) if home < N else 0
        b.line(u, i, addr, rng.choice(VALUES + (mem, mem)), rng.choice((0, 1, 2, 2, 3)))
        last = (u, addr)
    return b.nodes


def candidates(N, CS, count, seed=0):
    rng = random.Random(1000 * N + CS + 100003 * seed)
    return [candidate(rng, N, CS) for _ in range(count)]


def hand_built(N, CS):
    """The hand-built states of tests/test_coherence_spec.py at address t << 4 | 5 for every home t,
    their lines on the nodes after t (wrapping) and, when the nodes run out, on further lines. A state
    that needs more lines than the shape has is left out."""
    out = []
    for t in range(N):
        A = t << 4 | 5
        slots = [((t + 1 + k) % N, i) for i in range(CS) for k in range(N)]

        def build(lines, entry=None, extra=()):
            if len(lines) > len(slots):
                return
            b = Builder(N, CS)
            mem0 = b.mem(A)
            for (u, i), (val, st) in zip(slots, lines):
                b.line(u, i, A, mem0 if val is None else val, st)
            if entry:
                b.entry(A, *entry)
            for e in extra:
                e(b)
            out.append(b.nodes)

        u0, u1 = slots[0][0], slots[min(1, len(slots) - 1)][0]
        two = (1 << u0) | (1 << u1)
        build([(7, cr.MODIFIED), (7, cr.SHARED)], (3, two, 7))                 # SWMR alone
        build([(None, cr.SHARED)])                                            # DIR_U_HELD
        build([], (cr.EM, 0))                                                 # DIR_EM
        build([], (cr.S, 0))                                                  # DIR_S
        build([(None, cr.SHARED), (None, cr.SHARED)], (cr.S, 1 << u0))        # LOST_SHARER
        build([(None, cr.SHARED)], (cr.S, 1 << u0 | 1 << ((u0 + 1) % 8)))     # STALE_SHARER
        build([(46, cr.SHARED)], (cr.S, 1 << u0))                             # STALE_VALUE
        build([(8, cr.MODIFIED), (7, cr.SHARED)], (3, two, 7))                # SWMR | VALUE_SPLIT
        build([(None, cr.SHARED), (44, cr.SHARED)], (cr.S, two))              # STALE_VALUE | VALUE_SPLIT
        build([(None, cr.SHARED), (None, cr.SHARED)], (cr.S, two))            # clean
        build([(99, cr.INVALID)])                                             # an INVALID line
        build([], None, [lambda b: b.line(u0, 0, 0xFF, 3, cr.MODIFIED)])      # the initial address, valid
        build([], None, [lambda b: b.line(u0, 0, ((N + t) & 15) << 4 | 5, 3, cr.MODIFIED)])  # homed past N
        build([(None, cr.SHARED)], (cr.S, 1 << u0))                           # clean
        if N < 8:
            build([(None, cr.SHARED)], (cr.S, 1 << u0 | 1 << N))              # a bitVector bit at N
        build([(9, cr.EXCLUSIVE)], (cr.EM, 1 << u0, 9))                       # clean
        if CS >= 2:  # the same address twice in one cache
            build([], (cr.EM, 1 << u0, 9), [lambda b: b.line(u0, 0, A, 9, cr.EXCLUSIVE),
                                            lambda b: b.line(u0, CS - 1, A, 9, cr.EXCLUSIVE)])
        if N >= 2:   # the holder of the higher address is the lower node: first_addr is by address
            lo, hi = sorted((((t + 1) % N) << 4 | 3, A))
            build([], None, [lambda b: b.line(0, 0, hi, b.mem(hi), cr.SHARED),
                             lambda b: b.line(N - 1, 0, lo, 0, cr.SHARED)])
    return out


# ---------------------------------------------------------------- exemptions

def _exemptions():
    """(mutant, shape) -> why the slip cannot change a record at that shape."""
    ex = {}
    for N, CS in SHAPES:
        if N == 8:
            ex[10, (N, CS)] = "the mask of num_procs = 8 bits is the whole byte"
        if N & (N - 1) == 0:
            ex[19, (N, CS)] = "num_procs is a power of two: P = num_procs, no node lies in [num_procs, P)"
        if N == 1:
            ex[18, (N, CS)] = "one home: every order of the homes is the same order"
        if N * CS == 1:
            one = "the system has one line, so n2 is never set"
            ex[1, (N, CS)] = one + ": SWMR is never set either way"
            ex[2, (N, CS)] = one + ": SWMR is never set either way"
            ex[4, (N, CS)] = one + " and !n2 is always true"
            ex[17, (N, CS)] = one + ": `had` is only ever evaluated for a first copy, where both forms are false"
            ex[25, (N, CS)] = "line 0 of node 0 is the only line: both indices are 0"
        if CS == 1:
            ex[13, (N, CS)] = "a node has one line, so no node holds a second line of an address"
            ex[16, (N, CS)] = "a node has one line, so the copies of an address are as many as its holders"
    return ex


EXEMPT = _exemptions()


# ---------------------------------------------------------------- the corpus

def records(nodes, N, CS, slips=cm.SLIPS):
    """{0: the reference's record, m: the record under slip m}."""
    init = initial(N, CS)
    return {m: cm.check(nodes, N, CS, m, pristine=init)[0] for m in (0,) + tuple(slips)}


def kills(nodes, N, CS, slips=cm.SLIPS):
    rec = records(nodes, N, CS, slips)
    return frozenset(m for m in slips if rec[m] != rec[0])


def state_key(nodes):
    return tuple(s.key() for s in nodes)


@functools.lru_cache(maxsize=None)
def pool(N, CS):
    seen, out = set(), []
    for nodes in hand_built(N, CS) + candidates(N, CS, POOL):
        k = state_key(nodes)
        if k not in seen:
            seen.add(k)
            out.append(nodes)
    return out


@functools.lru_cache(maxsize=None)
def corpus(N, CS):
    """The fewest states a greedy cover finds such that every slip that is not exempt at the shape
    changes the record of at least NEED of them; in the pool's order. The initial state comes first."""
    cand = pool(N, CS)
    killed = [kills(nodes, N, CS) for nodes in cand]
    need = {m: NEED for m in cm.SLIPS if (m, (N, CS)) not in EXEMPT}
    chosen = []
    while any(need.values()):
        gain = [(sum(1 for m in k if need.get(m, 0) > 0), -idx) for idx, k in enumerate(killed)]
        best, neg = max(gain)
        if best == 0:
            break  # the adequacy test reports the cells left short
        idx = -neg
        chosen.append(idx)
        for m in killed[idx]:
            if need.get(m, 0) > 0:
                need[m] -= 1
        killed[idx] = frozenset()
    return [list(initial(N, CS))] + [cand[i] for i in sorted(chosen)]
