"""Delay words and their enumeration (include/dash.h, dash_set_system_delays and dash_delay_space),
restated in Python for the tests: nothing here calls libdash. The enumeration comes from
itertools.combinations, the schedule of a word from its definition, and the outcome lists from the CPU
oracle run under the explicit table of every schedule of a space."""
import functools
import itertools
import json
from math import comb

import numpy as np

import coherence_ref as cr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN, ROOT

EMPTY, LOCKSTEP, SIT_OUT = 0xFFFF, (1 << 64) - 1, 0xFF
SCHED_DIR = ROOT / "tests" / "golden" / "schedules"
OUTCOMES_JSON = ROOT / "tests" / "golden" / "delay_outcomes.json"
OUT_FIELDS = ("digest", "count", "seed", "rounds", "errors")
# the accepted racy outputs of the reference and the fewest delays that reach them
ACCEPTED = {("test_3", "run_1"): 0, ("test_3", "run_2"): 1, ("test_4", "run_1"): 0, ("test_4", "run_2"): 1,
            ("test_4", "run_3"): 1, ("test_4", "run_4"): 2}


def slot(t, e, r):
    return t | e << 3 | r << 6


def pack(slots):
    """A delay word from up to four 16-bit slots, slot s at bits 16 s; the rest are empty."""
    word = LOCKSTEP
    for s, f in enumerate(slots):
        word = word & ~(0xFFFF << (16 * s)) | f << (16 * s)
    return word


def sits(word, t, rnd):
    for s in range(4):
        f = (word >> (16 * s)) & 0xFFFF
        if f != EMPTY and f & 7 == t and f >> 6 <= rnd < (f >> 6) + (1 << ((f >> 3) & 7)):
            return True
    return False


def schedule(word, N, rounds):
    """The rounds [0, rounds) of a delay word as a round table: SIT_OUT or the node's own position."""
    return np.array([[SIT_OUT if sits(word, t, r) else t for t in range(N)] for r in range(rounds)],
                    np.uint8).reshape(rounds, N)


def last_round(word):
    """One past the last round any slot of the word covers (0 for lockstep)."""
    ends = [((f >> 6) + (1 << ((f >> 3) & 7))) for f in ((word >> (16 * s)) & 0xFFFF for s in range(4)) if f != EMPTY]
    return max(ends, default=0)


def cell_slot(c, N, E):
    """Cell c = (r * N + t) * E + e as a slot."""
    return slot((c // E) % N, c % E, c // (E * N))


def count(R, N, E, D):
    return sum(comb(R * N * E, d) for d in range(D + 1))


def words(R, N, E, D):
    """Every delay word of the space in index order: by delay count, then the cell sets c_d > .. > c_1 in
    the order of their rank C(c_d, d) + .. + C(c_1, 1), which is ascending order of (c_d, .., c_1); slot s
    holds c_(s+1)."""
    M = R * N * E
    for d in range(D + 1):
        for cells in sorted(itertools.combinations(range(M), d), key=lambda c: c[::-1]):
            yield pack(cell_slot(c, N, E) for c in cells)


def words_fast(R, N, E, D):
    """words() without the sort, for the large spaces: the largest cell ascends outermost."""
    M = R * N * E

    def sets(d, below):
        if d == 0:
            yield ()
            return
        for top in range(d - 1, below):
            for rest in sets(d - 1, top):
                yield rest + (top,)

    for d in range(D + 1):
        for cells in sets(d, M):
            yield pack(cell_slot(c, N, E) for c in cells)


def word_at(R, N, E, D, index):
    """The word of one index: its block, then greedily the largest cell whose binomial fits the rank."""
    M, d, j = R * N * E, 0, index
    while j >= comb(M, d):
        j -= comb(M, d)
        d += 1
    assert d <= D
    cells = []
    for k in range(d, 0, -1):
        c = k - 1
        while comb(c + 1, k) <= j:
            c += 1
        j -= comb(c, k)
        cells.append(c)
    return pack(cell_slot(c, N, E) for c in reversed(cells))


def delay_count_of(word):
    return sum(((word >> (16 * s)) & 0xFFFF) != EMPTY for s in range(4))


def run_word(tr, lens, word, N=4, CS=4, **kw):
    """The oracle under the word's table (rounds past the table are lockstep there too)."""
    return oc.run_system(tr, lens, num_procs=N, cache_size=CS, sched=schedule(word, N, max(last_round(word), 1)), **kw)


def oracle_list(tr, lens, R, E, D, N=4, CS=4, coherence=True):
    """The distinct (digest, errors) outcomes of the space on the oracle, in witness-index order: count,
    the lowest index, that witness's rounds and the reference's coherence record of its final state."""
    found = {}
    for i, w in enumerate(words_fast(R, N, E, D)):
        r = run_word(tr, lens, w, N, CS)
        o = found.get((r.digest, r.errors))
        if o is None:
            o = found[(r.digest, r.errors)] = dict(digest=r.digest, count=0, seed=i, rounds=r.rounds, errors=r.errors)
            if coherence:
                o.update(cr.check(r.node, N, CS)[0])
        o["count"] += 1
    return list(found.values())


@functools.lru_cache(maxsize=None)
def golden(test):
    return oc.load_test_dir(GOLDEN / test)


@functools.lru_cache(maxsize=None)
def lockstep_rounds(test):
    return int(oc.run_system(*golden(test)).rounds)


@functools.lru_cache(maxsize=None)
def golden_list(test, D):
    """test_3 / test_4 at R = lockstep rounds, E = 7 (the spaces of DESIGN.md §2), run live."""
    return oracle_list(*golden(test), lockstep_rounds(test), 7, D)


def accepted_digest(test, run):
    return int(json.loads((SCHED_DIR / f"{test}_{run}.json").read_text())["digest"], 16)


def recorded(test):
    """tests/golden/delay_outcomes.json (written by tests/golden/make_delay_outcomes.py): the D = 2 list."""
    rec = json.loads(OUTCOMES_JSON.read_text())[test]
    assert (rec["starts"], rec["lens"], rec["max_delays"]) == (lockstep_rounds(test), 7, 2)
    return [{**o, "digest": int(o["digest"], 16)} for o in rec["outcomes"]]


# the generated 8-node source: 6 instructions per node, writes and reads crowded onto four addresses of
# node 0 so that a delayed node changes who wins; GEN_SEED is the first seed whose (8, 3, 2) space has
# more than one outcome
GEN_SEED, GEN_SPACE = 0, (8, 3, 2)


@functools.lru_cache(maxsize=None)
def generated(seed=GEN_SEED, N=8, L=6):
    rng = np.random.default_rng(0xDE1A + seed)
    is_w = rng.random((N, L)) < 0.6
    addr = rng.integers(0, 4, size=(N, L))  # node 0, blocks 0..3
    val = np.where(is_w, rng.integers(1, 256, size=(N, L)), 0)
    tr = ((is_w.astype(np.uint32) << 15) | (addr.astype(np.uint32) << 8) | val).astype(np.uint16)
    return tr, np.full(N, L, np.uint32)


@functools.lru_cache(maxsize=None)
def generated_list():
    return oracle_list(*generated(), *GEN_SPACE, N=8, CS=4)
