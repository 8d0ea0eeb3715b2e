"""TEST INFRASTRUCTURE (oracle only; never touches the engine): are the parity inputs adequate?

Every GPU parity test compares sim_kernel with the oracle on some traces. A wrong term of the
kernel's mask algebra shows only on traces that reach the protocol state the term guards. This
module measures that reach with the oracle's mutant builds (oracle/Makefile `mutants`, oracle/
dash_oracle.c ORC_MUTANT): build k deviates from the checker in one handler, so a trace on which
build k and the checker give the same (digest, rounds, errors, hist) would let a kernel with
that deviation pass.

  * MUTANTS: 1..13 are ref_pin.MUTANTS (misreadings of the reference), 14.. are slips of single
    terms of the kernel's dispatch (csrc/dash_kernels.hip), each named by the expression it
    mirrors. EQUIVALENT lists the candidates that no input tells apart (they are not built).
  * kills(): per system, whether a mutant differs from the checker under the round model
    (lockstep, or each system's own schedule seed: what MODE 0/2 and MODE 1/3 kernels see).
  * micro_kills(): the same for a STRICT micro-step walk (orc_random_walk): the mutant rejects
    the walk, ends non-terminal, or ends in another digest / hist / error bits (MODE 4).
  * candidates(): the deterministic candidate generator of the adequacy corpus
    (tests/golden/make_adequacy_corpus.py), greedy_cover(): the set-cover selection.
  * `python tests/adequacy.py --audit [OUT.md]`: the kill table of the existing GPU corpora
    (generators imported from their test modules) and of the adequacy corpus.
"""
from __future__ import annotations

import ctypes
import functools
import json
import pathlib
import subprocess
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import oracle_ctypes as oc  # noqa: E402
import ref_pin  # noqa: E402

MUTANTS = dict(ref_pin.MUTANTS)
MUTANTS.update({
    14: "EVICT_SHARED at home with one sharer left elsewhere sends it no notice (mEsOne & ~mOwnHome in mVA)",
    15: "EVICT_SHARED at home with no sharer left does not set the directory U (es_pop == 0 in nds)",
    16: "EVICT_SHARED at home with one sharer left does not set the directory EM (mEsOne in nds)",
    17: "FLUSH_INVACK at home ORs the requester into the bitVector instead of replacing it (mFIA in hbv)",
    18: "FLUSH at home replaces the bitVector instead of OR-ing the requester in (hbv)",
    19: "FLUSH_INVACK at home does not write memory (mHomeH in ebase)",
    20: "FLUSH at home sets the directory S only when it was EM (mFLUSH & mtH in nds)",
    21: "WRITEBACK_INT sends its second FLUSH also when home == requester (H != msr in mVB)",
    22: "REPLY_RD / REPLY_ID / FLUSH / FLUSH_INVACK fills notify an eviction also when the line already "
        "holds the address (~mSame in mEv)",
    23: "evicting an EXCLUSIVE line sends EVICT_MODIFIED (evb)",
    24: "an RD issue leaves instr.value at the last WR's value (last_val)",
    25: "a WR hit on SHARED sends WRITE_REQUEST (the tA patch of miW & mHit)",
    26: "UPGRADE at a home whose entry is not S is dispatched as a WRITE_REQUEST (the UPGRADE rows of tatab / vstab)",
    27: "REPLY_ID's INVs are queued after its eviction notice (arrival bits 0 / 1)",
    28: "FLUSH_INVACK clears waitingForReply only at the requester (mFIA in wmask)",
    29: "WRITEBACK_INV invalidates only a line with the message's address (mWBINV in mToI)",
    30: "a matching INVALID line counts as a hit (~mlI in mHit)",
    31: "EVICT_MODIFIED does not write memory (mEMOD in ebase)",
    32: "INV invalidates the indexed line whatever its address (mSame in mToI)",
})
# candidates of the issue's table that no input told apart (50,000 candidates each at N = 4 and
# N = 8, every CACHE_SIZE class, lockstep and seeded): removed from MUTANTS by the search below
EQUIVALENT: dict[int, str] = {}
ISSUE_SIDE = (13, 24, 25, 30)  # mutants of issue_instruction: the only ones with a meaning at N = 1
CACHE_SIZES = (1, 2, 4, 8, 16, 3, 12)  # the five specialised kernels, the generic one below and above 8
MICRO_CS = (1, 4, 3)
NODE_COUNTS = (2, 3, 4, 5, 8)
MIN_KILLS = 3  # a condition, not a measurement: one coincidence must not carry a state
MAX_LEN = 24
MAX_SYSTEMS, MAX_MICRO = 256, 32
ROUND_CAP = 1024 + 256 * MAX_LEN  # the engine's default round cap at max_instr = MAX_LEN
BAD_ERRORS = oc.ERR_ROUNDCAP | oc.ERR_STUCK | oc.ERR_OVERFLOW
FIXTURE_DIR = oc.ROOT / "tests" / "golden" / "adequacy"
THREADS = 8


@functools.lru_cache(maxsize=None)
def lib(k=0):
    """The checker (k = 0) or mutant build k, made on demand like ref_pin does."""
    if k == 0:
        L = oc.lib()
    else:
        path = ref_pin.MUT_DIR / f"libdash_oracle_m{k}.so"
        if not path.exists():
            subprocess.run(["make", "-s", "-C", str(oc.ORACLE_DIR), "mutants"], check=True)
        L = oc.bind(path)
    V, U64, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.orc_run_many.argtypes = [ctypes.POINTER(oc.OrcCfg), V, U64, U64, V, V, U64, I, V, V, V, V, V]
    L.orc_run_many.restype = None
    return L


def run_many(L, packed, lens, N, CS, seeds=None, threads=THREADS):
    """Every system of a batch ([nsys][N][len] uint16, lens [nsys][N]) under one oracle build:
    (sig, max_depth, errors). sig is one row per system: digest (two words), rounds, errors and
    the 13 histogram counts -- two systems behave alike exactly when their rows are equal."""
    packed = np.ascontiguousarray(packed, np.uint16)
    lens = np.ascontiguousarray(lens, np.uint32)
    n = len(packed)
    assert packed.shape[1] == N and lens.shape == (n, N)
    cfg = oc.OrcCfg(N, CS, 256, ROUND_CAP if packed.shape[2] <= MAX_LEN else 1024 + 256 * packed.shape[2])
    sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
    dig, rnd, err = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    hist, depth = np.zeros((n, oc.NTXN), np.uint32), np.zeros(n, np.uint32)
    L.orc_run_many(ctypes.byref(cfg), packed.ctypes.data, N * packed.shape[2], packed.shape[2], lens.ctypes.data,
                   None if sd is None else sd.ctypes.data, n, threads if n >= 512 else 1, dig.ctypes.data, rnd.ctypes.data,
                   err.ctypes.data, hist.ctypes.data, depth.ctypes.data)
    sig = np.concatenate([dig.view(np.uint32).reshape(n, 2), rnd[:, None], err[:, None], hist], axis=1)
    return sig, depth, err


def kills(L, packed, lens, N, CS, seeds=None, base=None):
    """Per system: does build L give another (digest, rounds, errors, hist) than the checker under
    that system's arb_seed (seeds None: all lockstep)? base: the checker's run_many, if at hand."""
    base = base or run_many(lib(0), packed, lens, N, CS, seeds)
    return (run_many(L, packed, lens, N, CS, seeds)[0] != base[0]).any(axis=1)


# ---------------------------------------------------------------- micro-step form

def walk(tr, lens, N, CS, seed, weights):
    """One weighted random walk of the checker's STRICT model: (outcome, steps), or None when a
    queue of the model overflowed (it holds 40 messages: the model, not the reference, drops)."""
    out, steps = oc.random_walk(tr, lens, seed, weights=weights, num_procs=N, cache_size=CS)
    return None if out.errors & oc.ERR_OVERFLOW else (out, steps)


def replay(L, tr, lens, N, CS, steps):
    """The witness under build L: None if a step is not enabled or the end is not terminal, else
    (digest, error bits, hist)."""
    tr, lens = oc._tr(tr, lens)
    cfg = oc.OrcCfg(N, CS, 256, 0, 0, oc.MICRO_STRICT, 0)
    cfg.count_msgs = 1
    st = np.ascontiguousarray(steps, np.uint16)
    out, term = oc.OrcOutcome(), ctypes.c_int()
    rc = L.orc_replay_steps(ctypes.byref(cfg), tr.ctypes.data, tr.shape[1], lens.ctypes.data, 0, st.ctypes.data,
                            len(st), ctypes.addressof(out), ctypes.addressof(term))
    if rc != 0 or not term.value:
        return None
    return out.digest, out.errors, tuple(out.hist)


def micro_kills(L, tr, lens, N, CS, steps):
    """A mutant is told apart when it rejects the checker's walk, ends it non-terminal, or ends
    with another digest, other error bits or another hist."""
    want = replay(lib(0), tr, lens, N, CS, steps)
    assert want is not None, "the checker rejects its own walk"
    return replay(L, tr, lens, N, CS, steps) != want


# ---------------------------------------------------------------- candidates and selection

CHUNK = 1024


@functools.lru_cache(maxsize=8)
def _chunk(N, c):
    rng = np.random.default_rng([0xADE9, N, c])
    shape = (CHUNK, N, MAX_LEN)
    span = rng.choice([2, 4], CHUNK)                      # a small address span
    stride = rng.choice([1, 2, 3, 4, 8], CHUNK)           # blocks that share a line or do not
    b0 = rng.integers(0, 16, CHUNK)
    nh = rng.integers(1, N + 1, CHUNK)                    # 1..N homes in use
    perm = np.argsort(rng.random((CHUNK, N)), axis=1)     # the homes: the first nh of a permutation
    p_wr = rng.choice([0.3, 0.5, 0.7], CHUNK)
    p_pair = rng.choice([0.0, 0.0, 0.4], CHUNK)           # a read followed by a write of its line
    top = rng.choice([6, 12, MAX_LEN], CHUNK)
    lens = (rng.random((CHUNK, N)) * (top[:, None] + 1)).astype(np.uint32)
    hsel = (rng.random(shape) * nh[:, None, None]).astype(np.int64)
    home = np.take_along_axis(np.broadcast_to(perm[:, None, :], (CHUNK, N, N)), hsel, axis=2)
    blk = (b0[:, None, None] + stride[:, None, None] * (rng.random(shape) * span[:, None, None]).astype(np.int64)) % 16
    addr = (home << 4) | blk
    wr = rng.random(shape) < p_wr[:, None, None]
    pair = rng.random(shape) < p_pair[:, None, None]
    val = rng.integers(1, 256, shape)
    prev_ok = np.zeros((CHUNK, N), bool)
    prev_addr = np.zeros((CHUNK, N), np.int64)
    for i in range(MAX_LEN):
        use = pair[:, :, i] & prev_ok
        addr[:, :, i] = np.where(use, prev_addr, addr[:, :, i])
        wr[:, :, i] |= use
        prev_ok, prev_addr = ~wr[:, :, i], addr[:, :, i]
    packed = (wr.astype(np.uint32) << 15) | (addr.astype(np.uint32) << 8) | np.where(wr, val, 0).astype(np.uint32)
    packed = np.where(np.arange(MAX_LEN)[None, None, :] < lens[:, :, None], packed, 0).astype(np.uint16)
    seeds = rng.integers(1, 1 << 63, size=CHUNK, dtype=np.uint64) * 2 + 1  # 64-bit, never 0
    wseeds = rng.integers(1, 1 << 62, size=CHUNK, dtype=np.uint64)
    weights = rng.integers(1, 16, size=(CHUNK, N)).astype(np.uint32)
    for a in (packed, lens, seeds, wseeds, weights):
        a.setflags(write=False)
    return packed, lens, seeds, wseeds, weights


def candidates(N, ids):
    """Candidates `ids` of node count N: (packed [n][N][24], lens [n][N], schedule seeds, walk
    seeds, walk weights [n][N]). Candidate k is the same whatever else is asked for."""
    ids = np.asarray(ids, np.int64)
    parts = [[], [], [], [], []]
    for k in ids:
        ch = _chunk(N, int(k) // CHUNK)
        for p, a in zip(parts, ch):
            p.append(a[int(k) % CHUNK])
    return tuple(np.array(p) for p in parts)


def greedy_cover(K, need, limit):
    """Set cover with multiplicity. K: bool [cells][candidates]; every cell wants `need` chosen
    candidates that are True in it (a cell with fewer gets them all). Greedy: the candidate that
    serves most cells still short, lowest index first on ties. Returns (chosen indices in order
    of choice, cells still short)."""
    K = np.asarray(K, bool)
    want = np.minimum(K.sum(axis=1), need).astype(np.int64)
    left = np.ones(K.shape[1], bool)
    chosen = []
    while (want > 0).any() and len(chosen) < limit:
        gain = (K[want > 0] & left).sum(axis=0)
        c = int(np.argmax(gain))
        if gain[c] == 0:
            break
        chosen.append(c)
        left[c] = False
        want -= K[:, c]
        np.maximum(want, 0, out=want)
    return chosen, np.flatnonzero(want > 0).tolist()


# ---------------------------------------------------------------- the fixture

def load_fixture(N):
    """tests/golden/adequacy/n{N}.json -> dict with packed, lens, seeds (arrays) and micro (list of
    (packed [N][len], lens, walk seed, weights)), exempt (list)."""
    d = json.loads((FIXTURE_DIR / f"n{N}.json").read_text())
    n = len(d["systems"])
    packed = np.zeros((n, N, MAX_LEN), np.uint16)
    lens = np.zeros((n, N), np.uint32)
    for s, rec in enumerate(d["systems"]):
        for t, row in enumerate(rec["rows"]):
            words = [int(row[i:i + 4], 16) for i in range(0, len(row), 4)]
            packed[s, t, :len(words)] = words
            lens[s, t] = len(words)
    seeds = np.array([int(rec["seed"], 16) for rec in d["systems"]], np.uint64)
    micro = []
    for rec in d["micro"]:
        tr = np.zeros((N, MAX_LEN), np.uint16)
        ln = np.zeros(N, np.uint32)
        for t, row in enumerate(rec["rows"]):
            words = [int(row[i:i + 4], 16) for i in range(0, len(row), 4)]
            tr[t, :len(words)] = words
            ln[t] = len(words)
        micro.append((tr, ln, int(rec["walk_seed"], 16), np.array(rec["weights"], np.uint32)))
    return {"raw": d, "packed": packed, "lens": lens, "seeds": seeds, "micro": micro,
            "exempt": d.get("exempt", [])}


def n1_batch():
    """N = 1 has no fixture: every message is a self-message, so only the mutants of
    issue_instruction mean anything there. 64 one-node systems on 2 blocks of a CACHE_SIZE 1
    line, generated here and shared by the CPU and the GPU test."""
    rng = np.random.default_rng(0xADE91)
    packed = np.zeros((64, 1, MAX_LEN), np.uint16)
    lens = rng.integers(4, MAX_LEN + 1, size=(64, 1)).astype(np.uint32)
    for s in range(64):
        blocks = [int(b) for b in rng.choice(16, 2, replace=False)]
        for i in range(int(lens[s, 0])):
            w = rng.random() < 0.5
            packed[s, 0, i] = oc.pack("W" if w else "R", int(rng.choice(blocks)), int(rng.integers(1, 256)) if w else 0)
    seeds = rng.integers(1, 1 << 63, size=64, dtype=np.uint64) * 2 + 1
    return packed, lens, seeds


# ---------------------------------------------------------------- audit

def kill_counts(packed, lens, N, CS, seeds=None, mutants=None):
    base = run_many(lib(0), packed, lens, N, CS, seeds)
    return {k: int(kills(lib(k), packed, lens, N, CS, seeds, base).sum()) for k in (mutants or MUTANTS)}


def audit_rows():
    """(corpus, shapes x seeds, systems per row, per mutant: rows that tell it apart by fewer than
    MIN_KILLS systems, and the smallest count) for the GPU suite's own corpora."""
    sys.path.insert(0, str(oc.ROOT))  # the test modules import bench
    import test_gpu_parity as tp
    import test_gpu_system_seeds as tss
    import test_gpu_tiers as tt

    def table(name, rows):
        counts = [kill_counts(p, ln, N, CS, sd) for p, ln, N, CS, sd in rows]
        return name, len(rows), len(rows[0][0]), {k: (sum(c[k] < MIN_KILLS for c in counts), min(c[k] for c in counts))
                                                  for k in MUTANTS}

    shapes = [sh for sh in tp.test_random_traces_bit_exact.pytestmark[0].args[1] if sh[0] >= 2]
    yield table("test_random_traces_bit_exact (N >= 2)",
                [(*tp.random_batch(np.random.default_rng(1000 * N + CS), 160, N, 40), N, CS, None) for N, CS in shapes])
    rows = []
    for N, CS in tt.SHAPES:
        if N < 2:
            continue
        bs = tt.forced_batches(N, CS)
        p, ln = np.concatenate([b[0] for b in bs]), np.concatenate([b[1] for b in bs])
        for seed in tt.SEEDS[:2]:
            rows.append((p, ln, N, CS, None if seed == 0 else np.full(len(p), seed, np.uint64)))
    yield table("test_forced_tier_shape_matrix (N >= 2)", rows)
    rows = []
    for N, CS in tss.SHAPES:
        rng = np.random.default_rng(3100 + 16 * N + CS)
        p, ln = tp.random_batch(rng, 96, N, 48, hot_frac=0.3)
        sd = rng.integers(1, 1 << 64, size=96, dtype=np.uint64)
        sd[0] = sd[50] = 0
        rows.append((p, ln, N, CS, sd))
    yield table("test_parity_per_system", rows)
    for N in NODE_COUNTS:
        fx = load_fixture(N)
        rows = [(fx["packed"], fx["lens"], N, CS, sd) for CS in CACHE_SIZES for sd in (None, fx["seeds"])]
        yield table(f"adequacy corpus n{N}", rows)


def audit_markdown():
    out = ["| corpus | rows | systems per row | mutants told apart by fewer than 3 systems in some row "
           "(rows short / fewest systems) |", "|---|---|---|---|"]
    for name, nrows, nsys, per in audit_rows():
        short = ", ".join(f"m{k} ({a}/{b})" for k, (a, b) in per.items() if a)
        out.append(f"| {name} | {nrows} | {nsys} | {short or 'none'} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    if "--audit" in sys.argv:
        text = audit_markdown()
        args = [a for a in sys.argv[1:] if a != "--audit"]
        if args:
            pathlib.Path(args[0]).write_text(text)
        print(text, end="")
