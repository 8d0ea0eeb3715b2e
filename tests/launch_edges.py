"""Shapes at which the helper kernels' launches take a second trip, block or slab, and the inputs
of tests/test_gpu_launch_edges.py.

TEST INFRASTRUCTURE: used by tests/test_launch_edges_spec.py (CPU) and tests/test_gpu_launch_edges.py.

Every cap the GPU tests cross is stated here once, with the file it comes from;
tests/test_launch_edges_spec.py finds each in that file's text, so a changed cap fails there instead
of silently moving a test back under its boundary.

A large batch of S systems is a tile of T = 97 systems repeated: system k holds tile[k % T]. T is
prime, so every tile entry lands on every lane position of a wave, and a run is deterministic, so
every per-system result must satisfy got[k] == got[k % T]: the comparison over the whole batch is one
numpy expression, and only the first T systems go through the CPU references.
"""
import functools
import json
import pathlib

import numpy as np

import coherence_ref as cr
import oracle_ctypes as oc
from test_gpu_parity import random_batch

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "ue22cs343bb1-openmp-assignment_amd" / "csrc"

# ---------------------------------------------------------------- the caps, and where they are written

# file -> the text that states a cap there (whitespace as in the file)
CAP_SOURCES = {
    "dash_kernels.hip": [
        # launch_clear_rd, launch_broadcast: grids of at most 256 * 64 blocks of 256 threads
        "const uint64_t blocks = std::min<uint64_t>((words + 255) / 256, 256ull * 64);",
        "const uint64_t blocks = std::min<uint64_t>((work + 255) / 256, 256ull * 64);",
        # launch_mark: at most 1,024 blocks of 256 threads
        "const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1024);",
    ],
    "dash_outcomes.hip": [  # launch_replicate: as launch_broadcast
        "constexpr uint32_t THREADS = 256;",
        "const uint64_t blocks = std::min<uint64_t>((work + THREADS - 1) / THREADS, 256ull * 64);",
    ],
    "dash_shrink.hip": [  # row_grid: gridDim.y <= 65,535, 1,024 (node, chunk) items per x-block
        "constexpr uint32_t THREADS = 256;",
        "constexpr uint32_t ITEMS_PER_BLOCK = 4 * THREADS;",
        "(uint32_t)std::min<uint64_t>(rows, 65535)",
        # base_wchunks: a row's own share of the engine's wchunks
        "return min(cap, (longest + 3u) / 4u + 2u);",
    ],
    "dash_shrink.cpp": [  # the engine's wchunks: the longest source trace and its two refill chunks
        "std::min<uint64_t>(h->nchunks, ((uint64_t)src_max + 3) / 4 + 2)",
    ],
    "dash_coherence.hip": [  # launch_coherence: 4 waves per workgroup, at most 1,024 trips of one
        "constexpr uint32_t WAVES = 4;",
        "constexpr uint32_t MAX_TRIPS = 1024;",
        "grid = std::max<uint64_t>(grid, (blocks + MAX_TRIPS - 1) / MAX_TRIPS);",
    ],
    "dash_coherence.cpp": ["a.max_grid = (h->cfg.flags & DASH_TEST_ONE_GROUP) ? 1u : 0u;"],
    "dash_load.cpp": [  # dash_load_dirs_device: slabs of about 64 MiB, a 16-byte aligned share per file
        "(64ull << 20) / (slot * N)",
        "const uint64_t slot = std::max<uint64_t>((limit + 15) & ~15ull, 16);",
    ],
    "dash_text.h": ["return 19ull * max_instr;"],
    "dash_tools.cpp": [  # dash_write_digests: windows of 2 chunks of 65,536 lines per thread
        "constexpr uint64_t CHUNK = 1u << 16;",
        "const unsigned nt = host_threads(16);",
        "std::min<uint64_t>(n, 2ull * nt * CHUNK)",
    ],
    "dash_internal.h": ["std::min<uint64_t>({work, 16, std::thread::hardware_concurrency()})"],
    "dash_core.cpp": [  # the lane stride of the trace layout, and the event log's layout
        "h->nchunks = (lines + ((lines && !(lines & 1)) ? 1u : 0u)) * 16;",
        "h->d_events + sys * N * (uint64_t)R",
    ],
}

GRID_STRIDE_THREADS = 256 * 64 * 256   # clear_rd, broadcast, replicate: threads of the capped grid
MARK_THREADS = 1024 * 256              # mark_kernel's
VARIANT_MAX_Y = 65535                  # many_variant_kernel: systems per y-trip
VARIANT_ITEMS_PER_BLOCK = 1024         # and (node, chunk) items per x-block
COH_WAVES, COH_MAX_TRIPS = 4, 1024     # coherence_kernel
SLAB_BYTES = 64 << 20                  # dash_load_dirs_device
DIGEST_CHUNK, DIGEST_THREADS = 1 << 16, 16  # dash_write_digests

SHRINK_Y_SYSTEMS = 65_600                    # one more y-trip than VARIANT_MAX_Y systems
MARK_SYSTEMS = 300_000                       # more overflowing systems than MARK_THREADS
DIGEST_SYSTEMS = 2 * 16 * 65_536 + 70_000    # one full window of dash_write_digests and a partial one


def nchunks(max_instr):
    """dash_create's lane stride of the trace layout in 8-B chunks: an odd number of 128-B lines."""
    lines = (-(-max_instr // 4) * 8 + 127) // 128
    return (lines + (1 if lines and lines % 2 == 0 else 0)) * 16


def write_chunks(max_instr, max_len):
    """The shrink engine's chunks written per stream over a base whose longest trace is max_len."""
    return max(1, min(nchunks(max_instr), (max_len + 3) // 4 + 2))


def text_slot(max_instr):
    """dash_load_dirs_device's room per file in a slab."""
    return max((19 * max_instr + 15) & ~15, 16)


def per_slab(max_instr, num_procs, n):
    return max(1, min(max(n, 1), SLAB_BYTES // (text_slot(max_instr) * num_procs)))


# ---------------------------------------------------------------- the shared large shape

T = 97            # the tile: prime, so system k % T meets every lane position
S = 40_000        # systems of the large batch
N, CS, MAXLEN, MAX_INSTR = 8, 4, 40, 64
ROW = N * nchunks(MAX_INSTR)  # chunks of a system row
TILE_RNG = 97
EVENT_ROUNDS = 4096


@functools.lru_cache(maxsize=None)
def tile():
    """(packed [T, N, MAXLEN], lens [T, N]): contention on a small address space; system 0 is empty."""
    packed, lens = random_batch(np.random.default_rng(TILE_RNG), T, N, MAXLEN, block_span=4, hot_frac=0.3)
    lens[0] = 0
    packed[0] = 0
    return packed, lens


def tiled(arr, count=S):
    """arr[k % T] for k < count."""
    return arr[np.arange(count) % T]


def is_tiled(arr):
    """Every entry equals that of its tile system (structured arrays included)."""
    return np.array_equal(arr, arr[np.arange(len(arr)) % T])


@functools.lru_cache(maxsize=None)
def tile_runs(seed=0):
    """The oracle's runs of the tile (with their DEBUG logs) under the lockstep schedule or a seed."""
    packed, lens = tile()
    return [oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS, log=True, log_msgs=True, arb_seed=seed)
            for s in range(T)]


@functools.lru_cache(maxsize=None)
def tile_coherence(seed=0):
    """tests/coherence_ref.py's record of every tile system's final state on the oracle."""
    return [cr.check(res.node, N, CS)[0] for res, _ in tile_runs(seed)]


def clear_rd(packed, lens):
    """dash_load_traces' rule, in numpy: an RD word carries value 0, a WR word is untouched, and
    words at or past a node's length read as 0."""
    out = np.where(packed & 0x8000, packed, packed & 0xFF00).astype(np.uint16)
    out[np.arange(packed.shape[2])[None, None, :] >= lens[:, :, None]] = 0
    return out


def with_rd_garbage(packed, rng):
    """The words with non-zero garbage in the value bits of every RD word (words past a length too)."""
    rd = (packed & 0x8000) == 0
    dirty = packed.copy()
    dirty[rd] |= rng.integers(1, 256, size=int(rd.sum())).astype(np.uint16)
    return dirty


# ---------------------------------------------------------------- racy sources of few outcomes

SRC_G, SRC_K, SRC_LEN, SRC_RNG, SRC_PROBE = 13, 3100, 3, 13, 64


@functools.lru_cache(maxsize=None)
def racy_sources():
    """(packed [G, N, SRC_LEN], lens [G, N]): the first SRC_G systems of a random batch of short 8-node
    traces that reach more than one outcome under the seeded round schedules 0 .. SRC_PROBE - 1 (on
    the oracle). Short traces keep the outcome lists short, so every witness can be re-run."""
    packed, lens = random_batch(np.random.default_rng(SRC_RNG), 128, N, SRC_LEN, block_span=4, hot_frac=0.3)
    pick = []
    for s in range(len(packed)):
        seen = {(r.digest, r.errors) for r in (oc.run_system(packed[s], lens[s], num_procs=N, cache_size=CS,
                                                             arb_seed=seed) for seed in range(SRC_PROBE))}
        if len(seen) > 1:
            pick.append(s)
        if len(pick) == SRC_G:
            break
    assert len(pick) == SRC_G, "too few racy systems in the batch"
    return packed[pick], lens[pick]


# ---------------------------------------------------------------- the long shrink source (two x-blocks)

LONG_N, LONG_CS, LONG_M, LONG_S = 8, 4, 600, 4096
LONG_FIXTURE = ROOT / "tests" / "golden" / "shrink_long.json"


def long_source(rng_seed):
    """The first system of random_batch(default_rng(rng_seed), 8, 8, 600, fixed_len) that is incoherent
    with no error bit under the lockstep schedule: (index, trace, lens, bits), or None."""
    import shrink_ref as sr
    packed, lens = random_batch(np.random.default_rng(rng_seed), 8, LONG_N, LONG_M, block_span=4, hot_frac=0.3,
                                fixed_len=True)
    for k in range(8):
        bits, err = sr.outcome(packed[k], lens[k], LONG_N, LONG_CS, 0)
        if bits and not err:
            return k, packed[k], lens[k], bits
    return None


@functools.lru_cache(maxsize=None)
def long_fixture():
    """tests/golden/shrink_long.json (made by tests/golden/make_shrink_long.py): the source's rng seed
    and index, the goal bit, and the twin's steps, lengths and traces."""
    rec = json.loads(LONG_FIXTURE.read_text())
    lens = np.array(rec["lens"], np.uint32)
    trace = np.zeros((LONG_N, max(int(lens.max()), 1)), np.uint16)
    for t, row in enumerate(rec["trace"]):
        trace[t, :len(row)] = [int(w, 16) for w in row]
    rec["twin"] = (trace, lens, [tuple(s) for s in rec["steps"]])
    return rec


# ---------------------------------------------------------------- directories for the slab test

DIR_M, DIR_ENTRIES, DIR_DISTINCT = 4096, 250, 12


def dir_traces():
    """DIR_DISTINCT trace sets of 8 nodes at max_instr 4,096: ragged lengths, one file at the full
    4,096 records (set 0, node 3) and one empty (set 1, node 5)."""
    rng = np.random.default_rng(250)
    packed, lens = random_batch(rng, DIR_DISTINCT, N, DIR_M, block_span=4, hot_frac=0.3)
    lens = (lens % 300).astype(np.uint32)  # short files but for the full one: the text stays small
    lens[0, 3] = DIR_M
    lens[1, 5] = 0
    packed[np.arange(DIR_M)[None, None, :] >= lens[:, :, None]] = 0
    return packed, lens


def dir_order():
    """Which of the DIR_DISTINCT sets entry k of the list names: repeats, in no regular order."""
    return np.random.default_rng(251).integers(0, DIR_DISTINCT, DIR_ENTRIES)
