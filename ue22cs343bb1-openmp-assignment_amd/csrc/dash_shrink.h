// dash_shrink.h -- the device side of dash_shrink (dash_shrink.hip): the candidate enumeration, stated
// once for the host and the kernels, and the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

constexpr uint32_t SHRINK_MAX_LEN = 1u << 24;  // dash_create's bound on max_instr

struct ShrinkCand {
    uint32_t node, start, count;
};

// The candidate enumeration of include/dash.h (dash_shrink): by node ascending, by level j = J .. 0
// (2^J >= lens[t] > 2^(J-1)), by block start. Returns C, the number of candidates of the base, and sets
// `out` to candidate c when c < C (it is left alone otherwise). dash_shrink_candidate, the candidate
// kernel and the apply kernel all decode through this one function. lens[t] <= SHRINK_MAX_LEN.
__host__ __device__ inline uint64_t shrink_decode(const uint32_t* lens, uint32_t num_procs, uint64_t c, ShrinkCand& out) {
    uint64_t total = 0;  // the candidates of the nodes and levels before this one; c >= total until found
    bool found = false;
    for (uint32_t t = 0; t < num_procs; t++) {
        const uint32_t L = lens[t];
        if (!L) continue;
        uint32_t J = 0;
        while ((1u << J) < L) J++;
        for (uint32_t j = J + 1; j-- > 0;) {
            const uint32_t blocks = (L + (1u << j) - 1u) >> j;
            if (!found && c - total < blocks) {
                const uint32_t s = (uint32_t)(c - total) << j;
                out.node = t;
                out.start = s;
                out.count = L - s < (1u << j) ? L - s : 1u << j;
                found = true;
            }
            total += blocks;
        }
    }
    return total;
}

// The winner cell of a round: count << 32 | (0xFFFFFFFF - c), 0 = no candidate passed. Its maximum is the
// passing candidate that deletes the most, the lowest index among equals (C < 2^32 for any base).
__host__ __device__ inline unsigned long long shrink_key(uint32_t count, uint64_t c) {
    return (unsigned long long)count << 32 | (0xFFFFFFFFu - (uint32_t)c);
}
__host__ __device__ inline uint64_t shrink_key_candidate(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

// ---- the chunk arithmetic of the variant kernel (dash_shrink.hip), host-callable so that a CPU program
// can check it against a plain deletion ----

__host__ __device__ inline uint64_t chunk_load(const uint2* p) {
    const uint2 v = *p;
    return (uint64_t)v.y << 32 | v.x;
}

// the low n instructions (16 bits each) of a chunk, n < 4
__host__ __device__ inline uint64_t low_instrs(uint32_t n) { return (1ull << (16u * n)) - 1ull; }

// Chunk q of a stream of the base (L instructions, nchunks chunks) without instructions
// [start, start + count); count == 0: the base's own chunk, cleared past L.
__host__ __device__ inline uint64_t variant_chunk(const uint2* stream, uint32_t nchunks, uint32_t L, uint32_t q,
                                                  uint32_t start, uint32_t count) {
    const uint32_t i0 = 4u * q, newL = L - count;
    if (i0 >= newL) return 0ull;
    uint64_t v;
    if (count == 0 || i0 + 4u <= start) {
        v = chunk_load(stream + q);
    } else {
        const uint32_t o = i0 + count, a = o >> 2, sh = 16u * (o & 3u);
        // i0 < newL, so o < L: chunk a holds instructions of the base; a + 1 may be past the stream
        const uint64_t lo = chunk_load(stream + a);
        v = lo;
        if (sh) {
            const uint64_t hi = a + 1u < nchunks ? chunk_load(stream + a + 1u) : 0ull;
            v = lo >> sh | hi << (64u - sh);
        }
        if (i0 < start) {  // start cuts this chunk: 1..3 instructions stay
            const uint64_t keep = low_instrs(start - i0);
            v = (chunk_load(stream + q) & keep) | (v & ~keep);
        }
    }
    if (newL - i0 < 4u) v &= low_instrs(newL - i0);
    return v;
}

enum ShrinkMode : uint32_t {
    SHRINK_CANDIDATES = 0,  // system k := the base without candidate first + k (past C: the base itself)
    SHRINK_COPY = 1,        // every system := the base
    SHRINK_APPLY = 2,       // system 0 := the base without the winner in *cell; nothing when *cell == 0
};

// One launch of variant_kernel: `nsys` systems written from one base. All rows are in the engine's
// lane-contiguous layout: a system is `row` consecutive 8-B chunks, node t's stream the nchunks chunks at
// t * nchunks, four packed instructions per chunk.
struct VariantArgs {
    const uint2* base;          // one system row
    const uint32_t* base_lens;  // [num_procs]
    uint2* dst;                 // nsys rows
    uint32_t* dst_lens;         // [nsys * num_procs]
    uint32_t* dst_count;        // optional [nsys]: the instructions system k's candidate deletes (0: none)
    uint64_t nsys, row, first;
    uint32_t nchunks, num_procs;
    uint32_t wchunks;           // chunks written per stream, 1 .. nchunks: covers the base's longest trace
                                // (the simulator reads nothing past a stream's length but its two refill chunks)
    uint32_t mode;              // ShrinkMode
    const unsigned long long* cell;  // SHRINK_APPLY
};
hipError_t launch_variants(const VariantArgs& a, hipStream_t s);

// The goal over systems [0, counted) of a sub-pass whose system 0 holds candidate `first`: the key of every
// passing one into *cell (one 64-bit atomicMax per wave that has any)
hipError_t launch_select(const uint32_t* errors, const uint4* coh, const uint32_t* count, uint64_t counted,
                         uint64_t first, uint32_t coh_all, uint32_t err_all, uint32_t err_none,
                         unsigned long long* cell, hipStream_t s);
// seeds[k] = seed for k < n
hipError_t launch_fill_u64(uint64_t* seeds, uint64_t n, uint64_t seed, hipStream_t s);

}  // namespace dash
