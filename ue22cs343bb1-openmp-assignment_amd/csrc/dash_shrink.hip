// dash_shrink.hip -- the device side of dash_shrink: every variant of a shrink round is written,
// checked and ranked without leaving the device (include/dash.h states the rule).
//
// Per round:  [clear the cell];  per sub-pass:  variants (SHRINK_CANDIDATES), [dash_run], [the coherence
// launch], select;  then:  variants (SHRINK_APPLY) into the other base row. The base is one system row
// and its lengths in a buffer of the handle; shrink_decode (dash_shrink.h) is the enumeration for all of
// them.
//
// variant_kernel writes whole 8-B chunks, four packed instructions each, along a node's stream: lane i
// of a wave holds chunk q0 + i, so a wave's store is 512 contiguous bytes. A workgroup serves one system
// (blockIdx.y, grid-stride) and so one candidate: its index and its decode depend on the block alone and
// stay in scalar registers. Deleting `count` instructions at `start` from a stream leaves
//   chunks wholly below start              as they are;
//   chunks wholly at or past start         instructions 4q + count .. 4q + count + 3 of the base: base
//                                          chunks a = (4q + count) / 4 and a + 1, joined by one funnel
//                                          shift of 16 * ((4q + count) % 4) bits;
//   the one chunk that start cuts          the same, with its instructions below start from base chunk q;
// and every instruction at or past the new length is 0.
#include "dash_shrink.h"

#include <algorithm>

namespace dash {
namespace {

constexpr uint32_t THREADS = 256;
constexpr uint32_t ITEMS_PER_BLOCK = 4 * THREADS;  // chunks a workgroup writes per system

__global__ __launch_bounds__(THREADS) void variant_kernel(VariantArgs a) {
    const uint32_t N = a.num_procs, W = a.wchunks;
    const uint32_t items = N * W;  // (node, chunk) pairs of one system
    uint64_t c = 0;
    bool decode = a.mode == SHRINK_CANDIDATES;
    if (a.mode == SHRINK_APPLY) {
        const unsigned long long key = *a.cell;
        if (key == 0ull) return;  // no winner: the other row stays as it is
        c = shrink_key_candidate(key);
        decode = true;
    }
    for (uint64_t k = blockIdx.y; k < a.nsys; k += gridDim.y) {
        ShrinkCand cand{0u, 0u, 0u};
        if (decode) {
            if (a.mode == SHRINK_CANDIDATES) c = a.first + k;
            shrink_decode(a.base_lens, N, c, cand);  // past C: cand stays {0, 0, 0}, the base itself
        }
        uint2* out = a.dst + k * a.row;
        const uint32_t end = min(items, (blockIdx.x + 1u) * ITEMS_PER_BLOCK);
        for (uint32_t i = blockIdx.x * ITEMS_PER_BLOCK + threadIdx.x; i < end; i += THREADS) {
            const uint32_t t = i / W, q = i - t * W;
            const uint32_t L = a.base_lens[t];
            const uint32_t cut = t == cand.node ? cand.count : 0u;
            const uint64_t v = variant_chunk(a.base + (uint64_t)t * a.nchunks, a.nchunks, L, q, cand.start, cut);
            out[(uint64_t)t * a.nchunks + q] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
            if (q == 0) a.dst_lens[k * N + t] = L - cut;
        }
        if (a.dst_count && blockIdx.x == 0 && threadIdx.x == 0) a.dst_count[k] = cand.count;
    }
}

__global__ __launch_bounds__(THREADS) void select_kernel(const uint32_t* errors, const uint4* coh, const uint32_t* count,
                                                         uint64_t counted, uint64_t first, uint32_t coh_all,
                                                         uint32_t err_all, uint32_t err_none, unsigned long long* cell) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < counted) {
        const uint32_t e = errors[i], bits = coh[i].x;
        if ((bits & coh_all) == coh_all && (e & err_all) == err_all && (e & err_none) == 0u)
            key = shrink_key(count[i], first + i);
    }
    // the wave's maximum, then one atomic for the wave
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), d, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u && key != 0ull) atomicMax(cell, key);
}

__global__ __launch_bounds__(THREADS) void fill_u64_kernel(uint64_t* p, uint64_t n, uint64_t v) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

hipError_t launch_variants(const VariantArgs& a, hipStream_t s) {
    if (a.num_procs < 1 || a.num_procs > 8 || a.mode > SHRINK_APPLY || (a.mode == SHRINK_APPLY && !a.cell))
        return hipErrorInvalidValue;
    if (a.wchunks < 1 || a.wchunks > a.nchunks || (uint64_t)a.num_procs * a.nchunks > a.row) return hipErrorInvalidValue;
    if (a.nsys == 0) return hipSuccess;
    const uint32_t items = a.num_procs * a.wchunks;  // <= 8 * 2^22 chunks
    const dim3 grid((items + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK, (uint32_t)std::min<uint64_t>(a.nsys, 65535));
    hipLaunchKernelGGL(variant_kernel, grid, dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_select(const uint32_t* errors, const uint4* coh, const uint32_t* count, uint64_t counted,
                         uint64_t first, uint32_t coh_all, uint32_t err_all, uint32_t err_none,
                         unsigned long long* cell, hipStream_t s) {
    if (counted == 0) return hipSuccess;
    const uint64_t blocks = (counted + THREADS - 1) / THREADS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_kernel, dim3((uint32_t)blocks), dim3(THREADS), 0, s, errors, coh, count, counted, first,
                       coh_all, err_all, err_none, cell);
    return hipGetLastError();
}

hipError_t launch_fill_u64(uint64_t* p, uint64_t n, uint64_t v, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + THREADS - 1) / THREADS;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_u64_kernel, dim3((uint32_t)blocks), dim3(THREADS), 0, s, p, n, v);
    return hipGetLastError();
}

}  // namespace dash
