// dash_coherence.hip -- the coherence invariants of every system's final state, checked on the
// device (include/dash.h states the definitions).
//
// One pass over d_state with the mapping of its writer (sim_kernel's epilogue): one lane per node,
// P = next_pow2(num_procs) lanes per system, 64 / P systems per wave. The states of a wave's
// systems are one contiguous span of (64 / P) * N * (16 + CS) words, at most 8 KB, whose base is
// 32-B aligned (64 / P >= 8). The wave stages it in LDS with 16-B loads, all issued before the
// first is stored; the span of the last wave is cut at the buffer's end, which need not fall on a
// 16-B boundary (N = 5, CS = 1), so its last chunk is loaded word by word.
//
// Lane t is the home of addresses t * 16 .. t * 16 + 15. It scans its system's N * CS lines --
// the lanes of a system read the same LDS word, a broadcast -- and keeps one accumulator word per
// block in a per-wave LDS table laid out [block][lane], so that any mix of blocks among the lanes
// of a wave hits 32 distinct banks per half-wave:
//   first value [7:0]  memory [15:8]  holders [23:16]  n >= 1 [24]  n >= 2 [25]  own >= 1 [26]
//   stale value [27]  value split [28]
// (two copies differ exactly when some copy differs from the first one seen). The bits of a block
// are then formed against the lane's own directory word, kept in registers. The record is reduced
// over the system's lanes (OR, add, min of address << 8 | bits) and stored by lane 0 as 16 bytes.
//
// A workgroup walks the batch in strides of the grid, which the launch sizes to the device (a few
// workgroups per CU). A wave loads its next span into registers before it scans the staged one,
// so the loads are in flight during the scan. The totals stay in per-lane registers over the walk
// (16-bit fields for the per-bit counts; the launch bounds the trips per workgroup so that none
// overflows) and are reduced once at the end: over the wave, over the workgroup's waves in LDS,
// then 20 device atomics per workgroup. With one wave per span and 20 atomics per wave, the first
// version spent nearly all of its time at 2^20 systems queueing on those 20 words.
#include "dash_coherence.h"

#include <algorithm>

#include "dash.h"

namespace dash {
namespace {

constexpr uint32_t WAVES = 4;          // per workgroup
constexpr uint32_t MAX_CHUNKS = 8;     // 16-B chunks per lane of the largest span (8 KB / 64 / 16)
constexpr uint32_t TABLE_WORDS = 16 * 64;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MAX_TRIPS = 1024;   // per workgroup: 16 addresses per lane and trip fit a 16-bit field

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// fields of a block's accumulator word
constexpr uint32_t F_MEM = 8, F_MASK = 16, F_N1 = 24, F_N2 = 25, F_OWN = 26, F_STALE = 27, F_SPLIT = 28;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// bits 0..3 of x to the low bits of bytes 0..3
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (x * 0x00204081u) & 0x01010101u; }

// Words [gw, gw + span) of the state buffer, cut at its end (`total` words), as this lane's 16-B
// chunks k * 64 + lane; zeros past the end. wid: the wave's index in the batch.
__device__ __forceinline__ void load_span(u32x4 (&v)[MAX_CHUNKS], const uint32_t* state, uint64_t total, uint64_t wid,
                                          uint32_t span, uint32_t lane) {
    const uint64_t gw = wid * span;
    const uint32_t valid = gw < total ? (uint32_t)(total - gw < span ? total - gw : span) : 0u;
    const uint32_t* src = state + gw;
#pragma unroll
    for (uint32_t k = 0; k < MAX_CHUNKS; k++) {
        const uint32_t w0 = (k * 64u + lane) * 4u;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (w0 + 4u <= valid) {
            v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + w0));
        } else if (w0 < valid) {  // the buffer ends inside this chunk
            v[k].x = src[w0];
            if (w0 + 1u < valid) v[k].y = src[w0 + 1u];
            if (w0 + 2u < valid) v[k].z = src[w0 + 2u];
        }
    }
}

// the 8-bit fields of x as 16-bit fields: bytes 0, 2 and bytes 1, 3
__device__ __forceinline__ void widen(uint32_t x, uint32_t& even, uint32_t& odd) {
    even += x & 0x00FF00FFu;
    odd += (x >> 8) & 0x00FF00FFu;
}

// 4 waves per SIMD: 128 VGPRs hold the next span's 32 and the 16 directory words without a spill,
// and four workgroups' LDS fit a CU at 8 nodes, CACHE_SIZE 4
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void coherence_kernel(
    CoherenceArgs a, uint32_t stage_words, uint32_t work) {
    extern __shared__ u32x4 smem[];  // per wave: the staged span, then the [block][lane] table
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t P = a.seg, N = a.num_procs, CS = a.cache_size, W = 16u + CS;
    const uint32_t spw = 64u / P, t = lane & (P - 1u), ls = lane / P;
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem) + wave * (stage_words + TABLE_WORDS);
    uint32_t* table = stage + stage_words;
    const uint32_t span = spw * N * W;
    const uint64_t total = a.nsys * N * W;
    // the totals of this lane over the walk; per-bit counts in 16-bit fields (bits 0, 2 | 1, 3 | 4, 6 | 5, 7)
    uint32_t t_systems = 0, t_bad = 0, t_bad_clean = 0, t_addrs = 0, t_bsys[4] = {0, 0, 0, 0}, t_baddr[4] = {0, 0, 0, 0};

    u32x4 v[MAX_CHUNKS];
    load_span(v, a.state, total, (uint64_t)blockIdx.x * WAVES + wave, span, lane);
    for (uint32_t blk = blockIdx.x; blk < work; blk += gridDim.x) {  // the same trips for a workgroup's waves
        const uint64_t wid = (uint64_t)blk * WAVES + wave;
        const uint64_t sys = wid * spw + ls;
        const bool live = sys < a.nsys && t < N;
        const bool head = sys < a.nsys && t == 0u;

        // ---- stage the wave's span, and start the loads of its next one ----
#pragma unroll
        for (uint32_t k = 0; k < MAX_CHUNKS; k++) {
            const uint32_t w0 = (k * 64u + lane) * 4u;
            if (w0 < stage_words) reinterpret_cast<u32x4*>(stage)[k * 64u + lane] = v[k];
        }
        __syncthreads();
        if (blk + gridDim.x < work) load_span(v, a.state, total, wid + (uint64_t)gridDim.x * WAVES, span, lane);

        // ---- this home's directory words, and its table column: memory set, nothing seen ----
        const uint32_t* mine = stage + (live ? (ls * N + t) * W : 0u);
        uint32_t dir[16];
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            dir[b] = mine[b];
            table[b * 64u + lane] = (dir[b] & 0xFFu) << F_MEM;
        }

        // ---- the scan: every line of the system, kept when it is a copy of one of this home's ----
        const uint32_t* lines = stage + (live ? ls * N * W : 0u) + 16u;
        for (uint32_t u = 0; u < N; u++) {
            for (uint32_t i = 0; i < CS; i++) {
                const uint32_t l = lines[u * W + i];
                const uint32_t addr = l & 0xFFu, val = (l >> 8) & 0xFFu, st = (l >> 16) & 3u;
                if (live && st != 3u && (addr >> 4) == t) {
                    uint32_t* cell = &table[(addr & 15u) * 64u + lane];
                    uint32_t x = *cell;
                    const uint32_t had = (x >> F_N1) & 1u;
                    const uint32_t split = had & ((x & 0xFFu) != val ? 1u : 0u);
                    const uint32_t stale = ((st == 1u) | (st == 2u)) & (((x >> F_MEM) & 0xFFu) != val ? 1u : 0u);
                    x |= had ? 0u : val;  // the first copy's value
                    x |= 1u << (F_MASK + u) | 1u << F_N1 | had << F_N2 | (st < 2u ? 1u : 0u) << F_OWN |
                     stale << F_STALE | split << F_SPLIT;
                    *cell = x;
                }
            }
        }

        // ---- the bits of this home's 16 addresses ----
        uint32_t bits_or = 0, addrs = 0, first = NONE, cnt_lo = 0, cnt_hi = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t x = table[b * 64u + lane];
            const uint32_t d = (dir[b] >> 16) & 3u, bv = (dir[b] >> 8) & 0xFFu, mask = (x >> F_MASK) & 0xFFu;
            const bool n1 = (x >> F_N1) & 1u, n2 = (x >> F_N2) & 1u, own = (x >> F_OWN) & 1u;
            uint32_t bits = 0;
            if (own && n2) bits |= DASH_COH_SWMR;
            if (d == 2u && n1) bits |= DASH_COH_DIR_U_HELD;
            if (d == 0u && !(n1 && !n2 && own)) bits |= DASH_COH_DIR_EM;
            if (d == 1u && (own || !n1)) bits |= DASH_COH_DIR_S;
            if (d != 2u && (mask & ~bv)) bits |= DASH_COH_LOST_SHARER;
            if (d != 2u && (bv & ~mask)) bits |= DASH_COH_STALE_SHARER;
            bits |= ((x >> F_STALE) & 1u) * DASH_COH_STALE_VALUE | ((x >> F_SPLIT) & 1u) * DASH_COH_VALUE_SPLIT;
            bits = live ? bits : 0u;  // dead lanes and dead systems contribute nothing
            bits_or |= bits;
            addrs += bits ? 1u : 0u;
            first = bits && first == NONE ? (t << 4 | b) << 8 | bits : first;  // ascending b: the lowest
            cnt_lo += spread4(bits & 15u);
            cnt_hi += spread4(bits >> 4);
        }

        // ---- the system's record: reduced over its P lanes, stored by lane 0 ----
        uint32_t sbits = bits_or, saddrs = addrs, skey = first;
        for (uint32_t n = 1; n < P; n <<= 1) {
            sbits |= __shfl_xor(sbits, n, 64);
            saddrs += __shfl_xor(saddrs, n, 64);
            const uint32_t o = __shfl_xor(skey, n, 64);
            skey = o < skey ? o : skey;
        }
        uint32_t err = 0;
        if (head) {
            a.records[sys] = make_uint4(sbits, saddrs, skey == NONE ? NONE : skey >> 8, skey == NONE ? 0u : skey & 0xFFu);
            err = a.errors[sys];
        }

        // ---- this lane's share of the totals: dead lanes hold zeros ----
        const uint32_t hbits = head ? sbits : 0u;
        t_systems += head ? 1u : 0u;
        t_bad += hbits ? 1u : 0u;
        t_bad_clean += hbits && err == 0u ? 1u : 0u;
        t_addrs += addrs;
        widen(spread4(hbits & 15u), t_bsys[0], t_bsys[1]);
        widen(spread4(hbits >> 4), t_bsys[2], t_bsys[3]);
        widen(cnt_lo, t_baddr[0], t_baddr[1]);
        widen(cnt_hi, t_baddr[2], t_baddr[3]);
        __syncthreads();  // the scan is done with the staged span before the next one is stored
    }

    // ---- totals: over the wave, over the workgroup's waves, then one atomic per word ----
    uint32_t sum[COH_TOT_WORDS];
    sum[COH_SYSTEMS] = wave_sum(t_systems);
    sum[COH_VIOLATING] = wave_sum(t_bad);
    sum[COH_VIOLATING_CLEAN] = wave_sum(t_bad_clean);
    sum[COH_ADDRS] = wave_sum(t_addrs);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {  // bit k: register k / 4 * 2 + k % 2, field k % 4 / 2
        const uint32_t r = k / 4u * 2u + k % 2u, sh = k % 4u / 2u * 16u;
        sum[COH_BIT_SYSTEMS + k] = wave_sum((t_bsys[r] >> sh) & 0xFFFFu);
        sum[COH_BIT_ADDRS + k] = wave_sum((t_baddr[r] >> sh) & 0xFFFFu);
    }
    if (lane == 0u)
#pragma unroll
        for (uint32_t k = 0; k < COH_TOT_WORDS; k++) table[k] = sum[k];
    __syncthreads();
    if (threadIdx.x < COH_TOT_WORDS) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < WAVES; w++)
            s += reinterpret_cast<uint32_t*>(smem)[w * (stage_words + TABLE_WORDS) + stage_words + threadIdx.x];
        if (s) atomicAdd(&a.totals[threadIdx.x], s);
    }
}

}  // namespace

hipError_t launch_coherence(const CoherenceArgs& a, uint64_t groups, hipStream_t s) {
    if (groups == 0) return hipSuccess;
    const uint64_t blocks = (groups + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // the span of 64 / seg systems, rounded up to whole 16-B chunks (<= MAX_CHUNKS * 64 of them)
    const uint32_t span = 64u / a.seg * a.num_procs * (16u + a.cache_size);
    const uint32_t stage_words = (span + 3u) & ~3u;
    if (stage_words > MAX_CHUNKS * 64u * 4u) return hipErrorInvalidValue;
    const size_t lds = (size_t)WAVES * (stage_words + TABLE_WORDS) * sizeof(uint32_t);
    // a grid the device holds at once (the LDS allows 3 to 5 workgroups per CU), and never more
    // than MAX_TRIPS trips per workgroup
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    uint64_t grid = std::min<uint64_t>(blocks, a.max_grid ? a.max_grid : (uint64_t)std::max(cus, 1) * 4u);
    grid = std::max<uint64_t>(grid, (blocks + MAX_TRIPS - 1) / MAX_TRIPS);
    hipLaunchKernelGGL(coherence_kernel, dim3((uint32_t)grid), dim3(WAVES * 64), lds, s, a, stage_words,
                       (uint32_t)blocks);
    return hipGetLastError();
}

}  // namespace dash
