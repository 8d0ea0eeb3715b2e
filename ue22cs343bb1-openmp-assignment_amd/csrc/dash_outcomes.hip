// dash_outcomes.hip -- the device side of dash_explore_sources: many trace sets explored at once,
// their outcomes merged and classified without leaving the device (include/dash.h states the call;
// DESIGN.md §2, §4).
//
// Per call:  replicate, clear_table;  per pass:  fill_seeds, [dash_run], insert, [the coherence
// launch], witness;  at the end:  compact. All on the handle's stream, one thread per system (or per
// slot). dash_explore_assign (csrc/dash_host.c) states the pass assignment once; assign() below is
// its twin, and fill_seeds, insert and witness all go through it. dash_explore_delays is the same call
// with fill_delays in place of fill_seeds: the seed is a schedule index, the system follows its delay word.
//
// The table is open addressing with linear probing over a power-of-two number of 64-B slots
// (OutcomeSlot, dash_outcomes.h). There is no 128-bit compare-and-swap, so a key is two words, each
// claimed by a 64-bit one, and nobody ever waits for anybody:
//   an inserter does CAS(w0, 0, its w0); when w0 is now its own value (it won, or the value was
//   there), it does CAS(w1, 0, its w1) and looks at what w1 settled to: its own w1 means the slot is
//   its key's, anything else sends it to the next slot. A lane that finds w1 == 0 behind a matching
//   w0 settles it with its own w1 instead of waiting for the lane that claimed w0 -- which may be a
//   lane of its own wave and would then never get to run. Both words are written once, so every
//   inserter of one key decides alike at every slot and a key never sits in two slots. Each probe
//   loop is bounded by the slot count; a key that finds no slot counts in OC_UNPLACED, and since slots
//   are never freed it finds none later either.
//
// Insert aggregates before it touches the table. Thread i takes system k = row * G + source with
// source = i / R, row = i % R (the transposed index), so the lanes of a wave share a source, except
// across a boundary, and within one source the seeds rise with the lane. A wave then takes the key
// of its first unserved lane, ballots the lanes that hold the same key, and that first lane alone
// probes and does one atomicAdd(count, lanes in the group) and one atomicMin(seed, its own seed: the
// group's lowest). After GROUP_KEYS such groups the lanes still unserved insert for themselves, all
// at once: thousands of schedules on one outcome cost one pair of atomics per wave, and a wave of 64
// distinct keys does not pay 64 serial probes (DESIGN.md §7 has the measurement).
#include "dash_outcomes.h"

#include <algorithm>

namespace dash {
namespace {

constexpr uint32_t THREADS = 256;

// dash_explore_assign for system k of the pass: source, seed, counted
__device__ __forceinline__ void assign(const AssignArgs& a, uint64_t k, uint64_t& source, uint64_t& seed,
                                       bool& counted) {
    const uint64_t row = k / a.G;
    const uint64_t left = a.K - a.base, fresh = left < a.R ? left : a.R;
    source = k - row * a.G;
    counted = row < fresh;  // fresh <= R, so also k < G * R
    seed = a.F + a.base + (counted ? row : row % fresh);
}

// Thread i of insert / witness: the counted system it stands for, by the transposed index.
__device__ __forceinline__ bool counted_system(const AssignArgs& a, uint64_t i, uint64_t& k, uint64_t& source,
                                               uint64_t& seed) {
    source = i / a.R;
    const uint64_t row = i - source * a.R;
    k = row * a.G + source;
    seed = a.F + a.base + row;
    return source < a.G && a.base + row < a.K;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t slot_hash(uint64_t w0, uint64_t w1) {
    uint64_t h = w0 * 0x9E3779B97F4A7C15ull ^ w1 * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    return h ^ h >> 32;
}

// The slot of key (w0, w1), claimed if it had none; NOT_PLACED when all `mask + 1` slots hold other keys.
__device__ __forceinline__ uint32_t place_key(OutcomeSlot* table, uint64_t mask, unsigned long long w0,
                                              unsigned long long w1) {
    uint64_t idx = slot_hash(w0, w1) & mask;
    for (uint64_t tries = 0; tries <= mask; tries++, idx = (idx + 1) & mask) {
        OutcomeSlot* s = &table[idx];
        const unsigned long long had0 = atomicCAS(&s->w0, 0ull, w0);
        if (had0 != 0ull && had0 != w0) continue;
        const unsigned long long had1 = atomicCAS(&s->w1, 0ull, w1);
        if (had1 == 0ull || had1 == w1) return (uint32_t)idx;
    }
    return NOT_PLACED;
}

__global__ __launch_bounds__(THREADS) void replicate_kernel(uint2* trace, uint32_t* lens, uint64_t nsys, uint64_t G,
                                                            uint64_t row, uint32_t N) {
    // broadcast_kernel's arithmetic (dash_kernels.hip): a system is `row` consecutive chunks and N lengths
    const uint64_t total = nsys * row, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = gid; i < total; i += stride) {
        const uint64_t s = i / row;
        if (s >= G) trace[i] = trace[(s % G) * row + (i - s * row)];
    }
    for (uint64_t i = gid; i < nsys * N; i += stride) {
        const uint64_t s = i / N;
        if (s >= G) lens[i] = lens[(s % G) * N + (i - s * N)];
    }
}

__global__ __launch_bounds__(THREADS) void fill_seeds_kernel(uint64_t* seeds, AssignArgs a, uint32_t pairs,
                                                             uint64_t weights) {
    const uint64_t k = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= a.S) return;
    uint64_t source, seed;
    bool counted;
    assign(a, k, source, seed, counted);
    if (pairs) {
        seeds[2 * k] = seed;
        seeds[2 * k + 1] = weights;
    } else {
        seeds[k] = seed;
    }
}

// fill_seeds for dash_explore_delays: the system's seed is a schedule index, and what it follows is that
// index's delay word
__global__ __launch_bounds__(THREADS) void fill_delays_kernel(uint64_t* words, AssignArgs a, DelaySpace space) {
    const uint64_t k = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (k >= a.S) return;
    uint64_t source, index;
    bool counted;
    assign(a, k, source, index, counted);
    words[k] = delay_unrank(space, index);  // index < a.K = delay_count(space): counted or a repeat of one that is
}

__global__ __launch_bounds__(THREADS) void clear_table_kernel(OutcomeSlot* table, uint64_t slots,
                                                              unsigned long long* counters) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < OC_WORDS) counters[i] = 0ull;
    if (i >= slots) return;
    OutcomeSlot s{};
    s.seed = ~0ull;
    table[i] = s;
}

__global__ __launch_bounds__(THREADS) void insert_kernel(AssignArgs a, const uint64_t* digests, const uint32_t* errors,
                                                         OutcomeSlot* table, uint64_t mask, uint32_t* place,
                                                         unsigned long long* counters, uint32_t group_keys) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    uint64_t k, source, seed;
    const bool valid = counted_system(a, i, k, source, seed);
    unsigned long long w0 = 0, w1 = 0;
    if (valid) {
        const uint64_t d = digests[k];
        w0 = d | 1ull << 63;
        w1 = 1ull | (d >> 63) << 1 | (uint64_t)(errors[k] & 0x3FFFFFFFu) << 2 | source << 32;
    }
    uint32_t slot = NOT_PLACED;
    uint64_t left = __ballot(valid);  // the lanes not served yet: the same value in every lane
    for (uint32_t g = 0; g < group_keys && left; g++) {
        const int lead = __ffsll((long long)left) - 1;
        const unsigned long long k0 = shfl64(w0, lead), k1 = shfl64(w1, lead);
        const bool same = valid && w0 == k0 && w1 == k1;  // served lanes hold other keys than this one
        const uint64_t group = __ballot(same);
        uint32_t s = NOT_PLACED;
        if (lane == lead) {
            const unsigned long long n = (unsigned long long)__popcll(group);
            s = place_key(table, mask, w0, w1);
            if (s != NOT_PLACED) {
                atomicAdd(&table[s].count, n);
                atomicMin(&table[s].seed, (unsigned long long)seed);  // the group's lowest: seeds rise with the lane
            } else {
                atomicAdd(&counters[OC_UNPLACED], n);
            }
        }
        s = (uint32_t)__shfl((int)s, lead, 64);
        if (same) slot = s;
        left &= ~group;
    }
    if (valid && ((left >> lane) & 1ull)) {  // what the groups left: every lane for itself
        slot = place_key(table, mask, w0, w1);
        if (slot != NOT_PLACED) {
            atomicAdd(&table[slot].count, 1ull);
            atomicMin(&table[slot].seed, (unsigned long long)seed);
        } else {
            atomicAdd(&counters[OC_UNPLACED], 1ull);
        }
    }
    if (valid) place[k] = slot;
}

__global__ __launch_bounds__(THREADS) void witness_kernel(AssignArgs a, const uint32_t* place, const uint32_t* rounds,
                                                          const uint4* coh, OutcomeSlot* table) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    uint64_t k, source, seed;
    if (!counted_system(a, i, k, source, seed)) return;
    const uint32_t s = place[k];
    // the seeds of one source are distinct within a pass and rise from pass to pass: at most one
    // system matches, and a witness once written is final
    if (s == NOT_PLACED || table[s].seed != seed) return;
    table[s].rounds = rounds[k];
    table[s].coh = coh[k];
}

__global__ __launch_bounds__(THREADS) void compact_kernel(const OutcomeSlot* table, uint64_t slots, OutcomeOut* out,
                                                          uint64_t cap, unsigned long long* counters) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    OutcomeSlot s{};
    if (i < slots) s = table[i];
    const bool full = s.w0 != 0ull;  // (its w1 is settled: every claimer of a w0 goes on to settle it)
    const uint64_t group = __ballot(full);
    if (!group) return;
    const int lead = __ffsll((long long)group) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(&counters[OC_OUTCOMES], (unsigned long long)__popcll(group));
    base = shfl64(base, lead);
    const uint64_t at = base + (uint64_t)__popcll(group & ((1ull << lane) - 1ull));
    if (!full || at >= cap) return;
    OutcomeOut o{};
    o.digest = (s.w0 & ~(1ull << 63)) | ((s.w1 >> 1) & 1ull) << 63;
    o.count = s.count;
    o.seed = s.seed;
    o.rounds = s.rounds;
    o.errors = (uint32_t)(s.w1 >> 2) & 0x3FFFFFFFu;
    o.coh[0] = s.coh.x;
    o.coh[1] = s.coh.y;
    o.coh[2] = s.coh.z;
    o.coh[3] = s.coh.w;
    o.source = (uint32_t)(s.w1 >> 32);
    out[at] = o;
}

// one thread per item, THREADS per workgroup
hipError_t grid_for(uint64_t items, uint32_t& blocks) {
    const uint64_t b = (items + THREADS - 1) / THREADS;
    if (b > 0x7FFFFFFFull) return hipErrorInvalidValue;
    blocks = (uint32_t)std::max<uint64_t>(b, 1);
    return hipSuccess;
}

}  // namespace

hipError_t launch_replicate(uint2* trace, uint32_t* lens, uint64_t nsys, uint64_t G, uint64_t row, uint32_t N,
                            hipStream_t s) {
    if (G == 0 || G > nsys) return hipErrorInvalidValue;
    if (G == nsys) return hipSuccess;  // nothing to overwrite
    const uint64_t work = std::max<uint64_t>(nsys * row, nsys * N);
    const uint64_t blocks = std::min<uint64_t>((work + THREADS - 1) / THREADS, 256ull * 64);  // grid-stride
    hipLaunchKernelGGL(replicate_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(THREADS), 0, s, trace,
                       lens, nsys, G, row, N);
    return hipGetLastError();
}

hipError_t launch_fill_seeds(uint64_t* seeds, const AssignArgs& a, uint32_t pairs, uint64_t weights, hipStream_t s) {
    uint32_t blocks;
    if (hipError_t e = grid_for(a.S, blocks)) return e;
    hipLaunchKernelGGL(fill_seeds_kernel, dim3(blocks), dim3(THREADS), 0, s, seeds, a, pairs, weights);
    return hipGetLastError();
}

hipError_t launch_fill_delays(uint64_t* words, const AssignArgs& a, const DelaySpace& space, hipStream_t s) {
    if (!delay_space_valid(space) || a.F != 0 || a.K != delay_count(space) || a.base >= a.K) return hipErrorInvalidValue;
    uint32_t blocks;
    if (hipError_t e = grid_for(a.S, blocks)) return e;
    hipLaunchKernelGGL(fill_delays_kernel, dim3(blocks), dim3(THREADS), 0, s, words, a, space);
    return hipGetLastError();
}

hipError_t launch_clear_table(OutcomeSlot* table, uint64_t slots, unsigned long long* counters, hipStream_t s) {
    uint32_t blocks;
    if (hipError_t e = grid_for(slots, blocks)) return e;
    hipLaunchKernelGGL(clear_table_kernel, dim3(blocks), dim3(THREADS), 0, s, table, slots, counters);
    return hipGetLastError();
}

hipError_t launch_insert(const AssignArgs& a, const uint64_t* digests, const uint32_t* errors, OutcomeSlot* table,
                         uint64_t slots, uint32_t* place, unsigned long long* counters, uint32_t group_keys,
                         hipStream_t s) {
    if (slots == 0 || (slots & (slots - 1)) || slots > MAX_SLOTS) return hipErrorInvalidValue;
    uint32_t blocks;
    if (hipError_t e = grid_for(a.G * a.R, blocks)) return e;
    hipLaunchKernelGGL(insert_kernel, dim3(blocks), dim3(THREADS), 0, s, a, digests, errors, table, slots - 1, place,
                       counters, group_keys);
    return hipGetLastError();
}

hipError_t launch_witness(const AssignArgs& a, const uint32_t* place, const uint32_t* rounds, const uint4* coh,
                          OutcomeSlot* table, hipStream_t s) {
    uint32_t blocks;
    if (hipError_t e = grid_for(a.G * a.R, blocks)) return e;
    hipLaunchKernelGGL(witness_kernel, dim3(blocks), dim3(THREADS), 0, s, a, place, rounds, coh, table);
    return hipGetLastError();
}

hipError_t launch_compact(const OutcomeSlot* table, uint64_t slots, OutcomeOut* out, uint64_t cap,
                          unsigned long long* counters, hipStream_t s) {
    uint32_t blocks;
    if (hipError_t e = grid_for(slots, blocks)) return e;
    hipLaunchKernelGGL(compact_kernel, dim3(blocks), dim3(THREADS), 0, s, table, slots, out, cap, counters);
    return hipGetLastError();
}

}  // namespace dash
