// dash_delays.h -- delay words and their enumeration (include/dash.h states both), stated
// once for the host and the kernels: sim_kernel reads a delay word through delay_sits, dash_delay_schedule
// writes the same rounds as a table, and dash_delay_word and the fill kernel of dash_explore_delays
// (dash_outcomes.hip) unrank a schedule index through delay_unrank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

constexpr uint32_t DELAY_SLOTS = 4;          // slots of a delay word, 16 bits each
constexpr uint32_t DELAY_EMPTY = 0xFFFFu;    // an empty slot
constexpr uint64_t DELAY_LOCKSTEP = ~0ull;   // four empty slots
constexpr uint32_t DELAY_MAX_STARTS = 1023;  // start rounds 0 .. 1022
constexpr uint32_t DELAY_MAX_LENS = 8;       // lengths 1 .. 128
constexpr uint32_t DELAY_MAX_COUNT = 4;

// the space of dash_delay_space over N nodes, checked: cells = starts * N * lens <= 65,472
struct DelaySpace {
    uint32_t starts, lens, max_delays, num_procs;
};

__host__ __device__ inline bool delay_space_valid(const DelaySpace& s) {
    return s.starts >= 1 && s.starts <= DELAY_MAX_STARTS && s.lens >= 1 && s.lens <= DELAY_MAX_LENS &&
           s.max_delays <= DELAY_MAX_COUNT && s.num_procs >= 1 && s.num_procs <= 8;
}

__host__ __device__ inline uint64_t delay_cells(const DelaySpace& s) {
    return (uint64_t)s.starts * s.num_procs * s.lens;
}

// C(c, k) for k <= 4 by successive multiply-then-divide: every intermediate is a binomial times a
// factor <= c, below 2^64 for c <= 65,472; 0 for c < k
__host__ __device__ inline uint64_t delay_choose(uint64_t c, uint32_t k) {
    if (c < k) return 0;
    uint64_t v = 1;
    for (uint32_t i = 0; i < k; i++) v = v * (c - i) / (i + 1);
    return v;
}

// K: the schedules of the space, lockstep and every set of 1 .. max_delays cells
__host__ __device__ inline uint64_t delay_count(const DelaySpace& s) {
    const uint64_t M = delay_cells(s);
    uint64_t K = 0;
    for (uint32_t d = 0; d <= s.max_delays; d++) K += delay_choose(M, d);
    return K;
}

// cell c = (r * N + t) * E + e as a slot t | e << 3 | r << 6
__host__ __device__ inline uint32_t delay_cell_slot(const DelaySpace& s, uint64_t c) {
    const uint32_t q = (uint32_t)c / s.lens, e = (uint32_t)c - q * s.lens;
    const uint32_t r = q / s.num_procs, t = q - r * s.num_procs;
    return t | e << 3 | r << 6;
}

// The delay word of schedule `index` < K: the block d of its delay count, then the rank within the block
// by the combinatorial number system, cells c_d > ... > c_1 into slots d - 1 .. 0. The largest c with
// C(c, k) <= j is found by bisection over [k - 1, M - 1] (C(k - 1, k) = 0 <= j always holds).
__host__ __device__ inline uint64_t delay_unrank(const DelaySpace& s, uint64_t index) {
    const uint64_t M = delay_cells(s);
    uint32_t d = 0;
    uint64_t j = index;
    for (uint64_t n; d < s.max_delays && j >= (n = delay_choose(M, d)); d++) j -= n;
    uint64_t word = DELAY_LOCKSTEP, hi = M - 1;
    for (uint32_t k = d; k >= 1; k--) {
        uint64_t lo = k - 1;  // C(lo, k) <= j < C(hi + 1, k)
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (delay_choose(mid, k) <= j) lo = mid;
            else hi = mid - 1;
        }
        j -= delay_choose(lo, k);
        const uint32_t sh = 16u * (k - 1);
        word = (word & ~(0xFFFFull << sh)) | (uint64_t)delay_cell_slot(s, lo) << sh;
        hi = lo - 1;  // the next cell is lower (k > 1 implies lo >= 1)
    }
    return word;
}

// does node t sit out `round` under `word`: some non-empty slot names t and r <= round < r + (1 << e)
__host__ __device__ inline bool delay_sits(uint64_t word, uint32_t t, uint32_t round) {
    bool sits = false;
    for (uint32_t s = 0; s < DELAY_SLOTS; s++) {
        const uint32_t f = (uint32_t)(word >> (16u * s)) & 0xFFFFu;
        const uint32_t r = f >> 6, len = 1u << ((f >> 3) & 7u);
        sits |= (f != DELAY_EMPTY) & ((f & 7u) == t) & (round - r < len);  // unsigned: round < r wraps high
    }
    return sits;
}

}  // namespace dash
