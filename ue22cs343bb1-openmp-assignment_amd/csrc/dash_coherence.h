// dash_coherence.h -- argument block of the final-state coherence kernel (dash_coherence.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

// dash_coherence_totals as the kernel fills it (u64 words, all sums)
constexpr uint32_t COH_SYSTEMS = 0;
constexpr uint32_t COH_VIOLATING = 1;
constexpr uint32_t COH_VIOLATING_CLEAN = 2;
constexpr uint32_t COH_ADDRS = 3;
constexpr uint32_t COH_BIT_SYSTEMS = 4;  // [8]
constexpr uint32_t COH_BIT_ADDRS = 12;   // [8]
constexpr uint32_t COH_TOT_WORDS = 20;

struct CoherenceArgs {
    const uint32_t* state;   // [sys][node][16 + cache_size]: 16 directory words, then the lines
    const uint32_t* errors;  // [sys] DASH_ERR_* bits of the run
    uint64_t nsys;
    uint32_t num_procs;
    uint32_t seg;            // lanes per system (next pow2 of num_procs)
    uint32_t cache_size;
    uint32_t max_grid;       // workgroups at most; 0 = what the device holds at once
    uint4* records;          // [sys] dash_coherence
    unsigned long long* totals;  // [COH_TOT_WORDS], zeroed by the caller
};

hipError_t launch_coherence(const CoherenceArgs& a, uint64_t groups, hipStream_t s);

}  // namespace dash
