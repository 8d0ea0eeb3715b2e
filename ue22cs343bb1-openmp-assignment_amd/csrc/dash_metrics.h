// dash_metrics.h -- argument block of the event-log metrics kernel (dash_metrics.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

// dash_metrics_totals as the kernel fills it (u64 words): the 16 fields of dash_node_metrics in
// their order (sums; TOT_WAIT_MAX a maximum), then the two system counts
constexpr uint32_t MET_FIELDS = 16;    // uint32_t words of a dash_node_metrics record
constexpr uint32_t MET_WAIT_MAX = 13;  // the one field that is reduced by max
constexpr uint32_t TOT_SYSTEMS = 16;
constexpr uint32_t TOT_TRUNCATED = 17;
constexpr uint32_t TOT_WORDS = 18;

struct MetricsArgs {
    const uint32_t* events;    // [sys][round / 4][node][round % 4], ev_rounds rounds per system
    const uint32_t* rounds;    // [sys] rounds the system ran
    uint64_t nsys;
    uint32_t num_procs;
    uint32_t seg;              // lanes per system (next pow2 of num_procs)
    uint32_t ev_rounds;        // a multiple of 4
    uint4* records;            // [sys * num_procs + node] 64-B records (4 x uint4)
    uint8_t* truncated;        // [sys]
    unsigned long long* totals;  // [TOT_WORDS], zeroed by the caller
};

hipError_t launch_metrics(const MetricsArgs& a, uint64_t groups, hipStream_t s);

}  // namespace dash
