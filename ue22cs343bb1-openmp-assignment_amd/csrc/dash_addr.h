// dash_addr.h -- the per-address sharing profile (dash_addr.hip, dash_addr.cpp): the record's word
// order, the totals block, the classification, stated once for the host and the kernel, and the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

// uint32_t words of a dash_addr_metrics record, in the struct's order. Words ADR_READ_MISSES ..
// ADR_MSGS are the message fields: a message event counts in exactly one of them while the table is
// built (ADR_MSGS then holds the messages that count in no other field), and msgs is their sum.
enum : uint32_t {
    ADR_READS, ADR_WRITES, ADR_READ_MISSES, ADR_WRITE_MISSES, ADR_UPGRADES, ADR_INVALIDATIONS, ADR_INTERVENTIONS,
    ADR_FLUSHES, ADR_EVICT_SHARED, ADR_EVICT_MODIFIED, ADR_MSGS, ADR_NODES, ADR_FIELDS
};
constexpr uint32_t ADR_MAX_ADDRS = 128;  // DASH_MAX_PROCS * DASH_MEM_SIZE: the address field has 7 bits
constexpr uint32_t ADR_CLASSES = 5;      // DASH_ADDR_UNTOUCHED .. DASH_ADDR_MULTI_WRITER

// dash_addr_totals as the kernel fills it (u64 words): the sums of words ADR_READS .. ADR_MSGS, then
constexpr uint32_t ADT_MSGS_MAX = 11;
constexpr uint32_t ADT_FOREIGN = 12;
constexpr uint32_t ADT_CLASS_ADDRS = 13;   // [ADR_CLASSES]
constexpr uint32_t ADT_CLASS_MISSES = 18;  // [ADR_CLASSES]
constexpr uint32_t ADT_CLASS_INV = 23;     // [ADR_CLASSES]
constexpr uint32_t ADT_SYSTEMS = 28;
constexpr uint32_t ADT_TRUNCATED = 29;
constexpr uint32_t ADT_WORDS = 30;

// The class of a record (include/dash.h: DASH_ADDR_*), from its reads, writes and nodes words.
// dash_addr_class and the kernel's epilogue both decide through this one function.
__host__ __device__ inline uint32_t addr_class(uint32_t reads, uint32_t writes, uint32_t nodes) {
    if ((reads | writes) == 0u) return 0u;  // UNTOUCHED
    const uint32_t r = nodes & 0xFFu, w = (nodes >> 8) & 0xFFu;
    const int writers = __builtin_popcount(w);
    if (writers >= 2) return 4u;                        // MULTI_WRITER
    if (__builtin_popcount(r | w) <= 1) return 1u;      // PRIVATE
    return writers == 1 ? 3u : 2u;                      // ONE_WRITER : READ_SHARED
}

struct AddrArgs {
    const uint32_t* events;      // [sys][round / 4][node][round % 4], ev_rounds rounds per system
    const uint32_t* rounds;      // [sys] rounds the system ran
    uint64_t nsys;
    uint32_t num_procs;
    uint32_t seg;                // next pow2 of num_procs: lanes per log row
    uint32_t ev_rounds;          // a multiple of 4
    uint4* records;              // [sys * num_procs * 16 + address] 48-B records (3 x uint4)
    uint8_t* truncated;          // [sys]
    unsigned long long* totals;  // [ADT_WORDS], zeroed by the caller
};

hipError_t launch_addr_metrics(const AddrArgs& a, hipStream_t s);

}  // namespace dash
