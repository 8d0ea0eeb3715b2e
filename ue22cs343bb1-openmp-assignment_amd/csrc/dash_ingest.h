// dash_ingest.h -- argument block of the device-side trace-text parser (dash_ingest.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dash {

// first-failure cell: file index [63:28] | code [27:26] | 1-based record number [25:0];
// the lowest failing file wins a global atomic min (a file reports at most once)
constexpr unsigned long long INGEST_NO_FAILURE = ~0ull;
constexpr uint32_t INGEST_CODE_PARSE = 1;  // DASH_EPARSE
constexpr uint32_t INGEST_CODE_ADDR = 2;   // DASH_EADDR

struct IngestArgs {
    const uint8_t* text;       // slab of file bytes
    const uint64_t* offsets;   // [files] byte offset of each file in the slab (any alignment)
    const uint32_t* lengths;   // [files]
    uint64_t file_base;        // global index of this launch's file 0 (f = sys * num_procs + node)
    uint64_t num_files;
    uint16_t* trace;           // the handle's trace layout, in 16-bit words
    uint32_t* lens;            // [sys * num_procs + node], indexed by the global file index
    uint32_t nchunks;          // row stride in 4-word chunks
    uint32_t seg;              // lanes per system
    uint32_t num_procs;
    uint32_t max_instr;        // <= nchunks * 4
    unsigned long long* fail;  // the first-failure cell
};

hipError_t launch_ingest(const IngestArgs& a, hipStream_t s);

}  // namespace dash
