// dash_shrink.h -- the device side of the shrink engine (dash_shrink.hip), which dash_shrink_many drives
// with many jobs and dash_shrink with one: the candidate enumeration, the deletion, the winner key and the
// assignment of a sub-pass's systems to the jobs' candidates, stated once for the host and the kernels, the
// per-job record the kernels keep, and the launches.
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
// `out` to candidate c when c < C (it is left alone otherwise). dash_shrink_candidate, the scan, the variant
// kernel and the apply kernels all decode through this one function. lens[t] <= SHRINK_MAX_LEN.
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

// ---- the chunk arithmetic of a written row (dash_shrink.hip: write_row), host-callable so that a CPU
// program can check it against a plain deletion ----

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

constexpr uint32_t MANY_NO_JOB = 0xFFFFFFFFu;  // a system that holds no counted candidate

// The job of global candidate index g: the i < J with P[i] <= g < P[i + 1], for an exclusive prefix
// P[0 .. J] of the jobs' candidate counts (P[0] = 0, P[J] = T) and g < T. Jobs without candidates
// (P[i] == P[i + 1]) are never returned. A bisection: at most 17 steps for 65,536 jobs.
__host__ __device__ inline uint64_t many_find_job(const uint64_t* P, uint64_t J, uint64_t g) {
    uint64_t lo = 0, hi = J;  // P[lo] <= g < P[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (P[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The rule of include/dash.h (dash_shrink_many, "A round"): what system k < S of sub-pass `pass` holds.
// Returns whether it is counted; then job and cand are the candidate's, else job = k % J and cand = 0 (the
// unchanged base of that job). J >= 1, S >= 1.
__host__ __device__ inline bool many_assign(const uint64_t* P, uint64_t J, uint64_t S, uint64_t pass, uint64_t k,
                                            uint64_t& job, uint64_t& cand) {
    const uint64_t g = pass * S + k;
    if (g < P[J]) {
        job = many_find_job(P, J, g);
        cand = g - P[job];
        return true;
    }
    job = k % J;
    cand = 0;
    return false;
}

// What the device keeps per job: the host writes src, seed and the goal, the kernels the rest.
struct ManyJob {
    uint64_t src, seed;
    uint64_t variants;                    // counted candidates so far
    uint32_t coh_all, err_all, err_none;  // the goal
    uint32_t cur;                         // which of the job's two base rows holds its base
    uint32_t active;                      // still shrinking: met its goal, and a candidate passed in every round so far
    uint32_t status;                      // DASH_SHRINK_MINIMAL / DASH_SHRINK_UNMET
    uint32_t rounds;                      // winners applied
    uint32_t cands;                       // C_i of the round in flight (the scan writes it; 0 when not active)
    uint32_t src_coh_bits, src_errors;    // the source's own record and error word
};
static_assert(sizeof(ManyJob) == 64, "one 64-B record per job");

struct ManyStep {  // dash_shrink_step
    uint32_t node, start, count, candidates;
};

constexpr uint32_t MANY_LENS = 8;  // lengths per base row (DASH_MAX_PROCS)

// Everything the kernels of a call share. Rows are in the engine's lane-contiguous layout: a system is
// `row` consecutive 8-B chunks, node t's stream the nchunks chunks at t * nchunks, four packed instructions
// per chunk. Job i's two base rows are rows 2 i and 2 i + 1 of base, their lengths base_lens[(2 i + r) *
// MANY_LENS ..].
struct ManyArgs {
    ManyJob* jobs;             // [J]
    uint2* base;               // [2 J] system rows
    uint32_t* base_lens;       // [2 J][MANY_LENS]
    uint64_t* prefix;          // [J + 1]: P, with T = P[J]
    unsigned long long* cell;  // [J] the round's winner per job (shrink_key), 0 = none
    ManyStep* steps;           // [J][step_cap] the first step_cap winners of every job
    uint32_t* sys_job;         // [S] the job whose candidate system k holds, MANY_NO_JOB when it is not counted
    uint32_t* sys_cand;        // [S] that candidate's index within its job
    uint32_t* sys_count;       // [S] the instructions it deletes
    uint2* trace;              // the batch: S rows
    uint32_t* lens;            // [S * num_procs]
    uint64_t* seeds;           // [S] per-system schedule seeds, nullptr on a handle without a schedule seed
    const uint32_t* errors;    // [S] of the last run
    const uint4* coh;          // [S] its coherence records
    uint64_t J, S, row;
    uint32_t nchunks, num_procs;
    uint32_t wchunks;          // chunks per stream that cover the longest source trace and its two refill chunks
    uint32_t step_cap;
};

// base row 0 of every job := its source system, cleared past its lengths; the record's device fields reset
hipError_t launch_many_init(const ManyArgs& a, hipStream_t s);
// Round 0, after the run and the coherence launch over copies of the sources: src_coh_bits, src_errors,
// status and active of job i from system i
hipError_t launch_many_mark(const ManyArgs& a, hipStream_t s);
// cands of every job, P, T, and the cells cleared: one workgroup
hipError_t launch_many_scan(const ManyArgs& a, hipStream_t s);
// Every system of the batch written from the base of its job: many_assign's for sub-pass `pass`, or with
// copy the unchanged base of job k % J. Lengths, deleted count, job, candidate and seed per system.
hipError_t launch_many_variants(const ManyArgs& a, uint64_t pass, bool copy, hipStream_t s);
// the key of every counted system that passes its job's goal into cell[job]
hipError_t launch_many_select(const ManyArgs& a, hipStream_t s);
// Every job with a winner: its other base row written, then the step logged, rounds and variants added, the
// rows flipped; a job without one stops. Two launches: no row is read after its job's `cur` has flipped.
hipError_t launch_many_apply(const ManyArgs& a, hipStream_t s);

}  // namespace dash
