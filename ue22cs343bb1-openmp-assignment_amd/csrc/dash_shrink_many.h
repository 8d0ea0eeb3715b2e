// dash_shrink_many.h -- the device side of dash_shrink_many (dash_shrink_many.hip): the assignment of a
// sub-pass's systems to the candidates of many jobs, stated once for the host and the kernels, the per-job
// record the kernels keep, and the launches. The candidate enumeration, the deletion and the winner key
// are dash_shrink.h's, unchanged.
#pragma once
#include "dash_shrink.h"

namespace dash {

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

// Everything the kernels of a call share. Rows are in the engine's lane-contiguous layout (dash_shrink.h:
// VariantArgs); job i's two base rows are rows 2 i and 2 i + 1 of base, their lengths base_lens[(2 i + r) *
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
