// dash_shrink.hip -- the device side of the shrink engine: incoherent systems shrunk side by side, each job
// with its own two base rows, its own winner cell and its own seed; every variant of a round is written,
// checked and ranked without leaving the device (include/dash.h states the rule).
// dash_shrink_many runs it with the caller's jobs, dash_shrink with one.
//
// Before round 0:  init (base row 0 of every job := its source), variants (copy), [dash_run], [the coherence
// launch], mark.  Per round:  scan (C_i, P, T; cells cleared);  per sub-pass:  variants, [dash_run], [the
// coherence launch], select;  then apply (rows, then the records).  At the end: variants (copy) once more.
//
// A row is written in whole 8-B chunks, four packed instructions each, along a node's stream: lane i of a
// wave holds chunk q0 + i, so a wave's store is 512 contiguous bytes. A workgroup serves one system
// (blockIdx.y, grid-stride): its job, found by a bisection of P, its candidate and that candidate's decode
// (shrink_decode, dash_shrink.h) depend on the block alone and stay in scalar registers. A workgroup writes
// only the chunks that cover its own job's base (and the two chunks past it that the simulator's window
// refill may read), whatever the longest source of the call is. Deleting `count` instructions at `start`
// from a stream (variant_chunk, dash_shrink.h) leaves
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
constexpr uint32_t SCAN_THREADS = 1024;
constexpr uint32_t STATUS_MINIMAL = 0u, STATUS_UNMET = 1u;  // DASH_SHRINK_MINIMAL, DASH_SHRINK_UNMET

// chunks per stream that a row written from a base of these lengths needs, at most cap
__device__ inline uint32_t base_wchunks(const uint32_t* lens, uint32_t N, uint32_t cap) {
    uint32_t longest = 0;
    for (uint32_t t = 0; t < N; t++) longest = max(longest, lens[t]);
    return min(cap, (longest + 3u) / 4u + 2u);
}

// This workgroup's share (blockIdx.x) of one system row: the base without cand (count 0: the base itself,
// cleared past its lengths), W chunks per stream, and the row's lengths.
__device__ inline void write_row(const uint2* base, const uint32_t* base_lens, uint2* out, uint32_t* out_lens, uint32_t N,
                                 uint32_t nchunks, uint32_t W, const ShrinkCand& cand) {
    const uint32_t items = N * W;  // (node, chunk) pairs of the row
    const uint32_t end = min(items, (blockIdx.x + 1u) * ITEMS_PER_BLOCK);
    for (uint32_t i = blockIdx.x * ITEMS_PER_BLOCK + threadIdx.x; i < end; i += THREADS) {
        const uint32_t t = i / W, q = i - t * W;
        const uint32_t L = base_lens[t];
        const uint32_t cut = t == cand.node ? cand.count : 0u;
        const uint64_t v = variant_chunk(base + (uint64_t)t * nchunks, nchunks, L, q, cand.start, cut);
        out[(uint64_t)t * nchunks + q] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        if (q == 0) out_lens[t] = L - cut;
    }
}

__global__ __launch_bounds__(THREADS) void many_init_kernel(ManyArgs a) {
    const uint32_t N = a.num_procs;
    for (uint64_t i = blockIdx.y; i < a.J; i += gridDim.y) {
        const uint64_t src = a.jobs[i].src;  // < S: the host checked
        const uint32_t* lens = a.lens + src * N;
        write_row(a.trace + src * a.row, lens, a.base + 2 * i * a.row, a.base_lens + 2 * i * MANY_LENS, N, a.nchunks,
                  base_wchunks(lens, N, a.wchunks), ShrinkCand{0u, 0u, 0u});
    }
}

__global__ __launch_bounds__(THREADS) void many_mark_kernel(ManyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.J) return;
    ManyJob& j = a.jobs[i];
    const uint32_t e = a.errors[i], bits = a.coh[i].x;  // system i holds the source of job i
    const bool met = (bits & j.coh_all) == j.coh_all && (e & j.err_all) == j.err_all && (e & j.err_none) == 0u;
    j.src_coh_bits = bits;
    j.src_errors = e;
    j.status = met ? STATUS_MINIMAL : STATUS_UNMET;
    j.active = met ? 1u : 0u;
}

// One workgroup: thread x takes jobs [x * per, (x + 1) * per), the workgroup scans the threads' sums in LDS.
__global__ __launch_bounds__(SCAN_THREADS) void many_scan_kernel(ManyArgs a) {
    __shared__ uint64_t part[SCAN_THREADS];
    const uint32_t x = threadIdx.x;
    const uint64_t per = (a.J + SCAN_THREADS - 1) / SCAN_THREADS;
    const uint64_t lo = min(a.J, x * per), hi = min(a.J, lo + per);
    uint64_t sum = 0;
    for (uint64_t i = lo; i < hi; i++) {
        ManyJob& j = a.jobs[i];
        uint32_t C = 0;
        if (j.active) {
            ShrinkCand none{};
            C = (uint32_t)shrink_decode(a.base_lens + (2 * i + j.cur) * MANY_LENS, a.num_procs, ~0ull, none);
        }
        j.cands = C;
        a.cell[i] = 0ull;
        sum += C;
    }
    part[x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {
        const uint64_t below = x >= d ? part[x - d] : 0ull;
        __syncthreads();
        part[x] += below;
        __syncthreads();
    }
    uint64_t run = part[x] - sum;  // the candidates of the jobs before lo
    for (uint64_t i = lo; i < hi; i++) {
        a.prefix[i] = run;
        run += a.jobs[i].cands;
    }
    if (x == SCAN_THREADS - 1) a.prefix[a.J] = part[x];
}

__global__ __launch_bounds__(THREADS) void many_variant_kernel(ManyArgs a, uint64_t pass, uint32_t copy) {
    const uint32_t N = a.num_procs;
    for (uint64_t k = blockIdx.y; k < a.S; k += gridDim.y) {
        uint64_t job = k % a.J, c = 0;
        const bool counted = !copy && many_assign(a.prefix, a.J, a.S, pass, k, job, c);
        const uint64_t r = 2 * job + a.jobs[job].cur;
        const uint32_t* lens = a.base_lens + r * MANY_LENS;
        ShrinkCand cand{0u, 0u, 0u};
        if (counted) shrink_decode(lens, N, c, cand);
        write_row(a.base + r * a.row, lens, a.trace + k * a.row, a.lens + k * N, N, a.nchunks,
                  base_wchunks(lens, N, a.wchunks), cand);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.sys_job[k] = counted ? (uint32_t)job : MANY_NO_JOB;
            a.sys_cand[k] = (uint32_t)c;
            a.sys_count[k] = cand.count;
            if (a.seeds) a.seeds[k] = a.jobs[job].seed;
        }
    }
}

// The wave's maximum of key in every lane.
__device__ inline unsigned long long wave_max(unsigned long long key) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), d, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        key = other > key ? other : key;
    }
    return key;
}

// A lane per system. The wave serves the job of its first lane that still holds a key: the maximum over
// the lanes of that job, one atomic, and those lanes are done; then the next job, until no lane holds a
// key. A wave within one job takes one turn, a wave over several jobs one turn per job. Either way
// cell[job] ends as the maximum over that job's passing candidates.
__global__ __launch_bounds__(THREADS) void many_select_kernel(ManyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t job = MANY_NO_JOB;
    unsigned long long key = 0ull;
    if (i < a.S) {
        job = a.sys_job[i];
        if (job != MANY_NO_JOB) {
            const ManyJob& j = a.jobs[job];
            const uint32_t e = a.errors[i], bits = a.coh[i].x;
            if ((bits & j.coh_all) == j.coh_all && (e & j.err_all) == j.err_all && (e & j.err_none) == 0u)
                key = shrink_key(a.sys_count[i], a.sys_cand[i]);
        }
    }
    unsigned long long todo = __ballot(key != 0ull);
    while (todo != 0ull) {
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t turn = (uint32_t)__shfl((int)job, (int)leader, 64);
        const bool mine = key != 0ull && job == turn;
        const unsigned long long best = wave_max(mine ? key : 0ull);
        if (lane == leader) atomicMax(a.cell + turn, best);
        if (mine) key = 0ull;
        todo = __ballot(key != 0ull);
    }
}

__global__ __launch_bounds__(THREADS) void many_apply_rows_kernel(ManyArgs a) {
    const uint32_t N = a.num_procs;
    for (uint64_t i = blockIdx.y; i < a.J; i += gridDim.y) {
        const unsigned long long key = a.cell[i];
        if (!a.jobs[i].active || key == 0ull) continue;  // no winner: the other row stays as it is
        const uint64_t r = 2 * i + a.jobs[i].cur;
        const uint32_t* lens = a.base_lens + r * MANY_LENS;
        ShrinkCand cand{0u, 0u, 0u};
        shrink_decode(lens, N, shrink_key_candidate(key), cand);
        write_row(a.base + r * a.row, lens, a.base + (r ^ 1ull) * a.row, a.base_lens + (r ^ 1ull) * MANY_LENS, N, a.nchunks,
                  base_wchunks(lens, N, a.wchunks), cand);
    }
}

__global__ __launch_bounds__(THREADS) void many_apply_jobs_kernel(ManyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.J) return;
    ManyJob& j = a.jobs[i];
    if (!j.active) return;
    const unsigned long long key = a.cell[i];
    j.variants += j.cands;
    if (key == 0ull) {  // none of its candidates passed: the base is 1-minimal
        j.active = 0u;
        return;
    }
    ShrinkCand cand{0u, 0u, 0u};
    shrink_decode(a.base_lens + (2 * i + j.cur) * MANY_LENS, a.num_procs, shrink_key_candidate(key), cand);
    if (j.rounds < a.step_cap) a.steps[i * a.step_cap + j.rounds] = ManyStep{cand.node, cand.start, cand.count, j.cands};
    j.rounds++;
    j.cur ^= 1u;
}

bool valid(const ManyArgs& a) {
    return a.J >= 1 && a.J <= a.S && a.num_procs >= 1 && a.num_procs <= MANY_LENS && a.wchunks <= a.nchunks &&
           (uint64_t)a.num_procs * a.nchunks <= a.row;
}

// blockIdx.x over the chunks of a row, blockIdx.y over `rows` rows (grid-stride past 65,535)
dim3 row_grid(const ManyArgs& a, uint64_t rows) {
    const uint32_t items = a.num_procs * a.wchunks;  // <= 8 * 2^22 chunks
    return dim3(std::max(1u, (items + ITEMS_PER_BLOCK - 1) / ITEMS_PER_BLOCK), (uint32_t)std::min<uint64_t>(rows, 65535));
}

uint32_t lane_blocks(uint64_t n) { return (uint32_t)((n + THREADS - 1) / THREADS); }  // n <= 2^32

}  // namespace

hipError_t launch_many_init(const ManyArgs& a, hipStream_t s) {
    if (!valid(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_init_kernel, row_grid(a, a.J), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_many_mark(const ManyArgs& a, hipStream_t s) {
    if (!valid(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_mark_kernel, dim3(lane_blocks(a.J)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_many_scan(const ManyArgs& a, hipStream_t s) {
    if (!valid(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_many_variants(const ManyArgs& a, uint64_t pass, bool copy, hipStream_t s) {
    if (!valid(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_variant_kernel, row_grid(a, a.S), dim3(THREADS), 0, s, a, pass, copy ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_many_select(const ManyArgs& a, hipStream_t s) {
    if (!valid(a) || a.S > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_select_kernel, dim3(lane_blocks(a.S)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_many_apply(const ManyArgs& a, hipStream_t s) {
    if (!valid(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(many_apply_rows_kernel, row_grid(a, a.J), dim3(THREADS), 0, s, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(many_apply_jobs_kernel, dim3(lane_blocks(a.J)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace dash
