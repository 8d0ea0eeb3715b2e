// dash_shrink.cpp -- C-ABI of libdash over HIP: the shrink calls. dash_shrink_many, many incoherent systems
// shrunk side by side in lock-step rounds, each down to a 1-minimal trace set that still meets its goal, and
// dash_shrink, the same engine with one job; dash_shrink_candidate and dash_shrink_assign, the enumeration
// and the assignment of a sub-pass's systems as host code.
// The host enqueues the kernels of dash_shrink.hip around dash_run and the coherence launch and reads T, 8
// bytes, per round, however many jobs there are: no variant goes up, and records, steps and rows come down
// once at the end.
#include "dash_shrink.h"

#include "dash_internal.h"

static_assert(sizeof(dash_shrink_step) == sizeof(dash::ManyStep), "the device step log holds dash_shrink_step records");
static_assert(DASH_MAX_PROCS == dash::MANY_LENS, "a base row's lengths");
static_assert(sizeof(dash_shrink_job) == 32 && sizeof(dash_shrink_result) == 32, "the C-ABI's layouts");

extern "C" int dash_shrink_candidate(const uint32_t* lens, uint32_t num_procs, uint64_t c, uint32_t* node,
                                     uint32_t* start, uint32_t* count) {
    if (!lens || num_procs < 1 || num_procs > DASH_MAX_PROCS) return DASH_EINVAL;
    for (uint32_t t = 0; t < num_procs; t++)
        if (lens[t] > dash::SHRINK_MAX_LEN) return DASH_EINVAL;
    dash::ShrinkCand cand{0u, 0u, 0u};
    const uint64_t C = dash::shrink_decode(lens, num_procs, c, cand);  // <= 8 * (2^25 + 25)
    if (C == 0) return 0;
    if (c >= C) return DASH_EINVAL;
    if (node) *node = cand.node;
    if (start) *start = cand.start;
    if (count) *count = cand.count;
    return (int)C;
}

extern "C" int dash_shrink_assign(const uint64_t* cands, uint64_t J, uint64_t S, uint64_t pass, uint64_t k, uint64_t* job,
                                  uint64_t* cand, int* counted) {
    return guarded(nullptr, "dash_shrink_assign", [&]() -> int {
        if (!cands || J == 0 || J > DASH_SHRINK_MAX_JOBS || J > S || k >= S) return DASH_EINVAL;
        std::vector<uint64_t> P(J + 1, 0);
        for (uint64_t i = 0; i < J; i++) {
            if (cands[i] > 0xFFFFFFFFull) return DASH_EINVAL;  // C < 2^32 for any base
            P[i + 1] = P[i] + cands[i];
        }
        if (pass >= (P[J] + S - 1) / S) return DASH_EINVAL;
        uint64_t j = 0, c = 0;
        const bool is_counted = dash::many_assign(P.data(), J, S, pass, k, j, c);
        if (job) *job = j;
        if (cand) *cand = c;
        if (counted) *counted = is_counted ? 1 : 0;
        return DASH_OK;
    });
}

namespace {

// The engine: the jobs, checked by the caller (`what`, for the messages), shrunk side by side on a handle
// that is loaded, keeps its state and follows no micro-step table. The outputs are dash_shrink_many's.
// refuse_unmet: when a job's source does not meet its goal, return after results[] with no other output
// written.
int shrink_jobs(dash_t* h, const char* what, const dash_shrink_job* jobs, uint64_t J, bool refuse_unmet,
                uint16_t* packed_out, uint64_t stride, uint32_t* lens_out, dash_shrink_step* steps, uint32_t step_cap,
                dash_shrink_result* results, dash_shrink_many_report* report) {
    const uint64_t S = h->cfg.num_systems, row = (uint64_t)h->seg * h->nchunks;
    const uint32_t N = h->cfg.num_procs;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    auto& m = h->shm;
    if (!m.d_jobs || m.jobs_cap < J) {  // two base rows per job, and what the kernels keep per job and system
        m.jobs_cap = 0;
        if (int rc = alloc_group(h, "hipMalloc(shrink: two base rows per job)", m.d_base, 2 * J * row, m.d_jobs, J,
                                 m.d_words, 2 * J * dash::MANY_LENS + 3 * S, m.d_u64, 2 * J + 1))
            return rc;
        m.jobs_cap = J;
    }
    // a job has at most as many winners as its source has instructions
    const uint32_t dev_cap = (uint32_t)std::min<uint64_t>(step_cap, (uint64_t)N * h->cfg.max_instr);
    if (int rc = grow(h, m.d_steps, m.steps_cap, J * dev_cap, "hipMalloc(shrink: steps)")) return rc;
    if (h->d_arb)
        if (int rc = ensure_seeds(h, false)) return rc;
    stage_timer& timer = m.timer;
    HIPCHK(h, timer_ready(h, timer, 6));

    dash::ManyArgs a{};
    a.jobs = m.d_jobs;
    a.base = m.d_base;
    a.base_lens = m.d_words;
    a.sys_job = m.d_words + 2 * m.jobs_cap * dash::MANY_LENS;
    a.sys_cand = a.sys_job + S;
    a.sys_count = a.sys_cand + S;
    a.prefix = m.d_u64;
    a.cell = reinterpret_cast<unsigned long long*>(m.d_u64 + m.jobs_cap + 1);
    a.steps = m.d_steps;
    a.trace = h->d_trace;
    a.lens = h->d_lens;
    a.seeds = h->d_arb ? h->d_seeds : nullptr;
    a.errors = h->d_errors;
    a.J = J;
    a.S = S;
    a.row = row;
    a.nchunks = h->nchunks;
    a.num_procs = N;
    a.wchunks = h->nchunks;  // until the sources' lengths are known
    a.step_cap = dev_cap;

    // every job's source into its own base row 0, before the batch is overwritten
    std::vector<dash::ManyJob> rec(J, dash::ManyJob{});
    for (uint64_t i = 0; i < J; i++) {
        rec[i].src = jobs[i].src;
        rec[i].seed = jobs[i].seed;
        rec[i].coh_all = jobs[i].goal.coh_all;
        rec[i].err_all = jobs[i].goal.err_all;
        rec[i].err_none = jobs[i].goal.err_none;
    }
    std::vector<uint32_t> blens(2 * J * dash::MANY_LENS, 0);
    const size_t blens_bytes = blens.size() * sizeof(uint32_t);
    HIPCHK(h, hipMemcpyAsync(m.d_jobs, rec.data(), J * sizeof(dash::ManyJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(a.base_lens, 0, blens_bytes, h->stream));
    HIPCHK(h, dash::launch_many_init(a, h->stream));
    HIPCHK(h, hipMemcpyAsync(blens.data(), a.base_lens, blens_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    uint32_t src_max = 0;
    std::vector<uint32_t> before(J, 0);
    for (uint64_t i = 0; i < J; i++)
        for (uint32_t t = 0; t < N; t++) {
            const uint32_t L = blens[2 * i * dash::MANY_LENS + t];
            src_max = std::max(src_max, L);
            before[i] += L;
        }
    if (packed_out && stride < src_max)
        return fail(h, DASH_EINVAL, "%s: stride %llu below the longest source trace (%u)", what,
                    (unsigned long long)stride, src_max);
    // the trace and the two chunks past it that the simulator's window refill may read
    a.wchunks = (uint32_t)std::min<uint64_t>(h->nchunks, ((uint64_t)src_max + 3) / 4 + 2);

    dash_shrink_many_report rep{};
    rep.jobs = J;
    const sched_src seeds = sched_src::system_seeds;
    enum after_run { NOTHING, MARK, SELECT };
    // a sub-pass after its variants (marks 0, 1): the run, then the coherence records and what reads
    // them (marks 2, 3). The time of marks 2, 3 (and of an apply, marks 4, 5) is added once they have
    // completed: at the next sub-pass, or after the caller's wait.
    bool select_pending = false, apply_pending = false;
    auto settle = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (select_pending) e = timer.add(2, 3, rep.select_ms);
        if (apply_pending && e == hipSuccess) e = timer.add(4, 5, rep.gen_ms);
        select_pending = apply_pending = false;
        return e;
    };
    auto run_and_check = [&](after_run then) -> int {
        if (int rc = run_pass(h, h->d_arb ? &seeds : nullptr, rep.sim_ms)) return rc;  // returns with the stream idle
        rep.passes++;
        HIPCHK(h, timer.add(0, 1, rep.gen_ms));
        HIPCHK(h, settle());
        HIPCHK(h, timer.mark(2, h->stream));
        if (int rc = coherence_enqueue(h)) return rc;
        a.coh = h->coh.d_rec;
        if (then == MARK) HIPCHK(h, dash::launch_many_mark(a, h->stream));
        if (then == SELECT) HIPCHK(h, dash::launch_many_select(a, h->stream));
        HIPCHK(h, timer.mark(3, h->stream));
        select_pending = true;
        return DASH_OK;
    };
    auto variants = [&](uint64_t pass, bool copy) -> int {
        HIPCHK(h, timer.mark(0, h->stream));
        HIPCHK(h, dash::launch_many_variants(a, pass, copy, h->stream));
        HIPCHK(h, timer.mark(1, h->stream));
        return DASH_OK;
    };

    // system k := the source of job k % J under that job's seed; its run says which jobs meet their goal
    if (int rc = variants(0, true)) return rc;
    if (int rc = run_and_check(MARK)) return rc;

    for (;;) {
        uint64_t T = 0;
        HIPCHK(h, dash::launch_many_scan(a, h->stream));
        HIPCHK(h, hipMemcpyAsync(&T, a.prefix + J, sizeof T, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, settle());
        if (T == 0) break;  // no job is shrinking any more
        rep.rounds++;
        for (uint64_t pass = 0; pass * S < T; pass++) {
            if (int rc = variants(pass, false)) return rc;
            if (int rc = run_and_check(SELECT)) return rc;
        }
        HIPCHK(h, timer.mark(4, h->stream));
        HIPCHK(h, dash::launch_many_apply(a, h->stream));
        HIPCHK(h, timer.mark(5, h->stream));
        apply_pending = true;
    }

    // system k := the final set of job k % J, run once more with its coherence records
    if (int rc = variants(0, true)) return rc;
    if (int rc = run_and_check(NOTHING)) return rc;
    HIPCHK(h, hipMemcpyAsync(rec.data(), m.d_jobs, J * sizeof(dash::ManyJob), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(blens.data(), a.base_lens, blens_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, settle());
    h->coh.valid = true;

    std::vector<uint32_t> lens((size_t)J * N, 0);
    uint32_t most = 0;  // the longest step list that is wanted
    for (uint64_t i = 0; i < J; i++) {
        const dash::ManyJob& r = rec[i];
        dash_shrink_result res{};
        res.status = r.status;
        res.rounds = r.rounds;
        res.variants = r.variants;
        res.instr_before = before[i];
        res.src_coh_bits = r.src_coh_bits;
        res.src_errors = r.src_errors;
        for (uint32_t t = 0; t < N; t++) {
            lens[i * N + t] = blens[(2 * i + r.cur) * dash::MANY_LENS + t];
            res.instr_after += lens[i * N + t];
        }
        if (r.rounds > (uint64_t)N * h->cfg.max_instr || r.cur > 1u || res.instr_after > res.instr_before)
            return fail(h, DASH_EDEVICE, "%s: job %llu: the device reports %u rounds, %u -> %u instructions", what,
                        (unsigned long long)i, r.rounds, res.instr_before, res.instr_after);
        (r.status == DASH_SHRINK_UNMET ? rep.unmet : rep.minimal)++;
        rep.variants += res.variants;
        rep.instr_before += res.instr_before;
        rep.instr_after += res.instr_after;
        most = std::max(most, std::min(r.rounds, dev_cap));
        if (results) results[i] = res;
    }
    if (refuse_unmet && rep.unmet) return DASH_OK;
    if (most) {  // the step logs' used columns, in one copy
        std::vector<dash_shrink_step> log((size_t)J * most);
        HIPCHK(h, hipMemcpy2DAsync(log.data(), most * sizeof(dash_shrink_step), m.d_steps, dev_cap * sizeof(dash_shrink_step),
                                   most * sizeof(dash_shrink_step), J, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint64_t i = 0; i < J; i++)
            memcpy(steps + i * step_cap, log.data() + i * most, std::min(rec[i].rounds, dev_cap) * sizeof(dash_shrink_step));
    }
    if (packed_out && stride) {  // systems 0 .. J-1 hold the jobs' final sets
        if (h->seg == N) {
            if (int rc = copy_rows_out(h, h->d_trace, J * N, lens.data(), packed_out, stride)) return rc;
        } else {
            for (uint64_t i = 0; i < J; i++)
                if (int rc = copy_rows_out(h, h->d_trace + i * row, N, lens.data() + i * N, packed_out + i * N * stride, stride))
                    return rc;
        }
    }
    if (lens_out) memcpy(lens_out, lens.data(), lens.size() * sizeof(uint32_t));
    if (report) *report = rep;
    return DASH_OK;
}

}  // namespace

extern "C" int dash_shrink_many(dash_t* h, const dash_shrink_job* jobs, uint64_t num_jobs, uint16_t* packed_out,
                                uint64_t stride, uint32_t* lens_out, dash_shrink_step* steps, uint32_t step_cap,
                                dash_shrink_result* results, dash_shrink_many_report* report) {
    return guarded(h, "dash_shrink_many", [&]() -> int {
        if (!h) return DASH_EINVAL;
        const char* what = "dash_shrink_many";
        const uint64_t S = h->cfg.num_systems, J = num_jobs;
        if (!jobs) return fail(h, DASH_EINVAL, "%s: jobs == NULL", what);
        if (J == 0 || J > S || J > DASH_SHRINK_MAX_JOBS)
            return fail(h, DASH_EINVAL, "%s: %llu jobs on a handle of %llu systems (1 .. %u allowed)", what,
                        (unsigned long long)J, (unsigned long long)S, DASH_SHRINK_MAX_JOBS);
        if (step_cap && !steps) return fail(h, DASH_EINVAL, "%s: step_cap %u without steps", what, step_cap);
        if (!h->d_state) return fail(h, DASH_ESTATE, "%s: created without DASH_KEEP_STATE", what);
        if (!h->loaded) return fail(h, DASH_ESTATE, "%s: no traces loaded", what);
        if (h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "%s: the handle follows a micro-step schedule", what);
        for (uint64_t i = 0; i < J; i++) {
            if (jobs[i].seed && !h->d_arb)
                return fail(h, DASH_ESTATE, "%s: job %llu: seed %llu on a handle created with schedule_seed = 0", what,
                            (unsigned long long)i, (unsigned long long)jobs[i].seed);
            if (jobs[i].src >= S)
                return fail(h, DASH_EINVAL, "%s: job %llu: system %llu out of range", what, (unsigned long long)i,
                            (unsigned long long)jobs[i].src);
            if (jobs[i].goal.coh_all == 0 && jobs[i].goal.err_all == 0)
                return fail(h, DASH_EINVAL, "%s: job %llu: a goal needs a bit in coh_all or err_all", what,
                            (unsigned long long)i);
        }
        return shrink_jobs(h, what, jobs, J, false, packed_out, stride, lens_out, steps, step_cap, results, report);
    });
}

extern "C" int dash_shrink(dash_t* h, uint64_t src, uint64_t seed, const dash_shrink_goal* goal, uint16_t* packed_out,
                           uint64_t stride, uint32_t* lens_out, dash_shrink_step* steps, uint32_t cap, uint32_t* n,
                           dash_shrink_report* report) {
    return guarded(h, "dash_shrink", [&]() -> int {
        if (!h) return DASH_EINVAL;
        const char* what = "dash_shrink";
        if (n) *n = 0;
        if (cap && (!n || !steps)) return fail(h, DASH_EINVAL, "%s: cap %u without n or steps", what, cap);
        if (!goal || (goal->coh_all == 0 && goal->err_all == 0))
            return fail(h, DASH_EINVAL, "%s: a goal needs a bit in coh_all or err_all", what);
        if (!h->d_state) return fail(h, DASH_ESTATE, "%s: created without DASH_KEEP_STATE", what);
        if (!h->loaded) return fail(h, DASH_ESTATE, "%s: no traces loaded", what);
        if (h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "%s: the handle follows a micro-step schedule", what);
        if (seed && !h->d_arb) return fail(h, DASH_ESTATE, "%s: seed %llu on a handle created with schedule_seed = 0", what,
                                           (unsigned long long)seed);
        if (src >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "%s: system %llu out of range", what, (unsigned long long)src);

        // the one-job case of the engine: every system holds a candidate of this job, or its base
        const dash_shrink_job job{src, seed, *goal};
        dash_shrink_result res{};
        dash_shrink_many_report many{};
        if (int rc = shrink_jobs(h, what, &job, 1, true, packed_out, stride, lens_out, steps, cap, &res, &many)) return rc;
        if (res.status == DASH_SHRINK_UNMET)  // the batch holds copies of the source, run and checked
            return fail(h, DASH_EINVAL,
                        "%s: the source does not meet the goal itself: coherence bits 0x%X, errors 0x%X against "
                        "coh_all 0x%X err_all 0x%X err_none 0x%X",
                        what, res.src_coh_bits, res.src_errors, goal->coh_all, goal->err_all, goal->err_none);
        if (n) *n = res.rounds;
        if (report) {
            dash_shrink_report rep{};
            rep.rounds = res.rounds;
            rep.passes = many.passes;
            rep.variants = res.variants;
            rep.instr_before = res.instr_before;
            rep.instr_after = res.instr_after;
            rep.sim_ms = many.sim_ms;
            rep.gen_ms = many.gen_ms;
            rep.select_ms = many.select_ms;
            *report = rep;
        }
        return DASH_OK;
    });
}
