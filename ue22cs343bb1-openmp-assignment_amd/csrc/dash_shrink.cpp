// dash_shrink.cpp -- C-ABI of libdash over HIP: dash_shrink, the greedy cut of one system down to a
// 1-minimal trace set that still meets a goal, and dash_shrink_candidate, its enumeration on the host.
// The host enqueues the kernels of dash_shrink.hip around dash_run and the coherence launch, sub-pass by
// sub-pass, and reads one 8-byte cell per round: no variant goes up and no per-system result comes down.
#include "dash_shrink.h"

#include "dash_internal.h"

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

namespace {

// the chunks of a stream that a launch over a base whose longest trace is max_len writes: the trace and
// the two chunks past it that the simulator's window refill may read
uint32_t write_chunks(const dash_t* h, uint32_t max_len) {
    return std::max<uint32_t>(1u, std::min<uint64_t>(h->nchunks, ((uint64_t)max_len + 3) / 4 + 2));
}

// One launch of the variant kernel: nsys systems from dst on are written from the base, whose longest
// trace is max_len, as `mode` says (dash_shrink.h); SHRINK_CANDIDATES numbers them from `first` and
// counts what each deletes, SHRINK_APPLY takes the winner from the cell.
dash::VariantArgs variant_args(const dash_t* h, const uint2* base, const uint32_t* base_lens, uint2* dst,
                               uint32_t* dst_lens, uint64_t nsys, uint32_t max_len, uint32_t mode, uint64_t first = 0) {
    dash::VariantArgs a{};
    a.base = base;
    a.base_lens = base_lens;
    a.dst = dst;
    a.dst_lens = dst_lens;
    a.dst_count = dst == h->d_trace ? h->sh.d_count : nullptr;  // the batch: what each candidate deletes
    a.nsys = nsys;
    a.row = (uint64_t)h->seg * h->nchunks;
    a.first = first;
    a.nchunks = h->nchunks;
    a.num_procs = h->cfg.num_procs;
    a.wchunks = write_chunks(h, max_len);
    a.mode = mode;
    a.cell = mode == dash::SHRINK_APPLY ? h->sh.d_cell : nullptr;
    return a;
}

}  // namespace

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
        const uint64_t S = h->cfg.num_systems, row = (uint64_t)h->seg * h->nchunks;
        const uint32_t N = h->cfg.num_procs;
        if (src >= S) return fail(h, DASH_EINVAL, "%s: system %llu out of range", what, (unsigned long long)src);

        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (!h->sh.d_base)
            if (int rc = alloc_group(h, "hipMalloc(shrink)", h->sh.d_base, 2 * row, h->sh.d_lens, 2 * DASH_MAX_PROCS,
                                     h->sh.d_count, S, h->sh.d_cell, 1))
                return rc;
        if (h->d_arb)
            if (int rc = ensure_seeds(h, false)) return rc;
        stage_timer& timer = h->sh.timer;
        HIPCHK(h, timer_ready(h, timer, 6));

        // the source's lengths: the host's copy of the base's, kept in step with the device's by decoding
        // every winner with the same function
        uint32_t lens[DASH_MAX_PROCS] = {};
        HIPCHK(h, hipMemcpyAsync(lens, h->d_lens + src * N, N * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const uint32_t src_max = *std::max_element(lens, lens + N);
        if (packed_out && stride < src_max)
            return fail(h, DASH_EINVAL, "%s: stride %llu below the source's longest trace (%u)", what,
                        (unsigned long long)stride, src_max);
        dash_shrink_report rep{};
        for (uint32_t t = 0; t < N; t++) rep.instr_before += lens[t];

        // a seeded handle follows one seed for every system (0: lockstep), as dash_set_system_seeds leaves
        // it; a handle without a schedule seed runs its plain lockstep kernel
        if (h->d_arb) HIPCHK(h, dash::launch_fill_u64(h->d_seeds, S, seed, h->stream));
        const sched_src seeds = sched_src::system_seeds;

        int cur = 0;  // which of the two base rows holds the base
        auto base_row = [&](int i) { return h->sh.d_base + (uint64_t)i * row; };
        auto base_lens = [&](int i) { return h->sh.d_lens + i * DASH_MAX_PROCS; };
        // one launch of the variant kernel from the base: the round's winner into the other base row
        // (SHRINK_APPLY), else `mode` over the whole batch, from candidate `first` on
        auto variants = [&](uint32_t mode, uint64_t first) -> hipError_t {
            if (!h->nchunks) return hipSuccess;
            const uint32_t max_len = *std::max_element(lens, lens + N);
            const bool apply = mode == dash::SHRINK_APPLY;
            return dash::launch_variants(variant_args(h, base_row(cur), base_lens(cur), apply ? base_row(cur ^ 1) : h->d_trace,
                                                      apply ? base_lens(cur ^ 1) : h->d_lens, apply ? 1 : S, max_len, mode, first),
                                         h->stream);
        };
        // a sub-pass after its variants (marks 0, 1): the run, then the coherence records and, for
        // `counted` candidates from `first` on, the select (marks 2, 3). The time of marks 2, 3 is
        // added once they have completed: at the next sub-pass, or by the caller after its wait.
        bool select_pending = false;
        auto run_and_check = [&](uint64_t counted, uint64_t first) -> int {
            if (int rc = run_pass(h, h->d_arb ? &seeds : nullptr, rep.sim_ms)) return rc;  // the traces changed
            rep.passes++;
            HIPCHK(h, timer.add(0, 1, rep.gen_ms));
            if (select_pending) HIPCHK(h, timer.add(2, 3, rep.select_ms));
            HIPCHK(h, timer.mark(2, h->stream));
            if (int rc = coherence_enqueue(h)) return rc;
            if (counted)
                HIPCHK(h, dash::launch_select(h->d_errors, h->coh.d_rec, h->sh.d_count, counted, first, goal->coh_all,
                                              goal->err_all, goal->err_none, h->sh.d_cell, h->stream));
            HIPCHK(h, timer.mark(3, h->stream));
            select_pending = true;
            return DASH_OK;
        };
        // the wait for a sub-pass's records (and whatever was enqueued after them)
        auto checked = [&]() -> int {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            HIPCHK(h, timer.add(2, 3, rep.select_ms));
            select_pending = false;
            return DASH_OK;
        };

        // base row 0 := the source, cleared past its lengths; then the whole batch := the base, and its
        // run says whether the source meets the goal at all
        HIPCHK(h, timer.mark(0, h->stream));
        if (h->nchunks)
            HIPCHK(h, dash::launch_variants(variant_args(h, h->d_trace + src * row, h->d_lens + src * N, base_row(0),
                                                         base_lens(0), 1, src_max, dash::SHRINK_COPY),
                                            h->stream));
        else
            HIPCHK(h, hipMemsetAsync(base_lens(0), 0, DASH_MAX_PROCS * sizeof(uint32_t), h->stream));
        HIPCHK(h, variants(dash::SHRINK_COPY, 0));
        HIPCHK(h, timer.mark(1, h->stream));
        if (int rc = run_and_check(0, 0)) return rc;
        uint32_t src_err = 0;
        dash_coherence src_coh{};
        HIPCHK(h, hipMemcpyAsync(&src_err, h->d_errors, sizeof src_err, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&src_coh, h->coh.d_rec, sizeof src_coh, hipMemcpyDeviceToHost, h->stream));
        if (int rc = checked()) return rc;
        h->coh.valid = true;  // the batch holds copies of the source, run and checked
        if ((src_coh.bits & goal->coh_all) != goal->coh_all || (src_err & goal->err_all) != goal->err_all ||
            (src_err & goal->err_none) != 0)
            return fail(h, DASH_EINVAL,
                        "%s: the source does not meet the goal itself: coherence bits 0x%X, errors 0x%X against "
                        "coh_all 0x%X err_all 0x%X err_none 0x%X",
                        what, src_coh.bits, src_err, goal->coh_all, goal->err_all, goal->err_none);

        for (;;) {
            dash::ShrinkCand none{};
            const uint64_t C = dash::shrink_decode(lens, N, ~0ull, none);
            if (C == 0) break;  // nothing left to delete
            HIPCHK(h, hipMemsetAsync(h->sh.d_cell, 0, sizeof(unsigned long long), h->stream));
            for (uint64_t first = 0; first < C; first += S) {
                const uint64_t counted = std::min<uint64_t>(S, C - first);
                HIPCHK(h, timer.mark(0, h->stream));
                HIPCHK(h, variants(dash::SHRINK_CANDIDATES, first));
                HIPCHK(h, timer.mark(1, h->stream));
                if (int rc = run_and_check(counted, first)) return rc;
                rep.variants += counted;
            }
            // the winner, if any, into the other base row; the cell says which it was
            HIPCHK(h, timer.mark(4, h->stream));
            HIPCHK(h, variants(dash::SHRINK_APPLY, 0));
            HIPCHK(h, timer.mark(5, h->stream));
            unsigned long long key = 0;
            HIPCHK(h, hipMemcpyAsync(&key, h->sh.d_cell, sizeof key, hipMemcpyDeviceToHost, h->stream));
            if (int rc = checked()) return rc;
            HIPCHK(h, timer.add(4, 5, rep.gen_ms));
            if (key == 0) break;  // no candidate passed: the base is 1-minimal
            dash::ShrinkCand win{};
            const uint64_t c = dash::shrink_key_candidate(key);
            if (c >= C || (dash::shrink_decode(lens, N, c, win), win.count) != (uint32_t)(key >> 32))
                return fail(h, DASH_EDEVICE, "%s: round %llu: the device chose candidate %llu of %llu", what,
                            (unsigned long long)rep.rounds, (unsigned long long)c, (unsigned long long)C);
            if (rep.rounds < cap) steps[rep.rounds] = dash_shrink_step{win.node, win.start, win.count, (uint32_t)C};
            rep.rounds++;
            lens[win.node] -= win.count;
            cur ^= 1;
        }

        // every system := the minimal set, run once more with its coherence records
        HIPCHK(h, timer.mark(0, h->stream));
        HIPCHK(h, variants(dash::SHRINK_COPY, 0));
        HIPCHK(h, timer.mark(1, h->stream));
        if (int rc = run_and_check(0, 0)) return rc;
        if (int rc = checked()) return rc;
        h->coh.valid = true;

        for (uint32_t t = 0; t < N; t++) rep.instr_after += lens[t];
        if (packed_out && stride)
            if (int rc = copy_rows_out(h, base_row(cur), N, lens, packed_out, stride)) return rc;
        if (lens_out) memcpy(lens_out, lens, N * sizeof(uint32_t));
        if (n) *n = (uint32_t)std::min<uint64_t>(rep.rounds, 0xFFFFFFFFu);
        if (report) *report = rep;
        return DASH_OK;
    });
}
