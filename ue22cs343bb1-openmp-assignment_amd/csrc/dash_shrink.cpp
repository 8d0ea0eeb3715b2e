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
        if (!h->d_sh_base) {
            hipError_t e = buf_alloc(h, h->d_sh_base, 2 * row);
            if (e == hipSuccess) e = buf_alloc(h, h->d_sh_lens, 2 * DASH_MAX_PROCS);
            if (e == hipSuccess) e = buf_alloc(h, h->d_sh_count, S);
            if (e == hipSuccess) e = buf_alloc(h, h->d_sh_cell, 1);
            if (e != hipSuccess) {
                buf_free(h, h->d_sh_base);
                buf_free(h, h->d_sh_lens);
                buf_free(h, h->d_sh_count);
                buf_free(h, h->d_sh_cell);
                return hip_fail(h, e, "hipMalloc(shrink)");
            }
        }
        if (h->d_arb && !h->d_seeds) {
            const hipError_t e = buf_alloc(h, h->d_seeds, S);
            if (e != hipSuccess) return hip_fail(h, e, "hipMalloc(seeds)");
        }
        for (hipEvent_t& e : h->sh_ev)
            if (!e) HIPCHK(h, hipEventCreate(&e));
        hipEvent_t* ev = h->sh_ev;

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

        int cur = 0;  // which of the two base rows holds the base
        auto base_row = [&](int i) { return h->d_sh_base + (uint64_t)i * row; };
        auto base_lens = [&](int i) { return h->d_sh_lens + i * DASH_MAX_PROCS; };
        auto max_len = [&]() { return *std::max_element(lens, lens + N); };
        // one launch of the variant kernel from the base over the whole batch
        auto variants = [&](uint32_t mode, uint64_t first) -> hipError_t {
            dash::VariantArgs a{};
            a.base = base_row(cur);
            a.base_lens = base_lens(cur);
            a.dst = h->d_trace;
            a.dst_lens = h->d_lens;
            a.dst_count = h->d_sh_count;
            a.nsys = S;
            a.row = row;
            a.first = first;
            a.nchunks = h->nchunks;
            a.num_procs = N;
            a.wchunks = write_chunks(h, max_len());
            a.mode = mode;
            return h->nchunks ? dash::launch_variants(a, h->stream) : hipSuccess;
        };
        // the traces changed: the handle as dash_explore_sources marks it after its replicate, then the run
        auto simulate = [&]() -> int {
            HIPCHK(h, reset_hint(h));
            if (h->d_arb) h->follow = sched_src::system_seeds;
            h->ran = false;
            dash_stats st;
            if (int rc = dash_run(h, &st)) return rc;  // returns with the stream idle
            rep.sim_ms += st.kernel_ms;
            rep.passes++;
            return DASH_OK;
        };
        auto elapsed = [&](int a, int b, double& sum) -> hipError_t {
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, ev[a], ev[b]);
            sum += ms;
            return e;
        };

        // base row 0 := the source, cleared past its lengths; then the whole batch := the base, and its
        // run says whether the source meets the goal at all
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
        if (h->nchunks) {
            dash::VariantArgs a{};
            a.base = h->d_trace + src * row;
            a.base_lens = h->d_lens + src * N;
            a.dst = base_row(0);
            a.dst_lens = base_lens(0);
            a.nsys = 1;
            a.row = row;
            a.nchunks = h->nchunks;
            a.num_procs = N;
            a.wchunks = write_chunks(h, src_max);
            a.mode = dash::SHRINK_COPY;
            HIPCHK(h, dash::launch_variants(a, h->stream));
        } else {
            HIPCHK(h, hipMemsetAsync(base_lens(0), 0, DASH_MAX_PROCS * sizeof(uint32_t), h->stream));
        }
        HIPCHK(h, variants(dash::SHRINK_COPY, 0));
        HIPCHK(h, hipEventRecord(ev[1], h->stream));
        if (int rc = simulate()) return rc;
        HIPCHK(h, elapsed(0, 1, rep.gen_ms));
        HIPCHK(h, hipEventRecord(ev[2], h->stream));
        if (int rc = coherence_enqueue(h)) return rc;
        HIPCHK(h, hipEventRecord(ev[3], h->stream));
        uint32_t src_err = 0;
        dash_coherence src_coh{};
        HIPCHK(h, hipMemcpyAsync(&src_err, h->d_errors, sizeof src_err, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&src_coh, h->d_coh, sizeof src_coh, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->coherence = true;  // the batch holds copies of the source, run and checked
        HIPCHK(h, elapsed(2, 3, rep.select_ms));
        if ((src_coh.bits & goal->coh_all) != goal->coh_all || (src_err & goal->err_all) != goal->err_all ||
            (src_err & goal->err_none) != 0)
            return fail(h, DASH_EINVAL,
                        "%s: the source does not meet the goal itself: coherence bits 0x%X, errors 0x%X against "
                        "coh_all 0x%X err_all 0x%X err_none 0x%X",
                        what, src_coh.bits, src_err, goal->coh_all, goal->err_all, goal->err_none);

        bool select_pending = false;  // ev[2], ev[3] hold a sub-pass's select, not yet added
        for (;;) {
            dash::ShrinkCand none{};
            const uint64_t C = dash::shrink_decode(lens, N, ~0ull, none);
            if (C == 0) break;  // nothing left to delete
            HIPCHK(h, hipMemsetAsync(h->d_sh_cell, 0, sizeof(unsigned long long), h->stream));
            for (uint64_t first = 0; first < C; first += S) {
                const uint64_t counted = std::min<uint64_t>(S, C - first);
                HIPCHK(h, hipEventRecord(ev[0], h->stream));
                HIPCHK(h, variants(dash::SHRINK_CANDIDATES, first));
                HIPCHK(h, hipEventRecord(ev[1], h->stream));
                if (int rc = simulate()) return rc;
                HIPCHK(h, elapsed(0, 1, rep.gen_ms));
                if (select_pending) HIPCHK(h, elapsed(2, 3, rep.select_ms));
                HIPCHK(h, hipEventRecord(ev[2], h->stream));
                if (int rc = coherence_enqueue(h)) return rc;
                HIPCHK(h, dash::launch_select(h->d_errors, h->d_coh, h->d_sh_count, counted, first, goal->coh_all,
                                              goal->err_all, goal->err_none, h->d_sh_cell, h->stream));
                HIPCHK(h, hipEventRecord(ev[3], h->stream));
                select_pending = true;
                rep.variants += counted;
            }
            // the winner, if any, into the other base row; the cell says which it was
            HIPCHK(h, hipEventRecord(ev[4], h->stream));
            if (h->nchunks) {
                dash::VariantArgs a{};
                a.base = base_row(cur);
                a.base_lens = base_lens(cur);
                a.dst = base_row(cur ^ 1);
                a.dst_lens = base_lens(cur ^ 1);
                a.nsys = 1;
                a.row = row;
                a.nchunks = h->nchunks;
                a.num_procs = N;
                a.wchunks = write_chunks(h, max_len());
                a.mode = dash::SHRINK_APPLY;
                a.cell = h->d_sh_cell;
                HIPCHK(h, dash::launch_variants(a, h->stream));
            }
            HIPCHK(h, hipEventRecord(ev[5], h->stream));
            unsigned long long key = 0;
            HIPCHK(h, hipMemcpyAsync(&key, h->d_sh_cell, sizeof key, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            HIPCHK(h, elapsed(2, 3, rep.select_ms));
            HIPCHK(h, elapsed(4, 5, rep.gen_ms));
            select_pending = false;
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
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
        HIPCHK(h, variants(dash::SHRINK_COPY, 0));
        HIPCHK(h, hipEventRecord(ev[1], h->stream));
        if (int rc = simulate()) return rc;
        HIPCHK(h, elapsed(0, 1, rep.gen_ms));
        HIPCHK(h, hipEventRecord(ev[2], h->stream));
        if (int rc = coherence_enqueue(h)) return rc;
        HIPCHK(h, hipEventRecord(ev[3], h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->coherence = true;
        HIPCHK(h, elapsed(2, 3, rep.select_ms));

        for (uint32_t t = 0; t < N; t++) rep.instr_after += lens[t];
        if (packed_out && stride) {
            const uint64_t pitch = (uint64_t)h->nchunks * 8, width = std::min<uint64_t>(stride * 2, pitch);
            if (width) HIPCHK(h, hipMemcpy2DAsync(packed_out, stride * 2, base_row(cur), pitch, width, N,
                                                  hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (uint32_t t = 0; t < N; t++)  // only words below a row's length are defined on the device
                memset(packed_out + t * stride + lens[t], 0, (size_t)(stride - lens[t]) * 2);
        }
        if (lens_out) memcpy(lens_out, lens, N * sizeof(uint32_t));
        if (n) *n = (uint32_t)std::min<uint64_t>(rep.rounds, 0xFFFFFFFFu);
        if (report) *report = rep;
        return DASH_OK;
    });
}
