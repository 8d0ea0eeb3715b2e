// dash_coherence.cpp -- C-ABI of libdash over HIP: the coherence invariants of final states. One
// launch of dash_coherence.hip over the whole batch's state; the records stay on the device for
// dash_read_coherence until the next dash_run. dash_check_outcomes re-runs an explore's witnesses
// and classifies each outcome.
#include "dash_coherence.h"
#include "dash_internal.h"

static_assert(sizeof(dash_coherence) == sizeof(uint4), "one 16-B record per system");
static_assert(sizeof(dash_coherence_totals) == dash::COH_TOT_WORDS * sizeof(uint64_t), "the totals block's layout");
static_assert(offsetof(dash_coherence_totals, bit_systems) == dash::COH_BIT_SYSTEMS * sizeof(uint64_t) &&
                  offsetof(dash_coherence_totals, bit_addrs) == dash::COH_BIT_ADDRS * sizeof(uint64_t),
              "the per-bit counts' words");

// dash_check_coherence up to the launch (dash_internal.h): state checks, buffers on first use, the
// totals' memset and the kernel, all enqueued on the handle's stream
int coherence_enqueue(dash_t* h) {
    if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
    if (!h->d_state) return fail(h, DASH_ESTATE, "created without DASH_KEEP_STATE");
    const uint64_t nsys = h->cfg.num_systems;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->d_coh) {
        hipError_t e = buf_alloc(h, h->d_coh, nsys);
        if (e == hipSuccess) e = buf_alloc(h, h->d_coh_tot, dash::COH_TOT_WORDS);
        if (e != hipSuccess) {
            buf_free(h, h->d_coh);
            buf_free(h, h->d_coh_tot);
            return hip_fail(h, e, "hipMalloc(coherence)");
        }
    }
    h->coherence = false;
    dash::CoherenceArgs a{};
    a.state = h->d_state;
    a.errors = h->d_errors;
    a.nsys = nsys;
    a.num_procs = h->cfg.num_procs;
    a.seg = h->seg;
    a.cache_size = h->cfg.cache_size;
    a.max_grid = (h->cfg.flags & DASH_TEST_ONE_GROUP) ? 1u : 0u;
    a.records = h->d_coh;
    a.totals = h->d_coh_tot;
    HIPCHK(h, hipMemsetAsync(h->d_coh_tot, 0, dash::COH_TOT_WORDS * sizeof(unsigned long long), h->stream));
    HIPCHK(h, dash::launch_coherence(a, h->groups, h->stream));
    return DASH_OK;
}

extern "C" {

int dash_check_coherence(dash_t* h, dash_coherence_totals* totals) {
    return guarded(h, "dash_check_coherence", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (int rc = coherence_enqueue(h)) return rc;
        unsigned long long t[dash::COH_TOT_WORDS];
        HIPCHK(h, hipMemcpyAsync(t, h->d_coh_tot, sizeof t, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->coherence = true;
        if (totals) memcpy(totals, t, sizeof *totals);
        return DASH_OK;
    });
}

int dash_read_coherence(dash_t* h, uint64_t first, uint64_t count, dash_coherence* out) {
    if (!h || (!out && count)) return DASH_EINVAL;
    if (!h->ran || !h->coherence) return fail(h, DASH_ESTATE, "no dash_check_coherence since the last dash_run");
    if (first + count > h->cfg.num_systems || first + count < first) return fail(h, DASH_EINVAL, "range out of bounds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (count)
        HIPCHK(h, hipMemcpyAsync(out, h->d_coh + first, count * sizeof *out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

int dash_check_outcomes(dash_t* h, uint64_t src, const dash_outcome* outs, uint32_t n, const uint64_t* weights,
                        dash_coherence* out) {
    return guarded(h, "dash_check_outcomes", [&]() -> int {
        if (!h || ((!outs || !out) && n)) return DASH_EINVAL;
        if (!h->d_state) return fail(h, DASH_ESTATE, "dash_check_outcomes: created without DASH_KEEP_STATE");
        const uint64_t nsys = h->cfg.num_systems;
        if (n && !nsys) return fail(h, DASH_EINVAL, "dash_check_outcomes: the handle has no systems");
        // (the seed calls below refuse a handle without a schedule seed, as the explores do)
        int rc = dash_broadcast_system(h, src);
        if (rc != DASH_OK) return rc;
        std::vector<uint64_t> seeds(nsys), dig(nsys), wts(weights ? nsys : 0, weights ? *weights : 0);
        std::vector<uint32_t> err(nsys);
        for (uint64_t base = 0; base < n; base += nsys) {
            const uint64_t fresh = std::min<uint64_t>(nsys, n - base);
            // the last pass pads with repeats of its own witnesses
            for (uint64_t i = 0; i < nsys; i++) seeds[i] = outs[base + i % fresh].seed;
            rc = weights ? dash_set_micro_seeds(h, seeds.data(), wts.data(), nsys)
                         : dash_set_system_seeds(h, seeds.data(), nsys);
            if (rc != DASH_OK) return rc;
            if ((rc = dash_run(h, nullptr)) != DASH_OK) return rc;
            if ((rc = dash_read_results(h, 0, fresh, dig.data(), nullptr, err.data())) != DASH_OK) return rc;
            for (uint64_t i = 0; i < fresh; i++)
                if (dig[i] != outs[base + i].digest || err[i] != outs[base + i].errors)
                    return fail(h, DASH_ESTATE,
                                "dash_check_outcomes: outcome %llu: seed %llu gave digest %016llx errors %x, not %016llx %x",
                                (unsigned long long)(base + i), (unsigned long long)seeds[i], (unsigned long long)dig[i],
                                err[i], (unsigned long long)outs[base + i].digest, outs[base + i].errors);
            if ((rc = dash_check_coherence(h, nullptr)) != DASH_OK) return rc;
            if ((rc = dash_read_coherence(h, 0, fresh, out + base)) != DASH_OK) return rc;
        }
        return DASH_OK;
    });
}

}  // extern "C"
