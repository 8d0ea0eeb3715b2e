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
    if (!h->coh.d_rec)
        if (int rc = alloc_group(h, "hipMalloc(coherence)", h->coh.d_rec, nsys, h->coh.d_tot, dash::COH_TOT_WORDS))
            return rc;
    h->coh.valid = false;
    dash::CoherenceArgs a{};
    a.state = h->d_state;
    a.errors = h->d_errors;
    a.nsys = nsys;
    a.num_procs = h->cfg.num_procs;
    a.seg = h->seg;
    a.cache_size = h->cfg.cache_size;
    a.max_grid = (h->cfg.flags & DASH_TEST_ONE_GROUP) ? 1u : 0u;
    a.records = h->coh.d_rec;
    a.totals = h->coh.d_tot;
    HIPCHK(h, hipMemsetAsync(h->coh.d_tot, 0, dash::COH_TOT_WORDS * sizeof(unsigned long long), h->stream));
    HIPCHK(h, dash::launch_coherence(a, h->groups, h->stream));
    return DASH_OK;
}

extern "C" {

int dash_check_coherence(dash_t* h, dash_coherence_totals* totals) {
    return guarded(h, "dash_check_coherence", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (int rc = coherence_enqueue(h)) return rc;
        unsigned long long t[dash::COH_TOT_WORDS];
        HIPCHK(h, hipMemcpyAsync(t, h->coh.d_tot, sizeof t, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->coh.valid = true;
        if (totals) memcpy(totals, t, sizeof *totals);
        return DASH_OK;
    });
}

int dash_read_coherence(dash_t* h, uint64_t first, uint64_t count, dash_coherence* out) {
    if (!h || (!out && count)) return DASH_EINVAL;
    if (!h->ran || !h->coh.valid) return fail(h, DASH_ESTATE, "no dash_check_coherence since the last dash_run");
    if (first + count > h->cfg.num_systems || first + count < first) return fail(h, DASH_EINVAL, "range out of bounds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (count)
        HIPCHK(h, hipMemcpyAsync(out, h->coh.d_rec + first, count * sizeof *out, hipMemcpyDeviceToHost, h->stream));
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
        auto witness = [&](uint64_t k) { return outs[k].seed; };
        return for_each_seed_pass(h, src, n, weights, witness, [&](const seed_pass& p) -> int {
            for (uint64_t i = 0; i < p.fresh; i++) {
                const dash_outcome& o = outs[p.base + i];
                if (p.digests[i] != o.digest || p.errors[i] != o.errors)
                    return fail(h, DASH_ESTATE,
                                "dash_check_outcomes: outcome %llu: seed %llu gave digest %016llx errors %x, not %016llx %x",
                                (unsigned long long)(p.base + i), (unsigned long long)p.seeds[i],
                                (unsigned long long)p.digests[i], p.errors[i], (unsigned long long)o.digest, o.errors);
            }
            if (int rc = dash_check_coherence(h, nullptr)) return rc;
            return dash_read_coherence(h, 0, p.fresh, out + p.base);
        });
    });
}

}  // extern "C"
