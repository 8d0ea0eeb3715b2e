// dash_metrics.cpp -- C-ABI of libdash over HIP: per-node metrics from the event log. One launch of
// dash_metrics.hip over the whole batch's log; the records stay on the device for
// dash_read_metrics until the next dash_run.
#include "dash_internal.h"
#include "dash_metrics.h"

static_assert(sizeof(dash_node_metrics) == dash::MET_FIELDS * sizeof(uint32_t), "one 64-B record per node");
static_assert(sizeof(dash_metrics_totals) == dash::TOT_WORDS * sizeof(uint64_t), "the totals block's layout");
static_assert(offsetof(dash_node_metrics, wait_max) == dash::MET_WAIT_MAX * sizeof(uint32_t), "wait_max's word");

extern "C" {

int dash_compute_metrics(dash_t* h, dash_metrics_totals* totals) {
    return guarded(h, "dash_compute_metrics", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (!h->d_events) return fail(h, DASH_ESTATE, "created with trace_events = 0");
        const uint64_t nsys = h->cfg.num_systems;
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (!h->met.d_rec)
            if (int rc = alloc_group(h, "hipMalloc(metrics)", h->met.d_rec, nsys * h->cfg.num_procs * 4, h->met.d_cut, nsys,
                                     h->met.d_tot, dash::TOT_WORDS))
                return rc;
        h->met.valid = false;
        dash::MetricsArgs a{};
        a.events = h->d_events;
        a.rounds = h->d_rounds;
        a.nsys = nsys;
        a.num_procs = h->cfg.num_procs;
        a.seg = h->seg;
        a.ev_rounds = h->ev_rounds;
        a.records = h->met.d_rec;
        a.truncated = h->met.d_cut;
        a.totals = h->met.d_tot;
        unsigned long long t[dash::TOT_WORDS];
        HIPCHK(h, hipMemsetAsync(h->met.d_tot, 0, sizeof t, h->stream));
        HIPCHK(h, dash::launch_metrics(a, h->groups, h->stream));
        HIPCHK(h, hipMemcpyAsync(t, h->met.d_tot, sizeof t, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->met.valid = true;
        if (totals) memcpy(totals, t, sizeof *totals);
        return DASH_OK;
    });
}

int dash_read_metrics(dash_t* h, uint64_t first, uint64_t count, dash_node_metrics* out, uint8_t* truncated) {
    if (!h || (!out && count)) return DASH_EINVAL;
    if (!h->ran || !h->met.valid) return fail(h, DASH_ESTATE, "no dash_compute_metrics since the last dash_run");
    if (first + count > h->cfg.num_systems || first + count < first) return fail(h, DASH_EINVAL, "range out of bounds");
    const uint32_t N = h->cfg.num_procs;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (count) {
        HIPCHK(h, hipMemcpyAsync(out, h->met.d_rec + first * N * 4, count * N * sizeof *out, hipMemcpyDeviceToHost,
                                 h->stream));
        if (truncated)
            HIPCHK(h, hipMemcpyAsync(truncated, h->met.d_cut + first, count, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

}  // extern "C"
