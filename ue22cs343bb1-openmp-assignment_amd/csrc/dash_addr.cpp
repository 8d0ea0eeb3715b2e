// dash_addr.cpp -- C-ABI of libdash over HIP: the per-address sharing profile from the event log. One
// launch of dash_addr.hip over the whole batch's log; the records stay on the device for
// dash_read_addr_metrics until the next dash_run. Below them the host boundary: the rules once more
// in plain code over dash_event lists (dash_addr_metrics_from_events) and the classification
// (dash_addr_class, the kernel's own function).
#include "dash_internal.h"
#include "dash_addr.h"

static_assert(sizeof(dash_addr_metrics) == dash::ADR_FIELDS * sizeof(uint32_t), "one 48-B record per address");
static_assert(sizeof(dash_addr_totals) == dash::ADT_WORDS * sizeof(uint64_t), "the totals block's layout");
static_assert(offsetof(dash_addr_metrics, msgs) == dash::ADR_MSGS * sizeof(uint32_t), "msgs' word");
static_assert(offsetof(dash_addr_metrics, nodes) == dash::ADR_NODES * sizeof(uint32_t), "nodes' word");
static_assert(offsetof(dash_addr_totals, msgs_max) == dash::ADT_MSGS_MAX * sizeof(uint64_t), "msgs_max's word");
static_assert(offsetof(dash_addr_totals, class_addrs) == dash::ADT_CLASS_ADDRS * sizeof(uint64_t), "class_addrs' word");
static_assert(offsetof(dash_addr_totals, systems) == dash::ADT_SYSTEMS * sizeof(uint64_t), "systems' word");
static_assert(DASH_MAX_PROCS * DASH_MEM_SIZE == dash::ADR_MAX_ADDRS, "the address field's range");
static_assert(DASH_ADDR_MULTI_WRITER + 1 == dash::ADR_CLASSES, "the classes");

extern "C" {

int dash_compute_addr_metrics(dash_t* h, dash_addr_totals* totals) {
    return guarded(h, "dash_compute_addr_metrics", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (!h->d_events) return fail(h, DASH_ESTATE, "created with trace_events = 0");
        const uint64_t nsys = h->cfg.num_systems, A = (uint64_t)h->cfg.num_procs * DASH_MEM_SIZE;
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (!h->adr.d_rec)
            if (int rc = alloc_group(h, "hipMalloc(address metrics)", h->adr.d_rec, nsys * A * 3, h->adr.d_cut, nsys,
                                     h->adr.d_tot, dash::ADT_WORDS)) {
                (void)hipGetLastError();  // the handle stays usable: the next launch must not report this again
                return rc;
            }
        h->adr.valid = false;
        dash::AddrArgs a{};
        a.events = h->d_events;
        a.rounds = h->d_rounds;
        a.nsys = nsys;
        a.num_procs = h->cfg.num_procs;
        a.seg = h->seg;
        a.ev_rounds = h->ev_rounds;
        a.records = h->adr.d_rec;
        a.truncated = h->adr.d_cut;
        a.totals = h->adr.d_tot;
        unsigned long long t[dash::ADT_WORDS];
        HIPCHK(h, hipMemsetAsync(h->adr.d_tot, 0, sizeof t, h->stream));
        HIPCHK(h, dash::launch_addr_metrics(a, h->stream));
        HIPCHK(h, hipMemcpyAsync(t, h->adr.d_tot, sizeof t, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->adr.valid = true;
        if (totals) memcpy(totals, t, sizeof *totals);
        return DASH_OK;
    });
}

int dash_read_addr_metrics(dash_t* h, uint64_t first, uint64_t count, dash_addr_metrics* out, uint8_t* truncated) {
    if (!h || (!out && count)) return DASH_EINVAL;
    if (!h->ran || !h->adr.valid)
        return fail(h, DASH_ESTATE, "no dash_compute_addr_metrics since the last dash_run");
    if (first + count > h->cfg.num_systems || first + count < first) return fail(h, DASH_EINVAL, "range out of bounds");
    const uint64_t A = (uint64_t)h->cfg.num_procs * DASH_MEM_SIZE;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (count) {
        HIPCHK(h, hipMemcpyAsync(out, h->adr.d_rec + first * A * 3, count * A * sizeof *out, hipMemcpyDeviceToHost,
                                 h->stream));
        if (truncated)
            HIPCHK(h, hipMemcpyAsync(truncated, h->adr.d_cut + first, count, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

// ---- host boundary (pure C++, no device) ----

int dash_addr_class(const dash_addr_metrics* m) {
    if (!m) return DASH_EINVAL;
    return (int)dash::addr_class(m->reads, m->writes, m->nodes);
}

int dash_addr_metrics_from_events(const dash_event* ev, uint64_t n, uint32_t num_procs, uint32_t rounds,
                                  dash_addr_metrics* out, uint64_t* foreign) {
    if (num_procs < 1 || num_procs > DASH_MAX_PROCS || !out || (!ev && n)) return DASH_EINVAL;
    const uint32_t A = num_procs * DASH_MEM_SIZE;
    memset(out, 0, A * sizeof *out);
    uint64_t past = 0;
    for (uint64_t k = 0; k < n; k++) {
        const dash_event& e = ev[k];
        if (e.round >= rounds) continue;
        const uint32_t a = (e.word >> 8) & 0x7Fu;
        if (a >= A) {
            past++;
            continue;
        }
        dash_addr_metrics& m = out[a];
        if (e.kind == DASH_EV_INSTR) {
            const bool wr = e.word & 0x8000u;
            (wr ? m.writes : m.reads)++;
            m.nodes |= (1u << (e.node & 7u)) << (wr ? 8 : 0);
            continue;
        }
        m.msgs++;
        switch (e.word & 15u) {
        case DASH_READ_REQUEST: m.read_misses++; break;
        case DASH_WRITE_REQUEST: m.write_misses++; break;
        case DASH_UPGRADE: m.upgrades++; break;
        case DASH_INV:
            m.invalidations++;
            m.nodes |= 0x10000u << (e.node & 7u);
            break;
        case DASH_WRITEBACK_INV:
        case DASH_WRITEBACK_INT: m.interventions++; break;
        case DASH_FLUSH:
        case DASH_FLUSH_INVACK: m.flushes++; break;
        case DASH_EVICT_SHARED: m.evict_shared += e.node == a >> 4; break;
        case DASH_EVICT_MODIFIED: m.evict_modified += e.node == a >> 4; break;
        default: break;
        }
    }
    if (foreign) *foreign = past;
    return DASH_OK;
}

}  // extern "C"
