// dash_outcomes.cpp -- C-ABI of libdash over HIP: dash_explore_sources, the outcome search over many
// trace sets at once. The host enqueues the kernels of dash_outcomes.hip around dash_run and the
// coherence launch, pass by pass, and reads back the compacted table once: no seed vector goes up and
// no per-system result comes down.
#include "dash_outcomes.h"

#include "dash_internal.h"

static_assert(sizeof(dash_outcome_ex) == 56 && sizeof(dash::OutcomeOut) == sizeof(dash_outcome_ex),
              "the compacted entry is dash_outcome_ex");
static_assert(offsetof(dash_outcome_ex, coh) == offsetof(dash::OutcomeOut, coh) &&
                  offsetof(dash_outcome_ex, source) == offsetof(dash::OutcomeOut, source) &&
                  offsetof(dash_outcome, rounds) == offsetof(dash::OutcomeOut, rounds),
              "field for field");

static uint64_t next_pow2_64(uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// p := n elements, unless it already holds at least that many (have)
template <class T>
static int grow(dash_t* h, T*& p, uint64_t& have, uint64_t n, size_t elem, const char* what) {
    if (p && have >= n) return DASH_OK;
    uint8_t* raw = reinterpret_cast<uint8_t*>(p);
    const hipError_t e = buf_alloc(h, raw, std::max<uint64_t>(n, 1) * elem);
    p = reinterpret_cast<T*>(raw);
    have = e == hipSuccess ? n : 0;
    return e == hipSuccess ? DASH_OK : hip_fail(h, e, what);
}

extern "C" int dash_explore_sources(dash_t* h, uint64_t num_sources, uint64_t first_seed, uint64_t seeds_per_source,
                                    const uint64_t* weights, uint64_t table_slots, dash_outcome_ex* out, uint64_t cap,
                                    uint64_t* n, dash_source_summary* per_source, dash_explore_totals* totals) {
    return guarded(h, "dash_explore_sources", [&]() -> int {
        if (!h || !n || (!out && cap)) return DASH_EINVAL;
        *n = 0;
        const char* what = "dash_explore_sources";
        const uint64_t S = h->cfg.num_systems, G = num_sources, K = seeds_per_source, F = first_seed;
        if (!h->d_arb) return fail(h, DASH_ESTATE, "%s: handle created with schedule_seed = 0", what);
        if (!h->d_state) return fail(h, DASH_ESTATE, "%s: created without DASH_KEEP_STATE", what);
        if (!weights && h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "%s: the handle follows a micro-step schedule", what);
        if (!h->loaded) return fail(h, DASH_ESTATE, "%s: no traces loaded", what);
        if (G == 0 || G > S)
            return fail(h, DASH_EINVAL, "%s: %llu sources for %llu systems", what, (unsigned long long)G,
                        (unsigned long long)S);
        if (weights && (*weights & 0xE0E0E0E0E0E0E0E0ull)) return fail(h, DASH_EINVAL, "%s: a weight above 31", what);
        if (K > UINT64_MAX - F) return fail(h, DASH_EINVAL, "%s: first_seed + seeds_per_source wraps", what);
        const uint64_t R = S / G, passes = K / R + (K % R != 0);
        const uint64_t schedules = K > UINT64_MAX / G ? UINT64_MAX : G * K;  // saturated: only sizes use it
        const uint64_t slots = table_slots ? next_pow2_64(std::min(table_slots, dash::MAX_SLOTS))
                                           : std::max<uint64_t>(64, next_pow2_64(2 * std::min<uint64_t>(schedules, 1ull << 21)));
        if (table_slots > dash::MAX_SLOTS) return fail(h, DASH_EINVAL, "%s: table_slots above 2^31", what);
        const uint64_t out_cap = std::max<uint64_t>(std::min(slots, schedules), 1);  // outcomes <= schedules

        HIPCHK(h, hipSetDevice(h->cfg.device));
        dash::OutcomeSlot* table = static_cast<dash::OutcomeSlot*>(h->d_oc_table);
        dash::OutcomeOut* dense = static_cast<dash::OutcomeOut*>(h->d_oc_out);
        int rc = grow(h, table, h->oc_slots, slots, sizeof *table, "hipMalloc(outcome table)");
        h->d_oc_table = table;
        if (rc != DASH_OK) return rc;
        rc = grow(h, dense, h->oc_out_cap, out_cap, sizeof *dense, "hipMalloc(outcomes)");
        h->d_oc_out = dense;
        if (rc != DASH_OK) return rc;
        if (!h->d_oc_place) {
            hipError_t e = buf_alloc(h, h->d_oc_place, S);
            if (e == hipSuccess) e = buf_alloc(h, h->d_oc_counters, dash::OC_WORDS);
            if (e != hipSuccess) {
                buf_free(h, h->d_oc_place);
                buf_free(h, h->d_oc_counters);
                return hip_fail(h, e, "hipMalloc(outcome scratch)");
            }
        }
        uint64_t*& d_seeds = weights ? h->d_mseeds : h->d_seeds;
        if (!d_seeds) {
            const hipError_t e = buf_alloc(h, d_seeds, weights ? 2 * S : S);
            if (e != hipSuccess) return hip_fail(h, e, "hipMalloc(seeds)");
        }
        for (hipEvent_t& e : h->oc_ev)
            if (!e) HIPCHK(h, hipEventCreate(&e));
        hipEvent_t* ev = h->oc_ev;
        auto elapsed = [&](hipEvent_t a, hipEvent_t b, double& sum) -> hipError_t {
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, a, b);
            sum += ms;
            return e;
        };

        double sim_ms = 0, merge_ms = 0, insert_ms = 0;
        const sched_src src = weights ? sched_src::micro_seeds : sched_src::system_seeds;
        // before the first pass: the copies of the sources and an empty table. The traces changed and
        // the seeds will: earlier results and the overflow hint no longer stand.
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
        HIPCHK(h, dash::launch_replicate(h->d_trace, h->d_lens, S, G, (uint64_t)h->seg * h->nchunks, h->cfg.num_procs,
                                         h->stream));
        HIPCHK(h, dash::launch_clear_table(table, slots, h->d_oc_counters, h->stream));
        HIPCHK(h, reset_hint(h));
        h->ran = false;
        for (uint64_t p = 0; p < passes; p++) {
            const dash::AssignArgs a{S, G, K, F, R, p * R};
            if (p) HIPCHK(h, hipEventRecord(ev[0], h->stream));
            HIPCHK(h, dash::launch_fill_seeds(d_seeds, a, weights ? 1u : 0u, weights ? *weights : 0, h->stream));
            HIPCHK(h, hipEventRecord(ev[1], h->stream));
            // the handle now follows per-system seeds, as dash_set_system_seeds / dash_set_micro_seeds
            // leave it (the kernels above run before dash_run's on the same stream)
            HIPCHK(h, reset_hint(h));
            h->follow = src;
            h->ran = false;
            dash_stats st;
            if ((rc = dash_run(h, &st)) != DASH_OK) return rc;  // returns with the stream idle
            sim_ms += st.kernel_ms;
            HIPCHK(h, elapsed(ev[0], ev[1], merge_ms));
            if (p) {  // the previous pass's merge
                HIPCHK(h, elapsed(ev[2], ev[3], merge_ms));
                HIPCHK(h, elapsed(ev[2], ev[4], insert_ms));
            }
            HIPCHK(h, hipEventRecord(ev[2], h->stream));
            const uint32_t group_keys = (h->cfg.flags & DASH_TEST_INSERT_PER_LANE)  ? 0u
                                        : (h->cfg.flags & DASH_TEST_INSERT_GROUPS) ? 64u
                                                                                   : dash::GROUP_KEYS;
            HIPCHK(h, dash::launch_insert(a, h->d_digests, h->d_errors, table, slots, h->d_oc_place, h->d_oc_counters,
                                          group_keys, h->stream));
            HIPCHK(h, hipEventRecord(ev[4], h->stream));
            if ((rc = coherence_enqueue(h)) != DASH_OK) return rc;
            HIPCHK(h, dash::launch_witness(a, h->d_oc_place, h->d_rounds, h->d_coh, table, h->stream));
            HIPCHK(h, hipEventRecord(ev[3], h->stream));
        }
        if (passes == 0) HIPCHK(h, hipEventRecord(ev[1], h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (passes) {
            h->coherence = true;  // the records of the last pass
            HIPCHK(h, elapsed(ev[2], ev[3], merge_ms));
            HIPCHK(h, elapsed(ev[2], ev[4], insert_ms));
        } else {
            HIPCHK(h, elapsed(ev[0], ev[1], merge_ms));
        }
        unsigned long long counters[dash::OC_WORDS];
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
        HIPCHK(h, dash::launch_compact(table, slots, dense, out_cap, h->d_oc_counters, h->stream));
        HIPCHK(h, hipEventRecord(ev[1], h->stream));
        HIPCHK(h, hipMemcpyAsync(counters, h->d_oc_counters, sizeof counters, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, elapsed(ev[0], ev[1], merge_ms));
        const uint64_t found = counters[dash::OC_OUTCOMES];
        if (found > out_cap) return fail(h, DASH_EDEVICE, "%s: %llu outcomes of at most %llu", what,
                                         (unsigned long long)found, (unsigned long long)out_cap);
        std::vector<dash_outcome_ex> list(found);
        if (found) HIPCHK(h, hipMemcpy(list.data(), dense, found * sizeof(dash_outcome_ex), hipMemcpyDeviceToHost));
        std::sort(list.begin(), list.end(), [](const dash_outcome_ex& a, const dash_outcome_ex& b) {
            return a.source != b.source ? a.source < b.source : a.o.seed < b.o.seed;
        });

        dash_explore_totals t{};
        t.outcomes = found;
        t.unplaced = counters[dash::OC_UNPLACED];
        t.passes = passes;
        t.table_slots = slots;
        t.sim_ms = sim_ms;
        t.merge_ms = merge_ms;
        t.insert_ms = insert_ms;
        if (per_source) memset(per_source, 0, G * sizeof *per_source);
        for (const dash_outcome_ex& e : list) {
            const bool bad = e.coh.bits != 0;
            t.schedules += e.o.count;
            if (bad) {
                t.incoherent_outcomes++;
                t.incoherent_schedules += e.o.count;
                if (e.o.errors == 0) t.incoherent_clean_schedules += e.o.count;
            }
            for (uint32_t k = 0; k < 8; k++)
                if ((e.coh.bits >> k) & 1u) t.bit_schedules[k] += e.o.count;
            if (per_source && e.source < G) {
                dash_source_summary& s = per_source[e.source];
                s.schedules += e.o.count;
                s.outcomes++;
                s.top_count = std::max(s.top_count, e.o.count);
                s.coh_bits |= e.coh.bits;
                s.err_bits |= e.o.errors;
                if (bad) {
                    s.incoherent_outcomes++;
                    s.incoherent_schedules += e.o.count;
                }
            }
        }
        t.schedules += t.unplaced;  // every counted schedule: placed or not
        if (totals) *totals = t;
        *n = found;
        for (uint64_t k = 0; k < found && k < cap; k++) out[k] = list[k];
        if (t.unplaced)
            return fail(h, DASH_ETRUNC, "%s: the table of %llu slots filled: %llu schedules found no slot", what,
                        (unsigned long long)slots, (unsigned long long)t.unplaced);
        return DASH_OK;
    });
}
