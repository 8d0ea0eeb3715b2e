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

// dash_explore_sources, and with `delays` dash_explore_delays: the seed of a system is then its schedule
// index in that space and the pass's fill kernel writes the index's delay word where it would write the seed
static int explore_sources(dash_t* h, const char* what, uint64_t num_sources, uint64_t first_seed,
                           uint64_t seeds_per_source, const uint64_t* weights, const dash::DelaySpace* delays,
                           uint64_t table_slots, dash_outcome_ex* out, uint64_t cap, uint64_t* n,
                           dash_source_summary* per_source, dash_explore_totals* totals) {
    return guarded(h, what, [&]() -> int {
        if (!h || !n || (!out && cap)) return DASH_EINVAL;
        *n = 0;
        const uint64_t S = h->cfg.num_systems, G = num_sources, K = seeds_per_source, F = first_seed;
        if (!h->d_arb) return fail(h, DASH_ESTATE, "%s: handle created with schedule_seed = 0", what);
        if (!h->d_state) return fail(h, DASH_ESTATE, "%s: created without DASH_KEEP_STATE", what);
        if (!weights && h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "%s: the handle follows a micro-step schedule", what);
        if (!h->loaded) return fail(h, DASH_ESTATE, "%s: no traces loaded", what);
        if (G == 0 || G > S)
            return fail(h, DASH_EINVAL, "%s: %llu sources for %llu systems", what, (unsigned long long)G,
                        (unsigned long long)S);
        if (weights && !weights_valid(*weights)) return fail(h, DASH_EINVAL, "%s: a weight above 31", what);
        if (K > UINT64_MAX - F) return fail(h, DASH_EINVAL, "%s: first_seed + seeds_per_source wraps", what);
        const uint64_t R = S / G, passes = K / R + (K % R != 0);
        const uint64_t schedules = K > UINT64_MAX / G ? UINT64_MAX : G * K;  // saturated: only sizes use it
        const uint64_t slots = table_slots ? next_pow2(std::min(table_slots, dash::MAX_SLOTS))
                                           : std::max<uint64_t>(64, next_pow2(2 * std::min<uint64_t>(schedules, 1ull << 21)));
        if (table_slots > dash::MAX_SLOTS) return fail(h, DASH_EINVAL, "%s: table_slots above 2^31", what);
        const uint64_t out_cap = std::max<uint64_t>(std::min(slots, schedules), 1);  // outcomes <= schedules

        HIPCHK(h, hipSetDevice(h->cfg.device));
        int rc = grow(h, h->oc.d_table, h->oc.slots, slots, "hipMalloc(outcome table)");
        if (rc == DASH_OK) rc = grow(h, h->oc.d_out, h->oc.out_cap, out_cap, "hipMalloc(outcomes)");
        if (rc == DASH_OK && !h->oc.d_place)
            rc = alloc_group(h, "hipMalloc(outcome scratch)", h->oc.d_place, S, h->oc.d_counters, dash::OC_WORDS);
        if (rc == DASH_OK) rc = ensure_seeds(h, weights != nullptr);
        if (rc != DASH_OK) return rc;
        stage_timer& timer = h->oc.timer;
        HIPCHK(h, timer_ready(h, timer, 5));
        dash::OutcomeSlot* const table = h->oc.d_table;
        dash::OutcomeOut* const dense = h->oc.d_out;
        uint64_t* const d_seeds = weights ? h->d_mseeds : h->d_seeds;

        double sim_ms = 0, merge_ms = 0, insert_ms = 0;
        const sched_src src = weights  ? sched_src::micro_seeds
                              : delays ? sched_src::system_delays
                                       : sched_src::system_seeds;
        // before the first pass: the copies of the sources and an empty table
        HIPCHK(h, timer.mark(0, h->stream));
        HIPCHK(h, dash::launch_replicate(h->d_trace, h->d_lens, S, G, (uint64_t)h->seg * h->nchunks, h->cfg.num_procs,
                                         h->stream));
        HIPCHK(h, dash::launch_clear_table(table, slots, h->oc.d_counters, h->stream));
        HIPCHK(h, traces_changed(h));
        for (uint64_t p = 0; p < passes; p++) {
            const dash::AssignArgs a{S, G, K, F, R, p * R};
            if (p) HIPCHK(h, timer.mark(0, h->stream));
            if (delays)
                HIPCHK(h, dash::launch_fill_delays(d_seeds, a, *delays, h->stream));
            else
                HIPCHK(h, dash::launch_fill_seeds(d_seeds, a, weights ? 1u : 0u, weights ? *weights : 0, h->stream));
            HIPCHK(h, timer.mark(1, h->stream));
            // the handle now follows per-system seeds (or delay words), as dash_set_system_seeds /
            // dash_set_micro_seeds / dash_set_system_delays leave it (the kernels above run before
            // dash_run's on the same stream)
            if ((rc = run_pass(h, &src, sim_ms)) != DASH_OK) return rc;
            HIPCHK(h, timer.add(0, 1, merge_ms));
            if (p) {  // the previous pass's merge
                HIPCHK(h, timer.add(2, 3, merge_ms));
                HIPCHK(h, timer.add(2, 4, insert_ms));
            }
            HIPCHK(h, timer.mark(2, h->stream));
            const uint32_t group_keys = (h->cfg.flags & DASH_TEST_INSERT_PER_LANE)  ? 0u
                                        : (h->cfg.flags & DASH_TEST_INSERT_GROUPS) ? 64u
                                                                                   : dash::GROUP_KEYS;
            HIPCHK(h, dash::launch_insert(a, h->d_digests, h->d_errors, table, slots, h->oc.d_place, h->oc.d_counters,
                                          group_keys, h->stream));
            HIPCHK(h, timer.mark(4, h->stream));
            if ((rc = coherence_enqueue(h)) != DASH_OK) return rc;
            HIPCHK(h, dash::launch_witness(a, h->oc.d_place, h->d_rounds, h->coh.d_rec, table, h->stream));
            HIPCHK(h, timer.mark(3, h->stream));
        }
        if (passes == 0) HIPCHK(h, timer.mark(1, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (passes) {
            h->coh.valid = true;  // the records of the last pass
            HIPCHK(h, timer.add(2, 3, merge_ms));
            HIPCHK(h, timer.add(2, 4, insert_ms));
        } else {
            HIPCHK(h, timer.add(0, 1, merge_ms));
        }
        unsigned long long counters[dash::OC_WORDS];
        HIPCHK(h, timer.mark(0, h->stream));
        HIPCHK(h, dash::launch_compact(table, slots, dense, out_cap, h->oc.d_counters, h->stream));
        HIPCHK(h, timer.mark(1, h->stream));
        HIPCHK(h, hipMemcpyAsync(counters, h->oc.d_counters, sizeof counters, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, timer.add(0, 1, merge_ms));
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

extern "C" int dash_explore_sources(dash_t* h, uint64_t num_sources, uint64_t first_seed, uint64_t seeds_per_source,
                                    const uint64_t* weights, uint64_t table_slots, dash_outcome_ex* out, uint64_t cap,
                                    uint64_t* n, dash_source_summary* per_source, dash_explore_totals* totals) {
    return explore_sources(h, "dash_explore_sources", num_sources, first_seed, seeds_per_source, weights, nullptr,
                           table_slots, out, cap, n, per_source, totals);
}

extern "C" int dash_explore_delays(dash_t* h, uint64_t num_sources, const dash_delay_space* space, uint64_t table_slots,
                                   dash_outcome_ex* out, uint64_t cap, uint64_t* n, dash_source_summary* per_source,
                                   dash_explore_totals* totals) {
    if (!h || !n || (!out && cap)) return DASH_EINVAL;
    *n = 0;
    dash::DelaySpace s{};
    if (space) s = dash::DelaySpace{space->starts, space->lens, space->max_delays, h->cfg.num_procs};
    if (!space || !dash::delay_space_valid(s)) return fail(h, DASH_EINVAL, "dash_explore_delays: space out of range");
    return explore_sources(h, "dash_explore_delays", num_sources, 0, dash::delay_count(s), nullptr, &s, table_slots,
                           out, cap, n, per_source, totals);
}
