// dash_sched.cpp -- C-ABI of libdash over HIP: what the runs follow (round and micro-step
// tables, per-system seeds), dash_broadcast_system and the outcome search over seeds.
//
// The handle follows one source at a time (sched_src, dash_internal.h): the call made last
// decides. d_arb holds the handle seed's own round table until an explicit table overwrites it
// (tab_explicit); going back to the handle's seed rebuilds it.
#include <map>

#include "dash_delays.h"
#include "dash_internal.h"

// every schedule call needs a handle created with a schedule seed (it owns the round table)
static int need_seed(dash_t* h, const char* what) {
    return h->d_arb ? DASH_OK : fail(h, DASH_ESTATE, "%s: handle created with schedule_seed = 0", what);
}

// an explicit table of `rounds` rounds: the handle's table must span the run and hold them
static int table_fits(dash_t* h, const char* what, uint32_t rounds) {
    if (int rc = need_seed(h, what)) return rc;
    if (h->arb_len < h->cfg.max_rounds)
        return fail(h, DASH_EINVAL, "%s: the round table holds %u of max_rounds %llu rounds", what, h->arb_len,
                    (unsigned long long)h->cfg.max_rounds);
    if (rounds > h->arb_len) return fail(h, DASH_EINVAL, "%s: %u rounds > max_rounds", what, rounds);
    return DASH_OK;
}

// The end of every call that changes what the runs follow: schedule_changed, and the stream's
// work (uploads, the table kernel, the hint's memset) is done.
static int follow_now(dash_t* h, sched_src src, bool rehint) {
    HIPCHK(h, schedule_changed(h, src, rehint));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

// tab: the kernel's table layout (dash_kernels.hip arb_table_kernel), [round / 4][lane][round % 4]
static int upload_table(dash_t* h, const std::vector<uint32_t>& tab, sched_src src) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_arb, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    const int rc = follow_now(h, src, false);
    if (rc == DASH_OK) h->tab_explicit = true;
    return rc;
}

// dash_set_*_seeds(NULL, 0): back to the handle's own seed and its round table, which is
// rebuilt if an explicit table overwrote it
static int unset_seeds(dash_t* h, const char* what, uint64_t n, bool rehint) {
    if (n) return fail(h, DASH_EINVAL, "%s: null seeds with n = %llu", what, (unsigned long long)n);
    if (h->tab_explicit) {
        HIPCHK(h, dash::launch_arb_table(h->cfg.schedule_seed, h->seg, h->d_arb, h->arb_len, h->stream));
        h->tab_explicit = false;
    }
    return follow_now(h, sched_src::round_table, rehint);
}

// v[words] into the seed buffer of `src` (ensure_seeds), which the runs follow from here on
static int upload_seeds(dash_t* h, const uint64_t* v, uint64_t words, sched_src src) {
    if (int rc = ensure_seeds(h, src == sched_src::micro_seeds)) return rc;
    uint64_t* d = src == sched_src::micro_seeds ? h->d_mseeds : h->d_seeds;
    if (words) HIPCHK(h, hipMemcpyAsync(d, v, words * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    return follow_now(h, src, true);
}

extern "C" {

int dash_set_schedule(dash_t* h, const uint8_t* sched, uint32_t rounds) {
    return guarded(h, "dash_set_schedule", [&]() -> int {
        if (!h || (!sched && rounds)) return DASH_EINVAL;
        if (int rc = table_fits(h, "dash_set_schedule", rounds)) return rc;
        const uint32_t N = h->cfg.num_procs, P = h->seg;
        for (uint32_t r = 0; r < rounds; r++) {
            uint32_t used = 0;
            for (uint32_t t = 0; t < N; t++) {
                const uint8_t v = sched[(uint64_t)r * N + t];
                if (v == DASH_SIT_OUT) continue;
                if (v >= P || (used >> v) & 1u)
                    return fail(h, DASH_EINVAL, "dash_set_schedule: round %u node %u: position %u invalid or repeated",
                                r, t, (unsigned)v);
                used |= 1u << v;
            }
        }
        // each word 0 for a node sitting out, else its primary arrival bit 2 << 4 * position
        std::vector<uint32_t> tab(((uint64_t)h->arb_len + 4) * P, 0);
        for (uint64_t r = 0; r < (uint64_t)h->arb_len + 4; r++)
            for (uint32_t t = 0; t < P; t++) {
                uint32_t w = 0;
                if (t < N) {
                    const uint32_t v = r < rounds ? sched[r * N + t] : t;  // later rounds: lockstep
                    w = v == DASH_SIT_OUT ? 0u : 2u << (4u * v);
                }
                tab[((r >> 2) * P + t) * 4 + (r & 3)] = w;
            }
        return upload_table(h, tab, sched_src::round_table);
    });
}

int dash_set_micro_schedule(dash_t* h, const uint8_t* acts, uint32_t rounds) {
    return guarded(h, "dash_set_micro_schedule", [&]() -> int {
        if (!h || (!acts && rounds)) return DASH_EINVAL;
        if (int rc = table_fits(h, "dash_set_micro_schedule", rounds)) return rc;
        const uint32_t N = h->cfg.num_procs, P = h->seg;
        for (uint32_t r = 0; r < rounds; r++) {
            uint32_t acting = 0;
            for (uint32_t t = 0; t < N; t++) {
                const uint8_t v = acts[(uint64_t)r * N + t];
                if (v == DASH_SIT_OUT) continue;
                if (v != DASH_MICRO_STEP && v != DASH_MICRO_SEND)
                    return fail(h, DASH_EINVAL, "dash_set_micro_schedule: round %u node %u: action %u invalid", r, t,
                                (unsigned)v);
                ++acting;
            }
            if (acting > 1) return fail(h, DASH_EINVAL, "dash_set_micro_schedule: round %u: %u nodes act", r, acting);
        }
        // table words (dash_kernels.hip MODE 4): 0 = sits out, 1 = steps, 2 = sends one held
        // message; every node sits out past the schedule
        std::vector<uint32_t> tab(((uint64_t)h->arb_len + 4) * P, 0);
        for (uint64_t r = 0; r < rounds; r++)
            for (uint32_t t = 0; t < N; t++) {
                const uint8_t v = acts[r * N + t];
                tab[((r >> 2) * P + t) * 4 + (r & 3)] = v == DASH_SIT_OUT ? 0u : v == DASH_MICRO_STEP ? 1u : 2u;
            }
        return upload_table(h, tab, sched_src::micro_table);
    });
}

int dash_set_system_seeds(dash_t* h, const uint64_t* seeds, uint64_t n) {
    return guarded(h, "dash_set_system_seeds", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (int rc = need_seed(h, "dash_set_system_seeds")) return rc;
        if (h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "dash_set_system_seeds: the handle follows a micro-step schedule");
        HIPCHK(h, hipSetDevice(h->cfg.device));
        // leaving the seeds voids the hint they made; a round table's own hint still stands
        if (!seeds) return unset_seeds(h, "dash_set_system_seeds", n, per_system_rounds(h->follow));
        if (n != h->cfg.num_systems)
            return fail(h, DASH_EINVAL, "dash_set_system_seeds: %llu seeds for %llu systems", (unsigned long long)n,
                        (unsigned long long)h->cfg.num_systems);
        return upload_seeds(h, seeds, n, sched_src::system_seeds);
    });
}

int dash_set_system_delays(dash_t* h, const uint64_t* words, uint64_t n) {
    return guarded(h, "dash_set_system_delays", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (int rc = need_seed(h, "dash_set_system_delays")) return rc;
        if (h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "dash_set_system_delays: the handle follows a micro-step schedule");
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (!words) return unset_seeds(h, "dash_set_system_delays", n, per_system_rounds(h->follow));
        if (n != h->cfg.num_systems)
            return fail(h, DASH_EINVAL, "dash_set_system_delays: %llu words for %llu systems", (unsigned long long)n,
                        (unsigned long long)h->cfg.num_systems);
        return upload_seeds(h, words, n, sched_src::system_delays);  // the words ride in the seed buffer
    });
}

int dash_delay_schedule(uint64_t word, uint32_t num_procs, uint32_t rounds, uint8_t* sched) {
    if (num_procs < 1 || num_procs > DASH_MAX_PROCS || !sched) return DASH_EINVAL;
    for (uint64_t r = 0; r < rounds; r++)
        for (uint32_t t = 0; t < num_procs; t++)
            sched[r * num_procs + t] = dash::delay_sits(word, t, (uint32_t)r) ? (uint8_t)DASH_SIT_OUT : (uint8_t)t;
    return DASH_OK;
}

// a dash_delay_space over num_procs nodes as the shared arithmetic takes it; false when out of range
static bool delay_space_of(const dash_delay_space* sp, uint32_t num_procs, dash::DelaySpace& out) {
    if (!sp) return false;
    out = dash::DelaySpace{sp->starts, sp->lens, sp->max_delays, num_procs};
    return dash::delay_space_valid(out);
}

int dash_delay_count(const dash_delay_space* space, uint32_t num_procs, uint64_t* K) {
    dash::DelaySpace s;
    if (!K || !delay_space_of(space, num_procs, s)) return DASH_EINVAL;
    *K = dash::delay_count(s);
    return DASH_OK;
}

int dash_delay_word(const dash_delay_space* space, uint32_t num_procs, uint64_t index, uint64_t* word) {
    dash::DelaySpace s;
    if (!word || !delay_space_of(space, num_procs, s) || index >= dash::delay_count(s)) return DASH_EINVAL;
    *word = dash::delay_unrank(s, index);
    return DASH_OK;
}

int dash_set_micro_seeds(dash_t* h, const uint64_t* seeds, const uint64_t* weights, uint64_t n) {
    return guarded(h, "dash_set_micro_seeds", [&]() -> int {
        if (!h) return DASH_EINVAL;
        if (int rc = need_seed(h, "dash_set_micro_seeds")) return rc;
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (!seeds) return unset_seeds(h, "dash_set_micro_seeds", n, true);
        if (n != h->cfg.num_systems)
            return fail(h, DASH_EINVAL, "dash_set_micro_seeds: %llu seeds for %llu systems", (unsigned long long)n,
                        (unsigned long long)h->cfg.num_systems);
        std::vector<uint64_t> pairs(2 * n);
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t w = weights ? weights[k] : DASH_MICRO_UNIFORM;
            if (!weights_valid(w))
                return fail(h, DASH_EINVAL, "dash_set_micro_seeds: system %llu: a weight above 31", (unsigned long long)k);
            pairs[2 * k] = seeds[k];
            pairs[2 * k + 1] = w;
        }
        // (micro-step runs take no tiers: the hint of earlier runs is void)
        return upload_seeds(h, pairs.data(), pairs.size(), sched_src::micro_seeds);
    });
}

int dash_broadcast_system(dash_t* h, uint64_t src) {
    if (!h) return DASH_EINVAL;
    if (!h->loaded) return fail(h, DASH_ESTATE, "dash_broadcast_system: no traces loaded");
    if (src >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "dash_broadcast_system: system out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, dash::launch_broadcast(h->d_trace, h->d_lens, h->cfg.num_systems, src, (uint64_t)h->seg * h->nchunks,
                                     h->cfg.num_procs, h->stream));
    HIPCHK(h, traces_changed(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

// dash_explore and dash_explore_micro: broadcast, passes of num_systems seeds, the merge of their
// outcomes. weights == nullptr: seeded round schedules (dash_set_system_seeds); else seeded
// micro-step schedules under that one weight vector (dash_set_micro_seeds).
static int explore_impl(dash_t* h, const char* what, uint64_t src, uint64_t first_seed, uint64_t num_seeds,
                        const uint64_t* weights, dash_outcome* out, uint32_t cap, uint32_t* n) {
    return guarded(h, what, [&]() -> int {
        if (!h || !n || (!out && cap)) return DASH_EINVAL;
        *n = 0;
        const uint64_t nsys = h->cfg.num_systems;
        if (int rc = need_seed(h, what)) return rc;
        if (!weights && h->follow == sched_src::micro_table)
            return fail(h, DASH_ESTATE, "%s: the handle follows a micro-step schedule", what);
        if (num_seeds && !nsys) return fail(h, DASH_EINVAL, "%s: the handle has no systems", what);
        std::vector<dash_outcome> found;
        std::map<std::pair<uint64_t, uint32_t>, size_t> index;  // (digest, errors) -> found[]
        auto seed_of = [&](uint64_t k) { return first_seed + k; };
        // (the repeats that pad the last pass are not counted)
        const int rc = for_each_seed_pass(h, src, num_seeds, weights, seed_of, [&](const seed_pass& p) -> int {
            for (uint64_t i = 0; i < p.fresh; i++) {
                const auto it = index.emplace(std::make_pair(p.digests[i], p.errors[i]), found.size());
                if (it.second) found.push_back(dash_outcome{p.digests[i], 0, p.seeds[i], p.rounds[i], p.errors[i]});
                dash_outcome& o = found[it.first->second];
                o.count++;
                if (p.seeds[i] < o.seed) {  // only when first_seed + i wrapped past 2^64
                    o.seed = p.seeds[i];
                    o.rounds = p.rounds[i];
                }
            }
            return DASH_OK;
        });
        if (rc != DASH_OK) return rc;
        std::sort(found.begin(), found.end(), [](const dash_outcome& a, const dash_outcome& b) { return a.seed < b.seed; });
        *n = (uint32_t)std::min<size_t>(found.size(), 0xFFFFFFFFu);
        for (size_t k = 0; k < found.size() && k < cap; k++) out[k] = found[k];
        return DASH_OK;
    });
}

int dash_explore(dash_t* h, uint64_t src, uint64_t first_seed, uint64_t num_seeds, dash_outcome* out, uint32_t cap,
                 uint32_t* n) {
    return explore_impl(h, "dash_explore", src, first_seed, num_seeds, nullptr, out, cap, n);
}

int dash_explore_micro(dash_t* h, uint64_t src, uint64_t first_seed, uint64_t num_seeds, uint64_t weights,
                       dash_outcome* out, uint32_t cap, uint32_t* n) {
    if (h && !weights_valid(weights)) return fail(h, DASH_EINVAL, "dash_explore_micro: a weight above 31");
    return explore_impl(h, "dash_explore_micro", src, first_seed, num_seeds, &weights, out, cap, n);
}

}  // extern "C"
