// dash_core.cpp -- C-ABI of libdash over HIP: the handle's lifecycle, trace loading and
// generation, dash_run's tier loop and the read-back calls.
//
// Replaces main()'s OpenMP plumbing in /root/reference/assignment.c:
// omp_set_num_threads / queue + lock init (:135-144), the parallel region
// (:149-155) and the per-thread private processorNode (:145).
#include "dash_internal.h"

extern "C" {

// largest round cap: event words carry the round in bits 30..0 (bit 31 = issued instruction)
static constexpr uint64_t MAX_ROUNDS_CAP = 0x7FFFFFFCull;

const char* dash_last_error(const dash_t* h) { return h ? h->msg : g_msg; }

void* dash_stream(dash_t* h) { return h ? (void*)h->stream : nullptr; }

static void release(dash_t* h) {
    if (!h) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& o : h->owned)
        if (o.p) (void)(o.pinned ? hipHostFree(o.p) : hipFree(o.p));
    for (hipEvent_t e : h->events)
        if (e) (void)hipEventDestroy(e);
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

void dash_destroy(dash_t* h) {
    release(h);
    delete h;
}

int dash_create(const dash_cfg* cfg, dash_t** out) {
    set_global_msg("");  // dash_last_error(NULL) describes this call only
    auto invalid = [](const char* why) {
        set_global_msg(why);
        return DASH_EINVAL;
    };
    if (!cfg || !out) return invalid("dash_create: null cfg or out");
    *out = nullptr;
    const uint32_t N = cfg->num_procs, CS = cfg->cache_size;
    if (N < 1 || N > DASH_MAX_PROCS) return invalid("dash_create: num_procs must be 1..8");
    if (CS < 1 || CS > DASH_MAX_CACHE) return invalid("dash_create: cache_size must be 1..16");  // (ref :7)
    if (cfg->max_instr > (1u << 24)) return invalid("dash_create: max_instr above 2^24");
    if (cfg->num_systems > 0xFFFFFFFFull)  // system ids are u32 in the lists
        return invalid("dash_create: num_systems above 2^32 - 1");
    if (cfg->trace_events >= (1u << 30))
        return invalid("dash_create: trace_events must be below 2^30");
    if (cfg->trace_events && (double)cfg->num_systems * N * (cfg->trace_events + 3u) * 4.0 > 64.0 * (1ull << 30))
        return invalid("dash_create: event log larger than 64 GiB");
    dash_t* h = new (std::nothrow) dash_ctx();
    if (!h) {
        set_global_msg("dash_create: out of host memory");
        return DASH_ENOMEM;
    }
    h->cfg = *cfg;
    if (h->cfg.max_rounds == 0) h->cfg.max_rounds = 1024ull + 256ull * cfg->max_instr;
    // clamped below 2^31 (event words keep the round in bits 30..0) before it is rounded up to
    // the multiple of 4 the kernel tests at the first round of every trip (no wrap to 0)
    h->cfg.max_rounds = (std::min<uint64_t>(h->cfg.max_rounds, MAX_ROUNDS_CAP) + 3) & ~3ull;
    h->seg = (uint32_t)next_pow2(N);
    const uint64_t spw = 64 / h->seg;
    h->groups = (cfg->num_systems + spw - 1) / spw;
    {
        // lane stride of the trace layout: an odd number of 128-B lines, so the
        // streams of a wave's lanes (and of consecutive waves) spread over L2 sets
        // and channels instead of aliasing at a power-of-two stride
        const uint32_t raw = (cfg->max_instr + dash::CHUNK_INSTR - 1) / dash::CHUNK_INSTR;
        uint32_t lines = (raw * 8 + 127) / 128;
        // (measured: 359 vs 389 GB of L2 fills per 1M-system launch)
        h->nchunks = (lines + ((lines && !(lines & 1)) ? 1u : 0u)) * 16;
    }
    int rc = DASH_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == DASH_OK) rc = hip_fail(h, e, what);
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        delete h;
        set_global_msg("dash_create: no HIP device");
        return DASH_EDEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) {
        delete h;
        return invalid("dash_create: device ordinal out of range");
    }
    chk(hipSetDevice(cfg->device), "hipSetDevice");
    chk(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreate");
    chk(hipEventCreate(&h->ev0), "hipEventCreate");
    chk(hipEventCreate(&h->ev1), "hipEventCreate");
    const uint64_t nsys = cfg->num_systems;
    const uint64_t trace_words = h->groups * (uint64_t)std::max<uint32_t>(h->nchunks, 1) * 64;
    chk(buf_alloc(h, h->d_trace, trace_words + dash::TRACE_PAD), "hipMalloc(trace)");
    chk(buf_alloc(h, h->d_lens, nsys * N), "hipMalloc(lens)");
    chk(buf_alloc(h, h->d_digests, nsys), "hipMalloc(digests)");
    chk(buf_alloc(h, h->d_rounds, nsys), "hipMalloc(rounds)");
    chk(buf_alloc(h, h->d_errors, nsys), "hipMalloc(errors)");
    chk(buf_alloc(h, h->d_stats, dash::STAT_WORDS), "hipMalloc(stats)");
    chk(buf_alloc(h, h->d_hist, nsys * 13), "hipMalloc(hist)");
    chk(buf_alloc(h, h->d_list[0], nsys), "hipMalloc(list)");
    chk(buf_alloc(h, h->d_list[1], nsys), "hipMalloc(list)");
    chk(buf_alloc(h, h->d_count, 2), "hipMalloc(count)");
    chk(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking), "hipStreamCreate(side)");
    chk(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming), "hipEventCreate");
    chk(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming), "hipEventCreate");
    chk(buf_alloc(h, h->d_hint, nsys), "hipMalloc(hint)");
    chk(buf_alloc(h, h->d_skip, nsys), "hipMalloc(skip)");
    if (rc == DASH_OK) chk(hipMemset(h->d_skip, 0, std::max<uint64_t>(nsys, 1)), "hipMemset(skip)");
    if (cfg->trace_events) {
        h->ev_rounds = (cfg->trace_events + 3u) & ~3u;
        chk(buf_alloc(h, h->d_events, nsys * N * h->ev_rounds), "hipMalloc(events)");
        chk(buf_alloc(h, h->d_event_count, nsys * N), "hipMalloc(event_count)");
    }
    if (cfg->schedule_seed) {  // the seeded schedule's round words, built once per handle
        // DASH_TEST_SHORT_ARB (tests only) cuts the table to 8 rounds so the in-kernel hashing
        // past its end runs
        const uint64_t cap = (cfg->flags & DASH_TEST_SHORT_ARB) ? 8u : dash::ARB_TABLE_MAX;
        h->arb_len = (uint32_t)std::min<uint64_t>(h->cfg.max_rounds, std::min<uint64_t>(cap, dash::ARB_TABLE_MAX));
        chk(buf_alloc(h, h->d_arb, ((uint64_t)h->arb_len + 4) * h->seg), "hipMalloc(arb)");
        if (rc == DASH_OK) chk(dash::launch_arb_table(cfg->schedule_seed, h->seg, h->d_arb, h->arb_len, h->stream),
                               "arb table");
        if (rc == DASH_OK) chk(hipStreamSynchronize(h->stream), "arb table");
    }
    if (cfg->flags & DASH_KEEP_STATE) chk(buf_alloc(h, h->d_state, nsys * N * (16 + CS)), "hipMalloc(state)");
    if (rc != DASH_OK) {
        set_global_msg(h->msg);  // no stderr from the library: dash_last_error(NULL) has it
        dash_destroy(h);
        return rc;
    }
    *out = h;
    return DASH_OK;
}

int dash_load_traces(dash_t* h, const uint16_t* packed, uint64_t stride, const uint32_t* lens,
                     uint64_t num_systems) {
    return guarded(h, "dash_load_traces", [&]() -> int {
        if (!h || (!packed && num_systems) || !lens) return DASH_EINVAL;
        const uint32_t N = h->cfg.num_procs, P = h->seg;
        if (num_systems != h->cfg.num_systems) return fail(h, DASH_EINVAL, "num_systems mismatch");
        for (uint64_t i = 0; i < num_systems * N; i++)
            if (lens[i] > h->cfg.max_instr || lens[i] > stride)
                return fail(h, DASH_EINVAL, "trace %llu longer than max_instr", (unsigned long long)i);
        // the 3-bit node field cannot name a node >= 8, so only N < 8 needs the address scan
        if (N < 8)
            for (uint64_t r = 0; r < num_systems * N; r++)
                for (uint32_t i = 0; i < lens[r]; i++) {
                    const uint16_t w = packed[r * stride + i];
                    if (((w >> 12) & 7u) >= N)
                        return fail(h, DASH_EADDR, "system %llu node %u: address 0x%02X homed on node >= %u",
                                    (unsigned long long)(r / N), (unsigned)(r % N), (w >> 8) & 0x7F, N);
                }
        // lane-contiguous layout: [group][lane][chunk][4 x u16]
        const uint64_t words = h->groups * (uint64_t)h->nchunks * 64;
        constexpr uint32_t C = dash::CHUNK_INSTR;
        const uint64_t pitch = (uint64_t)h->nchunks * 8;  // lane stride in bytes
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (P == N) {
            // system s node t is lane row s*N + t in both layouts: one strided H2D copy, no
            // host staging. Words past a node's length are never issued (the kernel's pc < len
            // guard), so they need no zeroing.
            if (num_systems)
                HIPCHK(h, hipMemcpy2DAsync(h->d_trace, pitch, packed, stride * 2, std::min<uint64_t>(stride * 2, pitch),
                                           num_systems * N, hipMemcpyHostToDevice, h->stream));
        } else {
            std::vector<uint16_t> host(words * C, 0);
            for (uint64_t s = 0; s < num_systems; s++) {
                const uint64_t g = s / (64 / P);
                const uint32_t lane0 = (uint32_t)(s % (64 / P)) * P;
                for (uint32_t t = 0; t < N; t++) {
                    const uint16_t* src = packed + (s * N + t) * stride;
                    for (uint32_t i = 0; i < lens[s * N + t]; i++)
                        host[((g * 64 + lane0 + t) * h->nchunks + i / C) * C + (i % C)] = src[i];
                }
            }
            if (words)
                HIPCHK(h, hipMemcpyAsync(h->d_trace, host.data(), words * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));  // `host` is pageable and local
        }
        // RD carries value 0 whatever the caller's bits 7..0 say (ref :839; dash.h)
        HIPCHK(h, dash::launch_clear_rd(h->d_trace, words, h->stream));
        if (num_systems)
            HIPCHK(h, hipMemcpyAsync(h->d_lens, lens, num_systems * N * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, traces_changed(h));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->loaded = true;
        return DASH_OK;
    });
}

int dash_generate(dash_t* h, const dash_gen* g) {
    if (!h || !g) return DASH_EINVAL;
    if (g->len > h->cfg.max_instr) return fail(h, DASH_EINVAL, "gen len > max_instr");
    if (g->kind > DASH_GEN_LOCALITY) return fail(h, DASH_EINVAL, "unknown generator kind");
    dash::GenArgs a{};
    a.trace = h->d_trace;
    a.lens = h->d_lens;
    a.nsys = h->cfg.num_systems;
    a.ngroups = h->groups;
    a.seed = g->seed;
    a.sys_base = g->sys_base;
    a.nchunks = h->nchunks;
    a.num_procs = h->cfg.num_procs;
    a.seg = h->seg;
    a.kind = g->kind;
    a.locality = g->locality;
    a.len = g->len;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, dash::launch_gen(a, h->stream));
    HIPCHK(h, traces_changed(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->loaded = true;
    return DASH_OK;
}

// A pass's arguments but for its tier and lists. The schedule the handle follows decides what
// the kernel reads through arb_tab: a table of arb_len rounds, or, with arb_len == 0, the
// per-system seeds (dash_device.h).
static dash::SimArgs sim_args(const dash_t* h) {
    dash::SimArgs a{};
    a.trace = h->d_trace;
    a.lens = h->d_lens;
    a.nsys = h->cfg.num_systems;
    a.nchunks = h->nchunks;
    a.num_procs = h->cfg.num_procs;
    a.max_rounds = (uint32_t)h->cfg.max_rounds;
    a.digests = h->d_digests;
    a.rounds = h->d_rounds;
    a.errors = h->d_errors;
    a.state = h->d_state;
    a.hist = h->d_hist;
    a.keep = (h->cfg.flags & DASH_KEEP_STATE) ? 1u : 0u;
    a.event_cap = h->ev_rounds;
    a.arb_seed = h->cfg.schedule_seed;
    a.micro = micro_steps(h->follow) ? 1u : 0u;
    switch (h->follow) {
    case sched_src::round_table:
    case sched_src::micro_table:
        a.arb_tab = h->d_arb;
        a.arb_len = h->arb_len;
        break;
    case sched_src::system_seeds:
        a.arb_tab = reinterpret_cast<const uint32_t*>(h->d_seeds);
        a.arb_seed = dash::ARB_SYSTEM_SEEDS;
        break;
    case sched_src::system_delays:  // the same buffer, holding delay words
        a.arb_tab = reinterpret_cast<const uint32_t*>(h->d_seeds);
        a.arb_seed = dash::ARB_SYSTEM_DELAYS;
        break;
    case sched_src::micro_seeds:  // (seed, weights) pairs
        a.arb_tab = reinterpret_cast<const uint32_t*>(h->d_mseeds);
        break;
    }
    a.cache_size = h->cfg.cache_size;
    for (uint32_t b = 0; b < 16; b++)  // b % CACHE_SIZE for the generic (non-power-of-two) kernels
        a.cs_lut |= (uint64_t)(b % h->cfg.cache_size) << (4 * b);
    a.events = h->d_events;
    a.event_count = h->d_event_count;
    a.stats = h->d_stats;
    return a;
}

int dash_run(dash_t* h, dash_stats* stats) {
    if (!h) return DASH_EINVAL;
    if (!h->loaded) return fail(h, DASH_ESTATE, "no traces loaded");
    h->met.valid = false;  // dash_compute_metrics' records are the previous run's
    h->coh.valid = false;  // and dash_check_coherence's
    h->adr.valid = false;  // and dash_compute_addr_metrics'
    dash::SimArgs a = sim_args(h);
    const uint64_t spw = 64 / h->seg;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemsetAsync(h->d_stats, 0, dash::STAT_WORDS * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    // queue-depth tiers: every system runs at the first depth; systems that would
    // overflow it are listed and re-run from scratch at the next depth (exact:
    // the lockstep schedule is deterministic); the last tier drops like the reference.
    // Without a DASH_TIER_FROM_* flag the first depth adapts: when more than 1/32 of
    // the systems overflowed the first depth of a run, later runs start one deeper.
    uint64_t todo = h->cfg.num_systems;
    const uint32_t* list = nullptr;
    const uint32_t f = h->cfg.flags;
    const int first = (micro_steps(h->follow) || (f & DASH_TIER_FROM_256)) ? 2 : (f & DASH_TIER_FROM_32) ? 1 : h->auto_tier;
    if (h->hint_n && h->hint_tier != first) HIPCHK(h, reset_hint(h));
    // Systems that overflowed the first tier in an earlier run of these traces (the
    // schedule is deterministic, so they will again) start one tier deeper on the side
    // stream right away, while the first tier -- which skips them -- runs on the main
    // stream: the deeper pass no longer waits for the first tier's tail.
    const bool hint = h->hint_n > 0 && first < dash::NUM_TIERS - 1;
    const int ht = first + 1;
    if (hint) {
        HIPCHK(h, hipMemsetAsync(h->d_count + (ht & 1), 0, sizeof(uint32_t), h->stream));
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->side, h->ev_fork, 0));
        dash::SimArgs b = a;
        b.sys_list = h->d_hint;
        b.list_len = h->hint_n;
        b.final_tier = ht == dash::NUM_TIERS - 1 ? 1u : 0u;
        b.ovf_list = h->d_list[ht & 1];  // shared with the main stream's pass at this tier
        b.ovf_count = h->d_count + (ht & 1);
        HIPCHK(h, dash::launch_sim(b, h->seg, h->cfg.cache_size, dash::RING_TIERS[ht],
                                   (h->hint_n + spw - 1) / spw, h->side));
        HIPCHK(h, hipEventRecord(h->ev_join, h->side));
    }
    uint64_t first_ovf = 0;  // systems that overflowed the first tier in this run
    for (int tier = 0; tier < dash::NUM_TIERS; ++tier) h->tier_systems[tier] = 0;
    for (int tier = first; tier < dash::NUM_TIERS; ++tier) {
        const bool last = tier == dash::NUM_TIERS - 1;
        const bool joined = hint && tier == ht;  // the hinted pass ran this tier too
        h->tier_systems[tier] = todo + (joined ? h->hint_n : 0);
        uint32_t* out = h->d_list[tier & 1];
        uint32_t* cnt = h->d_count + (tier & 1);
        if (!joined) HIPCHK(h, hipMemsetAsync(cnt, 0, sizeof(uint32_t), h->stream));
        if (todo) {
            a.sys_list = list;
            a.list_len = todo;
            a.final_tier = last ? 1u : 0u;
            a.ovf_list = out;
            a.ovf_count = cnt;
            a.skip = (hint && tier == first) ? h->d_skip : nullptr;
            HIPCHK(h, dash::launch_sim(a, h->seg, h->cfg.cache_size, dash::RING_TIERS[tier],
                                       (todo + spw - 1) / spw, h->stream));
        }
        if (joined) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
        if (last) break;
        uint32_t next = 0;
        if (todo || joined) {
            HIPCHK(h, hipMemcpyAsync(&next, cnt, sizeof next, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        if (tier == first) first_ovf = next;
        todo = next;
        list = out;
    }
    if (first < dash::NUM_TIERS - 1 && first_ovf) {  // they join the hint for the next run
        HIPCHK(h, hipMemcpyAsync(h->d_hint + h->hint_n, h->d_list[first & 1], first_ovf * sizeof(uint32_t),
                                 hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, dash::launch_mark(h->d_list[first & 1], first_ovf, h->d_skip, h->stream));
        h->hint_n += first_ovf;
        h->hint_tier = first;
    }
    if (!(f & (DASH_TIER_FROM_32 | DASH_TIER_FROM_256)) && first < dash::NUM_TIERS - 1 &&
        h->tier_systems[first + 1] * 32 > h->tier_systems[first])
        h->auto_tier = first + 1;
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    unsigned long long s[dash::STAT_WORDS];
    HIPCHK(h, hipMemcpyAsync(s, h->d_stats, sizeof s, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->ran = true;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        for (int k = 0; k < DASH_NUM_TXN; k++) stats->hist[k] = s[dash::STAT_HIST + k];
        stats->instructions = s[dash::STAT_INSTR];
        stats->rounds_total = s[dash::STAT_ROUNDS];
        stats->rounds_max = s[dash::STAT_ROUNDS_MAX];
        stats->systems = s[dash::STAT_SYSTEMS];
        stats->err_systems = s[dash::STAT_ERRSYS];
        stats->err_bits = s[dash::STAT_ERRBITS];
        stats->dropped = s[dash::STAT_DROPS];
        stats->max_depth = s[dash::STAT_MAXDEPTH];
        stats->kernel_ms = ms;
        for (int k = 0; k < dash::NUM_TIERS; k++) stats->tier_systems[k] = h->tier_systems[k];
        stats->wave_rounds = s[dash::STAT_WAVE_ROUNDS];
    }
    return DASH_OK;
}

int dash_read_results(dash_t* h, uint64_t first, uint64_t count, uint64_t* digests,
                      uint32_t* rounds, uint32_t* errors) {
    if (!h) return DASH_EINVAL;
    if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
    if (first + count > h->cfg.num_systems || first + count < first)
        return fail(h, DASH_EINVAL, "range out of bounds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (digests && count)
        HIPCHK(h, hipMemcpyAsync(digests, h->d_digests + first, count * 8, hipMemcpyDeviceToHost, h->stream));
    if (rounds && count)
        HIPCHK(h, hipMemcpyAsync(rounds, h->d_rounds + first, count * 4, hipMemcpyDeviceToHost, h->stream));
    if (errors && count)
        HIPCHK(h, hipMemcpyAsync(errors, h->d_errors + first, count * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

int dash_read_state(dash_t* h, uint64_t sys, dash_node_state* out) {
    return guarded(h, "dash_read_state", [&]() -> int {
        if (!h || !out) return DASH_EINVAL;
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (!h->d_state) return fail(h, DASH_ESTATE, "created without DASH_KEEP_STATE");
        if (sys >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "system out of range");
        const uint32_t N = h->cfg.num_procs, CS = h->cfg.cache_size, W = 16 + CS;
        std::vector<uint32_t> w((size_t)N * W);
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, hipMemcpyAsync(w.data(), h->d_state + sys * N * W, w.size() * 4, hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint32_t t = 0; t < N; t++) {
            dash_node_state* s = &out[t];
            memset(s, 0, sizeof *s);
            for (uint32_t b = 0; b < 16; b++) {
                const uint32_t e = w[t * W + b];
                s->memory[b] = (uint8_t)(e & 0xFF);
                s->dir_bitvector[b] = (uint8_t)((e >> 8) & 0xFF);
                s->dir_state[b] = (uint8_t)((e >> 16) & 3);
            }
            for (uint32_t i = 0; i < CS; i++) {
                const uint32_t l = w[t * W + 16 + i];
                s->cache_addr[i] = (uint8_t)(l & 0xFF);
                s->cache_value[i] = (uint8_t)((l >> 8) & 0xFF);
                s->cache_state[i] = (uint8_t)((l >> 16) & 3);
            }
        }
        return DASH_OK;
    });
}

// testing only: dash_read_state's unpacking, inverted, over systems [first, first + count)
int dash_test_write_states(dash_t* h, uint64_t first, uint64_t count, const dash_node_state* nodes) {
    return guarded(h, "dash_test_write_states", [&]() -> int {
        if (!h || (!nodes && count)) return DASH_EINVAL;
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (!h->d_state) return fail(h, DASH_ESTATE, "created without DASH_KEEP_STATE");
        if (first + count > h->cfg.num_systems || first + count < first)
            return fail(h, DASH_EINVAL, "range out of bounds");
        const uint32_t N = h->cfg.num_procs, CS = h->cfg.cache_size, W = 16 + CS;
        std::vector<uint32_t> w((size_t)count * N * W);
        for (uint64_t k = 0; k < count * N; k++) {
            const dash_node_state* s = &nodes[k];
            uint32_t* o = &w[(size_t)k * W];
            for (uint32_t b = 0; b < 16; b++)
                o[b] = s->memory[b] | (uint32_t)s->dir_bitvector[b] << 8 | (uint32_t)(s->dir_state[b] & 3) << 16;
            for (uint32_t i = 0; i < CS; i++)
                o[16 + i] = s->cache_addr[i] | (uint32_t)s->cache_value[i] << 8 | (uint32_t)(s->cache_state[i] & 3) << 16;
        }
        h->coh.valid = false;  // the records are of the states that were
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (count) {
            HIPCHK(h, hipMemcpyAsync(h->d_state + first * N * W, w.data(), w.size() * 4, hipMemcpyHostToDevice,
                                     h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));  // w is pageable and leaves scope
        }
        return DASH_OK;
    });
}

int dash_read_hist(dash_t* h, uint64_t sys, uint32_t* hist) {
    if (!h || !hist) return DASH_EINVAL;
    if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
    if (!(h->cfg.flags & DASH_KEEP_STATE)) return fail(h, DASH_ESTATE, "created without DASH_KEEP_STATE");
    if (sys >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "system out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(hist, h->d_hist + sys * 13, 13 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DASH_OK;
}

// The event log of one system, as both readers take it: rounds[sys] (and, with cnt, the N
// per-node event counts), then the system's event words of this run's rounds. Only those: the
// kernel writes the log up to its wave's last trip and never clears it, so rows past the
// system's last active round may hold an earlier run's words. Events only happen in
// rounds < rounds[sys]; `ev` gets whole 4-round rows of those, as many as the log holds.
// count_only: a log that holds every round the system ran cannot be truncated and the counts
// are the answer, so the row copy is skipped.
static int fetch_events(dash_t* h, uint64_t sys, uint32_t* cnt, bool count_only, uint32_t* sys_rounds,
                        std::vector<uint32_t>& ev) {
    const uint32_t N = h->cfg.num_procs, R = h->ev_rounds;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (cnt) HIPCHK(h, hipMemcpyAsync(cnt, h->d_event_count + sys * N, N * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(sys_rounds, h->d_rounds + sys, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (count_only && *sys_rounds <= R) return DASH_OK;
    const uint32_t Rs = (uint32_t)std::min<uint64_t>(R, ((uint64_t)*sys_rounds + 3u) & ~3ull);
    ev.resize((size_t)N * Rs);
    if (Rs) {
        HIPCHK(h, hipMemcpyAsync(ev.data(), h->d_events + sys * N * (uint64_t)R, ev.size() * 4, hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return DASH_OK;
}

// node t's word of round r in fetch_events' rows: [round / 4][node][round % 4]
static uint32_t event_word(const std::vector<uint32_t>& ev, uint32_t N, uint32_t r, uint32_t t) {
    return ev[(size_t)(r / 4) * N * 4 + t * 4 + r % 4];
}

int dash_read_events(dash_t* h, uint64_t sys, dash_event* out, uint32_t cap, uint32_t* n) {
    return guarded(h, "dash_read_events", [&]() -> int {
        if (!h || (!out && cap) || !n) return DASH_EINVAL;
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (!h->d_events) return fail(h, DASH_ESTATE, "created with trace_events = 0");
        if (sys >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "system out of range");
        const uint32_t N = h->cfg.num_procs, R = h->ev_rounds;
        std::vector<uint32_t> cnt(N), ev;
        uint32_t sys_rounds = 0;
        int rc = fetch_events(h, sys, cnt.data(), !out, &sys_rounds, ev);
        if (rc != DASH_OK) return rc;
        uint64_t total = 0, logged = 0;
        for (uint32_t t = 0; t < N; t++) total += cnt[t];
        *n = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
        if (!out && sys_rounds <= R) return DASH_OK;  // the count-only call: nothing fetched
        // the log is round-major (a node logs at most one event per round): reading it round by
        // round, node by node, is the lockstep order
        uint32_t k = 0;
        for (uint32_t r = 0; r < std::min(R, sys_rounds); r++)
            for (uint32_t t = 0; t < N; t++) {
                const uint32_t w = event_word(ev, N, r, t);
                if (!(w & dash::EV_EVENT)) continue;
                ++logged;
                if (k < cap) {
                    out[k].round = r;
                    out[k].node = t;
                    out[k].kind = (w & dash::EV_INSTR) ? DASH_EV_INSTR : DASH_EV_MSG;
                    // a message word without the kernel's internal bits (7: REPLY_RD's dirState,
                    // 15: the reply-table flag, 24) and with secondReceiver moved from bits 30..28
                    // to 26..24, as include/dash.h documents it
                    out[k].word = (w & dash::EV_INSTR) ? (w & 0xFFFFu) : (w & 0x00FF7F7Fu) | (((w >> 28) & 7u) << 24);
                }
                ++k;
            }
        // events past the log's rounds were counted, not stored
        return logged < total ? fail(h, DASH_ETRUNC, "event log truncated at %u rounds", R) : DASH_OK;
    });
}

int dash_read_micro_acts(dash_t* h, uint64_t sys, uint8_t* acts, uint32_t cap_rounds, uint32_t* rounds) {
    return guarded(h, "dash_read_micro_acts", [&]() -> int {
        if (!h || !rounds || (!acts && cap_rounds)) return DASH_EINVAL;
        *rounds = 0;
        if (h->follow != sched_src::micro_seeds) return fail(h, DASH_ESTATE, "dash_read_micro_acts: no micro seeds set");
        if (!h->d_events) return fail(h, DASH_ESTATE, "dash_read_micro_acts: created with trace_events = 0");
        if (!h->ran) return fail(h, DASH_ESTATE, "dash_run has not completed");
        if (sys >= h->cfg.num_systems) return fail(h, DASH_EINVAL, "system out of range");
        const uint32_t N = h->cfg.num_procs, R = h->ev_rounds;
        std::vector<uint32_t> ev;
        int rc = fetch_events(h, sys, nullptr, false, rounds, ev);
        if (rc != DASH_OK) return rc;
        if (*rounds > R)
            return fail(h, DASH_ETRUNC, "dash_read_micro_acts: the run took %u rounds, the log holds %u", *rounds, R);
        if (*rounds > cap_rounds)
            return fail(h, DASH_EINVAL, "dash_read_micro_acts: %u rounds > cap_rounds %u", *rounds, cap_rounds);
        // a round's acting node left an event word (it stepped) or the delivery marker
        for (uint32_t r = 0; r < *rounds; r++)
            for (uint32_t t = 0; t < N; t++) {
                const uint32_t w = event_word(ev, N, r, t);
                acts[(uint64_t)r * N + t] =
                    (w & dash::EV_EVENT) ? DASH_MICRO_STEP : w == dash::EV_MICRO_SEND ? DASH_MICRO_SEND : DASH_SIT_OUT;
            }
        return DASH_OK;
    });
}

int dash_read_traces(dash_t* h, uint16_t* packed, uint64_t stride, uint32_t* lens) {
    return guarded(h, "dash_read_traces", [&]() -> int {
        if (!h || !lens) return DASH_EINVAL;
        if (!h->loaded) return fail(h, DASH_ESTATE, "no traces loaded");
        const uint32_t N = h->cfg.num_procs, P = h->seg;
        const uint64_t rows = h->cfg.num_systems * N;
        if (!packed && rows && stride) return DASH_EINVAL;
        HIPCHK(h, hipSetDevice(h->cfg.device));
        if (rows) HIPCHK(h, hipMemcpyAsync(lens, h->d_lens, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint64_t r = 0; r < rows; r++)
            if (lens[r] > stride)
                return fail(h, DASH_EINVAL, "dash_read_traces: trace %llu holds %u words, stride %llu",
                            (unsigned long long)r, lens[r], (unsigned long long)stride);
        // system s node t is row s * N + t in both layouts
        if (P == N) return copy_rows_out(h, h->d_trace, rows, lens, packed, stride);
        constexpr uint32_t C = dash::CHUNK_INSTR;
        if (rows && stride && h->nchunks) {
            const uint64_t words = h->groups * (uint64_t)h->nchunks * 64;
            std::vector<uint16_t> host(words * C);
            HIPCHK(h, hipMemcpyAsync(host.data(), h->d_trace, words * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (uint64_t s = 0; s < h->cfg.num_systems; s++) {
                const uint64_t g = s / (64 / P);
                const uint32_t lane0 = (uint32_t)(s % (64 / P)) * P;
                for (uint32_t t = 0; t < N; t++)
                    memcpy(packed + (s * N + t) * stride, &host[(g * 64 + lane0 + t) * h->nchunks * C],
                           (size_t)lens[s * N + t] * 2);
            }
        }
        zero_past_lens(packed, stride, rows, lens);
        return DASH_OK;
    });
}

}  // extern "C"
