// dash_internal.h -- what the host files of libdash share: the handle, the error plumbing and
// the helpers for device buffers and threads. Internal: not installed, not part of dash.h.
// (dash_core.cpp, dash_sched.cpp, dash_load.cpp, dash_tools.cpp, dash_metrics.cpp,
// dash_coherence.cpp, dash_outcomes.cpp, dash_shrink.cpp, dash_addr.cpp)
//
// Four mechanisms are written here once, and a new search call is written against them:
//  * What voids results. traces_changed and schedule_changed are the only places that mark the
//    handle as not run, say what it follows and drop the overflow hint; every load, every
//    dash_set_* call and every pass of a search goes through one of them.
//  * Buffers on first use. alloc_group allocates all of a feature's buffers or none, ensure_seeds
//    the per-system seed buffers, grow a buffer that is kept while it fits. All of it is entered
//    into owned[], which release() frees.
//  * Stage timing. A stage_timer's events are created on first use and entered into events[], which
//    release() destroys; mark(i) records one, add(a, b, sum) adds the time between two.
//  * One pass of a search. run_pass for the calls that write traces or seeds on the device
//    (dash_explore_sources, dash_shrink, dash_shrink_many): the change, dash_run, its kernel time. for_each_seed_pass
//    for the host-driven search over seeds (dash_explore, dash_explore_micro, dash_check_outcomes).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <thread>
#include <vector>

#include "dash.h"
#include "dash_device.h"

namespace dash {
struct OutcomeSlot;  // dash_outcomes.h
struct OutcomeOut;
struct ManyJob;  // dash_shrink.h
struct ManyStep;
}  // namespace dash

// Stage timing with device events: mark(i) records event i on a stream, add(a, b, sum) adds the
// milliseconds between two completed marks. timer_ready (below) creates the events.
struct stage_timer {
    hipEvent_t ev[6] = {};
    hipError_t mark(int i, hipStream_t s) const { return hipEventRecord(ev[i], s); }
    hipError_t add(int a, int b, double& sum) const {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, ev[a], ev[b]);
        sum += ms;
        return e;
    }
};

// which schedule dash_run follows (the dash_set_* call made last decides)
enum class sched_src : uint8_t {
    round_table,   // the round table in d_arb: the handle seed's, or dash_set_schedule's
    micro_table,   // d_arb holds a micro-step table (dash_set_micro_schedule, MODE 4)
    system_seeds,  // d_seeds: a seeded round schedule per system (dash_set_system_seeds)
    micro_seeds,   // d_mseeds: a seeded micro-step schedule per system (dash_set_micro_seeds)
    system_delays, // d_seeds holds a delay word per system (dash_set_system_delays)
};

// a micro-step schedule (sim_kernel MODE 4): it runs at the reference's queue depth only
inline bool micro_steps(sched_src s) { return s == sched_src::micro_table || s == sched_src::micro_seeds; }
// a round schedule of its own per system, read from d_seeds: its runs made the overflow hint
inline bool per_system_rounds(sched_src s) { return s == sched_src::system_seeds || s == sched_src::system_delays; }

struct dash_ctx {
    dash_cfg cfg{};
    uint32_t seg = 0;       // lanes per system (next pow2 of num_procs)
    uint64_t groups = 0;    // waves (64/seg systems each)
    uint32_t nchunks = 0;   // lane stride of the trace layout in 4-instruction (8-B) chunks
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // device and pinned memory of the handle: buf_alloc enters it here, release() frees what is listed
    struct {
        void* p;
        bool pinned;
    } owned[56] = {};
    hipEvent_t events[18] = {};  // the stage timers' events: timer_ready enters them, release() destroys them
    uint2* d_trace = nullptr;
    uint32_t* d_lens = nullptr;
    uint64_t* d_digests = nullptr;
    uint32_t* d_rounds = nullptr;
    uint32_t* d_errors = nullptr;
    uint32_t* d_state = nullptr;
    uint32_t* d_hist = nullptr;
    unsigned long long* d_stats = nullptr;
    uint32_t* d_list[2] = {nullptr, nullptr};  // overflow hand-off lists (ping-pong)
    uint32_t* d_count = nullptr;
    uint32_t* d_events = nullptr;       // [sys][round / 4][node][round % 4] (rounds: ev_rounds)
    uint32_t* d_arb = nullptr;          // seeded schedule: one word per node and round (dash::arb_node)
    uint32_t arb_len = 0;
    bool tab_explicit = false;          // d_arb holds an explicit table (dash_set_schedule,
                                        // dash_set_micro_schedule), not the handle seed's own
    sched_src follow = sched_src::round_table;
    uint64_t* d_seeds = nullptr;        // [num_systems] per-system schedule seeds (dash_set_system_seeds)
    uint64_t* d_mseeds = nullptr;       // [num_systems][2] seed, weights (dash_set_micro_seeds)
    uint32_t* d_event_count = nullptr;  // [sys*N+node]
    uint32_t ev_rounds = 0;             // trace_events rounded up to a multiple of 4
    uint64_t tier_systems[dash::NUM_TIERS] = {};  // systems run per queue-depth tier, last run
    int auto_tier = 0;                         // adaptive first tier
    // overflow hint: the systems that overflowed the first tier in earlier
    // runs of the same traces; the next run starts them one tier deeper on a side stream,
    // concurrently with the first tier, which skips them. Reset whenever traces change.
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    uint32_t* d_hint = nullptr;  // [num_systems] system ids
    uint8_t* d_skip = nullptr;   // [num_systems] 1 = in the hint
    uint64_t hint_n = 0;
    int hint_tier = -1;
    bool loaded = false;
    bool ran = false;
    char msg[256] = {0};
    // What follows is allocated on first use, one group per host file that owns it.
    struct {  // dash_compute_metrics (dash_metrics.cpp); dash_run invalidates the records
        uint4* d_rec = nullptr;                // [num_systems * num_procs] 64-B records
        uint8_t* d_cut = nullptr;              // [num_systems] log shorter than the run
        unsigned long long* d_tot = nullptr;   // [dash::TOT_WORDS]
        bool valid = false;                    // the records are those of the last run
    } met;
    struct {  // dash_compute_addr_metrics (dash_addr.cpp): likewise
        uint4* d_rec = nullptr;                // [num_systems * num_procs * 16] 48-B records, 3 uint4 each
        uint8_t* d_cut = nullptr;              // [num_systems] log shorter than the run
        unsigned long long* d_tot = nullptr;   // [dash::ADT_WORDS]
        bool valid = false;                    // the records are those of the last run
    } adr;
    struct {  // dash_check_coherence (dash_coherence.cpp): likewise
        uint4* d_rec = nullptr;                // [num_systems] dash_coherence records
        unsigned long long* d_tot = nullptr;   // [dash::COH_TOT_WORDS]
        bool valid = false;                    // the records are those of the last run
    } coh;
    struct {  // dash_explore_sources (dash_outcomes.cpp): kept and reused while they fit
        dash::OutcomeSlot* d_table = nullptr;  // [slots]
        uint64_t slots = 0;
        dash::OutcomeOut* d_out = nullptr;     // [out_cap] compacted entries (dash_outcome_ex)
        uint64_t out_cap = 0;
        uint32_t* d_place = nullptr;           // [num_systems] the slot of every system of the pass
        unsigned long long* d_counters = nullptr;  // [dash::OC_WORDS]
        stage_timer timer;                     // 5 marks: around the kernels before / after dash_run, and after the insert
    } oc;
    struct {  // dash_shrink, dash_shrink_many (dash_shrink.cpp): sized by the jobs of a call, kept and reused while they fit
        uint2* d_base = nullptr;               // [2 * jobs_cap] system rows: two per job
        dash::ManyJob* d_jobs = nullptr;       // [jobs_cap] the jobs' records
        uint32_t* d_words = nullptr;           // [2 * jobs_cap][DASH_MAX_PROCS] the rows' lengths, then per system its
                                               // job, its candidate and what that deletes: [3][num_systems]
        uint64_t* d_u64 = nullptr;             // [jobs_cap + 1] P and T, then [jobs_cap] the jobs' winner cells
        uint64_t jobs_cap = 0;
        dash::ManyStep* d_steps = nullptr;     // [jobs][step_cap] the device step log
        uint64_t steps_cap = 0;
        stage_timer timer;                     // 6 marks: around the variant, select and apply launches
    } shm;
    struct {  // device-side text ingest (dash_load.cpp): grown on first use and kept, so a repeated
              // load allocates nothing
        uint8_t* d_text = nullptr;  // text slab
        uint64_t text_cap = 0;
        uint64_t* d_foff = nullptr;  // per file of a launch: offset, length
        uint32_t* d_flen = nullptr;
        uint64_t files_cap = 0;
        unsigned long long* d_fail = nullptr;  // first-failure cell (dash_ingest.h)
        char* pin[2] = {nullptr, nullptr};     // pinned slabs of dash_load_dirs_device
        uint64_t pin_cap = 0;
        uint64_t* pin_off[2] = {nullptr, nullptr};
        uint32_t* pin_len[2] = {nullptr, nullptr};
        uint64_t pin_files_cap = 0;
        stage_timer timer[2];  // per pinned slab, 3 marks: before its copy, after it, after its parse
        dash_ingest_report report{};
    } ingest;
};

inline int fail(dash_t* h, int code, const char* fmt, ...) {
    if (h) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(h->msg, sizeof h->msg, fmt, ap);
        va_end(ap);
    }
    return code;
}

// a failed HIP call as a DASH_E* code: out of device memory is DASH_ENOMEM
inline int hip_fail(dash_t* h, hipError_t e, const char* what) {
    return fail(h, e == hipErrorOutOfMemory ? DASH_ENOMEM : DASH_EDEVICE, "%s: %s", what, hipGetErrorString(e));
}

#define HIPCHK(h, expr)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail((h), DASH_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

// Frees p (device or pinned memory from buf_alloc; nullptr is fine) and forgets it.
template <class T>
void buf_free(dash_t* h, T*& p) {
    for (auto& o : h->owned)
        if (p && o.p == p) {
            (void)(o.pinned ? hipHostFree(p) : hipFree(p));
            o.p = p = nullptr;
        }
}

// p := n elements of device (or pinned host) memory owned by the handle, in place of what p
// held. At least one element: a buffer of an empty batch still has an address to pass on.
template <class T>
hipError_t buf_alloc(dash_t* h, T*& p, uint64_t n, bool pinned = false) {
    buf_free(h, p);
    auto slot = std::find_if(std::begin(h->owned), std::end(h->owned), [](const auto& o) { return !o.p; });
    if (slot == std::end(h->owned)) return hipErrorOutOfMemory;
    const size_t bytes = std::max<uint64_t>(n, 1) * sizeof(T);
    const hipError_t e = pinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) p = nullptr;
    slot->p = p;
    slot->pinned = pinned;
    return e;
}

// All of a feature's buffers or none: (pointer, elements) pairs, allocated in order; after a failure
// those already made are freed again.
inline hipError_t alloc_all(dash_t*) { return hipSuccess; }
template <class T, class... Rest>
hipError_t alloc_all(dash_t* h, T*& p, uint64_t n, Rest&&... rest) {
    hipError_t e = buf_alloc(h, p, n);
    if (e == hipSuccess) e = alloc_all(h, rest...);
    if (e != hipSuccess) buf_free(h, p);
    return e;
}
template <class... Bufs>
int alloc_group(dash_t* h, const char* what, Bufs&&... bufs) {
    const hipError_t e = alloc_all(h, bufs...);
    return e == hipSuccess ? DASH_OK : hip_fail(h, e, what);
}

// p := n elements, unless it already holds at least that many (have); what it held is not kept
template <class T>
int grow(dash_t* h, T*& p, uint64_t& have, uint64_t n, const char* what) {
    if (p && have >= n) return DASH_OK;
    const hipError_t e = buf_alloc(h, p, n);
    have = e == hipSuccess ? n : 0;
    return e == hipSuccess ? DASH_OK : hip_fail(h, e, what);
}

// the per-system seed buffer (micro: the (seed, weights) pairs), allocated on first use and kept
inline int ensure_seeds(dash_t* h, bool micro) {
    uint64_t*& d = micro ? h->d_mseeds : h->d_seeds;
    if (d) return DASH_OK;
    const hipError_t e = buf_alloc(h, d, (micro ? 2 : 1) * h->cfg.num_systems);
    return e == hipSuccess ? DASH_OK : hip_fail(h, e, micro ? "hipMalloc(micro seeds)" : "hipMalloc(seeds)");
}

// the first n events of t exist: created on first use and entered into the handle's list
inline hipError_t timer_ready(dash_t* h, stage_timer& t, int n) {
    for (int i = 0; i < n; i++) {
        if (t.ev[i]) continue;
        hipEvent_t* slot = std::find(std::begin(h->events), std::end(h->events), nullptr);
        if (slot == std::end(h->events)) return hipErrorOutOfMemory;
        const hipError_t e = hipEventCreate(&t.ev[i]);
        if (e != hipSuccess) return e;
        *slot = t.ev[i];
    }
    return hipSuccess;
}

// the overflow hint no longer applies (below, and dash_run when its first tier changed)
inline hipError_t reset_hint(dash_t* h) {
    if (h->hint_n == 0) return hipSuccess;
    h->hint_n = 0;
    h->hint_tier = -1;
    return hipMemsetAsync(h->d_skip, 0, std::max<uint64_t>(h->cfg.num_systems, 1), h->stream);
}

// The traces changed, or are about to be written in place: earlier results no longer stand, and
// neither does the overflow hint, whose memset is enqueued here. rehint = false: a load that has
// only begun; it calls again once the new traces are on the stream.
inline hipError_t traces_changed(dash_t* h, bool rehint = true) {
    h->ran = false;
    return rehint ? reset_hint(h) : hipSuccess;
}

// What the runs follow changed: earlier results no longer stand. rehint: which systems overflow a
// tier depends on their schedules, so the overflow hint of earlier runs is void too.
inline hipError_t schedule_changed(dash_t* h, sched_src src, bool rehint) {
    h->follow = src;
    h->ran = false;
    return rehint ? reset_hint(h) : hipSuccess;
}

// One pass of a search that wrote its traces or seeds on the device: the handle follows *follow from
// here on (nullptr: only the traces changed), then dash_run, which returns with the stream idle;
// its kernel time is added to sim_ms.
inline int run_pass(dash_t* h, const sched_src* follow, double& sim_ms) {
    HIPCHK(h, follow ? schedule_changed(h, *follow, true) : traces_changed(h));
    dash_stats st;
    if (int rc = dash_run(h, &st)) return rc;
    sim_ms += st.kernel_ms;
    return DASH_OK;
}

// One pass of the host-driven search over seeds, as for_each_seed_pass hands it on: the seeds of all
// systems, of which the first `fresh` are new (the others repeat them), and those systems' results.
struct seed_pass {
    uint64_t base, fresh;  // the pass covers items [base, base + fresh) of the search
    const uint64_t* seeds;
    const uint64_t* digests;
    const uint32_t* rounds;
    const uint32_t* errors;
};

// dash_explore, dash_explore_micro and dash_check_outcomes: every system becomes a copy of src; then,
// num_systems items per pass, system i follows seed_of(item) (weights == nullptr: a seeded round
// schedule, dash_set_system_seeds; else a seeded micro-step schedule under that one vector,
// dash_set_micro_seeds), the batch runs and body(seed_pass) takes the results of the new items. The
// last pass pads with repeats of its own items.
template <class SeedOf, class Body>
int for_each_seed_pass(dash_t* h, uint64_t src, uint64_t n, const uint64_t* weights, SeedOf&& seed_of, Body&& body) {
    const uint64_t nsys = h->cfg.num_systems;
    int rc = dash_broadcast_system(h, src);
    if (rc != DASH_OK) return rc;
    std::vector<uint64_t> seeds(nsys), dig(nsys), wts(weights ? nsys : 0, weights ? *weights : 0);
    std::vector<uint32_t> rnd(nsys), err(nsys);
    for (uint64_t base = 0; base < n; base += nsys) {
        const uint64_t fresh = std::min<uint64_t>(nsys, n - base);
        for (uint64_t i = 0; i < nsys; i++) seeds[i] = seed_of(base + i % fresh);
        rc = weights ? dash_set_micro_seeds(h, seeds.data(), wts.data(), nsys)
                     : dash_set_system_seeds(h, seeds.data(), nsys);
        if (rc != DASH_OK) return rc;
        if ((rc = dash_run(h, nullptr)) != DASH_OK) return rc;
        if ((rc = dash_read_results(h, 0, fresh, dig.data(), rnd.data(), err.data())) != DASH_OK) return rc;
        if ((rc = body(seed_pass{base, fresh, seeds.data(), dig.data(), rnd.data(), err.data()})) != DASH_OK) return rc;
    }
    return DASH_OK;
}

// the least power of two >= n
inline uint64_t next_pow2(uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// a micro-step weight vector: every node's weight is at most 31
inline bool weights_valid(uint64_t w) { return !(w & 0xE0E0E0E0E0E0E0E0ull); }

// words at or past a row's length have no defined content on the device: they read as 0
inline void zero_past_lens(uint16_t* packed, uint64_t stride, uint64_t rows, const uint32_t* lens) {
    for (uint64_t r = 0; r < rows; r++)
        if (stride > lens[r]) memset(packed + r * stride + lens[r], 0, (size_t)(stride - lens[r]) * 2);
}

// `rows` consecutive lane rows from src_row on, out to packed at `stride` words per row, zeroed past
// each row's length. The stream is idle afterwards.
inline int copy_rows_out(dash_t* h, const uint2* src_row, uint64_t rows, const uint32_t* lens, uint16_t* packed,
                         uint64_t stride) {
    const uint64_t pitch = (uint64_t)h->nchunks * 8;  // device row stride in bytes
    const uint64_t width = std::min<uint64_t>(stride * 2, pitch);
    if (rows && width) {
        HIPCHK(h, hipMemcpy2DAsync(packed, stride * 2, src_row, pitch, width, rows, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    zero_past_lens(packed, stride, rows, lens);
    return DASH_OK;
}

// dash_check_coherence up to and including its launch, without the copy of the totals and the wait
// (dash_coherence.cpp); the caller sets h->coherence once the stream has passed it
int coherence_enqueue(dash_t* h);

// message of the last failed handle-less call (dash_create, dash_run_host_batched, ...) on this thread
inline thread_local char g_msg[256] = "";

inline void set_global_msg(const char* m) { snprintf(g_msg, sizeof g_msg, "%s", m ? m : ""); }

// Runs an entry point's body so that no C++ exception crosses the C-ABI: a failed allocation
// becomes DASH_ENOMEM (on the handle, or dash_last_error(NULL) without one).
template <class F>
int guarded(dash_t* h, const char* what, F&& body) {
    char m[256];
    try {
        return body();
    } catch (const std::bad_alloc&) {
        snprintf(m, sizeof m, "%s: out of host memory", what);
        if (h) return fail(h, DASH_ENOMEM, "%s", m);
        set_global_msg(m);
        return DASH_ENOMEM;
    } catch (...) {
        snprintf(m, sizeof m, "%s: unexpected host failure", what);
        if (h) return fail(h, DASH_EDEVICE, "%s", m);
        set_global_msg(m);
        return DASH_EDEVICE;
    }
}

// threads for `work` independent pieces of host work: at most 16, whatever the machine has
inline unsigned host_threads(uint64_t work) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({work, 16, std::thread::hardware_concurrency()}));
}

// fn(j) for every j < nt, on up to nt threads: the caller runs j = 0 and every index whose
// thread could not start, then joins the rest
template <class F>
void run_indexed(unsigned nt, F&& fn) {
    std::vector<std::thread> pool;
    unsigned started = 1;
    try {
        for (; started < nt; started++) pool.emplace_back(std::ref(fn), started);
    } catch (...) {  // no thread: the calling thread takes the remaining indices
    }
    if (nt) fn(0u);
    for (unsigned j = started; j < nt; j++) fn(j);
    for (auto& th : pool) th.join();
}
