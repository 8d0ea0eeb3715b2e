// dash_internal.h -- what the host files of libdash share: the handle, the error plumbing and
// the helpers for device buffers and threads. Internal: not installed, not part of dash.h.
// (dash_core.cpp, dash_sched.cpp, dash_load.cpp, dash_tools.cpp, dash_metrics.cpp,
// dash_coherence.cpp, dash_outcomes.cpp, dash_shrink.cpp)
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

// which schedule dash_run follows (the dash_set_* call made last decides)
enum class sched_src : uint8_t {
    round_table,   // the round table in d_arb: the handle seed's, or dash_set_schedule's
    micro_table,   // d_arb holds a micro-step table (dash_set_micro_schedule, MODE 4)
    system_seeds,  // d_seeds: a seeded round schedule per system (dash_set_system_seeds)
    micro_seeds,   // d_mseeds: a seeded micro-step schedule per system (dash_set_micro_seeds)
};

// a micro-step schedule (sim_kernel MODE 4): it runs at the reference's queue depth only
inline bool micro_steps(sched_src s) { return s == sched_src::micro_table || s == sched_src::micro_seeds; }

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
    } owned[48] = {};
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
    // dash_compute_metrics (dash_metrics.cpp): allocated on first use; dash_run invalidates them
    uint4* d_metrics = nullptr;                  // [num_systems * num_procs] 64-B records
    uint8_t* d_metrics_cut = nullptr;            // [num_systems] log shorter than the run
    unsigned long long* d_metrics_tot = nullptr;  // [dash::TOT_WORDS]
    bool metrics = false;                        // the records are those of the last run
    // dash_check_coherence (dash_coherence.cpp): likewise
    uint4* d_coh = nullptr;                      // [num_systems] dash_coherence records
    unsigned long long* d_coh_tot = nullptr;     // [dash::COH_TOT_WORDS]
    bool coherence = false;                      // the records are those of the last run
    // dash_explore_sources (dash_outcomes.cpp): allocated by the call, kept and reused while they fit
    void* d_oc_table = nullptr;                  // [oc_slots] dash::OutcomeSlot
    uint64_t oc_slots = 0;
    void* d_oc_out = nullptr;                    // [oc_out_cap] compacted entries (dash_outcome_ex)
    uint64_t oc_out_cap = 0;
    uint32_t* d_oc_place = nullptr;              // [num_systems] the slot of every system of the pass
    unsigned long long* d_oc_counters = nullptr;  // [dash::OC_WORDS]
    hipEvent_t oc_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // around the kernels before / after
                                                                          // dash_run, and after the insert
    // dash_shrink (dash_shrink.cpp): allocated on first use and kept
    uint2* d_sh_base = nullptr;                  // [2] system rows: the base and the row the next one is written to
    uint32_t* d_sh_lens = nullptr;               // [2][DASH_MAX_PROCS] their lengths
    uint32_t* d_sh_count = nullptr;              // [num_systems] instructions each system's candidate deletes
    unsigned long long* d_sh_cell = nullptr;     // the round's winner (dash::shrink_key), 0 = none
    hipEvent_t sh_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // around the variant, select
                                                                                  // and apply launches
    char msg[256] = {0};
    // device-side text ingest (dash_load_text / dash_load_dirs_device): buffers grown on first
    // use and kept, so a repeated load allocates nothing
    uint8_t* d_text = nullptr;  // text slab
    uint64_t d_text_cap = 0;
    uint64_t* d_foff = nullptr;  // per file of a launch: offset, length
    uint32_t* d_flen = nullptr;
    uint64_t d_files_cap = 0;
    unsigned long long* d_fail = nullptr;  // first-failure cell (dash_ingest.h)
    char* pin[2] = {nullptr, nullptr};     // pinned slabs of dash_load_dirs_device
    uint64_t pin_cap = 0;
    uint64_t* pin_off[2] = {nullptr, nullptr};
    uint32_t* pin_len[2] = {nullptr, nullptr};
    uint64_t pin_files_cap = 0;
    hipEvent_t iev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    dash_ingest_report ingest{};
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

// new traces: the overflow hint no longer applies
inline hipError_t reset_hint(dash_t* h) {
    if (h->hint_n == 0) return hipSuccess;
    h->hint_n = 0;
    h->hint_tier = -1;
    return hipMemsetAsync(h->d_skip, 0, std::max<uint64_t>(h->cfg.num_systems, 1), h->stream);
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
