// dash_tools.cpp -- C-ABI of libdash over HIP: what is built on the core calls. The digest
// writer, the state dump, the box probe, dash_simulate_dir and dash_run_host_batched.
#include <sys/stat.h>

#include <atomic>
#include <cerrno>
#include <memory>

#include "dash_internal.h"

extern "C" {

int dash_dump_system(dash_t* h, uint64_t sys, const char* out_dir) {
    return guarded(h, "dash_dump_system", [&]() -> int {
        if (!h || !out_dir) return DASH_EINVAL;
        std::vector<dash_node_state> st(h->cfg.num_procs);
        int rc = dash_read_state(h, sys, st.data());
        if (rc != DASH_OK) return rc;
        if (mkdir(out_dir, 0755) != 0 && errno != EEXIST) return fail(h, DASH_EIO, "mkdir %s", out_dir);
        for (uint32_t t = 0; t < h->cfg.num_procs; t++) {
            char path[4200];
            snprintf(path, sizeof path, "%s/core_%u_output.txt", out_dir, t);
            rc = dash_dump_file(&st[t], t, h->cfg.cache_size, path);
            if (rc != DASH_OK) return fail(h, rc, "write %s", path);
        }
        return DASH_OK;
    });
}

// dash_write_digests: the lines of fprintf("%llu %016llx %u %x\n") for every system, formatted by
// hand in parallel chunks (one fprintf per line ran at ~4e6 lines/s) and written in order. The
// results are read and formatted one window of chunks (2 per thread) at a time, into buffers
// reused from window to window, so host memory stays bounded (~8 MiB of text per thread) at
// any num_systems.
static int write_digests_impl(dash_t* h, const char* path) {
    const uint64_t n = h->cfg.num_systems;
    constexpr uint64_t CHUNK = 1u << 16;  // lines per chunk: <= 64 B each
    const unsigned nt = host_threads(16);
    const uint64_t window = std::max<uint64_t>(1, std::min<uint64_t>(n, 2ull * nt * CHUNK));
    // default-initialised (new T[]): zero-filling ~100 MB of buffers the writer overwrites anyway
    // cost as much as the formatting (round 4: 26.5 ms per 1M systems)
    std::unique_ptr<uint64_t[]> d(new uint64_t[window]);
    std::unique_ptr<uint32_t[]> r(new uint32_t[window]), e(new uint32_t[window]);
    const uint64_t wch = (window + CHUNK - 1) / CHUNK;
    std::vector<std::unique_ptr<char[]>> buf(wch);
    for (auto& b : buf) b.reset(new char[CHUNK * 64]);
    std::vector<size_t> used(wch);
    FILE* f = fopen(path, "w");
    if (!f) return fail(h, DASH_EIO, "open %s", path);
    bool ok = true;
    for (uint64_t w0 = 0; ok && w0 < n; w0 += window) {
        const uint64_t wn = std::min(window, n - w0);
        int rc = dash_read_results(h, w0, wn, d.get(), r.get(), e.get());
        if (rc != DASH_OK) {
            fclose(f);
            return rc;
        }
        const uint64_t nch = (wn + CHUNK - 1) / CHUNK;
        std::atomic<uint64_t> next{0};
        // every thread takes chunks until none is left; it touches only its chunks' preallocated
        // buffers: nothing here allocates
        run_indexed((unsigned)std::min<uint64_t>(nch, nt), [&](unsigned) {
            static const char HEX[] = "0123456789abcdef";
            for (uint64_t c; (c = next.fetch_add(1)) < nch;) {
                char* o = buf[c].get();
                auto dec = [&o](uint64_t v) {
                    char t[20];
                    int m = 0;
                    do t[m++] = (char)('0' + v % 10); while ((v /= 10) != 0);
                    while (m) *o++ = t[--m];
                };
                for (uint64_t k = c * CHUNK; k < std::min<uint64_t>(wn, (c + 1) * CHUNK); k++) {
                    dec(w0 + k);
                    *o++ = ' ';
                    for (int sh = 60; sh >= 0; sh -= 4) *o++ = HEX[(d[k] >> sh) & 15];
                    *o++ = ' ';
                    dec(r[k]);
                    *o++ = ' ';
                    int sh = 28;
                    while (sh > 0 && ((e[k] >> sh) & 15) == 0) sh -= 4;
                    for (; sh >= 0; sh -= 4) *o++ = HEX[(e[k] >> sh) & 15];
                    *o++ = '\n';
                }
                used[c] = (size_t)(o - buf[c].get());
            }
        });
        for (uint64_t c = 0; ok && c < nch; c++) ok = fwrite(buf[c].get(), 1, used[c], f) == used[c];
    }
    return (fclose(f) == 0 && ok) ? DASH_OK : fail(h, DASH_EIO, "write %s", path);
}

int dash_write_digests(dash_t* h, const char* path) {
    if (!h || !path) return DASH_EINVAL;
    try {  // no C++ exception crosses the C-ABI
        return write_digests_impl(h, path);
    } catch (const std::bad_alloc&) {
        return fail(h, DASH_ENOMEM, "dash_write_digests: out of host memory");
    } catch (...) {
        return fail(h, DASH_EIO, "dash_write_digests: unexpected failure");
    }
}

int dash_probe_box(int device, dash_box_probe* out) {
    return guarded(nullptr, "dash_probe_box", [&]() -> int {
        set_global_msg("");
        if (!out) return DASH_EINVAL;
        memset(out, 0, sizeof *out);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
            set_global_msg("dash_probe_box: no such HIP device");
            return DASH_EDEVICE;
        }
        hipDeviceProp_t p;
        if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&p, device) != hipSuccess) {
            set_global_msg("dash_probe_box: hipGetDeviceProperties failed");
            return DASH_EDEVICE;
        }
        snprintf(out->name, sizeof out->name, "%s", p.name);
        if (!out->name[0] && hipDeviceGetName(out->name, (int)sizeof out->name, device) != hipSuccess) out->name[0] = 0;
        snprintf(out->arch, sizeof out->arch, "%s", p.gcnArchName);
        out->compute_units = p.multiProcessorCount;
        out->clock_khz = p.clockRate;
        out->mem_clock_khz = p.memoryClockRate;
        out->pci_domain = p.pciDomainID;
        out->pci_bus = p.pciBusID;
        out->pci_device = p.pciDeviceID;
        out->total_mem = p.totalGlobalMem;
        const uint32_t blocks = (uint32_t)std::max(1, p.multiProcessorCount) * 8u;
        // ~170 ms at 2.4 GHz (2 wave64 VALU per cycle per CU): long enough for the clock to settle
        // (a 20-ms probe measured 1.88 GHz on a box whose sysfs clock read 2.39 GHz under load)
        const uint32_t iters = 1u << 21;
        uint32_t* sink = nullptr;
        unsigned long long* clk = nullptr;
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        int rc = DASH_OK;
        auto chk = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && rc == DASH_OK) {
                rc = DASH_EDEVICE;
                char m[256];
                snprintf(m, sizeof m, "dash_probe_box: %s: %s", what, hipGetErrorString(e));
                set_global_msg(m);
            }
        };
        chk(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "stream");
        chk(hipEventCreate(&e0), "event");
        chk(hipEventCreate(&e1), "event");
        chk(hipMalloc(&sink, 4), "hipMalloc");
        chk(hipMalloc(&clk, (size_t)blocks * 2 * sizeof(unsigned long long)), "hipMalloc");
        if (rc == DASH_OK) chk(dash::launch_probe(blocks, 1024, sink, clk, st), "warm-up launch");
        if (rc == DASH_OK) chk(hipEventRecord(e0, st), "event");
        if (rc == DASH_OK) chk(dash::launch_probe(blocks, iters, sink, clk, st), "launch");
        if (rc == DASH_OK) chk(hipEventRecord(e1, st), "event");
        std::vector<unsigned long long> c((size_t)blocks * 2);
        if (rc == DASH_OK) chk(hipMemcpyAsync(c.data(), clk, c.size() * sizeof(c[0]), hipMemcpyDeviceToHost, st), "copy");
        if (rc == DASH_OK) chk(hipStreamSynchronize(st), "sync");
        float ms = 0.f;
        if (rc == DASH_OK) chk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
        if (rc == DASH_OK) {
            double cyc = 0, ref = 0, lo = 1e30, hi = 0;
            for (uint32_t b = 0; b < blocks; b++) {
                cyc += (double)c[2 * b];
                ref += (double)c[2 * b + 1];
                if (c[2 * b + 1]) {
                    const double f = (double)c[2 * b] / (double)c[2 * b + 1] * 100.0;  // MHz
                    lo = std::min(lo, f);
                    hi = std::max(hi, f);
                }
            }
            out->probe_ms = ms;
            out->probe_valu_per_s = (double)blocks * 4.0 * iters * dash::PROBE_VALU_PER_TRIP / (ms / 1e3);
            out->probe_sclk_mhz = ref > 0 ? cyc / ref * 100.0 : 0.0;
            out->probe_sclk_min_mhz = hi > 0 ? lo : 0.0;
            out->probe_sclk_max_mhz = hi;
        }
        (void)hipFree(sink);
        (void)hipFree(clk);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (st) (void)hipStreamDestroy(st);
        return rc;
    });
}

int dash_simulate_dir(const char* dir, uint32_t num_procs, uint32_t cache_size, uint32_t max_instr,
                      const char* out_dir, int device, dash_stats* stats) {
    return guarded(nullptr, "dash_simulate_dir", [&]() -> int {
        dash_cfg cfg{};
        cfg.num_procs = num_procs;
        cfg.cache_size = cache_size;
        cfg.max_instr = max_instr;
        cfg.flags = DASH_KEEP_STATE;
        cfg.num_systems = 1;
        cfg.device = device;
        dash_t* h = nullptr;
        int rc = dash_create(&cfg, &h);
        if (rc != DASH_OK) return rc;
        rc = dash_load_dir(h, dir, 0);
        if (rc != DASH_OK) {
            set_global_msg(h->msg);
            dash_destroy(h);
            return rc;
        }
        rc = dash_run(h, stats);
        std::vector<dash_node_state> st(num_procs);
        if (rc == DASH_OK) rc = dash_read_state(h, 0, st.data());
        for (uint32_t t = 0; rc == DASH_OK && t < num_procs; t++) {
            char path[4200];
            snprintf(path, sizeof path, "%s/core_%u_output.txt", out_dir ? out_dir : ".", t);
            rc = dash_dump_file(&st[t], t, cache_size, path);
        }
        if (rc != DASH_OK) set_global_msg(h->msg);
        dash_destroy(h);
        return rc;
    });
}

// dst += src: sums, but the maxima stay maxima and err_bits is an OR
static void stats_add(dash_stats& dst, const dash_stats& src) {
    for (int k = 0; k < DASH_NUM_TXN; k++) dst.hist[k] += src.hist[k];
    dst.instructions += src.instructions;
    dst.rounds_total += src.rounds_total;
    dst.rounds_max = std::max(dst.rounds_max, src.rounds_max);
    dst.systems += src.systems;
    dst.err_systems += src.err_systems;
    dst.err_bits |= src.err_bits;
    dst.dropped += src.dropped;
    dst.max_depth = std::max(dst.max_depth, src.max_depth);
    dst.kernel_ms += src.kernel_ms;
    for (int k = 0; k < DASH_NUM_TIERS; k++) dst.tier_systems[k] += src.tier_systems[k];
    dst.wave_rounds += src.wave_rounds;
}

// ---- host-buffer throughput path: batches on two handles, copies overlapped with runs ----
int dash_run_host_batched(const dash_cfg* cfg, const uint16_t* packed, uint64_t stride,
                          const uint32_t* lens, uint64_t num_systems, uint32_t batches,
                          dash_stats* stats, uint64_t* digests, uint32_t* rounds,
                          uint32_t* errors) {
    return guarded(nullptr, "dash_run_host_batched", [&]() -> int {
        if (!cfg || !packed || !lens || !stats || batches == 0 || num_systems == 0 || num_systems % batches)
            return DASH_EINVAL;
        const uint64_t nb = num_systems / batches, N = cfg->num_procs;
        dash_cfg c = *cfg;
        c.num_systems = nb;
        // throughput path: per-system state snapshots and event logs are not returned here,
        // so the handles do not allocate them
        c.flags &= ~(uint32_t)DASH_KEEP_STATE;
        c.trace_events = 0;
        const unsigned nh = batches < 2 ? 1u : 2u;
        dash_t* h[2] = {nullptr, nullptr};
        set_global_msg("");
        int rc = DASH_OK;
        for (unsigned i = 0; i < nh && rc == DASH_OK; i++) rc = dash_create(&c, &h[i]);
        dash_stats part[2];
        memset(part, 0, sizeof part);
        int trc[2] = {DASH_OK, DASH_OK};
        std::atomic<bool> stop{false};  // the first failing lane stops the other one too
        // handle i (its own HIP stream) takes batches i, i+2, ...: while one copies, the other runs
        auto lane = [&](unsigned i) {
            for (uint64_t b = i; b < batches && !stop.load(); b += nh) {
                int r = dash_load_traces(h[i], packed + b * nb * N * stride, stride, lens + b * nb * N, nb);
                dash_stats st;
                if (r == DASH_OK) r = dash_run(h[i], &st);
                if (r == DASH_OK && (digests || rounds || errors))
                    r = dash_read_results(h[i], 0, nb, digests ? digests + b * nb : nullptr,
                                          rounds ? rounds + b * nb : nullptr, errors ? errors + b * nb : nullptr);
                if (r != DASH_OK) {
                    trc[i] = r;
                    stop.store(true);
                    break;
                }
                stats_add(part[i], st);
            }
        };
        if (rc == DASH_OK) {
            run_indexed(nh, lane);
            rc = trc[0] != DASH_OK ? trc[0] : trc[1];
            if (rc != DASH_OK) set_global_msg(h[trc[0] != DASH_OK ? 0 : 1]->msg);
        }
        for (unsigned i = 0; i < nh; i++)
            if (h[i]) dash_destroy(h[i]);
        if (rc != DASH_OK) return rc;
        *stats = part[0];
        if (nh == 2) stats_add(*stats, part[1]);
        return DASH_OK;
    });
}

}  // extern "C"
