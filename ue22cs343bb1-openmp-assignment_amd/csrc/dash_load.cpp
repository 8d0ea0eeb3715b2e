// dash_load.cpp -- C-ABI of libdash over HIP: trace text into a handle. The host-side ingest
// (dash_load_dir, dash_load_dirs: parse on the CPU, then dash_load_traces) and the device-side
// one (dash_load_text, dash_load_dirs_device: the text goes up, dash_ingest.hip parses it).
#include <atomic>
#include <chrono>

#include "dash_ingest.h"
#include "dash_internal.h"
#include "dash_text.h"

// lowest := min(lowest, k), from any thread
static void atomic_min(std::atomic<uint64_t>& lowest, uint64_t k) {
    uint64_t prev = lowest.load();
    while (k < prev && !lowest.compare_exchange_weak(prev, k)) {
    }
}

extern "C" {

int dash_load_dir(dash_t* h, const char* dir, uint64_t sys) {
    return guarded(h, "dash_load_dir", [&]() -> int {
        if (!h || !dir) return DASH_EINVAL;
        if (h->cfg.num_systems != 1 || sys != 0)
            return fail(h, DASH_EINVAL, "dash_load_dir loads a batch of one system");
        char base[4096], path[4200];
        int rc = dash_resolve_dir(dir, base, sizeof base);
        const uint32_t N = h->cfg.num_procs, M = h->cfg.max_instr;
        std::vector<uint16_t> tr((size_t)N * std::max<uint32_t>(M, 1), 0);
        std::vector<uint32_t> lens(N, 0);
        for (uint32_t t = 0; t < N; t++) {
            snprintf(path, sizeof path, "%s/core_%u.txt", base, t);
            rc = dash_parse_core_file(path, N, M, tr.data() + (size_t)t * std::max<uint32_t>(M, 1), &lens[t]);
            if (rc != DASH_OK) return fail(h, rc, "%s: parse failed (%d)", path, rc);
            printf("Processor %u initialized\n", t); /* ref :850 */
        }
        return dash_load_traces(h, tr.data(), std::max<uint32_t>(M, 1), lens.data(), 1);
    });
}

int dash_load_dirs(dash_t* h, const char* const* dirs, uint64_t n) {
    return guarded(h, "dash_load_dirs", [&]() -> int {
        if (!h || (!dirs && n)) return DASH_EINVAL;
        if (n != h->cfg.num_systems) return fail(h, DASH_EINVAL, "%llu directories for %llu systems",
                                                 (unsigned long long)n, (unsigned long long)h->cfg.num_systems);
        const uint32_t N = h->cfg.num_procs, M = h->cfg.max_instr, stride = std::max<uint32_t>(M, 1);
        std::vector<uint16_t> tr((size_t)n * N * stride, 0);
        std::vector<uint32_t> lens((size_t)n * N, 0);
        std::atomic<uint64_t> next{0}, bad{~0ull};
        std::atomic<int> bad_rc{DASH_OK};
        run_indexed(host_threads(n), [&](unsigned) {  // every thread takes directories until none is left
            char base[4096], path[4200];
            for (uint64_t k; (k = next.fetch_add(1)) < n;) {
                int rc = dash_resolve_dir(dirs[k], base, sizeof base);
                for (uint32_t t = 0; rc == DASH_OK && t < N; t++) {
                    snprintf(path, sizeof path, "%s/core_%u.txt", base, t);
                    rc = dash_parse_core_file(path, N, M, tr.data() + (k * N + t) * stride, &lens[k * N + t]);
                }
                if (rc != DASH_OK) {
                    atomic_min(bad, k);
                    bad_rc = rc;
                }
            }
        });
        if (bad.load() != ~0ull)
            return fail(h, bad_rc.load(), "%s: trace directory rejected (%d)", dirs[bad.load()], bad_rc.load());
        return dash_load_traces(h, tr.data(), stride, lens.data(), n);
    });
}

// ---- device-side text ingest (dash_ingest.hip) ----

// The start of a device-side ingest. The parser writes the trace buffer in place: whatever was
// loaded is gone from here on. Then the device buffers for a launch over `files` files and
// `bytes` of text, the events, and the first-failure cell, cleared.
static int ingest_begin(dash_t* h, uint64_t bytes, uint64_t files) {
    h->ingest.report = dash_ingest_report{};
    h->loaded = false;
    HIPCHK(h, traces_changed(h, false));  // the hint goes once the new traces are on the stream
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->ingest.d_fail) HIPCHK(h, buf_alloc(h, h->ingest.d_fail, 1));
    for (stage_timer& t : h->ingest.timer) HIPCHK(h, timer_ready(h, t, 3));
    if (bytes > h->ingest.text_cap || !h->ingest.d_text) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->ingest.text_cap = 0;
        const uint64_t cap = std::max<uint64_t>(bytes, 16);
        if (buf_alloc(h, h->ingest.d_text, cap) != hipSuccess)
            return fail(h, DASH_ENOMEM, "text slab of %llu bytes: out of device memory", (unsigned long long)bytes);
        h->ingest.text_cap = cap;
    }
    if (files > h->ingest.files_cap || !h->ingest.d_foff) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->ingest.files_cap = 0;
        const uint64_t cap = std::max<uint64_t>(files, 1);
        if (buf_alloc(h, h->ingest.d_foff, cap) != hipSuccess || buf_alloc(h, h->ingest.d_flen, cap) != hipSuccess)
            return fail(h, DASH_ENOMEM, "file table of %llu entries: out of device memory", (unsigned long long)cap);
        h->ingest.files_cap = cap;
    }
    HIPCHK(h, hipMemsetAsync(h->ingest.d_fail, 0xFF, sizeof(unsigned long long), h->stream));
    return DASH_OK;
}

// slab e's events have completed: its copy and its parse, added to the report
static int ingest_times(dash_t* h, int e) {
    HIPCHK(h, h->ingest.timer[e].add(0, 1, h->ingest.report.copy_ms));
    HIPCHK(h, h->ingest.timer[e].add(1, 2, h->ingest.report.parse_ms));
    return DASH_OK;
}

static dash::IngestArgs ingest_args(dash_t* h, uint64_t file_base, uint64_t files) {
    dash::IngestArgs a{};
    a.text = h->ingest.d_text;
    a.offsets = h->ingest.d_foff;
    a.lengths = h->ingest.d_flen;
    a.file_base = file_base;
    a.num_files = files;
    a.trace = reinterpret_cast<uint16_t*>(h->d_trace);
    a.lens = h->d_lens;
    a.nchunks = h->nchunks;  // max_instr <= nchunks * 4 (dash_create)
    a.seg = h->seg;
    a.num_procs = h->cfg.num_procs;
    a.max_instr = h->cfg.max_instr;
    a.fail = h->ingest.d_fail;
    return a;
}

// The outcome of an ingest: the kernel's first-failure cell against the reader's first
// unreadable file (eio_file, ~0 = none); the lowest file index wins. dirs: the directory
// list (dash_load_dirs_device) or nullptr (dash_load_text).
static int ingest_finish(dash_t* h, const char* what, unsigned long long cell, uint64_t eio_file,
                         const char* const* dirs) {
    const uint32_t N = h->cfg.num_procs;
    dash_ingest_report& r = h->ingest.report;
    r.rc = DASH_OK;
    r.record = 0;
    r.file = 0;
    if (cell != dash::INGEST_NO_FAILURE && (cell >> 28) < eio_file) {
        r.file = cell >> 28;
        r.record = (uint32_t)(cell & ((1u << 26) - 1u));
        r.rc = ((cell >> 26) & 3u) == dash::INGEST_CODE_ADDR ? DASH_EADDR : DASH_EPARSE;
    } else if (eio_file != ~0ull) {
        r.file = eio_file;
        r.rc = DASH_EIO;
    }
    if (r.rc == DASH_OK) {
        h->loaded = true;
        return DASH_OK;
    }
    const unsigned long long sys = r.file / N;
    const unsigned node = (unsigned)(r.file % N);
    char where[160];
    if (dirs) snprintf(where, sizeof where, "%.120s (system %llu)", dirs[sys], sys);
    else snprintf(where, sizeof where, "system %llu", sys);
    if (r.rc == DASH_EIO)
        return fail(h, r.rc, "%s: %s: node %u: core_%u.txt missing or unreadable (%d)", what, where, node, node, r.rc);
    return fail(h, r.rc, "%s: %s: node %u: record %u %s (%d)", what, where, node, r.record,
                r.rc == DASH_EADDR ? "names an address homed on a node >= num_procs" : "is no RD / WR record", r.rc);
}

int dash_load_text(dash_t* h, const char* text, const uint64_t* offsets, const uint32_t* lengths,
                   uint64_t num_files) {
    return guarded(h, "dash_load_text", [&]() -> int {
        if (!h || ((!offsets || !lengths) && num_files)) return DASH_EINVAL;
        if (num_files != h->cfg.num_systems * h->cfg.num_procs)
            return fail(h, DASH_EINVAL, "dash_load_text: %llu files for %llu systems of %u nodes",
                        (unsigned long long)num_files, (unsigned long long)h->cfg.num_systems, h->cfg.num_procs);
        uint64_t bytes = 0;
        for (uint64_t f = 0; f < num_files; f++) {
            if (offsets[f] + lengths[f] < offsets[f]) return fail(h, DASH_EINVAL, "dash_load_text: file %llu wraps", (unsigned long long)f);
            bytes = std::max<uint64_t>(bytes, offsets[f] + lengths[f]);
        }
        if (!text && bytes) return DASH_EINVAL;
        int rc = ingest_begin(h, bytes, num_files);
        if (rc != DASH_OK) return rc;
        unsigned long long cell = dash::INGEST_NO_FAILURE;
        const stage_timer& timer = h->ingest.timer[0];
        HIPCHK(h, timer.mark(0, h->stream));
        if (bytes) HIPCHK(h, hipMemcpyAsync(h->ingest.d_text, text, bytes, hipMemcpyHostToDevice, h->stream));
        if (num_files) {
            HIPCHK(h, hipMemcpyAsync(h->ingest.d_foff, offsets, num_files * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(h->ingest.d_flen, lengths, num_files * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        }
        HIPCHK(h, timer.mark(1, h->stream));
        HIPCHK(h, dash::launch_ingest(ingest_args(h, 0, num_files), h->stream));
        HIPCHK(h, timer.mark(2, h->stream));
        HIPCHK(h, traces_changed(h));
        HIPCHK(h, hipMemcpyAsync(&cell, h->ingest.d_fail, sizeof cell, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((rc = ingest_times(h, 0)) != DASH_OK) return rc;
        h->ingest.report.text_bytes = bytes;
        return ingest_finish(h, "dash_load_text", cell, ~0ull, nullptr);
    });
}

int dash_load_dirs_device(dash_t* h, const char* const* dirs, uint64_t n) {
    return guarded(h, "dash_load_dirs_device", [&]() -> int {
        if (!h || (!dirs && n)) return DASH_EINVAL;
        if (n != h->cfg.num_systems) return fail(h, DASH_EINVAL, "%llu directories for %llu systems",
                                                 (unsigned long long)n, (unsigned long long)h->cfg.num_systems);
        const uint32_t N = h->cfg.num_procs;
        const uint64_t limit = dash_text_limit(h->cfg.max_instr);  // a file's share, < 2^32
        const uint64_t slot = std::max<uint64_t>((limit + 15) & ~15ull, 16);  // and its room in a slab
        // a slab: whole systems, about 64 MiB of room (every file has room for its full share, so
        // the readers need no sizes in advance; only the bytes read are copied)
        const uint64_t per_slab = std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(n, 1), (64ull << 20) / (slot * N)));
        const uint64_t slab_files = per_slab * N, slab_cap = slab_files * slot;
        int rc = ingest_begin(h, slab_cap, slab_files);
        if (rc != DASH_OK) return rc;
        if (h->ingest.pin_cap < slab_cap || h->ingest.pin_files_cap < slab_files) {
            h->ingest.pin_cap = h->ingest.pin_files_cap = 0;
            for (int i = 0; i < 2; i++) {  // both old slabs go before a new one comes
                buf_free(h, h->ingest.pin[i]);
                buf_free(h, h->ingest.pin_off[i]);
                buf_free(h, h->ingest.pin_len[i]);
            }
            for (int i = 0; i < 2; i++)
                if (buf_alloc(h, h->ingest.pin[i], slab_cap, true) != hipSuccess ||
                    buf_alloc(h, h->ingest.pin_off[i], slab_files, true) != hipSuccess ||
                    buf_alloc(h, h->ingest.pin_len[i], slab_files, true) != hipSuccess)
                    return fail(h, DASH_ENOMEM, "dash_load_dirs_device: two pinned slabs of %llu bytes: out of memory",
                                (unsigned long long)slab_cap);
            h->ingest.pin_cap = slab_cap;
            h->ingest.pin_files_cap = slab_files;
        }
        const unsigned max_threads = host_threads(std::max<uint64_t>(n, 1));
        std::atomic<uint64_t> eio{~0ull};  // lowest file the readers could not open
        unsigned long long cell = dash::INGEST_NO_FAILURE;
        bool pending[2] = {false, false};
        auto drain = [&](int e) -> int {  // slab e's copy and parse are done: its pinned slab is free
            if (!pending[e]) return DASH_OK;
            HIPCHK(h, hipEventSynchronize(h->ingest.timer[e].ev[2]));
            pending[e] = false;
            return ingest_times(h, e);
        };
        for (uint64_t s0 = 0, i = 0; s0 < n && eio.load() == ~0ull; s0 += per_slab, i++) {
            const int e = (int)(i & 1);
            if ((rc = drain(e)) != DASH_OK) return rc;
            const uint64_t cnt = std::min(per_slab, n - s0);
            const unsigned nt = (unsigned)std::min<uint64_t>(max_threads, cnt);
            char* slab = h->ingest.pin[e];
            uint64_t* off = h->ingest.pin_off[e];
            uint32_t* len = h->ingest.pin_len[e];
            std::vector<uint64_t> used(nt, 0);
            // reader j: systems [s0 + cnt * j / nt, s0 + cnt * (j + 1) / nt), back to back from
            // its region's start, each file on a 16-byte boundary (dash_read_dirs_text's layout)
            auto reader = [&](unsigned j) {
                const uint64_t a = cnt * j / nt, b = cnt * (j + 1) / nt;
                const uint64_t region = a * N * slot;
                for (uint64_t f = a * N; f < b * N; f++) {
                    off[f] = region;
                    len[f] = 0;  // a file not reached parses as empty
                }
                uint64_t pos = region, end = region;
                char base[4096], path[4200];
                int r = DASH_OK;
                for (uint64_t k = a; k < b && r == DASH_OK; k++) {
                    uint32_t t = 0;  // an unresolved directory fails at its node 0
                    r = dash_resolve_dir(dirs[s0 + k], base, sizeof base);
                    for (; r == DASH_OK && t < N; t++) {
                        pos = (end + 15) & ~15ull;
                        uint64_t got = 0;
                        snprintf(path, sizeof path, "%s/core_%u.txt", base, t);
                        // room: the region holds a full share for every file of its systems
                        if ((r = dashi_read_text_file(path, limit, slab + pos, limit, &got)) != DASH_OK) break;
                        off[k * N + t] = pos;
                        len[k * N + t] = (uint32_t)got;
                        end = pos + got;
                    }
                    if (r != DASH_OK) atomic_min(eio, (s0 + k) * N + t);
                }
                used[j] = end - region;
            };
            const auto t0 = std::chrono::steady_clock::now();
            run_indexed(nt, reader);
            h->ingest.report.read_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            HIPCHK(h, h->ingest.timer[e].mark(0, h->stream));
            for (unsigned j = 0; j < nt; j++) {
                const uint64_t region = (cnt * j / nt) * N * slot;
                if (used[j])
                    HIPCHK(h, hipMemcpyAsync(h->ingest.d_text + region, slab + region, used[j], hipMemcpyHostToDevice, h->stream));
                h->ingest.report.text_bytes += used[j];
            }
            HIPCHK(h, hipMemcpyAsync(h->ingest.d_foff, off, cnt * N * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(h->ingest.d_flen, len, cnt * N * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, h->ingest.timer[e].mark(1, h->stream));
            HIPCHK(h, dash::launch_ingest(ingest_args(h, s0 * N, cnt * N), h->stream));
            HIPCHK(h, h->ingest.timer[e].mark(2, h->stream));
            pending[e] = true;
        }
        HIPCHK(h, traces_changed(h));
        HIPCHK(h, hipMemcpyAsync(&cell, h->ingest.d_fail, sizeof cell, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((rc = drain(0)) != DASH_OK || (rc = drain(1)) != DASH_OK) return rc;
        return ingest_finish(h, "dash_load_dirs_device", cell, eio.load(), dirs);
    });
}

int dash_ingest_info(const dash_t* h, dash_ingest_report* out) {
    if (!h || !out) return DASH_EINVAL;
    *out = h->ingest.report;
    return DASH_OK;
}

}  // extern "C"
