// dash_ingest.hip -- core_<n>.txt text parsed on the device (gfx950), straight into the
// simulator's lane-contiguous trace layout. The rules are those of dash_parse_core_text
// (dash_text.c, its header comment): records of up to 19 bytes ending after '\n', long lines
// split at 19-byte steps from the line's start, RD %hhx / WR %hhx %hhu, first failing record
// ends the file, nothing past max_instr accepted records is looked at. The two conversions
// follow the C library's sscanf (any isspace byte is a blank, a sign before either number, a
// "0x" consumed without a digit, saturation at 17 significant hex digits), and no scan leaves
// its record: it stops at the record's '\n' even where the next record's text would continue
// the number. tests/test_gpu_text_sscanf.py holds parse_record to the library itself.
//
// One 256-thread workgroup per file walks it in tiles of DASH_TEXT_TILE bytes, 16 bytes per
// lane. Per tile:
//   1. the tile (+ a halo: a record that starts in the tile may end 18 bytes past it) goes to
//      LDS; each lane keeps a newline mask of its 16 bytes (SWAR);
//   2. an exclusive max-scan of "last line start" over lanes (wave shuffles), waves (LDS) and
//      tiles (a carry) gives every lane the line start in force at its first byte;
//   3. record starts are the bytes p with (p - line_start(p)) % 19 == 0; an exclusive sum-scan
//      with the same three levels ranks them;
//   4. start offsets are compacted into LDS by rank, so lane k parses records k, k + 256, ...
//      of the tile from LDS and stores word `rank` of the file's row (consecutive lanes,
//      consecutive 16-bit words);
//   5. the first failing record is an LDS atomic min of (rank, code).
// The tile loop ends uniformly once max_instr records are ranked or an error is known. An RD
// word is stored with value bits 0 (ref :839), so no clear pass follows. Words at or past a
// row's length are not written: the simulator never issues them.
#include "dash.h"
#include "dash_ingest.h"

namespace dash {

namespace {

constexpr uint32_t TILE = DASH_TEXT_TILE;
constexpr uint32_t THREADS = 256;
constexpr uint32_t LANE_BYTES = 16;
constexpr uint32_t HALO = 32;  // >= 18, a multiple of LANE_BYTES
constexpr uint32_t RECORD = 19;  // fgets(line, 20) (ref :831)
static_assert(TILE == THREADS * LANE_BYTES, "one 16-byte load per lane and tile");
static_assert(TILE <= 65536, "start offsets are staged as u16");

// bit k of the result = byte k of w is '\n' (exact zero-byte test of w ^ 0x0A0A0A0A; the
// multiply gathers the four per-byte flags, whose partial products never share a bit)
__device__ inline uint32_t newline_bits(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// 16 bytes of the file at position p, zero past its end; the caller's slab may be unaligned
__device__ inline uint4 load16(const uint8_t* src, uint32_t p, uint32_t L) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p >= L) return v;
    const uint8_t* q = src + p;
    if (L - p >= LANE_BYTES && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) return *reinterpret_cast<const uint4*>(q);
    uint32_t w[4] = {0, 0, 0, 0};
    const uint32_t n = L - p < LANE_BYTES ? L - p : LANE_BYTES;
    for (uint32_t j = 0; j < n; j++) w[j >> 2] |= (uint32_t)q[j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ inline int hexv(uint32_t c) {
    if (c - '0' < 10u) return (int)(c - '0');
    const uint32_t l = c | 0x20u;
    if (l - 'a' < 6u) return (int)(l - 'a' + 10);
    return -1;
}

// One record: bytes t[s .. lim) of the staged tile, where lim is the record's furthest possible
// end (19 bytes on, or the file's end), not its own: a record that ends sooner ends at its '\n',
// and the next record's bytes follow it below lim. So no scan may step over a '\n': it is no
// digit and no sign, and `blank` leaves it out (to the library it is a blank, but one that
// only the end of the line buffer can follow, where the conversion fails all the same). Past
// lim every byte reads as NUL, which no scan steps over either. Returns 0 and the packed word,
// or an INGEST_CODE_*.
__device__ inline uint32_t parse_record(const uint8_t* t, uint32_t s, uint32_t lim, uint32_t num_procs,
                                        uint32_t& word) {
    auto get = [&](uint32_t i) -> uint32_t { return i < lim ? t[i] : 0u; };
    const uint32_t c0 = get(s), c1 = get(s + 1);
    bool wr;
    if (c0 == 'R' && c1 == 'D') wr = false;
    else if (c0 == 'W' && c1 == 'R') wr = true;
    else return INGEST_CODE_PARSE;
    // isspace in the C locale without '\n': ' ' '\t' '\v' '\f' '\r'
    auto blank = [](uint32_t c) { return c == ' ' || c == '\t' || c - '\v' < 3u; };
    uint32_t p = s + 2, c;
    // %hhx: blanks, a sign, "0" with an x/X that is consumed with or without a digit after it
    // (the 0 is then the number), hex digits. The library's number is a 64-bit one that
    // saturates: more than 16 significant digits read 0xFF; otherwise the low byte of the
    // signed value, for which 32 bits of it are enough.
    while (blank(c = get(p))) p++;
    const bool aneg = c == '-';
    if (c == '+' || c == '-') c = get(++p);
    bool any = false;
    if (c == '0') {
        any = true;
        c = get(++p);
        if ((c | 0x20u) == 'x') c = get(++p);
    }
    uint32_t addr = 0, sig = 0;
    for (int d; (d = hexv(c)) >= 0; c = get(++p)) {
        addr = (addr << 4) | (uint32_t)d;
        sig += (sig | (uint32_t)d) != 0u;
        any = true;
    }
    if (!any) return INGEST_CODE_PARSE;
    addr = sig > 16u ? 0xFFu : (aneg ? 0u - addr : addr) & 0xFFu;
    uint32_t val = 0;
    if (wr) {  // %hhu: blanks, a sign, decimal digits; 15 at most fit, far from saturation
        while (blank(c = get(p))) p++;
        const bool neg = c == '-';
        if (c == '+' || c == '-') c = get(++p);
        if (c - '0' >= 10u) return INGEST_CODE_PARSE;
        do {
            val = val * 10u + (c - '0');
            c = get(++p);
        } while (c - '0' < 10u);
        val = (neg ? 0u - val : val) & 0xFFu;
    }
    if ((addr >> 4) >= num_procs) return INGEST_CODE_ADDR;
    word = (wr ? 0x8000u : 0u) | (addr << 8) | val;
    return 0;
}

__global__ __launch_bounds__(THREADS) void ingest_kernel(IngestArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[TILE + HALO];
    __shared__ uint16_t s_start[TILE];
    __shared__ uint32_t s_wls[THREADS / 64], s_wcnt[THREADS / 64];
    __shared__ uint32_t s_err;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t fl = blockIdx.x;
    if (fl >= a.num_files) return;  // uniform
    const uint64_t f = a.file_base + fl;
    const uint8_t* src = a.text + a.offsets[fl];
    const uint32_t M = a.max_instr;
    // only the first 19 * max_instr bytes can matter
    const uint64_t share = (uint64_t)RECORD * M;
    const uint32_t L = a.lengths[fl] < share ? a.lengths[fl] : (uint32_t)share;
    const uint64_t sys = f / a.num_procs;
    const uint32_t node = (uint32_t)(f % a.num_procs), spw = 64u / a.seg;
    const uint64_t row = (sys / spw) * 64u + (sys % spw) * a.seg + node;
    uint16_t* dst = a.trace + row * a.nchunks * 4u;

    if (tid == 0) s_err = 0xFFFFFFFFu;
    __syncthreads();

    uint32_t carry_ls = 0;   // start of the line the tile's first byte belongs to
    uint32_t rank_base = 0;  // records ranked before this tile (< M inside the loop)
    uint32_t err = 0xFFFFFFFFu;
    for (uint32_t tb = 0; tb < L && rank_base < M; tb += TILE) {
        const uint32_t p0 = tb + tid * LANE_BYTES;
        const uint4 v = load16(src, p0, L);
        *reinterpret_cast<uint4*>(s_text + tid * LANE_BYTES) = v;
        if (tid < HALO / LANE_BYTES)
            *reinterpret_cast<uint4*>(s_text + TILE + tid * LANE_BYTES) = load16(src, tb + TILE + tid * LANE_BYTES, L);
        // bytes past L were loaded as 0, so they are no newlines
        const uint32_t nl = newline_bits(v.x) | (newline_bits(v.y) << 4) | (newline_bits(v.z) << 8) |
                            (newline_bits(v.w) << 12);

        // line start in force at p0: max over earlier lanes of (last newline + 1), 0 = none
        uint32_t inc = nl ? p0 + (32u - (uint32_t)__clz(nl)) : 0u;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc = inc > o ? inc : o;
        }
        if (lane == 63) s_wls[wave] = inc;
        uint32_t ls = __shfl_up(inc, 1, 64);
        if (lane == 0) ls = 0;
        __syncthreads();
        ls = ls > carry_ls ? ls : carry_ls;
        uint32_t tile_ls = carry_ls;
        for (uint32_t w = 0; w < THREADS / 64; w++) {
            const uint32_t x = s_wls[w];
            if (w < wave) ls = ls > x ? ls : x;
            tile_ls = tile_ls > x ? tile_ls : x;
        }

        // record starts among this lane's bytes
        uint32_t r = (p0 - ls) % RECORD, starts = 0;
#pragma unroll
        for (uint32_t j = 0; j < LANE_BYTES; j++) {
            if (r == 0 && p0 + j < L) starts |= 1u << j;
            r = ((nl >> j) & 1u) ? 0u : (r + 1 == RECORD ? 0u : r + 1);
        }
        uint32_t cnt = (uint32_t)__popc(starts), sum = cnt;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(sum, d, 64);
            if (lane >= d) sum += o;
        }
        if (lane == 63) s_wcnt[wave] = sum;
        uint32_t k = sum - cnt;  // exclusive rank within the tile
        __syncthreads();
        uint32_t tile_cnt = 0;
        for (uint32_t w = 0; w < THREADS / 64; w++) {
            const uint32_t x = s_wcnt[w];
            if (w < wave) k += x;
            tile_cnt += x;
        }
        const uint32_t room = M - rank_base;
        const uint32_t nrec = tile_cnt < room ? tile_cnt : room;
        while (starts) {  // k < TILE: a tile holds at most TILE starts
            const uint32_t j = (uint32_t)__ffs(starts) - 1u;
            starts &= starts - 1u;
            if (k < nrec) s_start[k] = (uint16_t)(tid * LANE_BYTES + j);
            k++;
        }
        __syncthreads();

        const uint32_t left = L - tb;  // the file's bytes from the tile's start
        for (uint32_t i = tid; i < nrec; i += THREADS) {
            const uint32_t s = s_start[i];
            const uint32_t lim = s + RECORD < left ? s + RECORD : left;  // <= TILE + 18
            uint32_t word = 0;
            const uint32_t code = parse_record(s_text, s, lim, a.num_procs, word);
            if (code == 0) dst[rank_base + i] = (uint16_t)word;  // rank < M <= nchunks * 4
            else atomicMin(&s_err, ((rank_base + i) << 2) | code);
        }
        __syncthreads();
        err = s_err;
        if (err != 0xFFFFFFFFu) break;  // uniform
        rank_base += nrec;
        carry_ls = tile_ls;
    }
    if (tid == 0) {
        const uint32_t len = err != 0xFFFFFFFFu ? err >> 2 : rank_base;
        a.lens[f] = len;
        if (err != 0xFFFFFFFFu)
            atomicMin(a.fail, ((unsigned long long)f << 28) | ((unsigned long long)(err & 3u) << 26) |
                                  (unsigned long long)(len + 1u));
    }
}

}  // namespace

hipError_t launch_ingest(const IngestArgs& a, hipStream_t s) {
    // one workgroup per file; a grid holds at most 2^31 - 1 of them
    constexpr uint64_t STEP = 1ull << 30;
    for (uint64_t first = 0; first < a.num_files; first += STEP) {
        IngestArgs b = a;
        b.offsets = a.offsets + first;
        b.lengths = a.lengths + first;
        b.file_base = a.file_base + first;
        b.num_files = a.num_files - first < STEP ? a.num_files - first : STEP;
        hipLaunchKernelGGL(ingest_kernel, dim3((uint32_t)b.num_files), dim3(THREADS), 0, s, b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dash
