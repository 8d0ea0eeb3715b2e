// dash_metrics.hip -- per-node cache and coherence metrics, reduced on the device from the event
// log (include/dash.h states the definitions).
//
// One pass over the log with the mapping of its writer (sim_kernel's EVLOG block): one lane per
// node, 64 / P systems per wave, P = next_pow2(num_procs). A lane reads its own column of its
// system's round-major log, 16 B (four rounds) per row; at 8 nodes a system's row is one 128-B
// line. The wave walks its systems' rows in step up to the longest system's last row; a lane
// stops loading at its own system's last row (later rows may hold an earlier run's words) and
// drops the rounds >= rounds[sys] inside that row. UNROLL rows are loaded before the first is
// decoded, so a lane keeps UNROLL 16-B loads in flight: the kernel is meant to run at the
// memory's rate, not at its latency. While every lane of a wave still has UNROLL whole rows, the
// loop runs without those masks; the masked loop takes the rest. The decode is straight-line
// code (about 20 VALU instructions per word): the first, branchy version was bound by instruction
// issue at 31.6 % of the HBM peak.
//
// Counters of the node itself and the wait state (round of the last instruction while its span is
// open) stay in registers. The counters that belong to a message's sender go to lane seg + sender
// through a per-wave LDS table (ds_add_u32), read back once at the end. Each lane writes its
// 64-B record with four 16-B stores; the totals take one wave reduction and at most 18 device
// atomics per wave.
#include "dash_metrics.h"

#include "dash_device.h"

namespace dash {
namespace {

constexpr uint32_t WAVES = 4;   // per workgroup
constexpr uint32_t UNROLL = 4;  // rows (16-B loads) in flight per lane

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// sender-attributed counters (rows of the LDS table; decode() computes the row from the type)
enum : uint32_t { S_READ_MISS, S_WRITE_MISS, S_UPGRADE, S_EVICT_SHARED, S_EVICT_MODIFIED, S_ROWS };

// sets of transactionType ordinals (dash_txn), one bit per type
constexpr uint32_t REQUESTS = 1u << 0 | 1u << 1 | 1u << 6;                          // READ_/WRITE_REQUEST, UPGRADE
constexpr uint32_t COMPLETING = 1u << 2 | 1u << 3 | 1u << 4 | 1u << 9 | 1u << 10;  // REPLY_*, FLUSH, FLUSH_INVACK
constexpr uint32_t INTERVENTIONS = 1u << 7 | 1u << 8;                               // WRITEBACK_INV, WRITEBACK_INT
constexpr uint32_t EVICTS = 1u << 11 | 1u << 12;                                    // EVICT_SHARED, EVICT_MODIFIED

struct Node {
    uint32_t instrs = 0, writes = 0, msgs = 0, home = 0, inv = 0, intv = 0;
    uint32_t waits = 0, wait_rounds = 0, wait_max = 0, deliveries = 0;
    uint32_t issued = 0;  // round of the last instruction event + 1 while its span is open, else 0
};

// Node t's word w of round r1 - 1; tab = the wave's table at this lane's system (row stride 64).
// Straight-line code but for the LDS add: the lanes of a wave decode words of every kind at once,
// so each branch would be taken by some lane anyway.
__device__ __forceinline__ void decode(uint32_t w, uint32_t r1, uint32_t t, uint32_t num_procs, uint32_t* tab, Node& n) {
    const uint32_t ins = w >> 31;                 // EV_INSTR comes with EV_EVENT only
    const uint32_t msg = ((w >> 24) & 1u) ^ ins;  // an event that is no instruction
    const uint32_t type = w & 15u;
    const uint32_t bit = msg << type;             // the popped message's type as a one-hot set, else 0
    n.deliveries += w == EV_MICRO_SEND ? 1u : 0u;
    n.instrs += ins;
    n.writes += ins & (w >> 15);
    n.msgs += msg;
    n.home += (bit & REQUESTS) ? 1u : 0u;
    n.inv += (bit >> 5) & 1u;
    n.intv += (bit & INTERVENTIONS) ? 1u : 0u;
    // the wait span: opened by an instruction, closed by the next completing pop
    const uint32_t span = (bit & COMPLETING) && n.issued ? r1 - n.issued : 0u;  // >= 1 when one closes
    n.waits += span ? 1u : 0u;
    n.wait_rounds += span;
    n.wait_max = span > n.wait_max ? span : n.wait_max;
    n.issued = (bit & COMPLETING) ? 0u : n.issued;
    n.issued = ins ? r1 : n.issued;
    // what counts for the sender: its serviced requests, and its evictions as the home pops them
    const uint32_t sender = (w >> 4) & 7u, home = (w >> 12) & 7u;  // home = address >> 4
    const uint32_t counted = bit & (REQUESTS | (home == t ? EVICTS : 0u));
    if ((counted != 0u) & (sender < num_procs)) {
        // READ_REQUEST 0, WRITE_REQUEST 1, UPGRADE 6, EVICT_SHARED 11, EVICT_MODIFIED 12 -> rows 0..4
        const uint32_t row = type < 2u ? type : type == 6u ? 2u : type - 8u;
        atomicAdd(&tab[row * 64u + sender], 1u);
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(WAVES * 64) void metrics_kernel(MetricsArgs a) {
    __shared__ uint32_t table[WAVES][S_ROWS * 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t P = a.seg, N = a.num_procs, R = a.ev_rounds;
    const uint32_t t = lane & (P - 1u);
    const uint64_t sys = ((uint64_t)blockIdx.x * WAVES + wave) * (64u / P) + lane / P;
    const bool head = sys < a.nsys && t == 0u;  // one lane per live system
    const bool live = sys < a.nsys && t < N;
#pragma unroll
    for (uint32_t k = 0; k < S_ROWS; k++) table[wave][k * 64u + lane] = 0u;
    uint32_t* tab = &table[wave][lane - t];  // this system's columns: sender s at tab[row * 64 + s]
    __syncthreads();

    const uint32_t ran = live ? a.rounds[sys] : 0u;
    const uint32_t K = ran < R ? ran : R;  // the kept rounds
    const uint32_t rows = (K + 3u) / 4u;   // <= R / 4: every row read lies inside the system's log
    const uint32_t most = __builtin_amdgcn_readfirstlane(wave_max(rows));
    // this node's column: 16 B per row, rows N x 16 B apart
    const u32x4* col = reinterpret_cast<const u32x4*>(a.events + (live ? sys : 0u) * N * (uint64_t)R) + t;

    // while every lane of the wave has UNROLL whole rows left, loads and words need no mask
    const bool whole = __builtin_amdgcn_readfirstlane(wave_min(live ? K / 4u : 0u)) != 0u;
    const uint32_t plain = whole ? __builtin_amdgcn_readfirstlane(wave_min(K / 4u)) / UNROLL * UNROLL : 0u;
    Node n;
    uint32_t row0 = 0;
    for (; row0 < plain; row0 += UNROLL) {
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) v[i] = __builtin_nontemporal_load(col + (uint64_t)(row0 + i) * N);
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++)
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) decode(v[i][j], (row0 + i) * 4u + j + 1u, t, N, tab, n);
    }
    for (; row0 < most; row0 += UNROLL) {
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) {
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (row0 + i < rows) v[i] = __builtin_nontemporal_load(col + (uint64_t)(row0 + i) * N);
        }
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) {
            const uint32_t r = (row0 + i) * 4u;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)  // rounds >= K of the last row are not this run's
                decode(r + j < K ? v[i][j] : 0u, r + j + 1u, t, N, tab, n);
        }
    }
    __syncthreads();  // every lane's adds to the table are done

    uint32_t f[MET_FIELDS];
    f[0] = n.instrs - n.writes;
    f[1] = n.writes;
    f[2] = table[wave][S_READ_MISS * 64u + lane];
    f[3] = table[wave][S_WRITE_MISS * 64u + lane];
    f[4] = table[wave][S_UPGRADE * 64u + lane];
    f[5] = n.msgs;
    f[6] = n.home;
    f[7] = n.inv;
    f[8] = n.intv;
    f[9] = table[wave][S_EVICT_SHARED * 64u + lane];
    f[10] = table[wave][S_EVICT_MODIFIED * 64u + lane];
    f[11] = n.waits;
    f[12] = n.wait_rounds;
    f[MET_WAIT_MAX] = n.wait_max;
    f[14] = n.deliveries;
    f[15] = K - (n.instrs + n.msgs) - n.deliveries;  // a node logs at most one word per round
    if (live) {
        uint4* rec = a.records + (sys * N + t) * 4u;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) rec[q] = make_uint4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
    }
    if (head) a.truncated[sys] = ran > R ? 1 : 0;

    // totals: dead lanes hold zeros (no loads, an untouched table column, K = 0)
#pragma unroll
    for (uint32_t k = 0; k < MET_FIELDS; k++) {
        if (k == MET_WAIT_MAX) {
            const uint32_t m = wave_max(f[k]);
            if (lane == 0u && m) atomicMax(&a.totals[k], (unsigned long long)m);
        } else {
            const unsigned long long s = wave_sum(f[k]);
            if (lane == 0u && s) atomicAdd(&a.totals[k], s);
        }
    }
    const unsigned long long systems = wave_sum(head ? 1u : 0u), cut = wave_sum(head && ran > R ? 1u : 0u);
    if (lane == 0u && systems) atomicAdd(&a.totals[TOT_SYSTEMS], systems);
    if (lane == 0u && cut) atomicAdd(&a.totals[TOT_TRUNCATED], cut);
}

}  // namespace

hipError_t launch_metrics(const MetricsArgs& a, uint64_t groups, hipStream_t s) {
    if (groups == 0) return hipSuccess;
    const uint64_t blocks = (groups + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(metrics_kernel, dim3((uint32_t)blocks), dim3(WAVES * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace dash
