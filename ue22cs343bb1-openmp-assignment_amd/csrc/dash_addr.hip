// dash_addr.hip -- the per-address sharing profile, reduced on the device from the event log
// (include/dash.h states the definitions).
//
// The second axis of dash_metrics.hip: the same log, bucketed by the address in bits 14:8 of every
// event word. No field depends on order, so the log is not walked one lane per node and system: one
// wave takes one system and reads its round-major rows back to back. With P = next_pow2(num_procs) a
// lane is (row within a step, node): a step is 64 / P consecutive rows, 16 B (four rounds) per lane;
// at 8 nodes that is one contiguous 1-KB read. UNROLL steps are loaded before the first is decoded.
// While UNROLL whole steps lie below the system's last full row the loop needs no row or round
// mask; the masked loop takes the rest: rows past the last one (they may hold an earlier run's
// words) are not loaded, and the rounds >= K inside the last row are dropped. Lanes t >= num_procs
// never load.
//
// Each wave owns an LDS table of ADR_FIELDS words x 128 addresses, field-major, so lanes on different
// addresses fall on different banks. An instruction event is one ds_add_u32 (reads / writes) and one
// ds_or_b32 (its node's bit); a message event is one ds_add_u32 to the one field its type counts
// in (ADR_MSGS for the types that count nowhere else; msgs is summed at the end), and an INV one
// ds_or_b32 more for the popping node's bit. Lanes on the same address serialise in the LDS.
//
// Epilogue: lane l takes addresses l and l + 64, writes each 48-B record with three 16-B stores and
// classifies it with addr_class (dash_addr.h, the host's function). The totals take one wave
// reduction per word and at most ADT_WORDS device atomics per wave.
#include "dash_addr.h"

#include "dash_device.h"

namespace dash {
namespace {

constexpr uint32_t WAVES = 4;   // systems per workgroup: 4 x 6 KB of LDS
constexpr uint32_t UNROLL = 4;  // steps (16-B loads) in flight per lane
constexpr uint32_t TAB = ADR_FIELDS * ADR_MAX_ADDRS;  // words of a wave's table

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the field a popped message counts in, 4 bits per transactionType ordinal (dash_txn): READ_REQUEST,
// WRITE_REQUEST, REPLY_RD, REPLY_WR, REPLY_ID, INV, UPGRADE, WRITEBACK_INV, WRITEBACK_INT, FLUSH,
// FLUSH_INVACK, EVICT_SHARED, EVICT_MODIFIED, and three ordinals no message has
constexpr uint64_t lut(std::initializer_list<uint32_t> slots) {
    uint64_t v = 0;
    uint32_t k = 0;
    for (uint32_t s : slots) v |= (uint64_t)s << (4u * k++);
    return v;
}
constexpr uint64_t MSG_FIELD =
    lut({ADR_READ_MISSES, ADR_WRITE_MISSES, ADR_MSGS, ADR_MSGS, ADR_MSGS, ADR_INVALIDATIONS, ADR_UPGRADES,
         ADR_INTERVENTIONS, ADR_INTERVENTIONS, ADR_FLUSHES, ADR_FLUSHES, ADR_EVICT_SHARED, ADR_EVICT_MODIFIED,
         ADR_MSGS, ADR_MSGS, ADR_MSGS});
constexpr uint32_t TYPE_INV = 5, TYPE_EVICT_SHARED = 11, TYPE_EVICT_MODIFIED = 12;

// Node t's word w of one kept round; tab = the wave's table; A = num_procs * 16. Straight-line but
// for the two LDS atomics, as dash_metrics.hip's decode: the lanes hold words of every kind at once.
__device__ __forceinline__ void decode(uint32_t w, uint32_t t, uint32_t A, uint32_t* tab, uint32_t& foreign) {
    const uint32_t ev = (w >> 24) & 1u;  // EV_EVENT; a delivery marker has it clear
    const uint32_t ins = w >> 31;        // EV_INSTR comes with EV_EVENT only
    const uint32_t addr = (w >> 8) & 0x7Fu, type = w & 15u, wr = (w >> 15) & 1u;
    const bool mine = ev != 0u && addr < A;
    foreign += ev != 0u && addr >= A ? 1u : 0u;
    uint32_t field = (uint32_t)(MSG_FIELD >> (4u * type)) & 15u;
    // an eviction counts where the home pops it; the home's forwarded EVICT_SHARED is a message only
    const bool evict = type == TYPE_EVICT_SHARED || type == TYPE_EVICT_MODIFIED;
    field = evict && (addr >> 4) != t ? (uint32_t)ADR_MSGS : field;
    field = ins ? ADR_READS + wr : field;
    uint32_t bits = type == TYPE_INV ? 0x10000u << t : 0u;  // invalidated
    bits = ins ? (1u << t) << (8u * wr) : bits;             // readers, writers
    bits = mine ? bits : 0u;
    if (mine) atomicAdd(&tab[field * ADR_MAX_ADDRS + addr], 1u);
    if (bits) atomicOr(&tab[ADR_NODES * ADR_MAX_ADDRS + addr], bits);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(WAVES * 64) void addr_kernel(AddrArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t table[WAVES][TAB];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t P = a.seg, N = a.num_procs, R = a.ev_rounds, A = N * 16u;
    const uint32_t t = lane & (P - 1u), j = lane / P, step_rows = 64u / P;
    const uint64_t sys = (uint64_t)blockIdx.x * WAVES + wave;  // the same for the whole wave
    const bool have = sys < a.nsys;
    uint32_t* tab = table[wave];
    {
        uint4* z = reinterpret_cast<uint4*>(tab);
#pragma unroll
        for (uint32_t k = 0; k < TAB / 4u / 64u; k++) z[k * 64u + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();

    const uint32_t ran = have ? a.rounds[sys] : 0u;
    const uint32_t K = ran < R ? ran : R;  // the kept rounds
    const uint32_t rows = (K + 3u) / 4u;   // <= R / 4: every row read lies inside the system's log
    const uint32_t steps = (rows + step_rows - 1u) / step_rows;
    const bool node = have && t < N;
    // this lane's 16 B of row j: rows are N x 16 B apart, a step is step_rows rows
    const u32x4* at = reinterpret_cast<const u32x4*>(a.events + (have ? sys : 0u) * N * (uint64_t)R) + (uint64_t)j * N + t;
    const uint64_t stride = (uint64_t)step_rows * N;

    // steps whose rows all hold four kept rounds, in groups of UNROLL: no row or round mask
    const uint32_t plain = K / 4u / step_rows / UNROLL * UNROLL;
    uint32_t foreign = 0u, s0 = 0u;
    for (; s0 < plain; s0 += UNROLL) {
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) {
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (node) v[i] = __builtin_nontemporal_load(at + (s0 + i) * stride);
        }
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++)
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) decode(v[i][q], t, A, tab, foreign);
    }
    for (; s0 < steps; s0 += UNROLL) {
        u32x4 v[UNROLL];
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) {
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (node && (s0 + i) * step_rows + j < rows) v[i] = __builtin_nontemporal_load(at + (s0 + i) * stride);
        }
#pragma unroll
        for (uint32_t i = 0; i < UNROLL; i++) {
            const uint32_t r = ((s0 + i) * step_rows + j) * 4u;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)  // rounds >= K of the last row are not this run's
                decode(r + q < K ? v[i][q] : 0u, t, A, tab, foreign);
        }
    }
    __syncthreads();  // every lane's updates of the table are done

    unsigned long long tot[ADT_WORDS] = {};
#pragma unroll
    for (uint32_t half = 0; half < 2; half++) {
        const uint32_t addr = half * 64u + lane;
        uint32_t f[ADR_FIELDS];
#pragma unroll
        for (uint32_t k = 0; k < ADR_FIELDS; k++) f[k] = tab[k * ADR_MAX_ADDRS + addr];
#pragma unroll
        for (uint32_t k = ADR_READ_MISSES; k < ADR_MSGS; k++) f[ADR_MSGS] += f[k];
        if (have && addr < A) {
            uint4* rec = a.records + (sys * A + addr) * 3u;
#pragma unroll
            for (uint32_t q = 0; q < 3; q++) rec[q] = make_uint4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
            // addresses >= A hold zeros (decode never touches them) and are no records
            const uint32_t c = addr_class(f[ADR_READS], f[ADR_WRITES], f[ADR_NODES]);
            const unsigned long long misses = (unsigned long long)f[ADR_READ_MISSES] + f[ADR_WRITE_MISSES] + f[ADR_UPGRADES];
#pragma unroll
            for (uint32_t k = 0; k < ADR_CLASSES; k++) {
                tot[ADT_CLASS_ADDRS + k] += c == k ? 1u : 0u;
                tot[ADT_CLASS_MISSES + k] += c == k ? misses : 0ull;
                tot[ADT_CLASS_INV + k] += c == k ? f[ADR_INVALIDATIONS] : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k <= ADR_MSGS; k++) tot[k] += f[k];
            tot[ADT_MSGS_MAX] = f[ADR_MSGS] > tot[ADT_MSGS_MAX] ? f[ADR_MSGS] : tot[ADT_MSGS_MAX];
        }
    }
    tot[ADT_FOREIGN] = foreign;
    tot[ADT_SYSTEMS] = have && lane == 0u ? 1u : 0u;
    tot[ADT_TRUNCATED] = have && lane == 0u && ran > R ? 1u : 0u;
    if (have && lane == 0u) a.truncated[sys] = ran > R ? 1 : 0;

    // totals: a wave without a system holds zeros (no loads, an untouched table)
#pragma unroll
    for (uint32_t k = 0; k < ADT_WORDS; k++) {
        if (k == ADT_MSGS_MAX) {
            const unsigned long long m = wave_max(tot[k]);
            if (lane == 0u && m) atomicMax(&a.totals[k], m);
        } else {
            const unsigned long long s = wave_sum(tot[k]);
            if (lane == 0u && s) atomicAdd(&a.totals[k], s);
        }
    }
}

}  // namespace

hipError_t launch_addr_metrics(const AddrArgs& a, hipStream_t s) {
    if (a.nsys == 0) return hipSuccess;
    const uint64_t blocks = (a.nsys + WAVES - 1) / WAVES;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(addr_kernel, dim3((uint32_t)blocks), dim3(WAVES * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace dash
