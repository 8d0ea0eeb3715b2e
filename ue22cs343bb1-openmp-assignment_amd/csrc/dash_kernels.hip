// dash_kernels.hip -- gfx950 kernels of the batched DASH coherence simulator.
//
// Hot path replaced: the per-node event loop of /root/reference/assignment.c
// (:149-738) with its 13-way dispatch (:190-618), sendMessage (:741-765) and
// handleCacheReplacement (:767-804).
//
// Mapping:
//   * one lane = one node, P = next_pow2(N) lanes = one system, a wave64 holds
//     64/P systems; one wave per workgroup, so all per-system state sits in the
//     workgroup's LDS ([slot][lane] arrays: every per-lane access is bank-conflict
//     free) or in lane registers;
//   * lockstep rounds: each lane pops one message or issues one instruction,
//     then all sends of the round are delivered straight into the receivers'
//     LDS rings, lowest sender first and in program order inside a sender:
//     senders OR a bit into the receiver's LDS arrival mask and take the slot
//     `tail + (arrival bits below their own)` -- no locks, no scans;
//   * queue depth is tiered: a pass with RING-deep queues halts and lists any
//     system that would overflow; the listed systems are re-simulated from
//     scratch with deeper queues, the last tier being the reference's 256
//     (MSG_BUFFER_SIZE, ref :9). The schedule is deterministic, so a system that
//     never fills its queues is identical at every depth;
//   * traces stream from HBM in a lane-contiguous layout [group][lane][chunk]
//     (4 instructions = 8 B per lane-chunk; one lane's stream is contiguous, so
//     each fetched line is consumed by the same lane over its next refills)
//     into a 2-chunk LDS window with one chunk pending in registers, refilled
//     every 4 rounds, so no global-load latency sits on a round's critical path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "dash_delays.h"
#include "dash_device.h"

namespace dash {

// transactionType ordinals (ref :30-44) + two pseudo types for an issue slot
enum : uint32_t {
    T_RR = 0, T_WRQ = 1, T_RRD = 2, T_RWR = 3, T_RID = 4, T_INV = 5, T_UPG = 6,
    T_WBINV = 7, T_WBINT = 8, T_FLUSH = 9, T_FIA = 10, T_ES = 11, T_EMOD = 12,
    T_ISSUE_R = 13, T_ISSUE_W = 14, T_IDLE = 15
};
enum : uint32_t { ST_M = 0, ST_E = 1, ST_S = 2, ST_I = 3 };  // cacheLineState (ref :17); evb needs ST_M = 0
enum : uint32_t { D_EM = 0, D_S = 1, D_U = 2 };              // directoryEntryState (ref :28)

#ifndef DASH_WCHUNK
#define DASH_WCHUNK 4
#endif
constexpr uint32_t OUTBOX = 8;  // MODE 4: held sends per node (one step: at most 7 INVs + one notice)
constexpr uint32_t WIN = 2;        // trace window chunks per lane (enough: see the refill)
constexpr uint32_t CHUNK = CHUNK_INSTR;   // instructions per 8-B HBM trace chunk (layout unit)
#ifndef DASH_WCHUNK_CS8
#define DASH_WCHUNK_CS8 2
#endif
// instructions per window refill (2: 4-B, 4: 8-B loads). CACHE_SIZE 8 refills 2 at a time: its
// cache rows make 9,212 B of LDS with 4-instruction chunks, which admits 16 waves per CU (the
// measured residency, profiles/pmc_sweep_cs8_p0.json); 2-instruction chunks take the window from
// 1,024 to 512 B, so the kernel has CACHE_SIZE 4's 8,700 B and its 18 waves
template <int CS>
constexpr uint32_t wchunk_of() { return CS == 8 ? DASH_WCHUNK_CS8 : DASH_WCHUNK; }
static_assert(DASH_WCHUNK == 2 || DASH_WCHUNK == 4, "window chunk");
static_assert(DASH_WCHUNK_CS8 == 2 || DASH_WCHUNK_CS8 == 4, "window chunk");
#ifndef DASH_QCHECK
#define DASH_QCHECK 4              // rounds between quiescence votes: one trip of the round loop (WCHUNK or 2 x WCHUNK)
#endif
#ifndef DASH_WAVES_PER_EU
#define DASH_WAVES_PER_EU 0
#endif
#ifndef DASH_LINE_FIELD
#define DASH_LINE_FIELD 1          // 0: the CACHE_SIZE 4 lockstep kernels derive the line state from the type (A/B builds)
#endif
// Code layout of the CACHE_SIZE 4 lockstep kernels' round loop (A/B builds):
#ifndef DASH_HOT_LAYOUT
#define DASH_HOT_LAYOUT 1          // 1: the cold blocks of the round and of the trip start lie behind the loop
#endif
// Ring stores of the same kernels' non-final tiers (A/B builds):
#ifndef DASH_FLAT_PLACE
#define DASH_FLAT_PLACE 1          // 1: both receivers' slots are read and ranked in every lane, the masked regions hold the store alone
#endif

// message word (ref `message`, :70-79, 20 B -> 4 B):
//   [3:0] type  [6:4] sender  [7] dirState == S (REPLY_RD)  [14:8] address
//   [15] the sender's reply-table flag (ignored)  [23:16] value | bitVector
//   [27:24] ignored  [30:28] secondReceiver  [31] zero (secondReceiver is one shift)
// The lockstep kernels of CACHE_SIZE 4 (LINE_FIELD in sim_kernel) use two of the ignored bits:
//   [25:24] the cacheLineState the receiver's line takes if the receiver's line condition holds
//   (set by the sender from its constant tables; bit 7 is not read there)
__device__ __forceinline__ uint32_t mk(uint32_t type, uint32_t sender, uint32_t addr,
                                       uint32_t val, uint32_t sr, uint32_t ds_s) {
    return type | (sender << 4) | (ds_s << 7) | (addr << 8) | (val << 16) | (sr << 28);
}

__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// The seeded schedule's round: its key is fmix64(seed ^ round * golden), a node
// t < P sits the round out when bits 8t+1..8t of fmix64(key' ^ const) are zero, and senders
// deliver in the affine order (t * A + Bc) & (P - 1) with A = (key & (P - 1)) | 1 and
// Bc = (key >> 8) & (P - 1). One word per round: bit t = node t stalls, bits 8 + 3t .. 10 + 3t =
// node t's delivery position. The oracle twins (orc_arb_stall / orc_arb_prio) compute the same.
__device__ __forceinline__ uint32_t arb_word(uint64_t seed, uint32_t round, uint32_t P) {
    const uint64_t rk = seed ^ ((uint64_t)round * 0x9E3779B97F4A7C15ull);
    const uint64_t key = fmix64(rk), skey = fmix64(rk ^ 0xD1B54A32D192ED03ull);
    const uint32_t A = ((uint32_t)key & (P - 1)) | 1u, Bc = (uint32_t)(key >> 8) & (P - 1);
    uint32_t w = 0;
    for (uint32_t t = 0; t < P; ++t)
        w |= ((((skey >> (8 * t)) & 3u) == 0 ? 1u : 0u) << t) | (((t * A + Bc) & (P - 1)) << (8 + 3 * t));
    return w;
}
// node t's part of a round word, as the kernel consumes it: 0 when t sits the round out,
// else its primary arrival bit 2 << 4 * (delivery position) (the INV bit is one below it,
// the flush copy's one above)
__device__ __forceinline__ uint32_t arb_node(uint32_t w, uint32_t t) {
    return ((w >> t) & 1u) ? 0u : 2u << (4u * ((w >> (8 + 3 * t)) & 7u));
}
// arb_node(arb_word(seed, round, P), t) for a seed that differs from lane to lane (per-system
// seeds, dash_set_system_seeds): only node t's own fields of the round word, so the two hashes run
// once per lane on the vector unit. Seed 0 is the lockstep round: t steps and delivers at position t.
__device__ __forceinline__ uint32_t arb_lane(uint64_t seed, uint32_t round, uint32_t t, uint32_t P) {
    const uint64_t rk = seed ^ ((uint64_t)round * 0x9E3779B97F4A7C15ull);
    const uint64_t key = fmix64(rk), skey = fmix64(rk ^ 0xD1B54A32D192ED03ull);
    const uint32_t A = ((uint32_t)key & (P - 1)) | 1u, Bc = (uint32_t)(key >> 8) & (P - 1);
    const bool lock = seed == 0;
    const uint32_t pos = lock ? t : (t * A + Bc) & (P - 1);
    // Both hashes run on every lane and the word is built from their bits arithmetically, behind
    // a barrier: written as `(!lock && stall) ? 0 : 2 << 4 * pos` the compiler put the hashes
    // under a branch on the seed, and at P = 1 (pos is constant) the fourth word of a trip lost
    // its non-zero value there, so every round 4k + 3 of a one-node system sat out
    // (tests/test_gpu_adequacy.py, N = 1 under per-system seeds).
    uint32_t sbits = (uint32_t)(skey >> (8 * t)) & 3u;
    asm volatile("" : "+v"(sbits));
    const uint32_t go = (lock ? 1u : 0u) | (sbits != 0 ? 1u : 0u);  // 0: the node sits the round out
    return (go + go) << (4u * pos);
}

// Node t's words of the four rounds from `round` on under a delay word that differs from lane to lane
// (dash_set_system_delays; delay_sits in dash_delays.h states the rule): 0 where a non-empty slot names
// t and covers the round, else the lockstep word, t stepping and delivering at position t. Built
// arithmetically, as arb_lane's.
__device__ __forceinline__ uint4 delay_lane(uint64_t word, uint32_t round, uint32_t t) {
    uint32_t go[4] = {1u, 1u, 1u, 1u};
#pragma unroll
    for (uint32_t s = 0; s < DELAY_SLOTS; ++s) {
        const uint32_t f = (uint32_t)(word >> (16u * s)) & 0xFFFFu;
        const uint32_t mine = (f != DELAY_EMPTY ? 1u : 0u) & ((f & 7u) == t ? 1u : 0u);
        const uint32_t off = round - (f >> 6), len = 1u << ((f >> 3) & 7u);  // unsigned: round < r wraps high
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) go[k] &= ~(mine & (off + k < len ? 1u : 0u));
    }
    return make_uint4((go[0] + go[0]) << (4u * t), (go[1] + go[1]) << (4u * t), (go[2] + go[2]) << (4u * t),
                      (go[3] + go[3]) << (4u * t));
}

// The seeded micro-step schedule's pick (include/dash.h states the rule; host twin dash_micro_pick):
// the node that acts in `round` of the system whose enabled nodes are the bits of `en` (all below
// P), by the system's seed and weight bytes; the result is no node of the system when en == 0.
// Per lane on the vector unit, as arb_lane: a wave's systems differ in seed, weights and state.
template <uint32_t P>
__device__ __forceinline__ uint32_t micro_pick_lane(uint64_t seed, uint64_t wts, uint32_t round, uint32_t en) {
    constexpr uint64_t ONES = 0x0101010101010101ull;
    // byte t = 1 when node t is enabled: en's bit t alone in byte t, then any set bit to bit 0
    const uint64_t eb = (((((uint64_t)en * ONES) & 0x8040201008040201ull) + 0x7F7F7F7F7F7F7F7Full) >> 7) & ONES;
    uint64_t mw = wts & (eb * 0xFFull);  // the enabled nodes' weights (each <= 31)
    mw = mw ? mw : eb;                   // W == 0: every enabled node counts 1
    const uint64_t cum = mw * ONES;      // byte t = the inclusive weight sum (<= 248: no carries)
    const uint32_t W = (uint32_t)(cum >> 56);
    const uint32_t u = (uint32_t)(fmix64(seed ^ ((uint64_t)round * 0x9E3779B97F4A7C15ull)) >> 32);
    const uint32_t x = __umulhi(u, W);
    // the sums never fall and the last is W > x: the lowest node whose sum exceeds x is the
    // number of sums that do not (its own weight is positive, so it is enabled)
    uint32_t pick = 0;
#pragma unroll
    for (uint32_t t = 0; t < P; ++t) pick += ((uint32_t)(cum >> (8 * t)) & 0xFFu) <= x ? 1u : 0u;
    return pick;
}

// CS = CACHE_SIZE; CS = 0 is the generic kernel for a non-power-of-two CACHE_SIZE (read at
// run time, LDS sized for the maximum of 16 lines)
template <int CS>
constexpr int cs_rows() { return CS ? CS : 16; }

template <int P, int CS, uint32_t RING>
struct Lds {  // 32-bit word offsets
    // arrival masks u32 [64] at MQM, tails (| count << 16 at the final tier) u32 [64] at MQT:
    // one word per lane in each (publishing, exchanging: one bank per lane), and the pad
    // puts a receiver's mask and tail in different banks (they are read together, by one
    // ds_read2 whose 8-bit offsets reach them from the receiver's address with no base add:
    // hence at the bottom of the LDS)
    static constexpr uint32_t MQ = 0;
    static constexpr uint32_t MQM = MQ, MQT = MQ + 65, MQS = 1;
    static constexpr uint32_t HSTRIDE = 64 / P + 1;         // padded: a system's 13 rows hit 13 banks
    static constexpr uint32_t HST = MQ + 129;               // u32 [14][64/P+1] per-system counters
    static constexpr uint32_t HROWS = 14;                   // 13 types + row 13: lanes that do not pop
    static constexpr uint32_t ENT = HST + HROWS * HSTRIDE;  // u16 [16][64]  mem | bitVector<<8   (swizzled)
    static constexpr uint32_t CAC = ENT + 16 * 64 / 2;      // u16 [CS][64]  addr | value<<8      (swizzled)
    static constexpr uint32_t RNG = CAC + cs_rows<CS>() * 64 / 2;  // u32 [RING][64] message words
    static constexpr uint32_t WND = RNG + RING * 64;        // u16 [WIN*WCHUNK][64] trace window (swizzled)
    static constexpr uint32_t WORDS = WND + WIN * wchunk_of<CS>() * 64 / 2;
};

__device__ __forceinline__ void chunk_words(uint2 v, uint32_t& x, uint32_t& y) { x = v.x; y = v.y; }
__device__ __forceinline__ void chunk_words(uint32_t v, uint32_t& x, uint32_t& y) { x = v; y = 0; }

// wave-wide lane masks: M() makes one from a per-lane condition (the compare's own SGPR
// result), B() reads a lane's bit back as the condition of a select or branch
using mask_t = uint64_t;
__device__ __forceinline__ mask_t M(bool c) { return __builtin_amdgcn_ballot_w64(c); }
__device__ __forceinline__ bool B(mask_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ uint64_t vote(bool c) { return __builtin_amdgcn_ballot_w64(c); }
// bit 7 / bit 15 of a lane value as a lane mask: one SDWA compare of the sign-extended low
// byte / half word (the selector would otherwise extract the bit first)
// 2x as an add (the compiler would turn x + x into a left shift, a slow-kind VALU)
__device__ __forceinline__ uint32_t dbl(uint32_t x) {
    uint32_t r;
    asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
    return r;
}
// index of the lowest set bit, all ones for 0 (v_ffbl_b32; the callers never use the 0 case)
__device__ __forceinline__ uint32_t ffbl(uint32_t v) {
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ mask_t Mbit7(uint32_t v) {
    mask_t r;
    asm("v_cmp_gt_i32_sdwa %0, 0, sext(%1) src0_sel:DWORD src1_sel:BYTE_0" : "=s"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ mask_t Mbit15(uint32_t v) {
    mask_t r;
    asm("v_cmp_gt_i32_sdwa %0, 0, sext(%1) src0_sel:DWORD src1_sel:WORD_0" : "=s"(r) : "v"(v));
    return r;
}
// keeps a rarely taken branch a branch (no if-conversion onto the common path)
#define COLD() asm volatile("" ::: "memory")
// a COLD() block's test: where `hot` (a constant) holds, the block is also laid out of line, so the
// common path falls through a not-taken branch; elsewhere the test is the plain one
#define RARE(hot, c) ((hot) ? __builtin_expect((c), 0) : (c))

// MODE: 0 = the fast kernel, every node steps, lowest sender first; the rarely used run
// options get instantiations of their own, so neither they nor their kernel arguments cost
// the fast one anything:
//   1 = a seeded legal schedule (a.arb_seed != 0, DESIGN.md §2 -- per round, a node sits out
//       with probability 1/4 and senders deliver in a seeded affine order; oracle twins
//       orc_arb_stall, orc_arb_prio); with a.arb_len == 0 every system follows a seed of its own,
//       hashed per lane at each trip start (dash_set_system_seeds; seed 0 = the lockstep rounds),
//       or, with a.arb_seed == ARB_SYSTEM_DELAYS, a delay word of its own (dash_set_system_delays);
//   2 = the DEBUG_MSG / DEBUG_INSTR event log (a.events) under lockstep;
//   3 = the event log under a seeded (or explicit) schedule;
//   4 = an explicit micro-step schedule with the event log (a.micro, dash_set_micro_schedule): per
//       round one node either steps, holding its sends in an LDS outbox, or delivers its oldest
//       held message -- the reference's threads interleaved at sendMessage granularity, as in
//       the oracle's STRICT model (queue depth 256 only); with a.arb_len == 0 every system follows
//       a seeded micro-step schedule of its own (dash_set_micro_seeds): each round one of its
//       enabled nodes, picked by the system's seed and weights (micro_pick_lane), acts.
// Mode 1 without the event-log code keeps its loop free of SGPR spill reloads; the schedule is a
// compile-time property of every mode (a run-time test in the event-log kernel cost it 12 %).
template <int P, int CS, uint32_t RING, int MODE>
__global__ __launch_bounds__(64)
#if DASH_WAVES_PER_EU
__attribute__((amdgpu_waves_per_eu(DASH_WAVES_PER_EU)))
#endif
void sim_kernel(const SimArgs a) {
    constexpr bool SLOW = MODE != 0;
    constexpr bool MICRO = MODE == 4;              // an explicit micro-step schedule (held sends)
    constexpr bool ARB = MODE == 1 || MODE == 3 || MICRO;  // the seeded / explicit schedule is on
    constexpr bool EVLOG = MODE >= 2;              // the DEBUG event log is on
    // The lockstep kernels of CACHE_SIZE 4 (the headline's) carry no guard for a request at an
    // EM entry with an empty bitVector: the state is unreachable (the oracle keeps
    // the check). Every other instantiation keeps the guard, byte for byte.
    constexpr bool NO_CTZ0 = MODE == 0 && CS == 4;
    // The same kernels take a line's new state from the message word (bits 25..24):
    // for every type it is a constant of the type -- REPLY_RD's by the directory state its sender
    // reads -- so the sender's constant tables carry it and the receiver keeps one condition
    // (mLine) and one select instead of four of each. Every other instantiation keeps today's word.
    constexpr bool LINE_FIELD = DASH_LINE_FIELD && MODE == 0 && CS == 4;
    constexpr uint32_t FLD = 24;  // the field's low bit
    // The same kernels keep the round loop's common path free of taken branches: every rare block
    // (OOB accounting, REPLY_ID fan-out, round cap, overflow stop) is placed behind the loop
    constexpr bool HOT = DASH_HOT_LAYOUT && MODE == 0 && CS == 4;
    // Below the final tier the same kernels read and rank the slots of both ring stores of a round in
    // every lane, so each store's exec-masked region holds one LDS write and the compiler emits it
    // without a skip branch (the delivery tail of step(); the final tier keeps place(): its
    // capacity test and cold block)
    constexpr bool FLAT = DASH_FLAT_PLACE && MODE == 0 && CS == 4 && RING != 256;
    using L = Lds<P, CS, RING>;
    constexpr uint32_t WCHUNK = wchunk_of<CS>();
    using wchunk_t = typename std::conditional<WCHUNK == 4, uint2, uint32_t>::type;
    const uint32_t ncs = CS ? (uint32_t)CS : a.cache_size;  // cache lines per node
    constexpr uint32_t SPW = 64 / P;
    constexpr uint32_t SEGMASK = (1u << P) - 1u;
    // MODE 4 adds each node's outbox: 8 entries of (message word, receiver) after the common area
    __shared__ __attribute__((aligned(16))) uint32_t lds[MICRO ? L::WORDS + OUTBOX * 128 : L::WORDS];
    uint16_t* const lds16 = reinterpret_cast<uint16_t*>(lds);

    const uint32_t lane = threadIdx.x;
    // u16 rows: lane l's half-word sits in dword (l & 31), half (l >> 5), so the 32
    // lanes of each LDS lane group always touch 32 distinct banks whatever row each
    // of them indexes
    const uint32_t sw = ((lane & 31u) << 1) | (lane >> 5);
    const uint32_t t = lane & (P - 1);  // node id (threadId in the reference)
    const uint32_t seg = lane - t;
    const uint64_t slot_id = (uint64_t)blockIdx.x * SPW + lane / P;
    const uint32_t N = a.num_procs;
    bool live;
    uint64_t sys;
    if (a.sys_list) {  // re-run of systems that overflowed a shallower tier
        live = slot_id < a.list_len && t < N;
        sys = slot_id < a.list_len ? a.sys_list[slot_id] : 0;
    } else {
        // a system the host already runs at a deeper tier (its overflow hint) sits out
        live = slot_id < a.nsys && t < N && !(a.skip && a.skip[slot_id]);
        sys = slot_id;
    }
    uint32_t len = live ? a.lens[sys * N + t] : 0u;
    // event-log kernels: this node's column of its system's round-major log (four rounds of the
    // system's N nodes per 16N-B row, this node's 16 B at column t), written one row per four rounds
    uint4* evq = nullptr;
    if (EVLOG) {
        COLD();
        evq = reinterpret_cast<uint4*>(a.events + sys * N * (uint64_t)a.event_cap) + t;
    }
    const uint32_t rcv_mask = (1u << N) - 1u;

    // initializeProcessor's state part (ref :808-820); directory/line states
    // live in two lane registers (2 bits per entry), the rest in LDS
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) lds16[L::ENT * 2 + b * 64 + sw] = (uint16_t)((20u * t + b) & 0xFFu);
#pragma unroll
    for (uint32_t i = 0; i < ncs; ++i) lds16[L::CAC * 2 + i * 64 + sw] = 0xFFu;
    for (uint32_t w = lane; w < L::HROWS * L::HSTRIDE; w += 64) lds[L::HST + w] = 0u;
    lds[L::MQM + L::MQS * lane] = 0u;
    char* const ldsb = reinterpret_cast<char*>(lds);
    constexpr uint32_t SLOT = 64 * 4;                 // bytes per ring slot (one word per lane)
    constexpr uint32_t RMASK = RING * SLOT - 1;       // RING is a power of two
    constexpr bool FINAL = RING == 256;               // the reference's capacity: exact drops
    uint32_t dsv = 0xAAAAAAAAu;  // 16 x U
    uint32_t cst = 0xFFFFFFFFu;  // CS x INVALID

    // trace window prefill: chunks 0..WIN-1 landed, chunk WIN pending in registers
    // one lane's stream is contiguous (layout unit: 8-B chunks of 4), read in WCHUNK pieces
    const wchunk_t* tr = reinterpret_cast<const wchunk_t*>(
        a.trace + ((sys / SPW) * 64 + (sys % SPW) * P + t) * a.nchunks);
    // Chunks past a node's last instruction are read too (never issued: the pc < len guard);
    // the trace buffer carries TRACE_PAD spare chunks after the last lane's stream, so no
    // refill needs a bounds test
    // instruction i of a lane lives in window row i % (WIN*WCHUNK)
    auto put_chunk = [&](uint32_t c, wchunk_t v) {
        uint16_t* const w = lds16 + L::WND * 2 + ((c % WIN) * WCHUNK) * 64 + sw;
        uint32_t x, y;
        chunk_words(v, x, y);
        w[0] = (uint16_t)x;
        w[64] = (uint16_t)(x >> 16);
        if constexpr (WCHUNK == 4) {
            w[128] = (uint16_t)y;
            w[192] = (uint16_t)(y >> 16);
        }
    };
#pragma unroll
    for (uint32_t c = 0; c < WIN; ++c)
        put_chunk(c, tr[c]);
    wchunk_t pend = tr[WIN];

    // this node's incoming queue (messageBuffer, ref :81-87): tail and count of
    // its LDS ring in ring-slot bytes (x SLOT), owned by the node; senders learn
    // them through MQ each round. Below the final depth the count is not clamped:
    // exceeding RING is the overflow that hands the system to the next depth.
    uint32_t cq = 0, tq = lane * 4u;  // tail carries this node's ring column (bits below the slot)
    // program counter and trace length pre-scaled by the window row stride (128 B) and
    // offset by this lane's byte in a row (< 128), so the window address of the next
    // instruction is one and; pc / PCU is the instruction count
    constexpr uint32_t PCU = 128;
    const uint32_t sw2 = sw * 2u;  // byte offset of this lane's u16 in a 128-B row
    uint32_t pc = sw2, last_val = 0, lenx = len * PCU + sw2;
    static_assert(WIN == 2, "window row of the pending chunk from rth");
    // refill point: the pending chunk (index rth / CB + 1) lands once pc reaches rth, in
    // window row ((rth + CB) & CB); pp points at it in HBM
    constexpr uint32_t CB = WCHUNK * PCU;
    uint32_t rth = CB + sw2;
    const wchunk_t* pp = tr + WIN;
    // waitingForReply (ref :157) of every lane as one wave mask: updated by the scalar
    // unit, read per lane through inverse_ballot (no VALU)
    uint64_t wmask = 0;
    uint32_t err = 0, maxd = 0, drops = 0;  // maxd in ring-slot bytes until the end
    uint32_t last_act = ~0u;  // last round this node was active (rounds = max over the system + 1)
    uint32_t nev = 0;         // events logged (DEBUG_MSG / DEBUG_INSTR emission, off unless a.events)
    uint32_t ev0 = 0, ev1 = 0, ev2 = 0, ev3 = 0;  // this node's log words of the current four rounds (MODE 2, 3)
    uint32_t oh = 0, on = 0;  // MODE 4: this node's outbox head and count
    auto held = [&]() -> mask_t {
        if constexpr (MICRO) return M(on != 0u);
        else return 0;
    };
    // loop-invariant uniform values a round needs, kept in VGPRs: the round's lane masks
    // need the SGPRs (spilling them costs VALU)
    // rcv_all: the nodes a REPLY_ID fan-out reaches (every node of the system but this one:
    // the reply carries the directory's whole bitVector, the requester leaves itself out)
    uint32_t cap = a.max_rounds, nlim = N * 16u, rcv_all = rcv_mask & ~(1u << t);
    asm volatile("" : "+v"(cap), "+v"(nlim), "+v"(rcv_all));
    // bitop3 masks of the row offsets (bits 10..7 of mw >> 1: block; the cache index's low bits)
    uint32_t k_ent = 0x780u, k_cac = CS ? ((uint32_t)CS - 1u) << 7 : 0u;
    asm volatile("" : "+v"(k_ent), "+v"(k_cac));

    // eviction notice (ref :767-804), sender part by the line state: EVICT_MODIFIED for M,
    // EVICT_SHARED otherwise; byte k of evb is the first message byte for line state k
    // LINE_FIELD: byte 3 (line state I: never evicted) is the notice's byte 3 instead, line state E
    // in the field -- what the home's own line takes when the home is the last sharer (ref :586)
    const uint32_t evb = LINE_FIELD ? (T_EMOD | (t << 4)) | (T_ES | (t << 4)) * 0x00010100u | ((uint32_t)ST_E << FLD)
                                    : (T_EMOD | (t << 4)) | (T_ES | (t << 4)) * 0x01010100u;
    // reply table, one entry per lane, read with ds_bpermute: entry (step type s, dir state
    // d) at lane 4s + d. Step types: the message types, 13 = no step, 14 / 15 = issue RD / WR.
    // Bits 3..0: the reply type (READ_REQUEST: ref :199-236, WRITE_REQUEST: :417-453, issue:
    // :666-734); bit 7: REPLY_RD's dirState == S; bit 15 (SENDS): the step sends that reply,
    // subject to the per-lane conditions applied after the lookup (ctz(0), hits). The flag
    // travels in bit 15 of the message word, which receivers ignore (addresses are 7 bits).
    constexpr uint32_t SENDS = 1u << 15;
    uint32_t tatab = [&] {
        const uint32_t st = lane >> 2, d = lane & 3;
        switch (st) {
        case T_RR: return SENDS | (d == D_EM ? (uint32_t)T_WBINT : (uint32_t)T_RRD | (d == D_S ? 1u << 7 : 0u));
        case T_WRQ: return SENDS | (d == D_EM ? (uint32_t)T_WBINV : (d == D_S ? (uint32_t)T_RID : (uint32_t)T_RWR));
        case T_UPG: return SENDS | (uint32_t)T_RID;
        case T_WBINV: return SENDS | (uint32_t)T_FIA;
        case T_WBINT: return SENDS | (uint32_t)T_FLUSH;
        case T_ES: return (uint32_t)T_ES;  // sent only when the entry drops to one sharer elsewhere
        case 14: return SENDS | (uint32_t)T_RR;
        case 15: return SENDS | (uint32_t)T_WRQ;  // UPGRADE on a hit (patched per lane)
        default: return 0u;
        }
    }();
    // LINE_FIELD, bits 25..24 of an entry: the line state the reply's receiver takes, XORed with what
    // the field source table below copies into those bits (there the reply word is tA ^ av16): nothing
    // for most rows; the forwards (RR / WRQ at EM) copy the request's byte 0, whose low bits are its
    // type; the flushes copy the forward's byte 3, which carries the forward's own field (S / I).
    // REPLY_RD fills EXCLUSIVE unless the entry it was read from is SHARED (ref :252).
    if constexpr (LINE_FIELD) {
        const uint32_t st = lane >> 2, d = lane & 3;
        uint32_t f = ST_M;  // REPLY_WR, REPLY_ID; the requests and UPGRADE change no line
        if (st == T_RR) f = d == D_EM ? ST_S ^ T_RR : d == D_S ? ST_S : ST_E;
        if (st == T_WRQ && d == D_EM) f = ST_I ^ T_WRQ;
        if (st == T_WBINV) f = ST_M ^ ST_I;
        if (st == T_WBINT) f = ST_S ^ ST_S;
        if (st == T_ES) f = ST_E;
        tatab |= f << FLD;
    }

    // field source table, same index as the reply table: a v_perm selector that assembles
    // bytes 1..3 of the reply (address, value field, secondReceiver; byte 0 zero). Pool bytes:
    // 0..3 = mw (0: the issued value, or the message's type | sender << 4; 1: the address;
    // 2: the message value; 3: the message's secondReceiver << 4), 4 = memory, 5 = the
    // line's value, 6 = the directory's bitVector. secondReceiver sits in bits 30..28, the
    // high nibble of byte 3, so a byte copy of a message's byte 0 names its sender
    const uint32_t vstab = [&] {
        const uint32_t st = lane >> 2, d = lane & 3;
        uint32_t src = 4u;                                           // memory (RR, ES, ...)
        if (st == T_WBINV || st == T_WBINT) src = 5u;                // written-back line value
        // sharers to invalidate (ref :438-445 sends bitVector less the requester; the requester
        // leaves itself out when it fans the INVs out, :364-373, which is the same set)
        if (st == T_UPG || (st == T_WRQ && d != D_EM)) src = 6u;
        if (st == T_WRQ && d == D_EM) src = 2u;                      // forwarded write value
        if (st == 14 || st == 15) src = 0u;                          // issued value
        // a forwarded request's reply passes its secondReceiver on (ref :281, :498); a forward
        // (RR / WRQ at EM) names the requester, the message's sender (:219, :441); no other
        // receiver reads the field
        const uint32_t sr = (st == T_WBINV || st == T_WBINT) ? 3u
                            : ((st == T_RR || st == T_WRQ) && d == D_EM) ? 0u : 0x0Cu;
        return 0x0000010Cu | (src << 16) | (sr << 24);  // byte 0: 0x0C selects zero
    }();
    // round counter: rv (a VGPR copy, so the lane masks keep the SGPRs) is the round of
    // the trip's first step; the step at position k of the trip is round rv + k
    uint32_t rv = 0;
    asm volatile("" : "+v"(rv));
    // seeded schedule: this node's words (arb_node) of this trip's four rounds, and of the next
    // trip's (in flight); the table holds them as [round / 4][node][4]
    uint4 arbw = make_uint4(0, 0, 0, 0), arbn = make_uint4(0, 0, 0, 0);
    const uint4* const arbt = reinterpret_cast<const uint4*>(a.arb_tab) + t;
    if (ARB && a.arb_len) arbn = arbt[0];
    // per-system seeds (dash_set_system_seeds): no table -- arb_len == 0, which no table-driven run
    // has, so every trip hashes its words at the trip start -- and arb_tab holds one 64-bit seed
    // per system instead, indexed by the system's real id: the same seed on every tier's pass over
    // it. With no table to prefetch, arbn is idle in this mode and carries the seed in x, y, and
    // the mode is told by a value the loop tests anyway: the table-driven runs' round loop gains
    // no register.
    if (ARB && !MICRO && a.arb_len == 0u) {
        COLD();
        const uint64_t sd = live ? reinterpret_cast<const uint64_t*>(a.arb_tab)[sys] : 0ull;
        arbn = make_uint4((uint32_t)sd, (uint32_t)(sd >> 32), 0u, 0u);
    }
    // seeded micro-step schedules (dash_set_micro_seeds): the same convention, and arb_tab holds
    // one (seed, weights) pair per system; arbn carries both
    if constexpr (MICRO) {
        if (a.arb_len == 0u) {
            COLD();
            arbn = live ? reinterpret_cast<const uint4*>(a.arb_tab)[sys] : make_uint4(0, 0, 0, 0);
        }
    }

    // Every predicate of a step is a wave-wide lane mask (an SGPR pair): one compare makes
    // it, the scalar unit combines them, v_cndmask consumes them. The kernel is bound by
    // VALU issue, so no predicate is ever materialised in a VGPR.
    // Start-of-round state: a node can pop when its queue is non-empty -- at the final
    // (reference-depth) tier a queue that reached MSG_BUFFER_SIZE has head == tail and the
    // reference's drain loop (ref :167-170) never pops it again -- and can issue when it is
    // not waitingForReply (ref :624-629) and has instructions left.
    auto can_pop = [&]() -> mask_t { return FINAL ? M(cq != 0) & M(cq != RING * SLOT) : M(cq != 0); };
    auto can_issue = [&]() -> mask_t { return M(pc < lenx) & ~wmask; };

    // one lockstep round (WCHUNK of them per trip, unrolled)
    auto step = [&](const uint32_t k, const mask_t mMsg, const mask_t mIss) __attribute__((always_inline)) {
        // A system is active while any of its nodes has a message or can issue;
        // quiescence is absorbing, so the active rounds of a system are 0..R-1.
        last_act = B(mMsg | mIss | held()) ? rv + k : last_act;
        // ---- one step: pop one message (ref :167-177) or issue one instruction (ref :632-647) ----
        mask_t mStall = 0;
        uint32_t bitI = 1u << (4 * t);
        uint32_t wp = 0;
        if (ARB) {
            // this node's word of the round: from the table, loaded a trip ahead, or hashed at
            // the trip start past the table's end; 0 = the node sits the round out, else its
            // primary arrival bit
            wp = k == 0 ? arbw.x : k == 1 ? arbw.y : k == 2 ? arbw.z : arbw.w;
            if constexpr (MICRO) {  // 1: the node steps (its sends are held), 2: it sends one held message
                if (a.arb_len == 0u) {
                    // seeded micro-step schedule: the word comes from the round's own state -- of the
                    // system's enabled nodes (held sends, a queue to pop, an instruction to issue)
                    // the picked one acts: it sends if it holds sends, else it steps
                    COLD();
                    const uint32_t en = (uint32_t)((mMsg | mIss | held()) >> seg) & SEGMASK;
                    const uint32_t pick = micro_pick_lane<P>((uint64_t)arbn.x | ((uint64_t)arbn.y << 32),
                                                             (uint64_t)arbn.z | ((uint64_t)arbn.w << 32), rv + k, en);
                    wp = (t == pick && ((en >> t) & 1u)) ? (on != 0u ? 2u : 1u) : 0u;
                }
                mStall = M(wp != 1u);
                bitI = 1u;
            } else {
                mStall = M(wp == 0u);
                bitI = wp >> 1;
            }
        }
        const mask_t mHas = mMsg & ~mStall;           // pops this round
        const mask_t mDo = mIss & ~mMsg & ~mStall;    // issues this round
        const uint32_t m = *reinterpret_cast<const uint32_t*>(ldsb + L::RNG * 4 + ((tq - cq) & RMASK));
        const uint32_t ins = *reinterpret_cast<const uint16_t*>(ldsb + L::WND * 4 + (pc & (WIN * WCHUNK * PCU - 1)));
        pc += B(mDo) ? PCU : 0u;
        if constexpr (SLOW || FINAL)
            cq -= B(mHas) ? SLOT : 0u;
        else
            cq = __builtin_elementwise_sub_sat(cq, SLOT);  // pop (cq is a multiple of SLOT)
        // message addresses are < 0x80 (a send to a node >= N is dropped), so bits
        // 14..8 give the address of a message and of an instruction alike
        const uint32_t mw = B(mHas) ? m : ins;
        uint32_t addr;  // (mw >> 8) & 0x7F as one bfe (the selector would split it into a shift and an and)
        asm("v_bfe_u32 %0, %1, 8, 7" : "=v"(addr) : "v"(mw));
        const uint32_t H = addr >> 4;  // procNodeAddr (ref :186, :657)
        // byte offsets of the row entries (block << 7 | lane byte; cacheIndex = blockIndex %
        // CACHE_SIZE, ref :188) and the 2-bit field offsets 2 * block, 2 * cacheIndex, from
        // right shifts of the word and one bitop3 each: left shifts and shift-ors are
        // slow-kind VALU (tools/micro/valu_ops)
        uint32_t eoff, coff, b2, i2;
        if constexpr (CS != 0) {
            const uint32_t x1 = mw >> 1, x7 = mw >> 7;
            asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(eoff) : "v"(x1), "v"(k_ent), "v"(sw2));
            asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(coff) : "v"(x1), "v"(k_cac), "v"(sw2));
            b2 = x7 & 0x1Eu;
            i2 = x7 & (2u * ((uint32_t)CS - 1u));
        } else {
            const uint32_t b = addr & 15u;
            const uint32_t idx = (uint32_t)(a.cs_lut >> (4 * b)) & 15u;
            eoff = (b << 7) | sw2;
            coff = (idx << 7) | sw2;
            b2 = dbl(b);
            i2 = dbl(idx);
        }
        // they stay in VGPRs from the loads to the stores
        asm volatile("" : "+v"(eoff), "+v"(coff));
        uint16_t* const ent = reinterpret_cast<uint16_t*>(ldsb + L::ENT * 4 + eoff);
        uint16_t* const cac = reinterpret_cast<uint16_t*>(ldsb + L::CAC * 4 + coff);
        const uint32_t e16 = *ent;
        const uint32_t c16 = *cac;
        const uint32_t mty = m & 15u;
        // the popped message's type, or 13 (no transactionType) for a lane that does not pop:
        // the type masks below then need no AND with mHas
        const uint32_t pty = B(mHas) ? mty : 13u;
        // the event log (ref DEBUG_MSG :179-182, DEBUG_INSTR :649-652), staged in LDS; a plain `if`
        // with the COLD() barrier, not `if constexpr`: the fast kernel's code stays byte-identical
        if (EVLOG) {
            COLD();
            // one word per node and round: 0 = no event; else bit 24 set, bit 31 the kind, the
            // message word in bits 0..23 and 28..30 (dash_read_events drops 7 and 15) or the
            // instruction in bits 0..15
            const uint32_t evx = B(mHas) ? ((m & 0x70FFFFFFu) | EV_EVENT) : B(mDo) ? (ins | EV_INSTR | EV_EVENT) : 0u;
            // (named words, not an array indexed by k % 4: the fast kernel's code stays the same)
            uint32_t evw = evx;
            if constexpr (MICRO) {
                // a seeded micro-step schedule records its deliveries too: a marker in the sender's
                // slot, an encoding no event has (bit 24 clear; not counted, dash_read_events skips
                // it), so the log holds the whole schedule (dash_read_micro_acts)
                if (a.arb_len == 0u) evw = wp == 2u ? EV_MICRO_SEND : evx;
            }
            (k % 4u == 0u ? ev0 : k % 4u == 1u ? ev1 : k % 4u == 2u ? ev2 : ev3) = evw;
            nev += B(mHas | mDo) ? 1u : 0u;
        }
        // messages handled per transactionType, per system; a lane without a message counts
        // into row 13 (pty = 13), so no exec mask is needed (more LDS bank conflicts on that
        // row, 22.6 -> 26.6 % of LDS cycles, but 1.7 % less kernel time than exec-masking)
        __hip_atomic_fetch_add(&lds[L::HST + pty * L::HSTRIDE + lane / P], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);

        // ---- 13-way dispatch (ref :190-618) + issue (ref :662-735), straight-line ----
        const mask_t mRR = M(pty == T_RR), mWRQ = M(pty == T_WRQ);
        const mask_t mRRD = M(pty == T_RRD), mRWR = M(pty == T_RWR);
        const mask_t mRID = M(pty == T_RID), mINV = M(pty == T_INV);
        const mask_t mUPG = M(pty == T_UPG), mWBINV = M(pty == T_WBINV);
        const mask_t mWBINT = M(pty == T_WBINT), mFLUSH = M(pty == T_FLUSH);
        const mask_t mFIA = M(pty == T_FIA), mES = M(pty == T_ES);
        const mask_t mEMOD = M(pty == T_EMOD);
        const uint32_t sty = B(mDo) ? (ins >> 15) | 14u : pty;  // step type: 14 / 15 = issue RD / WR
        const mask_t miR = M(sty == 14u), miW = M(sty == 15u);

        const uint32_t bv = e16 >> 8, ds = (dsv >> b2) & 3u;
        const uint32_t laddr = c16 & 0xFFu, lst = (cst >> i2) & 3u;
        // the message's value field in bits 7..0 (secondReceiver above it: every consumer
        // takes the low byte only -- a byte permute, a u16 store, an AND)
        const uint32_t msender = (m >> 4) & 7u, mv16 = mw >> 16;
        const uint32_t msr = m >> 28;  // bit 31 is zero
        const uint32_t sbit = 1u << msender;

        const mask_t mEM = M(ds == D_EM), mS = M(ds == D_S), mU = ~(mEM | mS);
        const mask_t mlI = M(lst == ST_I), mlS = M(lst == ST_S);
        const mask_t mtH = M(t == H), mtSR = M(t == msr), mSame = M(laddr == addr);
        const mask_t mHit = mSame & ~mlI;                 // ref :662-664
        const mask_t mOwnHit = miW & mHit & ~mlS;         // WR hit on M/E (:706-710)
        const uint32_t es_bv = bv & ~sbit;                // also UPGRADE/WRITE_REQUEST's sharer list
        const uint32_t es_pop = (uint32_t)__builtin_popcount(es_bv);
        const uint32_t es_own = ffbl(es_bv);  // used only when es_pop == 1
        const uint32_t own = ffbl(bv);        // the owner at EM (bv == 0 is mCtz0: dropped, unused)
        const mask_t mEsH = mES & mtH;
        const mask_t mEsOne = mEsH & M(es_pop == 1u);
        const mask_t mReq = mRR | mWRQ;
        const mask_t mEmReq = mReq & mEM;
        // ref UB (:209, :451): drop + flag. Every write that leaves an entry in EM leaves exactly
        // one bit, so NO_CTZ0 kernels have no such lane (the cold block below tests mOob alone)
        const mask_t mCtz0 = NO_CTZ0 ? 0 : mEmReq & M(bv == 0u);
        const mask_t mHomeH = (mFLUSH | mFIA) & mtH;

        // directory entry + memory (ref :222,234 :304,517 :346,456 :561 :615)
        const mask_t mToReq = (mRR & mU) | mWRQ | mUPG;
        uint32_t nbv = B(mRR & mS) ? (bv | sbit) : bv;
        nbv = B(mToReq) ? sbit : nbv;
        // computed unconditionally (kept out of a branch the compiler would otherwise form)
        uint32_t hbv = (B(mFIA) ? 0u : bv) | (1u << msr);
        asm volatile("" : "+v"(hbv));
        nbv = B(mHomeH) ? hbv : nbv;
        nbv = B(mEsH) ? es_bv : nbv;
        nbv = B(mEMOD) ? 0u : nbv;
        uint32_t nds = B(mToReq | mEsOne) ? (uint32_t)D_EM : ds;
        nds = B(mFLUSH & mtH) ? (uint32_t)D_S : nds;
        nds = B(mEMOD | (mEsH & M(es_pop == 0u))) ? (uint32_t)D_U : nds;
        // memory takes the message's value (:307 :520 :602): the entry's byte 0 comes from
        // the message word instead of the old entry
        const uint32_t ebase = B(mHomeH | mEMOD) ? mv16 : e16;

        // cache line: the new state by the value it takes (the type sets are disjoint)
        const mask_t mFill = mRRD | mRWR | mRID | ((mFLUSH | mFIA) & mtSR) | mOwnHit;
        // REPLY_WR / REPLY_ID / FLUSH_INVACK fill with the last issued value (:470,383,531),
        // a WR hit with its own (= the new last value)
        last_val = B(mDo) ? ins : last_val;  // value in bits 7..0 (the address above it: dropped below)
        const uint32_t fval = B(mRRD | mFLUSH) ? mv16 : last_val;
        const mask_t mDsS = LINE_FIELD ? 0 : Mbit7(m);     // REPLY_RD's dirState == S (bit 7)
        const mask_t mOwnHome = M(es_own == H);
        uint32_t nst;
        if constexpr (LINE_FIELD) {
            // the word names the state (a WR hit's is the instruction: bits 25..24 zero = ST_M); the
            // receiver keeps the condition under which its line changes at all: a fill, a write-back,
            // an INV of the line it holds, an EVICT_SHARED away from home or at a home that is the
            // last sharer (:470 :383 :531 :709 :252 :284 :319 :501 :396-398 :558 :586)
            const mask_t mLine = mFill | mWBINV | mWBINT | (mINV & mSame) | (mES & (~mtH | (mEsOne & mOwnHome)));
            nst = B(mLine) ? (mw >> FLD) & 3u : lst;
        } else {
            const mask_t mToI = (mINV & mSame) | mWBINV;                                   // :396-398 :501
            const mask_t mToS = mWBINT | (mRRD & mDsS) | (mFLUSH & mtSR);                  // :284 :252 :319
            const mask_t mToE = (mES & (~mtH | (mEsOne & mOwnHome))) | (mRRD & ~mDsS);     // :558 :586 :252
            const mask_t mToM = mRWR | mRID | (mFIA & mtSR) | mOwnHit;                     // :470 :383 :531 :709
            nst = B(mToM) ? (uint32_t)ST_M : lst;
            nst = B(mToE) ? (uint32_t)ST_E : nst;
            nst = B(mToS) ? (uint32_t)ST_S : nst;
            nst = B(mToI) ? (uint32_t)ST_I : nst;
        }
        // handleCacheReplacement of the refilled line (:767-804); REPLY_WR unconditional (:467)
        const mask_t mEv = mFill & ~mlI & (mRWR | ~mSame);

        // primary outgoing message: the handler's reply/forward, or else the eviction
        // notice -- no handler sends both (fills never reply), so one slot serves both
        uint32_t tA = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((sty << 4) | (ds << 2)), (int)tatab);
        // a hit needs no request (:676-677, :706-710), except a WR hit on SHARED (UPGRADE)
        const mask_t mVA = (Mbit15(tA) & ~mCtz0 & ~((miR & mHit) | mOwnHit)) | (mEsOne & ~mOwnHome);
        uint32_t dA = B(mReq | mUPG) ? msender : H;
        dA = B(mEmReq) ? own : dA;
        dA = B(mEsH) ? es_own : dA;
        // reply type (READ_REQUEST: ref :199-236, WRITE_REQUEST: :417-453, issue: :666-734);
        // REPLY_RD carries dirState == S in bit 27 (the other receivers ignore it)
        tA = B(miW & mHit) ? (uint32_t)T_UPG : tA;
        const uint32_t vsel = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((sty << 4) | (ds << 2)), (int)vstab);
        const uint32_t vpool = __builtin_amdgcn_perm(c16, e16, 0x0C010500u);  // [mem, lval, bv, 0]
        const uint32_t av16 = __builtin_amdgcn_perm(vpool, mw, vsel);  // address and value fields, in place
        uint32_t wA;  // bit 15 of the address byte: ignored
        if constexpr (LINE_FIELD) {
            // (tA ^ av16) | t << 4 in one op, where the plain word takes an or3: the same word but
            // for bits 25..24 (the table holds the difference to the copied byte) and the ignored
            // bit 15; the UPGRADE patch above drops the table's field: UPGRADE changes no line
            const uint32_t t4 = t << 4;
            asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xde" : "=v"(wA) : "v"(tA), "v"(t4), "v"(av16));
        } else {
            wA = tA | (t << 4) | av16;
        }
        const uint32_t dE = laddr >> 4;
        const mask_t mInN = M(laddr < nlim);  // home node of the evicted line exists
        // one byte permute: [evb byte lst, line address, line value, 0]
        const uint32_t wE = __builtin_amdgcn_perm(c16, evb, lst | (LINE_FIELD ? 0x03050400u : 0x0C050400u));
        const mask_t mVP = mVA | (mEv & mInN);
        const uint32_t dP = B(mVA) ? dA : dE;
        const uint32_t wP = B(mVA) ? wA : wE;
        // second copy of a flush: WRITEBACK_INV always (:498), WRITEBACK_INT if sr != home (:281)
        const mask_t mVB = mWBINV | (mWBINT & M(H != msr));

        // an issue that sends a request waits for its reply (:687, :723, :733); replies clear
        // waitingForReply, and so do FLUSH and FLUSH_INVACK at any receiver (:254,473,386,322,535)
        wmask = (mVA & mDo) | (wmask & ~(mRRD | mRWR | mRID | mFLUSH | mFIA));
        const mask_t mOob = mEv & ~mInN;  // ref UB: messageBuffers[15] -> drop + flag
        if (RARE(HOT, (mOob | mCtz0) != 0)) {  // rare: one wave-uniform test keeps it off the common path
            COLD();
            err |= (B(mOob) ? DASH_ERR_OOB_D : 0u) | (B(mCtz0) ? DASH_ERR_CTZ0_D : 0u);
            drops += (B(mOob) ? 1u : 0u) + (B(mCtz0) ? 1u : 0u);
        }

        *ent = (uint16_t)__builtin_amdgcn_perm(nbv, ebase, 0x0C0C0400u);  // [memory, sharers]
        // the select stays 32-bit (an i16 select costs more conversions)
        uint32_t cw = B(mFill) ? (addr | (fval << 8)) : c16;
        asm volatile("" : "+v"(cw));
        *cac = (uint16_t)cw;
        // field updates as xor-of-differences: three plain VALU ops each (no bitop3)
        dsv ^= (ds ^ nds) << b2;
        cst ^= (lst ^ nst) << i2;

        // ---- end-of-round delivery: lowest sender first, program order within a sender ----
        // Each node publishes its queue tail and count (after this round's pop);
        // a sender ORs bit 4*sender+k into its receiver's arrival mask, k = 0: INV,
        // 1: primary, 2: flush copy (OR commutes: no ordering between lanes). The
        // arrivals' queue order is then ascending bit order = ascending sender,
        // program order within a sender (the INVs precede the eviction notice,
        // ref :364-379): a sender's slot is the receiver's tail plus the number of
        // bits below its own, and the receiver's capacity check (ref :754-761)
        // compares the receiver's count plus that rank with the ring depth.
        // tail (with ring column); the final tier adds count << 16 for the capacity check
        lds[L::MQT + L::MQS * lane] = FINAL ? tq | (cq << 8) : tq;
        // MODE 4 (micro-step schedule, dash_set_micro_schedule): the step's sends go to this
        // node's outbox in program order -- the INVs in ascending receiver order, then the
        // reply, forward or eviction notice, then the flush copy (ref :364-379, :281, :498) --
        // and a node whose word is 2 delivers the first one; one node acts per round, so every
        // delivery is the only arrival at its receiver
        mask_t xVP = mVP, xVB = mVB, xRID = mRID;
        uint32_t xdP = dP, xwP = wP;
        if constexpr (MICRO) {
            // a node told to step while its outbox still holds sends is not a reference
            // interleaving (sendMessage completes before the thread's next pop or issue) and
            // would overrun the 8-entry outbox: flagged and stopped below
            const mask_t mBad = M(wp == 1u && on != 0u);
            auto push = [&](uint32_t w, uint32_t d) {
                const uint32_t e = L::WORDS + ((oh + on) & (OUTBOX - 1u)) * 128u + lane;
                lds[e] = w;
                lds[e + 64] = d;
                ++on;
            };
            if (B(mRID)) {
                const uint32_t winv = mk(T_INV, t, addr, 0, 0, 0);
                for (uint32_t im = mv16 & rcv_all; im != 0; im &= im - 1u) push(winv, (uint32_t)__builtin_ctz(im));
            }
            if (B(mVP)) push(wP, dP);
            if (B(mVB)) push(wA, msr);
            // a seeded schedule holds an eviction notice to a node >= N too (flagged and counted
            // above): its sendMessage call is a micro-step of the thread like any other (the
            // oracle's STRICT model drops it at its SEND), so the node stays enabled as a sender
            // and the notice is dropped by its delivery below. No handler sends both this and
            // mVP's message, and it is the step's last send. A table-driven run keeps dropping it
            // at the step: there the notice's SEND act finds the outbox empty and does nothing.
            // DASH_ERR_OOB and `drops` are raised at the step in both (the oracle raises them at
            // the SEND): the same at the end of a completed run, one act early for a system the
            // round cap stops while it still holds the notice.
            if (a.arb_len == 0u && mOob != 0) {
                COLD();
                if (B(mOob)) push(wE, dE);
            }
            if (mBad != 0) {  // the pushes above stayed in this lane's own outbox column
                COLD();
                err |= B(mBad) ? DASH_ERR_SCHEDULE_D : 0u;
                const bool kill = ((uint32_t)(mBad >> seg) & SEGMASK) != 0;
                wmask &= ~M(kill);
                if (kill) {  // the system stops: nothing held, nothing to pop or issue
                    cq = 0;
                    lenx = pc;
                    on = 0;
                }
            }
            const bool snd = wp == 2u && on != 0u;
            xdP = lds[L::WORDS + oh * 128u + 64 + lane];
            xwP = lds[L::WORDS + oh * 128u + lane];
            oh = snd ? (oh + 1u) & (OUTBOX - 1u) : oh;
            on -= snd ? 1u : 0u;
            xVP = M(snd && xdP < N);  // a held notice to a node >= N (seeded schedules) leaves and is dropped
            xVB = 0;
            xRID = 0;
        }
        uint32_t bitP = bitI << 1, bitB = bitI << 2;
        if (ARB) {
            if constexpr (MICRO) {  // the round's only arrival at its receiver
                bitP = 2u;
                bitB = 4u;
            } else {
                bitP = wp;
                bitB = dbl(wp);
            }
        }
        if (B(xVP))
            __hip_atomic_fetch_or(&lds[L::MQM + L::MQS * (seg + xdP)], bitP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (HOT ? __builtin_expect(B(xVB), 1) : B(xVB))  // HOT: stays inline (live in most wave-rounds)
            __hip_atomic_fetch_or(&lds[L::MQM + L::MQS * (seg + msr)], bitB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        auto place = [&](mask_t v, uint32_t d, uint32_t bit, uint32_t w) {
            const uint32_t rcv = L::MQS * (seg + d);
            const uint2 q = make_uint2(lds[L::MQM + rcv], lds[L::MQT + rcv]);
            const uint32_t rank = (uint32_t)__builtin_popcount(q.x & (bit - 1u));
            // slot byte offset = receiver tail + rank slots, in the receiver's ring
            // column (bits 7..2, untouched by the add); the count bits above bit 15
            // fall off the mask
            const uint32_t off = (q.y + (rank << 8)) & RMASK;
            if constexpr (FINAL) {
                const mask_t ok = v & M((q.y >> 16) + rank < RING);
                if (B(ok)) *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + off) = w;
                if ((v & ~ok) != 0) {
                    COLD();
                    err |= B(v & ~ok) ? DASH_ERR_OVERFLOW_D : 0u;
                    drops += B(v & ~ok) ? 1u : 0u;
                }
            } else {
                if (B(v)) *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + off) = w;
            }
        };
        // REPLY_ID's INV fan-out (ref :364-373), ascending receivers, behind one wave-uniform
        // test: its arrival bits, then its ring stores. The primary and flush-copy bits are
        // already set above, so these ranks see every arrival of the round; the places below
        // read the masks after the INV bits too. Two plain waterfall loops over each lane's own
        // receivers (round 5: no exec test per lane and no capacity mask per store inside them;
        // at CACHE_SIZE 16, where 45 % of wave-rounds enter this block, 3.5 % less kernel time,
        // DESIGN.md §3.2)
        if (RARE(HOT, xRID != 0)) {
            COLD();
            // a lane without a REPLY_ID has no receivers
            const uint32_t im0 = B(xRID) ? (mv16 & rcv_all) : 0u;
            for (uint32_t im = im0; im != 0; im &= im - 1u)
                __hip_atomic_fetch_or(&lds[L::MQM + L::MQS * (seg + ffbl(im))], bitI, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t winv = mk(T_INV, t, addr, 0, 0, 0) | (LINE_FIELD ? (uint32_t)ST_I << FLD : 0u);
            for (uint32_t im = im0; im != 0; im &= im - 1u) {
                const uint32_t rcv = L::MQS * (seg + ffbl(im));
                const uint2 q = make_uint2(lds[L::MQM + rcv], lds[L::MQT + rcv]);
                const uint32_t rank = (uint32_t)__builtin_popcount(q.x & (bitI - 1u));
                const uint32_t off = (q.y + (rank << 8)) & RMASK;
                if constexpr (FINAL) {
                    if ((q.y >> 16) + rank < RING) {
                        *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + off) = winv;
                    } else {
                        err |= DASH_ERR_OVERFLOW_D;
                        ++drops;
                    }
                } else {
                    *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + off) = winv;
                }
            }
        }
        if constexpr (FLAT) {
            // Both receivers' (mask, tail) pairs are read and both slots ranked before either store,
            // in every lane, and the offsets and words are pinned in VGPRs: a masked region that held
            // the read, its wait and the rank arithmetic too (the store was their only user, so the
            // compiler sank them into it) was emitted behind an s_cbranch_execz; one that holds the
            // LDS write alone is s_and_saveexec / ds_write / s_or exec, like the arrival ORs above.
            // Every arrival OR of the round, the fan-out's included, is above, so the ranks see all
            // arrivals; the stores touch RNG alone, neither the masks nor the tails, so reading the
            // second receiver before the first store changes nothing its rank sees. The two reads
            // issue back to back.
            // Lanes that send nothing read too, so the index must be in range in every lane:
            //   msr = m >> 28 <= 15 whatever the ring word holds;
            //   xdP = dP is dE = laddr >> 4 <= 15 (laddr is a byte; 15: a never-filled line) where
            //   the lane has no reply to send, else dA: msender or H (<= 7), es_own under mEsOne (one
            //   bit in es_bv) or own at an EM entry, whose bitVector holds exactly one bit (the
            //   invariant of NO_CTZ0, which the masked arrival OR above relies on already). A lane
            //   whose own / es_own is ffbl(0) -- no request at EM, an EVICT_SHARED that leaves no or
            //   several sharers -- never selects it.
            // So a lane reads words seg + d and 65 + seg + d with seg <= 63, d <= 15: inside MQ or the
            // counters behind it, never outside the workgroup's allocation.
            static_assert(L::MQT + 63 + 15 < L::WORDS, "an idle lane's slot read stays inside the LDS");
            const uint32_t rP = L::MQS * (seg + xdP), rB = L::MQS * (seg + msr);
            const uint2 qP = make_uint2(lds[L::MQM + rP], lds[L::MQT + rP]);
            const uint2 qB = make_uint2(lds[L::MQM + rB], lds[L::MQT + rB]);
            const uint32_t rankP = (uint32_t)__builtin_popcount(qP.x & (bitP - 1u));
            const uint32_t rankB = (uint32_t)__builtin_popcount(qB.x & (bitB - 1u));
            uint32_t offP = (qP.y + (rankP << 8)) & RMASK, offB = (qB.y + (rankB << 8)) & RMASK;
            uint32_t swP = xwP, swB = wA;
            asm volatile("" : "+v"(offP), "+v"(swP), "+v"(offB), "+v"(swB));
            if (B(xVP)) *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + offP) = swP;
            if (B(xVB)) *reinterpret_cast<uint32_t*>(ldsb + L::RNG * 4 + offB) = swB;
        } else {
            place(xVP, xdP, bitP, xwP);
            place(xVB, msr, bitB, wA);
        }
        const uint32_t arrived = __hip_atomic_exchange(&lds[L::MQM + L::MQS * lane], 0u, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        uint32_t n = (uint32_t)__builtin_popcount(arrived) << 8;
        if constexpr (FINAL) n = min(n, RING * SLOT - cq);  // sendMessage's drop (ref :754-761)
        // below the final tier tq is not wrapped here: every reader masks it with RMASK
        tq = FINAL ? (tq + n) & RMASK : tq + n;
        cq += n;
        if constexpr (FINAL) {
            if (cq == RING * SLOT) {  // full: stuck for good (DASH_ERR_STUCK)
                COLD();
                err |= DASH_ERR_STUCK_D;
            }
        }
        maxd = max(maxd, cq);
    };

    // the round cap is a multiple of WCHUNK (dash_create rounds it up), so it can only
    // fall on the first round of a WCHUNK block
    auto cap_check = [&](const uint32_t r0, mask_t& mMsg, mask_t& mIss) __attribute__((always_inline)) {
        if (RARE(HOT, M(r0 == cap) != 0)) {  // wave-uniform: every system still active has run `cap` rounds
            COLD();
            const bool kill = ((uint32_t)((mMsg | mIss | held()) >> seg) & SEGMASK) != 0;
            const mask_t mKill = M(kill);
            wmask &= ~mKill;
            mMsg &= ~mKill;
            mIss &= ~mKill;
            if (kill) {
                err |= DASH_ERR_ROUNDCAP_D;
                cq = 0;
                lenx = pc;
                if constexpr (MICRO) on = 0;  // held sends die with the system (the loop must end)
            }
        }
    };
    // trace window refill. Invariant here: the window holds the two chunks before the
    // pending one, and pc advances <= WCHUNK per WCHUNK rounds, so the chunks read until the
    // next refill point are always resident; the pending chunk's load has WCHUNK rounds to land.
    auto refill = [&]() __attribute__((always_inline)) {
        if (pc >= rth) {
            rth += CB;
            uint16_t* const w = reinterpret_cast<uint16_t*>(ldsb + L::WND * 4 + ((rth & CB) | sw2));
            uint32_t x, y;
            chunk_words(pend, x, y);
            w[0] = (uint16_t)x;
            w[64] = (uint16_t)(x >> 16);
            if constexpr (WCHUNK == 4) {
                w[128] = (uint16_t)y;
                w[192] = (uint16_t)(y >> 16);
            }
            pend = *++pp;
        }
    };

    // MODE 2, 3: after round k (k % 4 == 3), this node's words of rounds k - 3 .. k, one 16-B store
    // (a system's N nodes fill 16N contiguous bytes: whole lines at N = 8); rounds past the log's
    // capacity are counted (nev), not stored
    auto store_events = [&](const uint32_t r0) __attribute__((always_inline)) {
        if (live && r0 < a.event_cap) evq[(r0 / 4u) * N] = make_uint4(ev0, ev1, ev2, ev3);
    };

    // TRIP rounds per trip of WCHUNK-round blocks, unrolled; the trip's start is the
    // housekeeping point (quiescence vote, overflow stop), each block's start the round-cap
    // test and the trace window refill
    constexpr uint32_t TRIP = DASH_QCHECK;
    static_assert(TRIP == WCHUNK || TRIP == 2 * WCHUNK, "one or two refill blocks per trip");
    static_assert(!SLOW || TRIP == 4, "the seeded schedule reads four round words per trip");
    static_assert(!EVLOG || TRIP % 4 == 0, "event rows end at trip ends");
    mask_t mMsg = can_pop(), mIss = can_issue();
    // quiescence is absorbing, so testing it once per trip only adds idle rounds (no
    // state changes, not counted in `rounds`)
    while ((mMsg | mIss | held()) != 0) {
        cap_check(rv, mMsg, mIss);
        // a non-final tier stops a system soon after its first overflow: it will be
        // re-simulated from scratch at the next depth, its results here are void
        if (!FINAL) {
            const mask_t ovf = M(maxd > RING * SLOT);
            if (RARE(HOT, ovf != 0)) {
                COLD();
                const bool stop = ((uint32_t)(ovf >> seg) & SEGMASK) != 0;
                const mask_t mStop = M(stop);
                wmask &= ~mStop;
                mMsg &= ~mStop;
                mIss &= ~mStop;
                if (stop) {
                    cq = 0;
                    lenx = pc;
                }
            }
        }
        refill();
        if (ARB) {
            arbw = arbn;
            if (rv + 4 < a.arb_len) arbn = arbt[((rv + 4) >> 2) * P];
            if (rv >= a.arb_len) {  // past the table (arb_len is a multiple of 4, like rv)
                COLD();
                if constexpr (MICRO) {  // past a micro-step table every node sits out
                    arbw = make_uint4(0, 0, 0, 0);
                } else if (a.arb_len == 0u) {  // per-system seeds: a lane value, hashed on the vector unit
                    COLD();
                    const uint64_t sd = (uint64_t)arbn.x | ((uint64_t)arbn.y << 32);
                    if (a.arb_seed == ARB_SYSTEM_DELAYS)  // or a delay word per system: no hash, four slot tests
                        arbw = delay_lane(sd, rv, t);
                    else
                        arbw = make_uint4(arb_lane(sd, rv, t, P), arb_lane(sd, rv + 1, t, P),
                                          arb_lane(sd, rv + 2, t, P), arb_lane(sd, rv + 3, t, P));
                } else {
                    const uint32_t r0 = __builtin_amdgcn_readfirstlane(rv);
                    arbw = make_uint4(arb_node(arb_word(a.arb_seed, r0, P), t),
                                      arb_node(arb_word(a.arb_seed, r0 + 1, P), t),
                                      arb_node(arb_word(a.arb_seed, r0 + 2, P), t),
                                      arb_node(arb_word(a.arb_seed, r0 + 3, P), t));
                }
            }
        }
        step(0, mMsg, mIss);
#pragma unroll
        for (uint32_t k = 1; k < WCHUNK; ++k) {
            step(k, can_pop(), can_issue());
            if constexpr (EVLOG)
                if (k % 4u == 3u) store_events(rv + k - 3u);
        }
        if constexpr (TRIP == 2 * WCHUNK) {
            mMsg = can_pop();
            mIss = can_issue();
            cap_check(rv + WCHUNK, mMsg, mIss);
            refill();
            step(WCHUNK, mMsg, mIss);
#pragma unroll
            for (uint32_t k = WCHUNK + 1; k < TRIP; ++k) {
                step(k, can_pop(), can_issue());
                if constexpr (EVLOG)
                    if (k % 4u == 3u) store_events(rv + k - 3u);
            }
        }
        rv += TRIP;
        mMsg = can_pop();
        mIss = can_issue();
    }

    // ---- results ----
    if (__builtin_amdgcn_inverse_ballot_w64(wmask)) err |= DASH_ERR_DEADLOCK_D;
    uint32_t serr = err;
    uint32_t rounds = last_act + 1u;  // ~0 + 1 = 0 for a system that never ran
#pragma unroll
    for (uint32_t n = 1; n < P; n <<= 1) {
        serr |= __shfl_xor(serr, n, P);
        rounds = max(rounds, (uint32_t)__shfl_xor(rounds, n, P));
    }
    // a non-final tier hands overflowed systems to the next tier: no outputs, no statistics
    bool ovf_sys = !FINAL && maxd > RING * SLOT;
#pragma unroll
    for (uint32_t n = 1; n < P; n <<= 1) ovf_sys |= __shfl_xor((int)ovf_sys, n, P) != 0;
    const bool handoff = ovf_sys;
    const bool report = live && !handoff;

    uint32_t hcnt[13];  // this system's per-type counts (read by its node-0 lane)
#pragma unroll
    for (uint32_t k = 0; k < 13; ++k) hcnt[k] = lds[L::HST + k * L::HSTRIDE + lane / P];
    uint64_t h = 0x243F6A8885A308D3ull ^ ((uint64_t)t << 56);
    for (uint32_t b = 0; b < 16; ++b)
        h = fmix64(h ^ (uint64_t)(lds16[L::ENT * 2 + b * 64 + sw] | (((dsv >> (2 * b)) & 3u) << 16)));
    for (uint32_t i = 0; i < ncs; ++i)
        h = fmix64(h ^ ((uint64_t)(lds16[L::CAC * 2 + i * 64 + sw] | (((cst >> (2 * i)) & 3u) << 16)) |
                        (1ull << 24)));
    uint64_t dg = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (uint32_t n = 0; n < P; ++n) {
        const uint64_t hn = __shfl(h, seg + n);
        if (n < N) dg = fmix64(dg ^ hn);
    }
    if (report && t == 0) {
        a.digests[sys] = dg;
        a.rounds[sys] = rounds;
        a.errors[sys] = serr;
    }
    if (live && t == 0 && handoff) a.ovf_list[atomicAdd(a.ovf_count, 1u)] = (uint32_t)sys;
    if (a.events && report) a.event_count[sys * N + t] = nev;
    maxd >>= 8;  // ring-slot bytes -> messages
    if (a.state && report) {
        uint32_t* st = a.state + (sys * N + t) * (16 + ncs);
        for (uint32_t b = 0; b < 16; ++b)
            st[b] = lds16[L::ENT * 2 + b * 64 + sw] | (((dsv >> (2 * b)) & 3u) << 16);
        for (uint32_t i = 0; i < ncs; ++i)
            st[16 + i] = lds16[L::CAC * 2 + i * 64 + sw] | (((cst >> (2 * i)) & 3u) << 16);
    }
    if (report && t == 0 && a.keep)
        for (uint32_t k = 0; k < 13; ++k) a.hist[sys * 13 + k] = hcnt[k];

    // ---- global statistics: wave reductions, one atomic per counter per wave ----
    const bool head_lane = report && t == 0;
    unsigned long long* S = a.stats;
    auto wsum = [](uint64_t v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    };
    auto wmax = [](uint64_t v) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t u = __shfl_xor(v, o);
            v = u > v ? u : v;
        }
        return v;
    };
    for (uint32_t k = 0; k < 13; ++k) {
        const uint64_t v = wsum(head_lane ? hcnt[k] : 0u);
        if (lane == 0 && v) atomicAdd(&S[STAT_HIST + k], (unsigned long long)v);
    }
    const uint64_t s_instr = wsum(report ? pc / PCU : 0u);
    const uint64_t s_rounds = wsum(head_lane ? rounds : 0u);
    const uint64_t m_rounds = wmax(head_lane ? rounds : 0u);
    const uint64_t s_sys = wsum(head_lane ? 1u : 0u);
    const uint64_t s_errsys = wsum((head_lane && serr) ? 1u : 0u);
    const uint64_t s_drops = wsum(report ? drops : 0u);
    const uint64_t m_depth = wmax(report ? maxd : 0u);
    uint64_t ebits = report ? err : 0u;
    for (int o = 32; o > 0; o >>= 1) ebits |= __shfl_xor(ebits, o);
    if (lane == 0) {
        if (s_instr) atomicAdd(&S[STAT_INSTR], (unsigned long long)s_instr);
        if (s_rounds) atomicAdd(&S[STAT_ROUNDS], (unsigned long long)s_rounds);
        atomicMax(&S[STAT_ROUNDS_MAX], (unsigned long long)m_rounds);
        if (s_sys) atomicAdd(&S[STAT_SYSTEMS], (unsigned long long)s_sys);
        if (s_errsys) atomicAdd(&S[STAT_ERRSYS], (unsigned long long)s_errsys);
        if (ebits) atomicOr(&S[STAT_ERRBITS], (unsigned long long)ebits);
        if (s_drops) atomicAdd(&S[STAT_DROPS], (unsigned long long)s_drops);
        atomicMax(&S[STAT_MAXDEPTH], (unsigned long long)m_depth);
        atomicAdd(&S[STAT_WAVE_ROUNDS], (unsigned long long)__builtin_amdgcn_readfirstlane(rv));
    }
}

// ---- synthetic trace generator (spec: DESIGN.md §5; host twin in oracle/) ----
__global__ __launch_bounds__(256) void gen_kernel(const GenArgs g) {
    const uint64_t total = g.ngroups * g.nchunks * 64ull;
    const uint32_t P = g.seg;
    const uint64_t N = g.num_procs;
    for (uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (uint64_t)gridDim.x * blockDim.x) {
        // lane-contiguous layout [group][lane][chunk]: consecutive threads write
        // consecutive chunks of one lane's stream
        const uint32_t chunk = (uint32_t)(gid % g.nchunks);
        const uint64_t rest = gid / g.nchunks;
        const uint32_t lane = (uint32_t)(rest & 63u);
        const uint64_t group = rest >> 6;
        const uint32_t t = lane % P;
        const uint64_t sys = group * (64u / P) + lane / P;
        const bool live = sys < g.nsys && t < g.num_procs;
        uint32_t w[2] = {0, 0};
        if (live) {
            const uint64_t key =
                fmix64(g.seed ^ ((g.sys_base + sys) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull));
#pragma unroll
            for (uint32_t k = 0; k < CHUNK; ++k) {
                const uint32_t i = chunk * CHUNK + k;
                if (i >= g.len) break;
                const uint64_t r = fmix64(key ^ (((uint64_t)t << 32) | i) ^ 0x8CB92BA72F3D8DD7ull);
                uint32_t value = (uint32_t)(r & 0xFF);
                uint32_t blk = (uint32_t)((r >> 8) & 0xF);
                uint32_t is_w = (uint32_t)((r >> 12) & 1);
                const uint32_t c16 = (uint32_t)((r >> 16) & 0xFFFF);
                const uint64_t u32 = r >> 32;
                uint32_t nd = (uint32_t)((u32 * N) >> 32);
                if (g.kind == 1u) {  // contention: 90 % WR to 0x00..0x03
                    if (c16 < 58982u) {
                        is_w = 1;
                        nd = 0;
                        blk &= 3u;
                    }
                } else if (g.kind == 2u) {  // locality
                    if (c16 < g.locality || N == 1)
                        nd = t;
                    else
                        nd = (uint32_t)((t + 1 + ((u32 * (N - 1)) >> 32)) % N);
                }
                if (!is_w) value = 0;  // RD carries value 0 (ref :839)
                const uint32_t rec = (is_w << 15) | (((nd << 4) | blk) << 8) | value;
                w[k >> 1] |= rec << (16 * (k & 1));
            }
            if (chunk == 0) g.lens[sys * g.num_procs + t] = g.len;
        }
        g.trace[gid] = make_uint2(w[0], w[1]);
    }
}

template <int P, int CS, uint32_t RING>
static hipError_t launch_sim_pcr(const SimArgs& a, uint64_t groups, hipStream_t s) {
    if (a.micro) {  // micro-step schedules run at the reference's queue depth only
        if constexpr (RING == 256)
            hipLaunchKernelGGL((sim_kernel<P, CS, RING, 4>), dim3((uint32_t)groups), dim3(64), 0, s, a);
        else
            return hipErrorInvalidValue;
    } else if (a.events && a.arb_seed)
        hipLaunchKernelGGL((sim_kernel<P, CS, RING, 3>), dim3((uint32_t)groups), dim3(64), 0, s, a);
    else if (a.events)
        hipLaunchKernelGGL((sim_kernel<P, CS, RING, 2>), dim3((uint32_t)groups), dim3(64), 0, s, a);
    else if (a.arb_seed)
        hipLaunchKernelGGL((sim_kernel<P, CS, RING, 1>), dim3((uint32_t)groups), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((sim_kernel<P, CS, RING, 0>), dim3((uint32_t)groups), dim3(64), 0, s, a);
    return hipGetLastError();
}

template <int P, int CS>
static hipError_t launch_sim_pc(const SimArgs& a, uint32_t ring, uint64_t groups, hipStream_t s) {
    switch (ring) {
    case 16: return launch_sim_pcr<P, CS, 16>(a, groups, s);
    case 32: return launch_sim_pcr<P, CS, 32>(a, groups, s);
    case 256: return launch_sim_pcr<P, CS, 256>(a, groups, s);
    default: return hipErrorInvalidValue;
    }
}

template <int P>
static hipError_t launch_sim_p(const SimArgs& a, uint32_t cs, uint32_t ring, uint64_t groups, hipStream_t s) {
    switch (cs) {
    case 1: return launch_sim_pc<P, 1>(a, ring, groups, s);
    case 2: return launch_sim_pc<P, 2>(a, ring, groups, s);
    case 4: return launch_sim_pc<P, 4>(a, ring, groups, s);
    case 8: return launch_sim_pc<P, 8>(a, ring, groups, s);
    case 16: return launch_sim_pc<P, 16>(a, ring, groups, s);
    default: return cs >= 1 && cs <= 16 ? launch_sim_pc<P, 0>(a, ring, groups, s) : hipErrorInvalidValue;
    }
}

hipError_t launch_sim(const SimArgs& a, uint32_t seg, uint32_t cs, uint32_t ring, uint64_t groups,
                      hipStream_t s) {
    if (groups == 0) return hipSuccess;
    switch (seg) {
    case 1: return launch_sim_p<1>(a, cs, ring, groups, s);
    case 2: return launch_sim_p<2>(a, cs, ring, groups, s);
    case 4: return launch_sim_p<4>(a, cs, ring, groups, s);
    case 8: return launch_sim_p<8>(a, cs, ring, groups, s);
    default: return hipErrorInvalidValue;
    }
}

// [round / 4][node][round % 4]: one 16-B load per node and trip in sim_kernel
__global__ __launch_bounds__(256) void arb_table_kernel(uint64_t seed, uint32_t P, uint32_t* out, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t w = arb_word(seed, r, P);
        for (uint32_t t = 0; t < P; ++t) out[((uint64_t)(r >> 2) * P + t) * 4 + (r & 3)] = arb_node(w, t);
    }
}

hipError_t launch_arb_table(uint64_t seed, uint32_t seg, uint32_t* out, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = std::min<uint32_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(arb_table_kernel, dim3(blocks), dim3(256), 0, s, seed, seg, out, n);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void clear_rd_kernel(uint2* trace, uint64_t words) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words;
         i += (uint64_t)gridDim.x * blockDim.x) {
        uint2 v = trace[i];
        // per 16-bit half: keep bits 7..0 only when bit 15 (WR) is set
        v.x &= (((v.x >> 15) & 0x00010001u) * 0xFFu) | 0xFF00FF00u;
        v.y &= (((v.y >> 15) & 0x00010001u) * 0xFFu) | 0xFF00FF00u;
        trace[i] = v;
    }
}

hipError_t launch_clear_rd(uint2* trace, uint64_t words, hipStream_t s) {
    if (words == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((words + 255) / 256, 256ull * 64);  // grid-stride
    hipLaunchKernelGGL(clear_rd_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, trace, words);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void mark_kernel(const uint32_t* list, uint64_t n, uint8_t* skip) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        skip[list[i]] = 1;
}

hipError_t launch_mark(const uint32_t* list, uint64_t n, uint8_t* skip, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(mark_kernel, dim3(blocks), dim3(256), 0, s, list, n, skip);
    return hipGetLastError();
}

// every system becomes a copy of system `src` (dash_broadcast_system). The trace layout
// [group][lane][chunk] is [sys][P lanes][nchunks] in memory (64 = P x systems per wave), so a
// system is `row` = P * nchunks consecutive chunks; lens hold N words per system.
__global__ __launch_bounds__(256) void broadcast_kernel(uint2* trace, uint32_t* lens, uint64_t nsys, uint64_t src,
                                                        uint64_t row, uint32_t N) {
    const uint64_t total = nsys * row, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = gid; i < total; i += stride) {
        const uint64_t s = i / row;
        if (s != src) trace[i] = trace[src * row + (i - s * row)];
    }
    for (uint64_t i = gid; i < nsys * N; i += stride) {
        const uint64_t s = i / N;
        if (s != src) lens[i] = lens[src * N + (i - s * N)];
    }
}

hipError_t launch_broadcast(uint2* trace, uint32_t* lens, uint64_t nsys, uint64_t src, uint64_t row, uint32_t N,
                            hipStream_t s) {
    if (nsys == 0 || src >= nsys) return nsys == 0 ? hipSuccess : hipErrorInvalidValue;
    const uint64_t work = std::max<uint64_t>(nsys * row, nsys * N);
    const uint64_t blocks = std::min<uint64_t>((work + 255) / 256, 256ull * 64);  // grid-stride
    hipLaunchKernelGGL(broadcast_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(256), 0, s, trace, lens,
                       nsys, src, row, N);
    return hipGetLastError();
}

// ---- box probe (dash_probe_box): a fixed VALU workload and the shader clock it ran at ----
// Eight add/xor chains per lane (full-rate VOP2 ops) for `iters` trips; each workgroup's first
// lane reads the shader-clock counter (s_memtime) and the constant 100-MHz counter
// (s_memrealtime) around its loop, so cycles / reference ticks give the clock the box held.
__global__ __launch_bounds__(256) void probe_kernel(uint32_t iters, uint32_t* sink, unsigned long long* clk) {
    const uint64_t c0 = __builtin_amdgcn_s_memtime();
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
    uint32_t a = threadIdx.x, b = a ^ 0x9E37u, c = a + 7u, d = a * 3u, e = a ^ 0x55u, f = a + 0x1234u,
             g = a ^ 0xF0F0u, h = a + 99u;
    for (uint32_t i = 0; i < iters; ++i) {
        a += b; b ^= c; c += d; d ^= e; e += f; f ^= g; g += h; h ^= a;
    }
    const uint64_t c1 = __builtin_amdgcn_s_memtime();
    const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
    if ((a ^ b ^ c ^ d ^ e ^ f ^ g ^ h) == 0x9E3779B9u) sink[0] = a;  // keeps the chains live
    if (threadIdx.x == 0) {
        clk[blockIdx.x * 2] = c1 - c0;
        clk[blockIdx.x * 2 + 1] = r1 - r0;
    }
}

hipError_t launch_probe(uint32_t blocks, uint32_t iters, uint32_t* sink, unsigned long long* clk, hipStream_t s) {
    hipLaunchKernelGGL(probe_kernel, dim3(blocks), dim3(256), 0, s, iters, sink, clk);
    return hipGetLastError();
}

hipError_t launch_gen(const GenArgs& g, hipStream_t s) {
    const uint64_t total = g.ngroups * g.nchunks * 64ull;
    if (total == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 256ull * 64);  // grid-stride
    hipLaunchKernelGGL(gen_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, g);
    return hipGetLastError();
}

}  // namespace dash
