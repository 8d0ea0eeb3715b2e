// dash_outcomes.h -- the device side of dash_explore_sources (dash_outcomes.hip): the pass
// assignment, the outcome table and the launches of its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dash_delays.h"

namespace dash {

// One pass of dash_explore_assign (include/dash.h) for the kernels: S systems, G sources, K seeds per
// source from F, R = S / G seeds of every source per pass, base = pass * R < K.
struct AssignArgs {
    uint64_t S, G, K, F, R, base;
};

// One slot of the outcome table, 64 B. The key is the pair (w0, w1), compared in full:
//   w0 = digest | 1 << 63                                           (never 0: 0 = empty)
//   w1 = 1 | digest bit 63 << 1 | errors << 2 | source << 32        (never 0: 0 = not settled yet)
// (errors are the DASH_ERR_* bits, 7 of them; the field takes 30.)
struct OutcomeSlot {
    unsigned long long w0, w1;
    unsigned long long count;  // counted systems that reached the key
    unsigned long long seed;   // the lowest of their seeds (cleared to ~0)
    uint4 coh;                 // the witness's dash_coherence record
    uint32_t rounds;           // the witness's rounds
    uint32_t _pad[3];
};
static_assert(sizeof(OutcomeSlot) == 64, "one 64-B slot");

constexpr uint32_t NOT_PLACED = 0xFFFFFFFFu;  // a system's entry of the place array: no slot
constexpr uint64_t MAX_SLOTS = 1ull << 31;    // slot indices are u32, and NOT_PLACED is none of them

// the counters block (u64 words), zeroed by launch_clear_table
constexpr uint32_t OC_UNPLACED = 0;  // counted systems that found no slot
constexpr uint32_t OC_OUTCOMES = 1;  // occupied slots, counted by the compaction
constexpr uint32_t OC_WORDS = 2;

// how many distinct keys of a wave are inserted as groups (one probe and one pair of atomics per key)
// before the lanes that are left insert for themselves
constexpr uint32_t GROUP_KEYS = 4;

// One compacted entry: dash_outcome_ex of include/dash.h, as the device writes it (56 B).
struct OutcomeOut {
    unsigned long long digest, count, seed;
    uint32_t rounds, errors;
    uint32_t coh[4];
    uint32_t source, _reserved;
};

// system k >= G := a copy of system k % G (trace rows of `row` chunks and N lengths), in place
hipError_t launch_replicate(uint2* trace, uint32_t* lens, uint64_t nsys, uint64_t G, uint64_t row, uint32_t N,
                            hipStream_t s);
// the pass's seeds: seeds[k] (pairs == 0) or seeds[2 * k], seeds[2 * k + 1] = seed, weights
hipError_t launch_fill_seeds(uint64_t* seeds, const AssignArgs& a, uint32_t pairs, uint64_t weights, hipStream_t s);
// dash_explore_delays: words[k] = the delay word of system k's seed, a schedule index of `space`
// (delay_unrank, dash_delays.h); a.F == 0 and a.K == delay_count(space)
hipError_t launch_fill_delays(uint64_t* words, const AssignArgs& a, const DelaySpace& space, hipStream_t s);
hipError_t launch_clear_table(OutcomeSlot* table, uint64_t slots, unsigned long long* counters, hipStream_t s);
// every counted system of the pass into the table; place[k] = its slot or NOT_PLACED. group_keys: as
// GROUP_KEYS (0 = every lane for itself, 64 = groups only)
hipError_t launch_insert(const AssignArgs& a, const uint64_t* digests, const uint32_t* errors, OutcomeSlot* table,
                         uint64_t slots, uint32_t* place, unsigned long long* counters, uint32_t group_keys,
                         hipStream_t s);
// every placed system whose seed is its slot's: its rounds and coherence record into the slot
hipError_t launch_witness(const AssignArgs& a, const uint32_t* place, const uint32_t* rounds, const uint4* coh,
                          OutcomeSlot* table, hipStream_t s);
// occupied slots, in any order, into out[0 .. counters[OC_OUTCOMES]); at most cap are written
hipError_t launch_compact(const OutcomeSlot* table, uint64_t slots, OutcomeOut* out, uint64_t cap,
                          unsigned long long* counters, hipStream_t s);

}  // namespace dash
