/*
 * dash.h -- C-ABI of libdash, the MI355X batched DASH directory-coherence
 * simulator (drop-in for the hot path of vibhav950/UE22CS343BB1-OpenMP-Assignment).
 *
 * The reference (assignment.c) simulates ONE system of NUM_PROCS nodes with
 * one OpenMP thread per node. libdash simulates up to millions of independent
 * systems per GPU under the deterministic lockstep schedule,
 * one wave64 lane per node. Plain pointers and sizes only; no torch types.
 *
 * Reference interfaces each entry point replaces (file:line in assignment.c):
 *   dash_parse_core_file   initializeProcessor's trace parse         :822-850
 *   dash_init_node_state   initializeProcessor's state init          :806-821
 *   dash_load_traces/_dir  per-thread traces in processorNode        :89-95, :152
 *   dash_run               the OpenMP parallel region: event loop,
 *                          13-way dispatch, sendMessage,
 *                          handleCacheReplacement, locks/queues      :135-155, :149-738,
 *                                                                    :741-765, :767-804
 *   dash_set_micro_seeds   the threads' interleaving itself: per system,
 *                          one seeded weighted walk over pops, issues
 *                          and single sendMessage calls                 :149-738, :741-765
 *   dash_read_state        the private processorNode after the run   :145, :149
 *   dash_dump_node/_file   printProcessorState                       :853-905
 *   dash_simulate_dir      main() end to end                         :126-739
 *
 * Errors: negative return codes (DASH_E*); nothing exits or throws across the
 * ABI. Per-system protocol faults are reported as DASH_ERR_* bits.
 */
#ifndef DASH_H
#define DASH_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DASH_MEM_SIZE 16   /* MEM_SIZE (ref :8) */
#define DASH_MAX_PROCS 8   /* bitVector is one byte (ref :63) */
#define DASH_MAX_CACHE 16
#define DASH_RING_DEPTH 256 /* per-node queue capacity = ref MSG_BUFFER_SIZE (:9); the engine
                              runs shallower LDS queues first and re-runs, from scratch, any
                              system that would fill one (16 -> 32 -> 256) */
#define DASH_NUM_TIERS 3
#define DASH_NUM_TXN 13    /* transactionType (ref :30-44) */

/* return codes */
#define DASH_OK 0
#define DASH_EINVAL -1   /* bad argument / configuration */
#define DASH_EIO -2      /* trace file missing or unreadable (ref :826-828) */
#define DASH_EPARSE -3   /* a line the reference would turn into garbage */
#define DASH_EADDR -4    /* trace address homed on a node >= num_procs */
#define DASH_EDEVICE -5  /* HIP runtime error (no device, launch failure, ...) */
#define DASH_ENOMEM -6
#define DASH_ESTATE -7   /* call out of order (e.g. read_state before run) */
#define DASH_ETRUNC -8   /* an event log reached its capacity: later events were not kept */

/* per-system protocol fault bits (reference UB made defined) */
#define DASH_ERR_OVERFLOW 1u  /* receiver queue (256) full: dropped (ref :754-761) */
#define DASH_ERR_OOB 2u       /* receiver >= N: dropped (ref :751 via :772,786) */
#define DASH_ERR_CTZ0 4u      /* ctz(0) on an EM entry: dropped (ref :209,451) */
#define DASH_ERR_DEADLOCK 8u  /* quiescent with a node still waiting */
#define DASH_ERR_ROUNDCAP 16u /* stopped at max_rounds */
#define DASH_ERR_STUCK 32u    /* a receiver queue reached MSG_BUFFER_SIZE (256): head == tail, so the
                                 reference never drains it again (:167-170); its messages stay
                                 unhandled and later sends to it drop (:754-761). Modelled exactly. */
#define DASH_ERR_SCHEDULE 64u /* a micro-step schedule stepped a node whose outbox still held sends
                                 (not a reference interleaving: sendMessage is synchronous,
                                 :741-765); the system stops there and its results are void */

/* transactionType ordinals (ref :30-44) */
enum dash_txn {
    DASH_READ_REQUEST, DASH_WRITE_REQUEST, DASH_REPLY_RD, DASH_REPLY_WR, DASH_REPLY_ID,
    DASH_INV, DASH_UPGRADE, DASH_WRITEBACK_INV, DASH_WRITEBACK_INT, DASH_FLUSH,
    DASH_FLUSH_INVACK, DASH_EVICT_SHARED, DASH_EVICT_MODIFIED
};

/* flags */
#define DASH_KEEP_STATE 1u    /* write full final node state (needed by dash_read_state) */
#define DASH_TIER_FROM_32 2u  /* start at queue depth 32 (testing: exercises that kernel) */
#define DASH_TIER_FROM_256 4u /* run every system at depth 256 directly; with no TIER flag
                                 the first depth adapts to the previous run's overflow rate */
#define DASH_TEST_SHORT_ARB 8u /* testing only: the seeded schedule's round table holds 8 rounds,
                                  so later rounds take the in-kernel hashing path */
#define DASH_TEST_ONE_GROUP 16u /* testing only: dash_check_coherence walks the batch with a single
                                   workgroup, so a small batch takes several trips of its loop */
#define DASH_TEST_INSERT_PER_LANE 32u /* testing and measurement only: dash_explore_sources inserts every
                                        system's outcome on its own, without grouping equal keys of a wave */
#define DASH_TEST_INSERT_GROUPS 64u   /* likewise: every distinct key of a wave is inserted as a group, however
                                        many there are (the default groups the first few) */
/* testing only as well: dash_test_write_states, declared after dash_read_state */

typedef struct dash_cfg {
    uint32_t num_procs;   /* NUM_PROCS (ref :6): 4 or 8 */
    uint32_t cache_size;  /* CACHE_SIZE (ref :7): 1..16 (powers of two have specialised kernels) */
    uint32_t max_instr;   /* longest trace per node (ref MAX_INSTR_NUM 32, :10) */
    uint32_t flags;       /* DASH_KEEP_STATE */
    uint64_t num_systems; /* independent systems in the batch */
    uint64_t max_rounds;  /* per-system round cap (engine-defined: the reference never exits),
                             clamped to 2^31 - 4, then rounded up to a multiple of 4;
                             0 = 1024 + 256*max_instr */
    int32_t device;       /* HIP device ordinal */
    uint32_t trace_events; /* event log capacity for DEBUG_MSG / DEBUG_INSTR emission
                              (ref :179-182, :649-652), in rounds: every node's events of the
                              first trace_events rounds, rounded up to a multiple of 4 (a node
                              logs at most one event per round, so also at most that many events
                              per node); 0 = no log; < 2^30; device memory num_systems x
                              num_procs x 4 B per kept round */
    uint64_t schedule_seed; /* 0: lowest-sender-first lockstep (the parity schedule); else a
                               seeded legal schedule: per round a node sits out w.p. 1/4 and
                               senders deliver in a seeded order */
} dash_cfg;

/* Final node state in the reference's own terms (processorNode, ref :89-95). */
typedef struct dash_node_state {
    uint8_t memory[DASH_MEM_SIZE];
    uint8_t dir_bitvector[DASH_MEM_SIZE];
    uint8_t dir_state[DASH_MEM_SIZE];     /* EM=0, S=1, U=2 (ref :28) */
    uint8_t cache_addr[DASH_MAX_CACHE];
    uint8_t cache_value[DASH_MAX_CACHE];
    uint8_t cache_state[DASH_MAX_CACHE];  /* MODIFIED=0 .. INVALID=3 (ref :17) */
} dash_node_state;

typedef struct dash_stats {
    uint64_t hist[DASH_NUM_TXN]; /* messages handled per transactionType */
    uint64_t instructions;       /* instructions issued */
    uint64_t rounds_total;       /* sum over systems of lockstep rounds */
    uint64_t rounds_max;
    uint64_t systems;
    uint64_t err_systems;        /* systems with any DASH_ERR_* bit */
    uint64_t err_bits;           /* OR of all DASH_ERR_* bits */
    uint64_t dropped;            /* messages dropped */
    uint64_t max_depth;          /* deepest queue after any delivery */
    double kernel_ms;            /* simulation kernel time (HIP events, engine stream) */
    uint64_t tier_systems[DASH_NUM_TIERS]; /* systems simulated at queue depth 16, 32, 256 */
    uint64_t wave_rounds;        /* lockstep-loop trips summed over wavefronts (all tiers) */
} dash_stats;

/* Synthetic trace generator (counter-based, identical host spec in DESIGN.md §gen). */
#define DASH_GEN_UNIFORM 0u
#define DASH_GEN_CONTENTION 1u /* 90 %: WR to 0x00..0x03 (homed on node 0) */
#define DASH_GEN_LOCALITY 2u   /* node == own w.p. locality/65536, else another node */
typedef struct dash_gen {
    uint64_t seed;
    uint64_t sys_base;  /* global id of this handle's system 0 (multi-GPU sharding) */
    uint32_t kind;
    uint32_t locality;
    uint32_t len;       /* instructions per node (<= cfg.max_instr) */
    uint32_t _reserved;
} dash_gen;

/* One logged step of one node (cfg.trace_events > 0), in lockstep order. */
#define DASH_EV_MSG 0u   /* handled a message: word = message word (type[3:0], sender[6:4],
                            address[14:8], value|bitVector[23:16], secondReceiver[26:24];
                            the other bits are zero; a REPLY_ID's bitVector is the directory's,
                            the receiving requester leaves itself out of the INV fan-out) */
#define DASH_EV_INSTR 1u /* issued an instruction: word = packed instruction */
typedef struct dash_event {
    uint32_t round;
    uint32_t node;
    uint32_t kind;
    uint32_t word;
} dash_event;

typedef struct dash_ctx dash_t;

/* ---- lifecycle / device path (libdash.so, HIP) ---- */
int dash_create(const dash_cfg *cfg, dash_t **out);
void dash_destroy(dash_t *h);
/* the handle's last error message; dash_last_error(NULL) = the message of the last failed
   handle-less call (dash_create, dash_run_host_batched) on the calling thread. The library
   never writes to stderr. */
const char *dash_last_error(const dash_t *h);

/* traces: packed u16 (bit15 = WR, bits 14..8 = address, bits 7..0 = value),
   layout [sys][node][stride]; lens[sys*num_procs + node]. Synchronous: the caller's
   buffer is read (for power-of-two num_procs, by one strided H2D copy) before return;
   words at or past a node's length are never simulated. An RD word's value bits are
   ignored: the reference parses every RD with value 0 (:839) and later fills REPLY_ID /
   REPLY_WR / FLUSH_INVACK lines with the last issued value (:383,470,531), so the library
   clears them on the device after the copy (one pass over the trace buffer). */
int dash_load_traces(dash_t *h, const uint16_t *packed, uint64_t stride, const uint32_t *lens,
                     uint64_t num_systems);
/* Host-buffer throughput path (replaces the same load+run for callers whose traces sit in
   host memory): num_systems (a multiple of batches) go through in `batches` equal batches
   on two handles made from *cfg (num_systems = the batch size), each driven by its own host
   thread and HIP stream, so one batch's H2D copy overlaps another's run. Results equal one
   dash_load_traces + dash_run over all systems: merged *stats (kernel_ms = sum over
   batches), and per-system digests / rounds / errors into the optional arrays. The handles
   are made without DASH_KEEP_STATE and event logs (nothing here returns them); the first
   failing batch stops both threads, and dash_last_error(NULL) then holds its message. */
int dash_run_host_batched(const dash_cfg *cfg, const uint16_t *packed, uint64_t stride,
                          const uint32_t *lens, uint64_t num_systems, uint32_t batches,
                          dash_stats *stats, uint64_t *digests, uint32_t *rounds, uint32_t *errors);
int dash_generate(dash_t *h, const dash_gen *g);
/* An explicit round schedule, replacing the seeded rounds of a handle created with
   schedule_seed != 0 (DASH_ESTATE otherwise): sched[r * num_procs + t] = DASH_SIT_OUT when node
   t sits round r out, else t's delivery position in round r (< next_pow2(num_procs), distinct
   among the round's stepping nodes; DASH_EINVAL otherwise). Rounds >= `rounds` are lockstep
   rounds (every node steps, ascending sender order). Every system of the batch follows it.
   The whole run must fit the handle's round table: cfg.max_rounds (rounded) <= 2^22 and no
   DASH_TEST_SHORT_ARB. Each round is a legal reference execution (the stepping
   threads run their handlers, then complete their sendMessage calls (:741-765) one thread after
   another in delivery order), so a schedule pins one chosen interleaving of the reference, e.g.
   the one behind an accepted racy-test output (tests/golden/schedules/). */
#define DASH_SIT_OUT 0xFFu
int dash_set_schedule(dash_t *h, const uint8_t *sched, uint32_t rounds);
/* A micro-step schedule, the finer-grained twin of dash_set_schedule (same handle requirements):
   acts[r * num_procs + t] = DASH_SIT_OUT, DASH_MICRO_STEP (node t pops or issues, as in a round,
   and its sends wait in its outbox) or DASH_MICRO_SEND (node t delivers its oldest held message);
   at most one node acts per round, and every node sits out past `rounds`. This is the
   reference's own granularity: a thread handles a message, then completes its sendMessage
   calls (:741-765) one by one while other threads run, so any interleaving of the reference's
   threads -- e.g. the one the oracle recovers from a reference run's DEBUG logs -- is one such
   schedule (tests/golden/ref_runs/). A valid schedule never steps a node whose outbox holds
   messages; a system whose schedule does stops at that round with DASH_ERR_SCHEDULE. Runs at
   queue depth 256 only (no tiers); pass max_rounds >= the schedule's rounds:
   a system still active (or holding sends) at the round cap stops with DASH_ERR_ROUNDCAP. */
#define DASH_MICRO_STEP 0u
#define DASH_MICRO_SEND 1u
int dash_set_micro_schedule(dash_t *h, const uint8_t *acts, uint32_t rounds);
/* A schedule seed per system (same handle requirement as dash_set_schedule: created with
   schedule_seed != 0, DASH_ESTATE otherwise, and on a handle that follows a micro-step schedule):
   system k follows the seeded legal schedule of seeds[k], exactly as a handle created with
   schedule_seed = seeds[k] would run it, whichever queue-depth tiers it passes through; a system
   whose seed is 0 runs the lockstep schedule, so a batch can carry its own lockstep baseline.
   n == cfg.num_systems (DASH_EINVAL otherwise); the seeds are on the device before return. No
   round table is built: each wave hashes its systems' round words as it goes. seeds == NULL with
   n == 0 returns the handle to its own seed and table. dash_set_system_seeds and
   dash_set_schedule replace each other: the last call wins. */
int dash_set_system_seeds(dash_t *h, const uint64_t *seeds, uint64_t n);
/* A delay word per system: lockstep but for up to four stated intervals in which one node sits out.
   A delay is 16 bits, t | e << 3 | r << 6: node t (0..7) sits out the 1 << e rounds (e 0..7) from round
   r (0..1022) on; 0xFFFF is an empty slot. A word holds four slots, slot s at bits 16 s, and the
   all-ones word DASH_DELAY_LOCKSTEP is lockstep. Under word w node t sits out round q iff some
   non-empty slot names t with r <= q < r + (1 << e); every other (round, node) is a lockstep step, the
   node stepping and delivering at position t. Slots may overlap or repeat; a slot whose node is >=
   num_procs has no effect. System k follows words[k], whichever queue-depth tiers it passes through.
   Everything else is dash_set_system_seeds': the handle requirements and error codes, n ==
   cfg.num_systems, words == NULL with n == 0 back to the handle's own seed and table, and the dash_set_*
   call made last wins. dash_delay_schedule (below) writes a word's rounds as a dash_set_schedule table. */
#define DASH_DELAY_EMPTY 0xFFFFu
#define DASH_DELAY_LOCKSTEP 0xFFFFFFFFFFFFFFFFull
#define DASH_DELAY(t, e, r) ((uint32_t)(t) | (uint32_t)(e) << 3 | (uint32_t)(r) << 6)
int dash_set_system_delays(dash_t *h, const uint64_t *words, uint64_t n);
/* After any successful load: every system becomes a copy of system src (trace rows and lengths,
   copied on the device). The handle stays loaded. */
int dash_broadcast_system(dash_t *h, uint64_t src);
/* Which final states can one system's traces reach, how often, and under which schedule?
   Broadcasts system src, then runs num_seeds schedules, seeds first_seed + i, in passes of
   cfg.num_systems systems (dash_set_system_seeds; the last pass pads with repeats that are not
   counted). The distinct (digest, errors) outcomes come back ordered by their witness, the lowest
   seed that reached them: up to cap into out, their total into *n, which may exceed cap (cap 0
   with out NULL: count only). Seed 0 is the lockstep schedule. Handle requirements as
   dash_set_system_seeds, and loaded. Afterwards the handle holds the last pass: its seeds stay
   set, and with DASH_KEEP_STATE its states are readable (dash_read_state, dash_dump_system).
   dash_seed_schedule turns a witness seed into a schedule for dash_set_schedule. */
typedef struct dash_outcome {
    uint64_t digest, count, seed; /* seed: the lowest one that reached it */
    uint32_t rounds, errors;      /* of that witness */
} dash_outcome;
int dash_explore(dash_t *h, uint64_t src, uint64_t first_seed, uint64_t num_seeds,
                 dash_outcome *out, uint32_t cap, uint32_t *n);
/* ---- seeded micro-step schedules: one weighted random walk of the reference's own granularity
   per system ----
   The schedule (seed, weights) is a micro-step schedule (dash_set_micro_schedule) decided round by
   round from the system's state. A node is enabled at the start of a round when it holds
   undelivered sends in its outbox, or its queue can be popped (non-empty and not stuck at 256), or
   it can issue (not waiting, instructions left). Exactly one enabled node acts in every round in
   which any node is enabled:
     - byte t of `weights` is node t's weight w_t, 0..31; W = the sum of w_t over the enabled nodes;
     - if W == 0 every enabled node counts with weight 1 (so a weight-0 node acts only when no
       enabled node has positive weight, and the schedule always progresses);
     - u = the high 32 bits of fmix64(seed ^ round * 0x9E3779B97F4A7C15) (the seeded round
       schedule's key), x = (u * W) >> 32;
     - the picked node is the lowest enabled t whose inclusive weight sum over the enabled nodes
       <= t exceeds x;
     - it delivers its oldest held send if it holds any (DASH_MICRO_SEND), else it steps
       (DASH_MICRO_STEP).
   A node with held sends is never stepped (no DASH_ERR_SCHEDULE), every such run is an execution
   of the reference at sendMessage granularity, and `rounds` is its number of micro-steps. A send
   to a node >= num_procs (DASH_ERR_OOB) is held like any other and dropped by its delivery. */
/* The node that acts in `round` of the seeded micro-step schedule (seed, weights), given the set
   of enabled nodes; < 0 = DASH_EINVAL (enabled == 0, a bit >= num_procs, a weight byte > 31).
   Pure host code. */
int dash_micro_pick(uint64_t seed, uint32_t round, uint32_t enabled, uint64_t weights, uint32_t num_procs);
#define DASH_MICRO_UNIFORM 0x0101010101010101ull /* every node weight 1 */
/* System k follows the seeded micro-step schedule (seeds[k], weights[k]); weights == NULL = uniform.
   Handle requirements as dash_set_system_seeds (schedule_seed != 0, DASH_ESTATE otherwise), but no
   round table is needed, so any max_rounds goes. n == cfg.num_systems and every weight byte <= 31
   (DASH_EINVAL otherwise). Runs at queue depth 256 only, as every micro-step schedule.
   seeds == NULL with n == 0 returns the handle to its own seed and table. It replaces, and is
   replaced by, dash_set_schedule, dash_set_micro_schedule and dash_set_system_seeds: the last call
   wins. With an event log (cfg.trace_events) the run records its acts, see dash_read_micro_acts. */
int dash_set_micro_seeds(dash_t *h, const uint64_t *seeds, const uint64_t *weights, uint64_t n);
/* The schedule system `sys` followed in the last run under dash_set_micro_seeds, as a
   dash_set_micro_schedule table acts[r * num_procs + t] for the *rounds rounds it took, rebuilt from
   the event log (a delivery leaves a marker word there, which dash_read_events never returns).
   Feeding the table to dash_set_micro_schedule reproduces the run: final state, digest, event log
   and, for a run that was not cut by the round cap, error bits. One difference: a held send to a
   node >= num_procs (DASH_ERR_OOB) is dropped by its delivery here but at the step under a table,
   where that DASH_MICRO_SEND act then finds an empty outbox and does nothing; if it was the
   system's last act, the replay reports one round fewer. DASH_ESTATE without micro seeds,
   without a log, or before a run; DASH_ETRUNC when the run is longer than the log; DASH_EINVAL when
   cap_rounds < *rounds (*rounds is still set, so a call with cap_rounds 0 sizes the table). */
int dash_read_micro_acts(dash_t *h, uint64_t sys, uint8_t *acts, uint32_t cap_rounds, uint32_t *rounds);
/* dash_explore over seeded micro-step schedules: seeds first_seed + i with one weight vector for
   all (dash_set_micro_seeds). Same outcome records, ordering, padding rule and post-state; no seed
   is special (seed 0 is a schedule like any other). */
int dash_explore_micro(dash_t *h, uint64_t src, uint64_t first_seed, uint64_t num_seeds, uint64_t weights,
                       dash_outcome *out, uint32_t cap, uint32_t *n);
int dash_run(dash_t *h, dash_stats *stats);
int dash_read_state(dash_t *h, uint64_t sys, dash_node_state *out /* [num_procs] */);
/* Testing only: overwrite the kept final states of systems [first, first + count) with hand-built ones,
   so that dash_check_coherence can be given states no run produces. The exact inverse of
   dash_read_state's unpacking: a directory word is memory | dir_bitvector << 8 | (dir_state & 3) << 16,
   a line word cache_addr | cache_value << 8 | (cache_state & 3) << 16; lines at or past cache_size are
   ignored. One copy on the handle's stream. DASH_ESTATE without DASH_KEEP_STATE or before a completed
   dash_run; DASH_EINVAL on a range outside the batch (an empty window at the end is inside). The
   coherence records become invalid: dash_read_coherence refuses until the next dash_check_coherence.
   Digests, rounds, error words, histograms, event log and metrics stay the run's and no longer
   describe the state. */
int dash_test_write_states(dash_t *h, uint64_t first, uint64_t count,
                           const dash_node_state *nodes /* [count * num_procs] */);
int dash_read_results(dash_t *h, uint64_t first, uint64_t count, uint64_t *digests,
                      uint32_t *rounds, uint32_t *errors);
int dash_read_hist(dash_t *h, uint64_t sys, uint32_t *hist /* [DASH_NUM_TXN] */);
/* The event log of one system, merged in lockstep order (round, then node): up to
   cap events into out, the total into *n (cap 0 with out NULL: count only). The log keeps
   trace_events rounds rounded up to a multiple of 4 (a node logs at most one event per round);
   DASH_ETRUNC if events fell past them (counted in *n, not kept). */
int dash_read_events(dash_t *h, uint64_t sys, dash_event *out, uint32_t cap, uint32_t *n);

/* ---- per-node cache and coherence metrics, reduced on the device from the event log
   (csrc/dash_metrics.hip) ----
   Every metric is a pure function of one system's event log over its kept rounds [0, K),
   K = min(rounds[sys], the log's rounds). A "word" is node t's log word of round r; an "event" is a
   word of a round in which t handled a message or issued an instruction (what dash_read_events
   returns); an event is an instruction (DASH_EV_INSTR) or a popped message (DASH_EV_MSG) with the
   type, sender and address fields documented for dash_event.word. The "completing types" are
   REPLY_RD, REPLY_WR, REPLY_ID, FLUSH and FLUSH_INVACK: exactly the pops that clear
   waitingForReply in the reference.

   reads, writes          instruction events of node t, by bit 15 of the instruction (set = WR)
   read_misses, write_misses, upgrades
                          READ_REQUEST / WRITE_REQUEST / UPGRADE message events at any node whose
                          sender is t. Requests are only ever popped at the home, so these are the
                          requests of t that were serviced
   msgs                   message events popped by t
   home_requests          READ_REQUEST + WRITE_REQUEST + UPGRADE popped by t: its directory load
   invalidations          INV popped by t
   interventions          WRITEBACK_INV + WRITEBACK_INT popped by t
   evict_shared, evict_modified
                          EVICT_SHARED / EVICT_MODIFIED events with sender t that are popped at node
                          address >> 4 (the home). This leaves out the home's forwarded EVICT_SHARED
                          to a new owner, which is popped elsewhere
   waits, wait_rounds, wait_max
                          for each instruction event of t at round r0, take t's next event of a
                          completing type, at round r1. If it comes before t's next instruction
                          event, the span r1 - r0 is counted: waits is the count, wait_rounds the
                          sum and wait_max the maximum of these spans. Spans are disjoint, so the
                          sum fits 32 bits. A span still open at round K is not counted
   deliveries             words equal to the delivery marker of a seeded micro-step schedule
                          (non-zero only under dash_set_micro_seeds)
   idle_rounds            K - (reads + writes + msgs) - deliveries

   These are the reference's behaviour, not an approximation of ours: hits are reads - read_misses
   (likewise for writes) for systems without DASH_ERR_OVERFLOW / _STUCK / _ROUNDCAP and with an
   untruncated log. The reference clears waitingForReply on any completing pop, so a stray FLUSH can
   release a waiting home early: a wait span is "issue to the pop that cleared waitingForReply", not
   "issue to the matching reply". */
typedef struct dash_node_metrics {
    uint32_t reads, writes;
    uint32_t read_misses, write_misses, upgrades;
    uint32_t msgs, home_requests, invalidations, interventions;
    uint32_t evict_shared, evict_modified;
    uint32_t waits, wait_rounds, wait_max;
    uint32_t deliveries, idle_rounds;
} dash_node_metrics; /* 16 x uint32_t: 64 B per node */
/* The 16 fields summed over every node of every system (wait_max: the maximum), the systems of the
   batch, and those whose log was shorter than their run. */
typedef struct dash_metrics_totals {
    uint64_t reads, writes;
    uint64_t read_misses, write_misses, upgrades;
    uint64_t msgs, home_requests, invalidations, interventions;
    uint64_t evict_shared, evict_modified;
    uint64_t waits, wait_rounds, wait_max;
    uint64_t deliveries, idle_rounds;
    uint64_t systems, truncated_systems;
} dash_metrics_totals;
/* One pass of the device over the whole batch's event log of the last dash_run (any schedule; after
   dash_explore*, the last pass): a dash_node_metrics record per node stays on the device until the
   next dash_run, and the totals (optional) are on the host at return. DASH_ESTATE before a
   completed dash_run and on a handle created with trace_events == 0. A log shorter than a system's
   run is no error: that system's metrics cover rounds [0, the log's rounds), its `truncated` byte
   is set and it counts in truncated_systems. */
int dash_compute_metrics(dash_t *h, dash_metrics_totals *totals);
/* Records of systems [first, first + count): out[(k - first) * num_procs + t], and (optional)
   truncated[k - first] = 1 when rounds[k] > the log's rounds. DASH_ESTATE when no
   dash_compute_metrics followed the last dash_run; DASH_EINVAL for a range outside the batch. */
int dash_read_metrics(dash_t *h, uint64_t first, uint64_t count, dash_node_metrics *out,
                      uint8_t *truncated);

/* ---- per-address sharing profile, reduced on the device from the event log
   (csrc/dash_addr.hip) ----
   The second axis of the per-node metrics: the same log, by address. An address is
   a = (home << 4) | block, a < A = num_procs * 16; an event's address is bits 14:8 of its word, for
   instructions and popped messages alike. The events are those of the kept rounds [0, K),
   K = min(rounds[sys], the log's rounds), exactly as above; the delivery markers of seeded micro-step
   schedules are not events. Every field of address a's record is a sum or an OR over the events whose
   address is a, so nothing depends on their order:

   reads, writes          instruction events, by bit 15 of the instruction (set = WR)
   read_misses, write_misses, upgrades
                          READ_REQUEST / WRITE_REQUEST / UPGRADE message events, whoever pops them
   invalidations          INV popped, at any node
   interventions          WRITEBACK_INV + WRITEBACK_INT popped
   flushes                FLUSH + FLUSH_INVACK popped: the cache-to-cache supplies
   evict_shared, evict_modified
                          EVICT_SHARED / EVICT_MODIFIED popped at the home only (node == a >> 4), as in
                          dash_node_metrics: the home's forwarded EVICT_SHARED is popped elsewhere
   msgs                   every message event
   nodes                  readers | writers << 8 | invalidated << 16: bit t of each byte is set when
                          node t issued an RD / issued a WR / popped an INV on a

   An event whose address is >= A belongs to no record; the totals count it in foreign_events, so the
   records and that count together hold every event. Every load refuses a trace address homed on a
   node >= num_procs (DASH_EADDR), so no run of loaded traces has one. A field wraps at 2^32, which
   takes more than 2^29 kept rounds of one system. */
typedef struct dash_addr_metrics {
    uint32_t reads, writes;
    uint32_t read_misses, write_misses, upgrades;
    uint32_t invalidations, interventions, flushes;
    uint32_t evict_shared, evict_modified;
    uint32_t msgs;
    uint32_t nodes;
} dash_addr_metrics; /* 12 x uint32_t: 48 B per address */
/* The class of a record, with r = nodes & 0xFF and w = (nodes >> 8) & 0xFF; "two or more nodes" is
   popcount(r | w) >= 2. A touched record has a bit in r | w, so exactly one class holds: */
#define DASH_ADDR_UNTOUCHED 0    /* reads + writes == 0 */
#define DASH_ADDR_PRIVATE 1      /* popcount(r | w) == 1 */
#define DASH_ADDR_READ_SHARED 2  /* w == 0, two or more nodes */
#define DASH_ADDR_ONE_WRITER 3   /* popcount(w) == 1, two or more nodes */
#define DASH_ADDR_MULTI_WRITER 4 /* popcount(w) >= 2 */
/* Pure host code, the arithmetic the device uses (addr_class in csrc/dash_addr.h); DASH_EINVAL for NULL.
   (A hand-made record with reads + writes != 0 and r | w == 0 comes back as DASH_ADDR_PRIVATE.) */
int dash_addr_class(const dash_addr_metrics *m);
/* Over every record of the batch: the sums of the first eleven fields, the largest msgs of any record,
   the events that fell in no record, and per class (DASH_ADDR_*) the records, their read_misses +
   write_misses + upgrades and their invalidations; the systems, and those whose log was shorter than
   their run. */
typedef struct dash_addr_totals {
    uint64_t reads, writes;
    uint64_t read_misses, write_misses, upgrades;
    uint64_t invalidations, interventions, flushes;
    uint64_t evict_shared, evict_modified;
    uint64_t msgs;
    uint64_t msgs_max;
    uint64_t foreign_events;
    uint64_t class_addrs[5], class_misses[5], class_invalidations[5];
    uint64_t systems, truncated_systems;
} dash_addr_totals;
/* One pass of the device over the whole batch's event log of the last dash_run (any schedule; after
   dash_explore*, the last pass): num_procs * 16 dash_addr_metrics records per system stay on the device
   until the next dash_run, and the totals (optional) are on the host at return. State rules as
   dash_compute_metrics: DASH_ESTATE before a completed dash_run and on a handle created with
   trace_events == 0; a log shorter than a system's run is no error (the records cover the log's
   rounds, the `truncated` byte is set and the system counts in truncated_systems). The record buffer,
   num_systems x num_procs x 16 x 48 B, is allocated by the first call: DASH_ENOMEM when it does not
   fit, and the handle stays usable. These records and dash_compute_metrics' are valid independently
   of each other. */
int dash_compute_addr_metrics(dash_t *h, dash_addr_totals *totals);
/* Records of systems [first, first + count): out[(k - first) * num_procs * 16 + a], and (optional)
   truncated[k - first]. DASH_ESTATE when no dash_compute_addr_metrics followed the last dash_run;
   DASH_EINVAL for a range outside the batch. */
int dash_read_addr_metrics(dash_t *h, uint64_t first, uint64_t count, dash_addr_metrics *out,
                           uint8_t *truncated);

/* ---- coherence invariants of final states (csrc/dash_coherence.hip) ----
   An address is a = (home << 4) | block with home < num_procs and block < 16: a system has
   num_procs * 16 addresses. Over the final state of one system, the copies of a are the cache lines
   (t, i), t < num_procs, i < cache_size, with cache_addr == a and cache_state != INVALID. Lines are
   found by scanning, wherever they sit: no placement is assumed, and two valid lines of one node with
   the same address are two copies. Lines with another address (the initial 0xFF) belong to no
   checked address. With
     n    = the number of copies,
     own  = the number of copies in MODIFIED or EXCLUSIVE,
     mask = the OR of 1 << t over the copies,
     d, bv, mem = the home's dir_state, dir_bitvector and memory at block,
   an address has the bit set when: */
#define DASH_COH_SWMR 1u           /* own >= 1 && n >= 2 */
#define DASH_COH_DIR_U_HELD 2u     /* d == U && n >= 1 */
#define DASH_COH_DIR_EM 4u         /* d == EM && !(n == 1 && own == 1) */
#define DASH_COH_DIR_S 8u          /* d == S && (own >= 1 || n == 0) */
#define DASH_COH_LOST_SHARER 16u   /* d != U && (mask & ~bv) != 0 */
#define DASH_COH_STALE_SHARER 32u  /* d != U && (bv & ~mask) != 0; bits of bv at or above num_procs count */
#define DASH_COH_STALE_VALUE 64u   /* some copy in SHARED or EXCLUSIVE has cache_value != mem */
#define DASH_COH_VALUE_SPLIT 128u  /* two copies differ in cache_value */
typedef struct dash_coherence {
    uint32_t bits;       /* OR over the system's addresses */
    uint32_t addrs;      /* addresses with any bit */
    uint32_t first_addr; /* lowest such address; 0xFFFFFFFF when addrs == 0 */
    uint32_t first_bits; /* that address's bits; 0 when addrs == 0 */
} dash_coherence;
/* Over the batch. bit_systems[k] / bit_addrs[k]: systems / addresses with bit 1 << k. Systems with
   DASH_ERR_* bits are checked like any other (a cut run's state is what it is);
   violating_clean_systems leaves them out. */
typedef struct dash_coherence_totals {
    uint64_t systems, violating_systems;
    uint64_t violating_clean_systems;    /* bits != 0 and errors[sys] == 0 */
    uint64_t addrs;
    uint64_t bit_systems[8], bit_addrs[8];
} dash_coherence_totals;
/* One pass of the device over the whole batch's final state of the last dash_run (after
   dash_explore*, the last pass): a dash_coherence record per system stays on the device until the
   next dash_run, and the totals (optional) are on the host at return. DASH_ESTATE before a completed
   dash_run and on a handle created without DASH_KEEP_STATE. */
int dash_check_coherence(dash_t *h, dash_coherence_totals *totals);
/* Records of systems [first, first + count). DASH_ESTATE when no dash_check_coherence followed the
   last dash_run; DASH_EINVAL for a range outside the batch. */
int dash_read_coherence(dash_t *h, uint64_t first, uint64_t count, dash_coherence *out);
/* Classifies the outcomes an explore returned: an outcome's digest is a digest of the final state,
   so its witness seed stands for it. Broadcasts system src and runs the witness seeds outs[k].seed in
   passes of cfg.num_systems (dash_set_system_seeds; with weights != NULL, dash_set_micro_seeds under
   the one weight vector *weights), the last pass padded with repeats; after each pass
   dash_check_coherence gives out[k], in the order given. DASH_ESTATE, with a message naming k, when
   witness k did not reproduce outs[k].digest and outs[k].errors. Handle requirements as the matching
   explore, plus DASH_KEEP_STATE. Afterwards the handle holds the last pass. */
int dash_check_outcomes(dash_t *h, uint64_t src, const dash_outcome *outs, uint32_t n,
                        const uint64_t *weights, dash_coherence *out /* [n] */);

/* ---- many trace sets at once: outcomes merged and classified on the device
   (csrc/dash_outcomes.hip) ----
   The sources are systems 0 .. num_sources - 1 of the loaded batch. Every source runs
   seeds_per_source schedules, seeds first_seed + j, under seeded round schedules (weights == NULL; seed
   0 is lockstep, as in dash_explore) or seeded micro-step schedules under the one vector *weights. The
   systems of a pass are assigned by dash_explore_assign (below) with S = cfg.num_systems: system k >=
   num_sources is overwritten by a copy of system k % num_sources on the device, the seeds of a pass are
   written on the device, and after each pass every counted system's (source, digest, errors) goes into
   a device hash table of table_slots slots (a power of two; another value is rounded up; 0 =
   next_pow2(2 * min(num_sources * seeds_per_source, 2^21)), at least 64). Keys are compared in full:
   two sources never share an entry, even with identical traces. dash_check_coherence's launch then
   runs over the pass's final states and every outcome's witness, the lowest seed that reached it, leaves
   its rounds and its coherence record in the table. Only the compacted table crosses to the host.

   Outcomes come back ordered by (source, witness seed): up to cap into out, their number into *n, which
   may exceed cap (cap 0 with out NULL: count only). per_source[i] (optional) and *totals (optional)
   are sums over the whole list, not just its first cap entries.

   Handle requirements as the matching explore (created with schedule_seed != 0, loaded, and for
   weights == NULL not following a micro-step table) plus DASH_KEEP_STATE: DASH_ESTATE otherwise.
   DASH_EINVAL: num_sources 0 or above cfg.num_systems, a weight byte above 31, first_seed +
   seeds_per_source wrapping 2^64, out == NULL with cap != 0, n == NULL. Afterwards the handle holds the
   last pass (its seeds stay set; states, results and coherence records are readable).

   A table that fills: a key is placed on its first insert or never (slots are never freed), so what is
   returned is exact for the keys it lists, totals->unplaced counts the schedules that found no slot,
   sum of count + unplaced == schedules, and the return code is DASH_ETRUNC (out, *n, per_source and
   totals are filled). With the default size and at most 2^21 schedules this cannot happen. */
typedef struct dash_outcome_ex {
    dash_outcome o;      /* digest, count, seed (lowest that reached it), rounds, errors of that witness */
    dash_coherence coh;  /* the invariants of that final state */
    uint32_t source, _reserved;
} dash_outcome_ex;       /* 56 B */
typedef struct dash_source_summary {
    uint64_t schedules, incoherent_schedules;   /* counted; those whose outcome has coh.bits != 0 */
    uint64_t top_count;                         /* count of the most frequent outcome */
    uint32_t outcomes, incoherent_outcomes, coh_bits /* OR */, err_bits /* OR */;
} dash_source_summary;
typedef struct dash_explore_totals {
    uint64_t schedules, outcomes, unplaced, passes, table_slots;
    uint64_t incoherent_outcomes, incoherent_schedules, incoherent_clean_schedules; /* clean: errors == 0 */
    uint64_t bit_schedules[8];                  /* schedules whose outcome has DASH_COH bit 1<<k */
    double sim_ms, merge_ms;                    /* device events: dash_run's kernels; the kernels of
                                                   dash_outcomes.hip + the coherence launch */
    double insert_ms;                           /* of merge_ms: the insert kernels alone */
} dash_explore_totals;
int dash_explore_sources(dash_t *h, uint64_t num_sources, uint64_t first_seed, uint64_t seeds_per_source,
                         const uint64_t *weights, uint64_t table_slots, dash_outcome_ex *out, uint64_t cap,
                         uint64_t *n, dash_source_summary *per_source /* [num_sources] or NULL */,
                         dash_explore_totals *totals /* or NULL */);

/* ---- every schedule within a few delays of lockstep (csrc/dash_delays.h) ----
   A bounded schedule space that can be enumerated: lockstep plus at most max_delays delays (delay
   words, dash_set_system_delays), each starting in one of the rounds 0 .. starts - 1 (starts 1..1023)
   and 1, 2, .., 2^(lens - 1) rounds long (lens 1..8); max_delays is 0..4. The rule, stated once:

   With N = num_procs and E = lens, cell c = (r * N + t) * E + e is the delay t | e << 3 | r << 6;
   there are M = starts * N * E cells. The schedules with d delays have the indices [B_d, B_d + C(M, d)),
   B_0 = 0, B_(d+1) = B_d + C(M, d), and K = B_(max_delays + 1) is the size of the space. Within a block
   the rank j = index - B_d names the cells c_d > ... > c_1 by the combinatorial number system,
   j = C(c_d, d) + ... + C(c_1, 1); slot s of the word holds cell c_(s+1) and the other slots are empty.
   Index 0 is lockstep, and indices rise with the delay count: the lowest index that reaches an outcome
   is a fewest-delays witness.

   dash_delay_count gives K, dash_delay_word the word of index < K: DASH_EINVAL for space == NULL, a
   field or num_procs outside the ranges above, index >= K, or a NULL result. Pure host code; the device
   uses the same arithmetic (delay_unrank in csrc/dash_delays.h).

   dash_explore_delays is dash_explore_sources (above) over this space: first_seed = 0,
   seeds_per_source = K, weights == NULL, and the seed of a system is its schedule index, whose delay
   word a kernel writes per system where dash_explore_sources writes the seed. Assignment, table, merge,
   coherence records, the full-table rule (DASH_ETRUNC) and the handle's state afterwards (the words of
   the last pass stay set, as after dash_set_system_delays) are that call's. out[k].o.seed is the lowest
   index that reached the outcome, out[k].o.count how many schedules of the space reach it. Handle
   requirements and error codes as dash_explore_sources, plus DASH_EINVAL for a space out of range. */
typedef struct dash_delay_space { uint32_t starts, lens, max_delays, _reserved; } dash_delay_space;
int dash_delay_count(const dash_delay_space *space, uint32_t num_procs, uint64_t *K);
int dash_delay_word(const dash_delay_space *space, uint32_t num_procs, uint64_t index, uint64_t *word);
int dash_explore_delays(dash_t *h, uint64_t num_sources, const dash_delay_space *space, uint64_t table_slots,
                        dash_outcome_ex *out, uint64_t cap, uint64_t *n,
                        dash_source_summary *per_source /* [num_sources] or NULL */,
                        dash_explore_totals *totals /* or NULL */);

/* ---- shrinking one system to a minimal reproducer (csrc/dash_shrink.hip) ----
   dash_check_coherence and the explores say that a system ends in a broken state, in 16 bytes.
   dash_shrink cuts the system down to a few instructions that still end in such a state: round by
   round it deletes the largest block of instructions of one node that keeps the goal true, until no
   single instruction can be deleted. Every variant of a round is written, simulated, checked and
   ranked on the device; the host reads 8 bytes per round. The rule, stated once:

   The base is a trace set with lens[t] instructions on node t < num_procs.

   Candidates of a round, in the order of their index c = 0, 1, ...: by node t ascending; for each node
   with lens[t] > 0 by level j = J, J - 1, ..., 0, where J is the least integer with 2^J >= lens[t];
   within a level by block start s = 0, 2^j, 2 * 2^j, ... < lens[t]. The candidate deletes instructions
   [s, min(s + 2^j, lens[t])) of node t: later instructions of that node move down, the other nodes are
   untouched, and words at or past the new length are 0. A node of length L so has the sum over j <= J of
   ceil(L / 2^j) candidates; C is the sum over the nodes. Level 0 holds every single deletion.

   A candidate passes when its run, under the same schedule as the base, ends with
     (coh.bits & goal.coh_all) == goal.coh_all  and
     (errors & goal.err_all) == goal.err_all    and  (errors & goal.err_none) == 0,
   coh being the dash_coherence record of its final state and errors its DASH_ERR_* bits.

   The winner of a round is the passing candidate that deletes the most instructions; among equals, the
   one with the lowest index. It becomes the new base. When no candidate passes the call ends: the base is
   then 1-minimal, deleting any one instruction breaks the goal.

   dash_shrink_candidate is the enumeration as pure host code (the device uses the same arithmetic,
   shrink_decode in csrc/dash_shrink.h): it returns C for lens[0 .. num_procs), and for c < C sets *node, *start and
   *count (each optional) to candidate c's. DASH_EINVAL for c >= C when C > 0 (with C == 0 it returns 0
   whatever c is), for lens == NULL, num_procs outside 1..8 or a length above 2^24. */
typedef struct dash_shrink_goal { uint32_t coh_all, err_all, err_none, _reserved; } dash_shrink_goal;
typedef struct dash_shrink_step { uint32_t node, start, count, candidates; } dash_shrink_step; /* one per round:
                                       the winner, and the C of the base it was taken from */
typedef struct dash_shrink_report {
    uint64_t rounds, passes, variants;          /* winners applied; dash_run calls (the check of the source
                                                   and the final run included); counted candidates run */
    uint64_t instr_before, instr_after;
    double sim_ms, gen_ms, select_ms;           /* device events: dash_run's kernels; the candidate and apply
                                                   kernels; the coherence launch and the select kernel */
} dash_shrink_report;
/* Shrinks system src of the loaded batch under the goal. seed == 0: the lockstep schedule (on a handle
   created without schedule_seed the plain lockstep kernel; on a seeded handle every system gets seed 0);
   seed != 0: every variant runs the seeded round schedule `seed`, as dash_set_system_seeds gives it
   (needs a handle created with schedule_seed != 0). A round takes ceil(C / cfg.num_systems) sub-passes:
   in sub-pass p system k holds candidate p * num_systems + k; systems past the last candidate repeat the
   base and are not counted.
   Results: the minimal set into packed_out[node * stride ..] (optional; the rest of a row is zeroed) and
   lens_out[node] (optional); the rounds' winners into steps[0 .. cap), their number into *n, which may
   exceed cap (n may be NULL when cap == 0); *report (optional). Afterwards every system of the handle
   holds the minimal set and has run it once more, with its coherence records in place: dash_read_state,
   dash_dump_system, dash_read_coherence and dash_read_traces work on it; on a seeded handle the seeds stay
   set.
   DASH_ESTATE: created without DASH_KEEP_STATE, no traces loaded, the handle follows a micro-step table,
   seed != 0 on a handle created with schedule_seed == 0. DASH_EINVAL: src out of range, goal NULL or
   coh_all == 0 && err_all == 0, packed_out with a stride below the source's longest trace, n == NULL
   with cap != 0, steps == NULL with cap != 0, and a source that does not itself meet the goal
   (dash_last_error says so, with the source's bits; the batch then holds copies of the source, run and
   checked). */
int dash_shrink(dash_t *h, uint64_t src, uint64_t seed, const dash_shrink_goal *goal,
                uint16_t *packed_out /* [num_procs][stride] or NULL */, uint64_t stride, uint32_t *lens_out,
                dash_shrink_step *steps, uint32_t cap, uint32_t *n, dash_shrink_report *report);

/* ---- shrinking many systems side by side (csrc/dash_shrink.hip) ----
   What dash_explore_sources returns, turned into reproducers in one call: a list of jobs (source system,
   round-schedule seed, goal) is shrunk in lock-step rounds, the handle's systems dealt out over the
   candidates of all jobs that are still shrinking. The rule, stated once:

   Per job, candidates, deletion, goal, winner and stopping are dash_shrink's (above), and every variant of
   job i runs the seeded round schedule jobs[i].seed (0 = lockstep). For every job with status
   DASH_SHRINK_MINIMAL its steps, final trace set, lengths, rounds, variants, instr_before and instr_after
   equal those of dash_shrink(h, src, seed, &goal, ...) on its own. Two jobs may name the same src: every
   job's source is copied into a base row of its own before the batch is overwritten.

   Before round 0, with J = num_jobs and S = cfg.num_systems: system k becomes a copy of the source of job
   k % J, cleared past its lengths, under that job's seed; one run and one coherence launch follow.
   src_coh_bits and src_errors of every job are those of system i < J. A job whose source does not pass
   its own goal gets status DASH_SHRINK_UNMET: it is left as it is, with 0 rounds and 0 variants, and the
   call goes on.

   A round: all jobs advance one round together. C_i is the candidate count of job i's current base; it
   is 0 for a job that is UNMET and for a job that has stopped, and a job stops in the round in which none
   of its candidates passed. P_i = C_0 + ... + C_(i-1), T = P_J. The round has ceil(T / S) sub-passes. In
   sub-pass p system k has the global index g = p * S + k:
     - if g < T it holds candidate g - P_i of the job i with P_i <= g < P_(i+1), under job i's seed, and
       it is counted;
     - otherwise it holds the unchanged base of job k % J under that job's seed, and it is not counted.
   After the round's last sub-pass every job with a passing candidate takes its winner as its new base, and
   C_i is added to the variants of every job that had candidates, its last (failing) round included. The
   call ends at the first round with T == 0.

   dash_shrink_assign (below) is this assignment as pure host code; the device uses the same arithmetic,
   many_assign in csrc/dash_shrink.h.

   Afterwards system k holds the final set of job k % J (the minimal set, or the untouched source of an
   UNMET job) and has run it once more under that job's seed, with its coherence records in place:
   dash_read_traces, dash_read_state, dash_dump_system, dash_read_coherence and dash_read_results work on
   it; on a seeded handle the seeds stay set.
   Results, each optional: job i's final set into packed_out[(i * num_procs + node) * stride ..] (the rest
   of a row is zeroed) and lens_out[i * num_procs + node]; its first step_cap winners into
   steps[i * step_cap ..], results[i].rounds saying how many there were; results[i]; *report.

   DASH_ESTATE, as for dash_shrink: created without DASH_KEEP_STATE, no traces loaded, the handle follows
   a micro-step table, a job with seed != 0 on a handle created with schedule_seed == 0. DASH_EINVAL:
   jobs == NULL; num_jobs 0, above cfg.num_systems or above DASH_SHRINK_MAX_JOBS; a src out of range; a
   goal with no bit in coh_all or err_all (dash_last_error names the job); packed_out with a stride below
   the longest source trace of any job; steps == NULL with step_cap != 0. DASH_ENOMEM when the base rows
   do not fit: the call keeps two system rows per job on the device. */
#define DASH_SHRINK_MAX_JOBS 65536u
#define DASH_SHRINK_MINIMAL 0u  /* cut down to a 1-minimal set (possibly in 0 rounds) */
#define DASH_SHRINK_UNMET   1u  /* the source does not meet its own goal: left as it is, 0 rounds, 0 variants */
typedef struct dash_shrink_job { uint64_t src, seed; dash_shrink_goal goal; } dash_shrink_job;
typedef struct dash_shrink_result {
    uint32_t status, rounds;              /* rounds: winners applied */
    uint32_t instr_before, instr_after;
    uint64_t variants;                    /* counted candidates of this job, its last (failing) round included */
    uint32_t src_coh_bits, src_errors;    /* the source's own record and error word under the job's seed */
} dash_shrink_result;
typedef struct dash_shrink_many_report {
    uint64_t jobs, minimal, unmet;
    uint64_t rounds;                      /* lock-step rounds of the call = the largest job's rounds + 1, 0 if no job is active */
    uint64_t passes, variants, instr_before, instr_after; /* passes: dash_run calls = 2 + the rounds' sub-passes;
                                                             the others: sums over the jobs */
    double sim_ms, gen_ms, select_ms;     /* as dash_shrink_report */
} dash_shrink_many_report;
int dash_shrink_many(dash_t *h, const dash_shrink_job *jobs, uint64_t num_jobs,
                     uint16_t *packed_out /* [num_jobs][num_procs][stride] or NULL */, uint64_t stride,
                     uint32_t *lens_out /* [num_jobs][num_procs] or NULL */,
                     dash_shrink_step *steps /* [num_jobs][step_cap] or NULL */, uint32_t step_cap,
                     dash_shrink_result *results /* [num_jobs] or NULL */, dash_shrink_many_report *report);
/* HIP stream the engine launches on (hipStream_t as void*) */
void *dash_stream(dash_t *h);

/* Box calibration (not a reference interface: it makes a benchmark line explain the box it ran
   on). The device's identity and clock limits, and one timed launch of a fixed VALU-bound
   probe kernel (CUs x 8 workgroups of 256 threads, eight add/xor chains per lane): its time,
   its rate, and the shader clock the box actually held meanwhile (shader-clock cycles over the
   100-MHz reference counter, read by every workgroup around its loop). A box whose clock or
   issue rate is low shows it here, whatever the simulation kernel did. */
typedef struct dash_box_probe {
    char name[64];
    char arch[32];
    int32_t compute_units;
    int32_t clock_khz;        /* hipDeviceProp_t.clockRate (the maximum shader clock) */
    int32_t mem_clock_khz;    /* hipDeviceProp_t.memoryClockRate */
    int32_t pci_domain, pci_bus, pci_device;
    uint64_t total_mem;
    double probe_ms;          /* the probe launch (HIP events) */
    double probe_valu_per_s;  /* wave64 VALU instructions of the chains per second */
    double probe_sclk_mhz;    /* mean shader clock over the workgroups' loops */
    double probe_sclk_min_mhz, probe_sclk_max_mhz;
} dash_box_probe;
int dash_probe_box(int device, dash_box_probe *out);

/* ---- host boundary (pure C, no device) ---- */
/* The seeded schedule of `seed` as a dash_set_schedule table: sched[r * num_procs + t] =
   DASH_SIT_OUT or node t's delivery position in round r, for rounds [0, rounds) -- what a handle
   created with schedule_seed = seed, or a system given that seed by dash_set_system_seeds, follows
   in those rounds (seed 0: the lockstep rounds, every node at position t). A table of at least
   the run's rounds reproduces the run; it can be read, edited and kept (tests/golden/schedules/).
   DASH_EINVAL for num_procs outside 1..8 or sched == NULL. */
int dash_seed_schedule(uint64_t seed, uint32_t num_procs, uint32_t rounds, uint8_t *sched);
/* Likewise the rounds [0, rounds) of a delay word (dash_set_system_delays): DASH_SIT_OUT where node t
   sits the round out, else position t. Slots on nodes >= num_procs write nothing. A table that covers
   the word's last interval reproduces the run (later rounds of a table are lockstep, as the word's
   are). DASH_EINVAL for num_procs outside 1..8 or sched == NULL. */
int dash_delay_schedule(uint64_t word, uint32_t num_procs, uint32_t rounds, uint8_t *sched);
/* Which source and seed system k of a pass of dash_explore_sources runs, and whether its outcome is
   counted: the rule the device follows, stated once. A handle of S systems explores G sources
   (1 <= G <= S) with K seeds each, F the first seed (F + K must not wrap 2^64):
     - R = S / G seeds of every source run per pass; there are ceil(K / R) passes;
     - in pass p, system k runs source k % G;
     - its seed index is j = p * R + k / G, its seed F + j;
     - it is counted iff k < G * R and j < K;
     - an uncounted system runs a repeat, seed index p * R + (k / G) % fresh with
       fresh = min(R, K - p * R), and is never counted.
   *source, *seed and *counted (each optional) are set for system k < S of pass `pass` < ceil(K / R);
   DASH_EINVAL outside these ranges. Pure host code. */
int dash_explore_assign(uint64_t S, uint64_t G, uint64_t K, uint64_t F, uint64_t pass, uint64_t k,
                        uint32_t *source, uint64_t *seed, int *counted);
/* Candidate c of a dash_shrink round over a base of lens[0 .. num_procs) (the rule is stated with
   dash_shrink, above). Returns C >= 0, or DASH_EINVAL. Pure host code. */
int dash_shrink_candidate(const uint32_t *lens, uint32_t num_procs, uint64_t c,
                          uint32_t *node, uint32_t *start, uint32_t *count);
/* What system k of sub-pass `pass` of a dash_shrink_many round holds, for jobs with cands[0 .. J)
   candidates on a handle of S systems (the rule is stated with dash_shrink_many, above): *counted, and
   for a counted system *job and *cand (its index within that job); for an uncounted one *job = k % J and
   *cand = 0. Each output is optional. DASH_EINVAL for cands == NULL, J == 0, J above S or above
   DASH_SHRINK_MAX_JOBS, a count of 2^32 or more, k >= S and pass >= ceil(T / S) (so every pass when
   T == 0). Pure host code. */
int dash_shrink_assign(const uint64_t *cands /* [J] */, uint64_t J, uint64_t S, uint64_t pass, uint64_t k,
                       uint64_t *job, uint64_t *cand, int *counted);
/* One trace set as a trace directory: out_dir/core_<n>.txt for n < num_procs (out_dir is created if
   missing), node n's lens[n] words of packed[n * stride ..] as the fixtures write them, "RD 0x3C" and
   "WR 0x00 110", one per line. dash_parse_core_file reads back the same words (an RD's value bits are
   not written: they mean nothing). DASH_EINVAL for a length above stride, DASH_EIO when a file cannot
   be written. */
int dash_write_dir(const uint16_t *packed, uint64_t stride, const uint32_t *lens, uint32_t num_procs,
                   const char *out_dir);
/* initializeProcessor's parse (ref :822-850): up to max_instr records into out[]. */
int dash_parse_core_file(const char *path, uint32_t num_procs, uint32_t max_instr,
                         uint16_t *out, uint32_t *len);
/* Resolve the reference's `tests/<dir>/core_<n>.txt` rule (ref :824); also accepts a
   directory that directly holds core_<n>.txt. Writes the resolved path. */
int dash_resolve_dir(const char *dir, char *resolved, size_t cap);
int dash_load_dir(dash_t *h, const char *dir, uint64_t sys);
/* Bulk ingest: system k = trace directory dirs[k] (same rules as dash_load_dir, ref
   :822-850; parsed on host threads, no "initialized" lines); n == cfg.num_systems. */
int dash_load_dirs(dash_t *h, const char *const *dirs, uint64_t n);
/* The same parse applied to a byte buffer (csrc/dash_text.c states the rules once): the
   return code, *len and out[0..*len) equal those of dash_parse_core_file on a file holding
   these bytes. Only the first 19 * max_instr bytes can matter. */
int dash_parse_core_text(const char *text, size_t length, uint32_t num_procs, uint32_t max_instr,
                         uint16_t *out, uint32_t *len);
/* Gathers trace text without parsing it: at most 19 * max_instr bytes of each
   <dirs[k]>/core_<t>.txt (t < num_procs; directories resolved by dash_resolve_dir), back to
   back into buf, each file starting on a 16-byte boundary; file f = k * num_procs + t is
   buf[offsets[f] .. offsets[f] + lengths[f]). *need = the bytes buf must hold; buf == NULL
   measures only (offsets / lengths, when given, are still filled). DASH_EINVAL when cap <
   *need; DASH_EIO on a missing file, after dash_parse_core_file's stderr line (ref :827). */
int dash_read_dirs_text(const char *const *dirs, uint64_t n, uint32_t num_procs,
                        uint32_t max_instr, char *buf, uint64_t cap, uint64_t *offsets,
                        uint32_t *lengths, uint64_t *need);

/* ---- device-side text ingest (libdash.so, HIP; csrc/dash_ingest.hip) ---- */
/* Bytes per tile of the device parser (256 lanes x 16 bytes); exported so that tests can
   place features on tile edges. */
#define DASH_TEXT_TILE 4096
/* Parses num_files == num_systems * num_procs trace texts on the device, straight into the
   simulator's layout: file f = sys * num_procs + node is text[offsets[f] .. offsets[f] +
   lengths[f]) (host pointers, any alignment; the slab is copied up to the largest offset +
   length). Rules and results are those of dash_parse_core_text with the handle's num_procs and
   max_instr. On success the handle is loaded exactly as dash_load_traces would have left it
   for the same words. On failure the lowest failing file decides: its DASH_EPARSE or
   DASH_EADDR is returned, dash_last_error names system, node and record, dash_ingest_info
   gives the same as numbers -- and, unlike dash_load_dirs (which parses on the host and
   leaves the device untouched), the handle is then NOT loaded: the device buffer was written
   in place, so dash_run gives DASH_ESTATE until a load succeeds. */
int dash_load_text(dash_t *h, const char *text, const uint64_t *offsets, const uint32_t *lengths,
                   uint64_t num_files);
/* dash_load_dirs with the parse on the device: host threads (at most 16, as dash_load_dirs
   sizes them) only read the files' bytes into two pinned slabs, each holding a whole number of
   files; a slab is copied and parsed while the other is being read. Same results as
   dash_load_dirs on accepted input. Failure as dash_load_text, with DASH_EIO for a file the
   reader could not open; the lowest failing file index wins whichever stage found it. */
int dash_load_dirs_device(dash_t *h, const char *const *dirs, uint64_t n);
/* The inverse of dash_load_traces: lens[sys * num_procs + node], and words [0, len) of every
   row into packed[(sys * num_procs + node) * stride ..] (the rest of a row is zeroed), read
   back from the device layout. stride >= the longest trace, else DASH_EINVAL. */
int dash_read_traces(dash_t *h, uint16_t *packed, uint64_t stride, uint32_t *lens);
/* The last dash_load_text / dash_load_dirs_device call of the handle. rc: its return code;
   for DASH_EIO / DASH_EPARSE / DASH_EADDR, file = the failing file index (system * num_procs +
   node) and record = the failing record, 1-based (0 for DASH_EIO). text_bytes: bytes copied to
   the device. read_ms: host time spent reading files (wall clock of the reader phases);
   copy_ms and parse_ms: H2D copies and the parse kernel, by device events. */
typedef struct dash_ingest_report {
    int32_t rc;
    uint32_t record;
    uint64_t file;
    uint64_t text_bytes;
    double read_ms, copy_ms, parse_ms;
} dash_ingest_report;
int dash_ingest_info(const dash_t *h, dash_ingest_report *out);
/* Bulk emission: one system's printProcessorState files (ref :853-905) into out_dir
   (created if missing; needs DASH_KEEP_STATE), and a text file with one line
   "system digest(hex) rounds errors(hex)" for every system. */
int dash_dump_system(dash_t *h, uint64_t sys, const char *out_dir);
int dash_write_digests(dash_t *h, const char *path);
void dash_init_node_state(dash_node_state *s, uint32_t node_id, uint32_t cache_size);
/* printProcessorState byte-exact (ref :853-905). Returns bytes written, or < 0. */
int dash_dump_node(const dash_node_state *s, uint32_t node_id, uint32_t cache_size, char *buf,
                   size_t cap);
int dash_dump_file(const dash_node_state *s, uint32_t node_id, uint32_t cache_size,
                   const char *path);
uint64_t dash_digest_node(const dash_node_state *s, uint32_t node_id, uint32_t cache_size);
/* The coherence invariants (DASH_COH_*, above) of one system whose states the caller holds, e.g.
   parsed dumps or dash_read_state output: the library's one statement of the rules on the host.
   addr_bits (optional, [num_procs * 16]) gets every address's bits. DASH_EINVAL outside num_procs
   1..8 or cache_size 1..16. */
int dash_check_states(const dash_node_state *nodes, uint32_t num_procs, uint32_t cache_size,
                      dash_coherence *out, uint32_t *addr_bits);
/* The per-address records (dash_addr_metrics, above) of one system whose events the caller holds, e.g.
   what dash_read_events returned: the library's one statement of the rules on the host. Events of
   rounds >= `rounds` are ignored, so `rounds` is the K of the rules; out gets all num_procs * 16
   records, *foreign (optional) the events whose address is num_procs * 16 or more. DASH_EINVAL for
   num_procs outside 1..8, a NULL out, or a NULL ev with n != 0. */
int dash_addr_metrics_from_events(const dash_event *ev, uint64_t n, uint32_t num_procs, uint32_t rounds,
                                  dash_addr_metrics *out /* [num_procs * 16] */, uint64_t *foreign /* or NULL */);
/* One event as the reference prints it: DEBUG_MSG "Processor %d msg from: %d, type: %d,
   address: 0x%02X" (ref :180-181) or DEBUG_INSTR "Processor %d: instr type=%c,
   address=0x%02X, value=%hhu" (ref :650-651), newline included. Returns bytes or < 0. */
int dash_format_event(const dash_event *e, char *buf, size_t cap);
/* main() end to end for one system: parse dir, run on the GPU, write
   core_<n>_output.txt into out_dir (ref :126-739, :860). */
int dash_simulate_dir(const char *dir, uint32_t num_procs, uint32_t cache_size,
                      uint32_t max_instr, const char *out_dir, int device, dash_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
