/*
 * cache_simulator.c -- CLI with the reference's argv contract
 * (/root/reference/assignment.c:126-131): `cache_simulator <test_directory>`
 * reads tests/<dir>/core_<n>.txt (or <dir>/core_<n>.txt), prints
 * "Processor N initialized" per node, simulates on the GPU and writes
 * core_<n>_output.txt (printProcessorState bytes) into the CWD. Unlike the
 * reference it exits 0 at quiescence instead of spinning until killed.
 *
 * Extra options (defaults = the reference's #defines, :6-10):
 *   -n NUM_PROCS (4)  -c CACHE_SIZE (4)  -m MAX_INSTR_NUM (32)
 *   -o OUT_DIR (.)    -d DEVICE (0)      -s  print run statistics to stderr
 *   --debug-instr / --debug-msg  print the reference's DEBUG_INSTR (:650-651) /
 *       DEBUG_MSG (:180-181) lines to stdout, in lockstep order (the reference's
 *       -D DEBUG_INSTR / -D DEBUG_MSG builds, README :104)
 *   --schedule SEED   a seeded legal schedule instead of lowest-sender-first (DESIGN.md §2;
 *       e.g. --schedule 87 lands tests/test_4 on its accepted run_2); also in bulk modes
 *   --rounds FILE     an explicit round schedule (dash_set_schedule): one row per round, one
 *       character per node, '-' = the node sits the round out, else its delivery position;
 *       later rounds are lockstep. FILE is plain rows, or a JSON record of tests/golden/schedules
 *       record (its "rounds" strings): e.g. tests/golden/schedules/test_4_run_3.json makes
 *       `cache_simulator test_4` write the accepted run_3
 *   --micro FILE      a micro-step schedule (dash_set_micro_schedule): whitespace-separated
 *       tokens, one per round, "P<t>" / "I<t>" / "S<t>" = node t steps (pops or issues, its
 *       sends held), "D<t>" = node t delivers its oldest held message; plain text, or the
 *       "steps" string of a JSON record (tests/golden/ref_runs/micro4.json's cases)
 *   --write-rounds FILE  after the run, write the schedule it followed (--schedule SEED, or
 *       lockstep) for the rounds it took as the plain rows --rounds reads, so that
 *       `--rounds FILE` writes the same dumps and the schedule can be read, edited and kept
 *   --metrics         per-node cache and coherence metrics, reduced on the GPU from the run's event
 *       log (dash_compute_metrics; the log is sized to the run): after the dumps are written, one
 *       stdout line per node, "metrics node=<t> instructions= reads= writes= read_misses=
 *       write_misses= upgrades= invalidations= interventions= evictions= evict_shared=
 *       evict_modified= home_requests= waits= wait_mean= wait_max= idle_rounds=" (wait_mean and
 *       wait_max in rounds; include/dash.h defines each count). Goes with --schedule, --rounds,
 *       --micro and --micro-seed; in the bulk modes it prints one "metrics total ..." line
 *   --addr-metrics    the per-address sharing profile, reduced on the GPU from the same log
 *       (dash_compute_addr_metrics); accepted wherever --metrics is, and together with it. After the dumps
 *       (and the --metrics lines), one stdout line per address whose class is not untouched, in ascending
 *       address order: "addr 0x<AA> class=<private|read_shared|one_writer|multi_writer> reads= writes=
 *       read_misses= write_misses= upgrades= invalidations= interventions= flushes= evict_shared=
 *       evict_modified= msgs= readers=0x<BB> writers=0x<BB> invalidated=0x<BB>" (include/dash.h defines
 *       each); in the bulk modes one "addr total ..." line with the totals and the five class counts
 *   --coherence       the coherence invariants of the final state, checked on the GPU
 *       (dash_check_coherence; include/dash.h defines the DASH_COH_* bits): after the dumps, one stdout
 *       line "coherence addrs=<K> bits=0x<BB>", K = addresses that break an invariant, followed by
 *       " first=0x<AA> first_bits=0x<BB>" (the lowest such address and its bits) when K > 0. Goes with
 *       --schedule, --rounds, --micro and --micro-seed; with --explore / --explore-micro every outcome
 *       line gains a sixth column, the outcome's bits in hex (dash_check_outcomes)
 *   --explore K       which outcomes can this directory reach? Runs K seeded legal schedules,
 *       seeds S0 .. S0 + K - 1 (S0 = --schedule, default 0 = lockstep first), in one GPU batch
 *       per 65,536 (dash_explore) and prints one line per distinct final state, "digest(hex)
 *       count seed rounds errors(hex)", ordered by seed = the lowest seed that reached it
 *       (`--schedule <seed>` then writes that state's dumps); writes no dumps, exits 0
 *   --micro-seed S [--weights a,b,..]  one seeded micro-step schedule (dash_set_micro_seeds): each
 *       round one enabled node, picked by seed S and the per-node weights (0..31, default all 1;
 *       a weight-0 node acts only when no other can), delivers one held send or steps
 *   --write-micro FILE  with --micro-seed: after the run, write the schedule it followed as the
 *       tokens --micro reads, so that `--micro FILE` writes the same dumps
 *   --explore-micro K [--weights a,b,..]  --explore over seeded micro-step schedules, seeds S0 ..
 *       S0 + K - 1 (S0 = --micro-seed, default 0) under one weight vector (dash_explore_micro);
 *       same output lines (`--micro-seed <seed> --weights ...` then writes that state's dumps):
 *       e.g. `test_4 --explore-micro 250 --weights 4,0,31,1` lists the accepted run_3
 *   --shrink OUTDIR [--shrink-bits 0xBB]  cut the directory's traces down, on the GPU, to a few instructions
 *       that still end in the same broken state (dash_shrink): per round the largest block of one node's
 *       instructions whose deletion keeps the goal, until no single instruction can go. The goal: the final
 *       state has the coherence bits 0xBB (default: the lowest bit of the directory's own record) and no
 *       error bit the directory's own run does not have; the schedule is lockstep or --schedule S. Prints
 *       one line "shrink node= start= count= candidates=" per round and a last line "shrunk
 *       instr=<before>-><after> rounds= variants= bits=0x..", writes OUTDIR/core_<n>.txt and no dumps; a
 *       coherent directory prints "shrink: nothing to shrink (coherent)" and writes nothing
 *   --shrink OUTDIR --sources FILE   the same for several directories in one call (dash_shrink_many):
 *       <test_directory> is source 0, FILE lists the others; every incoherent one is a job, all jobs are
 *       shrunk side by side, each to where --shrink alone takes it. Prints per job its lines "shrink
 *       source=<i> node= start= count= candidates=" and "shrunk source=<i> instr=a->b rounds= variants=
 *       bits=0x..", writes OUTDIR/<i>/core_<n>.txt, prints "source <i>: nothing to shrink (coherent)" for a
 *       coherent directory and a last line "shrunk sources= minimal= coherent= distinct=" (distinct: the
 *       different minimal trace sets)
 *   --explore K --coherence --shrink OUTDIR   the outcome lines of --explore K --coherence, then one job per
 *       incoherent outcome i of that list: the directory under the outcome's witness seed, with the lowest
 *       bit of the outcome's record as the goal. The same lines with "source=<i> seed=<witness>":
 *       `OUTDIR/<i> --schedule <witness>` replays the reproducer
 *   --sources FILE    with --explore / --explore-micro: several trace directories in one call
 *       (dash_explore_sources). <test_directory> is source 0, FILE lists the others, one per line; K
 *       schedules of every source run side by side in the batch and their outcomes are merged and
 *       classified on the GPU. Prints the outcome lines with a leading source-index column, ordered by
 *       (source, seed) (--coherence adds the same last column), then per source one line "source <i>
 *       <dir> outcomes=<n> schedules=<K> incoherent=<schedules whose final state breaks an invariant>"
 *   --delays t@r+len[,t@r+len..]   lockstep but for up to four delays: node t sits out len rounds (1, 2,
 *       .., 128) from round r (0..1022) on (dash_set_system_delays); "-" is lockstep itself. Writes the
 *       dumps; --debug-instr, --debug-msg, --metrics, --addr-metrics and --coherence work as under --schedule;
 *       e.g. `test_4 --delays 0@0+4,1@2+64`, the witness --explore-delays 2 prints for test_4's accepted
 *       run_4, writes that run's dumps
 *   --explore-delays D [--delay-starts R] [--delay-lens E]   every schedule within D (0..4) delays of
 *       lockstep, start rounds 0 .. R - 1 (default: the rounds of the directory's own lockstep run, at most
 *       1022) and lengths 1 .. 2^(E - 1) (default E = 7), enumerated and merged on the GPU
 *       (dash_explore_delays). Prints the --explore lines, the seed column holding the lowest schedule index
 *       that reached the outcome (a fewest-delays witness; --coherence adds its column), then that
 *       witness's delays as --delays takes them. With --sources FILE as --explore with --sources
 *
 * Bulk modes (one GPU batch, many systems; dumps go to OUT_DIR/<k>/):
 *   --batch LIST        system k = the k-th trace directory listed in LIST (one per line)
 *   --device-ingest     with --batch: parse the trace text on the GPU (dash_load_dirs_device)
 *   --synthetic COUNT   COUNT generated systems: --len L (4096) --kind uniform|contention|
 *                       locality --locality P (0.5) --seed S (0x5EED) --dump K[,K...]
 *   --digests FILE      "system digest rounds errors" for every system
 */
#define _POSIX_C_SOURCE 200809L
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "dash.h"

static const char *txn_names[DASH_NUM_TXN] = {
    "READ_REQUEST", "WRITE_REQUEST", "REPLY_RD", "REPLY_WR", "REPLY_ID", "INV", "UPGRADE",
    "WRITEBACK_INV", "WRITEBACK_INT", "FLUSH", "FLUSH_INVACK", "EVICT_SHARED", "EVICT_MODIFIED"};

/* --rounds FILE: rows of n characters ('-' or a position digit); from a JSON record, the quoted
   strings after its "rounds" key. Returns the row count, or -1 on a malformed file. */
static long read_micro(const char *path, unsigned n, uint8_t **out);

static long read_rounds(const char *path, unsigned n, uint8_t **out) {
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    static char text[1 << 20];
    size_t len = fread(text, 1, sizeof text - 1, f);
    const int more = fgetc(f) != EOF; /* a longer file would be cut: refuse it */
    fclose(f);
    if (more) return -1;
    text[len] = 0;
    const char *p = strstr(text, "\"rounds\"");
    const int json = p != NULL;
    if (!json) p = text;
    else p += 8;
    long rows = 0, cap = 0;
    uint8_t *r = NULL;
    while (*p) {
        const char *q;
        if (json) {  /* next quoted string, up to the array's end */
            while (*p && *p != '"' && *p != ']') p++;
            if (*p != '"') break;
            q = ++p;
            while (*p && *p != '"') p++;
        } else {     /* next non-empty line */
            while (*p == '\n' || *p == '\r' || *p == ' ') p++;
            if (!*p) break;
            q = p;
            while (*p && *p != '\n' && *p != '\r' && *p != ' ') p++;
        }
        if ((unsigned)(p - q) != n) { free(r); return -1; }
        if (rows == cap) {
            cap = cap ? 2 * cap : 64;
            r = (uint8_t *)realloc(r, (size_t)cap * n);
        }
        for (unsigned t = 0; t < n; t++) {
            const char c = q[t];
            if (c == '-') r[rows * n + t] = DASH_SIT_OUT;
            else if (c >= '0' && c <= '7') r[rows * n + t] = (uint8_t)(c - '0');
            else { free(r); return -1; }
        }
        rows++;
        if (*p) p++;
    }
    *out = r;
    return rows;
}

/* --micro FILE: one token per round, [PIS]<t> (a step) or D<t> (a delivery); from a JSON record, the
   string after its "steps" key. Returns the round count, or -1 on a malformed file. */
static long read_micro(const char *path, unsigned n, uint8_t **out) {
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    static char text[1 << 22];
    size_t len = fread(text, 1, sizeof text - 1, f);
    const int more = fgetc(f) != EOF;
    fclose(f);
    if (more) return -1;
    text[len] = 0;
    char *p = strstr(text, "\"steps\"");
    if (p) {
        p = strchr(p + 7, '"');
        if (!p) return -1;
        char *end = strchr(++p, '"');
        if (!end) return -1;
        *end = 0;
    } else {
        p = text;
    }
    long rows = 0, cap = 0;
    uint8_t *r = NULL;
    for (char *tok = strtok(p, " \t\r\n"); tok; tok = strtok(NULL, " \t\r\n")) {
        char *e;
        const long t = strtol(tok + 1, &e, 10);
        if (!strchr("PISD", tok[0]) || e == tok + 1 || *e || t < 0 || t >= (long)n) { free(r); return -1; }
        if (rows == cap) {
            cap = cap ? 2 * cap : 256;
            uint8_t *r2 = (uint8_t *)realloc(r, (size_t)cap * n);
            if (!r2) { free(r); return -1; }
            r = r2;
        }
        memset(r + rows * n, DASH_SIT_OUT, n);
        r[rows * n + t] = tok[0] == 'D' ? DASH_MICRO_SEND : DASH_MICRO_STEP;
        rows++;
    }
    *out = r;
    return rows;
}

/* --weights a,b,..: node t's weight in byte t. Returns 0, or -1 on a malformed list. */
static int parse_weights(const char *text, unsigned n, uint64_t *out) {
    uint64_t w = 0;
    unsigned t = 0;
    for (const char *p = text; *p; t++) {
        char *e;
        const unsigned long v = strtoul(p, &e, 10);
        if (e == p || v > 31 || t >= n || (*e && *e != ',')) return -1;
        w |= (uint64_t)v << (8 * t);
        p = *e ? e + 1 : e;
        if (*e == ',' && !*p) return -1;
    }
    if (t == 0) return -1;
    *out = w;
    return 0;
}

/* --write-micro FILE: the acts of the run under --micro-seed as --micro's tokens, P<t> / I<t> for a
   step by the kind of the event it logged, D<t> for a delivery */
static int write_micro(dash_t *h, const char *path, unsigned n) {
    uint32_t rounds = 0, cap = 0, total = 0;
    int rc = dash_read_micro_acts(h, 0, NULL, 0, &rounds);
    if (rc != DASH_OK && !(rc == DASH_EINVAL && rounds)) return rc;
    uint8_t *acts = (uint8_t *)malloc((size_t)rounds * n + 1);
    dash_event *ev = NULL;
    rc = acts ? dash_read_micro_acts(h, 0, acts, rounds, &rounds) : DASH_ENOMEM;
    if (rc == DASH_OK) rc = dash_read_events(h, 0, NULL, 0, &cap);
    if (rc == DASH_OK && !(ev = (dash_event *)malloc(sizeof *ev * (cap ? cap : 1)))) rc = DASH_ENOMEM;
    if (rc == DASH_OK) rc = dash_read_events(h, 0, ev, cap, &total);
    FILE *f = rc == DASH_OK ? fopen(path, "w") : NULL;
    if (rc == DASH_OK && !f) rc = DASH_EIO;
    uint32_t k = 0;
    for (uint32_t r = 0; f && r < rounds; r++)
        for (unsigned t = 0; t < n; t++) {
            const uint8_t a = acts[(size_t)r * n + t];
            if (a == DASH_SIT_OUT) continue;
            char c = 'D';
            if (a == DASH_MICRO_STEP) {  /* the step's event: one per stepping round, in round order */
                if (k >= total || ev[k].round != r || ev[k].node != t) rc = DASH_EINVAL;
                else c = ev[k].kind == DASH_EV_INSTR ? 'I' : 'P';
                k++;
            }
            if (fprintf(f, "%c%u\n", c, t) < 0) rc = DASH_EIO;
        }
    if (f && fclose(f) != 0) rc = DASH_EIO;
    free(ev);
    free(acts);
    return rc;
}

/* --metrics: the records of `count` systems' nodes, one line per node (count 1), or the totals */
static int print_metrics(dash_t *h, uint64_t count, unsigned n) {
    dash_metrics_totals tot;
    int rc = dash_compute_metrics(h, &tot);
    if (rc != DASH_OK) return rc;
    if (count != 1) {
        printf("metrics total systems=%llu truncated_systems=%llu", (unsigned long long)tot.systems,
               (unsigned long long)tot.truncated_systems);
        static const char *names[16] = {"reads", "writes", "read_misses", "write_misses", "upgrades", "msgs",
                                        "home_requests", "invalidations", "interventions", "evict_shared",
                                        "evict_modified", "waits", "wait_rounds", "wait_max", "deliveries",
                                        "idle_rounds"};
        uint64_t v[16]; /* the 16 fields lead the struct, in dash_node_metrics' order */
        memcpy(v, &tot, sizeof v);
        for (int k = 0; k < 16; k++) printf(" %s=%llu", names[k], (unsigned long long)v[k]);
        printf(" wait_mean=%.2f\n", tot.waits ? (double)tot.wait_rounds / (double)tot.waits : 0.0);
        return DASH_OK;
    }
    dash_node_metrics m[DASH_MAX_PROCS];
    rc = dash_read_metrics(h, 0, 1, m, NULL);
    for (unsigned t = 0; rc == DASH_OK && t < n; t++)
        printf("metrics node=%u instructions=%u reads=%u writes=%u read_misses=%u write_misses=%u upgrades=%u "
               "invalidations=%u interventions=%u evictions=%u evict_shared=%u evict_modified=%u home_requests=%u "
               "waits=%u wait_mean=%.2f wait_max=%u idle_rounds=%u\n",
               t, m[t].reads + m[t].writes, m[t].reads, m[t].writes, m[t].read_misses, m[t].write_misses,
               m[t].upgrades, m[t].invalidations, m[t].interventions, m[t].evict_shared + m[t].evict_modified,
               m[t].evict_shared, m[t].evict_modified, m[t].home_requests, m[t].waits,
               m[t].waits ? (double)m[t].wait_rounds / (double)m[t].waits : 0.0, m[t].wait_max, m[t].idle_rounds);
    return rc;
}

/* --addr-metrics: the one system's touched addresses, one line each (count 1), or the totals */
static int print_addr_metrics(dash_t *h, uint64_t count, unsigned n) {
    static const char *classes[5] = {"untouched", "private", "read_shared", "one_writer", "multi_writer"};
    dash_addr_totals tot;
    int rc = dash_compute_addr_metrics(h, &tot);
    if (rc != DASH_OK) return rc;
    if (count != 1) {
        printf("addr total systems=%llu truncated_systems=%llu", (unsigned long long)tot.systems,
               (unsigned long long)tot.truncated_systems);
        static const char *names[13] = {"reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations",
                                        "interventions", "flushes", "evict_shared", "evict_modified", "msgs",
                                        "msgs_max", "foreign_events"};
        uint64_t v[13]; /* these 13 fields lead the struct */
        memcpy(v, &tot, sizeof v);
        for (int k = 0; k < 13; k++) printf(" %s=%llu", names[k], (unsigned long long)v[k]);
        for (int k = 0; k < 5; k++) printf(" %s=%llu", classes[k], (unsigned long long)tot.class_addrs[k]);
        printf("\n");
        return DASH_OK;
    }
    dash_addr_metrics m[DASH_MAX_PROCS * DASH_MEM_SIZE];
    rc = dash_read_addr_metrics(h, 0, 1, m, NULL);
    for (unsigned a = 0; rc == DASH_OK && a < n * DASH_MEM_SIZE; a++) {
        const int c = dash_addr_class(&m[a]);
        if (c == DASH_ADDR_UNTOUCHED) continue;
        printf("addr 0x%02X class=%s reads=%u writes=%u read_misses=%u write_misses=%u upgrades=%u invalidations=%u "
               "interventions=%u flushes=%u evict_shared=%u evict_modified=%u msgs=%u readers=0x%02X writers=0x%02X "
               "invalidated=0x%02X\n",
               a, classes[c], m[a].reads, m[a].writes, m[a].read_misses, m[a].write_misses, m[a].upgrades,
               m[a].invalidations, m[a].interventions, m[a].flushes, m[a].evict_shared, m[a].evict_modified, m[a].msgs,
               m[a].nodes & 0xFFu, (m[a].nodes >> 8) & 0xFFu, (m[a].nodes >> 16) & 0xFFu);
    }
    return rc;
}

/* --coherence: the one system's record as a line */
static int print_coherence(dash_t *h) {
    dash_coherence c;
    int rc = dash_check_coherence(h, NULL);
    if (rc == DASH_OK) rc = dash_read_coherence(h, 0, 1, &c);
    if (rc != DASH_OK) return rc;
    printf("coherence addrs=%u bits=0x%X", c.addrs, c.bits);
    if (c.addrs) printf(" first=0x%02X first_bits=0x%X", c.first_addr, c.first_bits);
    printf("\n");
    return DASH_OK;
}

/* dash_simulate_dir plus a schedule (seed, explicit rounds, micro-steps, a micro seed with its
   weights, or a delay word) and the event log of the one system */
static int simulate_traced(const char *dir, unsigned n, unsigned cs, unsigned m, const char *out, int dev,
                           int dbg_instr, int dbg_msg, unsigned long long sched, const uint8_t *rounds,
                           long nrounds, int micro, const uint64_t *mseed, uint64_t weights,
                           const char *write_micro_file, int metrics, int addr_metrics, int coherence,
                           const uint64_t *delays, dash_stats *st) {
    dash_cfg cfg = {0};
    cfg.num_procs = n;
    cfg.cache_size = cs;
    cfg.max_instr = m;
    cfg.flags = DASH_KEEP_STATE;
    cfg.num_systems = 1;
    cfg.device = dev;
    /* the log holds every round the run may take (the default round cap, 1024 + 256 x max_instr,
       up to 2^22): n x 4 B per round on the device */
    uint64_t log_rounds = 1024u + 256ull * m;
    if (log_rounds > (1u << 22)) log_rounds = 1u << 22;
    cfg.trace_events = (dbg_instr || dbg_msg || write_micro_file || metrics || addr_metrics) ? (uint32_t)log_rounds : 0;
    cfg.schedule_seed = (rounds || mseed || delays) ? (sched ? sched : 1) : sched;
    dash_t *h = NULL;
    int rc = dash_create(&cfg, &h);
    if (rc != DASH_OK) return rc;
    if (rounds) rc = micro ? dash_set_micro_schedule(h, rounds, (uint32_t)nrounds)
                           : dash_set_schedule(h, rounds, (uint32_t)nrounds);
    if (mseed) rc = dash_set_micro_seeds(h, mseed, &weights, 1);
    if (delays) rc = dash_set_system_delays(h, delays, 1);
    if (rc == DASH_OK && (rc = dash_load_dir(h, dir, 0)) == DASH_OK && (rc = dash_run(h, st)) == DASH_OK) {
        dash_node_state nodes[DASH_MAX_PROCS];
        rc = dash_read_state(h, 0, nodes);
        for (unsigned t = 0; rc == DASH_OK && t < n; t++) {
            char path[4200];
            snprintf(path, sizeof path, "%s/core_%u_output.txt", out, t);
            rc = dash_dump_file(&nodes[t], t, cs, path);
        }
        uint32_t cap = 0, total = 0;
        dash_event *ev = NULL;
        if (rc == DASH_OK && write_micro_file) rc = write_micro(h, write_micro_file, n);
        if (rc == DASH_OK && (dbg_instr || dbg_msg)) {  /* the count first, then the events */
            int erc = dash_read_events(h, 0, NULL, 0, &cap);
            if (erc == DASH_OK || erc == DASH_ETRUNC)
                ev = (dash_event *)malloc(sizeof(dash_event) * (cap ? cap : 1));
            if (!ev) rc = (erc == DASH_OK || erc == DASH_ETRUNC) ? DASH_ENOMEM : erc;
        }
        if (rc == DASH_OK && ev) {
            int erc = dash_read_events(h, 0, ev, cap, &total);
            for (uint32_t k = 0; k < total && k < cap; k++) {
                char line[128];
                if ((ev[k].kind == DASH_EV_INSTR && dbg_instr) || (ev[k].kind == DASH_EV_MSG && dbg_msg))
                    if (dash_format_event(&ev[k], line, sizeof line) > 0) fputs(line, stdout);
            }
            if (erc != DASH_OK) rc = erc;
        }
        free(ev);
        if (rc == DASH_OK && metrics) rc = print_metrics(h, 1, n);
        if (rc == DASH_OK && addr_metrics) rc = print_addr_metrics(h, 1, n);
        if (rc == DASH_OK && coherence) rc = print_coherence(h);
    }
    if (rc != DASH_OK) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    return rc;
}

/* --write-rounds FILE: `rounds` rounds of seed `sched`'s schedule, one row of n characters per round */
static int write_rounds(const char *path, unsigned long long sched, unsigned n, uint32_t rounds) {
    uint8_t *tab = (uint8_t *)malloc((size_t)rounds * n + 1);
    if (!tab) return DASH_ENOMEM;
    int rc = dash_seed_schedule(sched, n, rounds, tab);
    FILE *f = rc == DASH_OK ? fopen(path, "w") : NULL;
    if (rc == DASH_OK && !f) rc = DASH_EIO;
    for (uint32_t r = 0; f && r < rounds; r++) {
        char row[DASH_MAX_PROCS + 2];
        for (unsigned t = 0; t < n; t++) {
            const uint8_t v = tab[(size_t)r * n + t];
            row[t] = v == DASH_SIT_OUT ? '-' : (char)('0' + v);
        }
        row[n] = '\n';
        if (fwrite(row, 1, n + 1, f) != n + 1) rc = DASH_EIO;
    }
    if (f && fclose(f) != 0) rc = DASH_EIO;
    free(tab);
    return rc;
}

/* The batch of a search call (--explore, --shrink): only the sources' rows are filled on the host, the
   call writes the other systems on the device. */
typedef struct {
    uint16_t *tr;   /* [nsys][n][stride], zero but for the sources */
    uint32_t *lens; /* [nsys][n] */
    size_t stride;
    uint64_t nsys;
} batch;

static void batch_free(batch *b) {
    free(b->tr);
    free(b->lens);
}

/* The trace sets of dirs[0 .. g) as systems 0 .. g-1 of a batch of g systems; a directory that cannot be
   resolved is named on stderr. */
static int batch_parse(batch *b, const char *const *dirs, size_t g, unsigned n, unsigned m) {
    char base[4096], path[4200];
    int rc = DASH_OK;
    b->stride = m ? m : 1;
    b->nsys = g;
    for (size_t s = 0; rc == DASH_OK && s < g; s++) {
        rc = dash_resolve_dir(dirs[s], base, sizeof base);
        if (rc != DASH_OK || n < 1 || n > DASH_MAX_PROCS) {
            fprintf(stderr, "Error: could not open %s/core_0.txt\n", base);
            return rc != DASH_OK ? rc : DASH_EINVAL;
        }
        if (!b->tr) {
            b->tr = (uint16_t *)calloc(g * n * b->stride, sizeof *b->tr);
            b->lens = (uint32_t *)calloc(g * n, sizeof *b->lens);
            if (!b->tr || !b->lens) return DASH_ENOMEM;
        }
        for (unsigned t = 0; rc == DASH_OK && t < n; t++) {
            snprintf(path, sizeof path, "%s/core_%u.txt", base, t);
            rc = dash_parse_core_file(path, n, m, b->tr + (s * n + t) * b->stride, &b->lens[s * n + t]);
        }
    }
    return rc;
}

/* The batch grown to `want` systems, of at most 65,536 and of fewer where its zeroed rows would pass
   64 MB, but never below its sources: the new systems are empty. */
static int batch_grow(batch *b, uint64_t want, unsigned n) {
    const size_t row = (size_t)n * b->stride;
    const uint64_t g = b->nsys;
    uint64_t nsys = want < 65536 ? want : 65536;
    if (nsys > (64u << 20) / (row * 2)) nsys = (64u << 20) / (row * 2);
    if (nsys < g) nsys = g;
    uint16_t *tr = (uint16_t *)realloc(b->tr, nsys * row * sizeof *tr);
    if (tr) b->tr = tr;
    uint32_t *lens = (uint32_t *)realloc(b->lens, nsys * n * sizeof *lens);
    if (lens) b->lens = lens;
    if (!tr || !lens) return DASH_ENOMEM;
    memset(tr + g * row, 0, (nsys - g) * row * sizeof *tr);
    memset(lens + g * n, 0, (nsys - g) * n * sizeof *lens);
    b->nsys = nsys;
    return DASH_OK;
}

/* a handle of the batch's size, loaded with it; *h stays NULL where it could not be created */
static int batch_handle(const batch *b, unsigned n, unsigned cs, unsigned m, int dev, unsigned long long sched,
                        uint32_t flags, dash_t **h) {
    dash_cfg cfg = {0};
    cfg.num_procs = n;
    cfg.cache_size = cs;
    cfg.max_instr = m;
    cfg.num_systems = b->nsys;
    cfg.device = dev;
    cfg.schedule_seed = sched;
    cfg.flags = flags;
    const int rc = dash_create(&cfg, h);
    return rc == DASH_OK ? dash_load_traces(*h, b->tr, b->stride, b->lens, b->nsys) : rc;
}

/* rc = CALL, which fills o[0 .. cap) and sets total, with room for `cap` entries and, in the rare case
   that there are more, once more with room for all of them */
#define CALL_WITH_ROOM(rc, o, cap, total, CALL)            \
    for (int again_ = 0; again_ < 2; again_++) {           \
        free(o);                                           \
        (o) = malloc((size_t)(cap) * sizeof *(o));         \
        (rc) = (o) ? (CALL) : DASH_ENOMEM;                 \
        if ((rc) != DASH_OK || (total) <= (cap)) break;    \
        (cap) = (total);                                   \
    }

/* --explore K / --explore-micro K (weights != NULL): the distinct outcomes of K seeded schedules of one
   trace directory */
static int explore_dir(const char *dir, unsigned n, unsigned cs, unsigned m, int dev, unsigned long long k,
                       unsigned long long s0, const uint64_t *weights, int coherence) {
    batch b = {0};
    dash_t *h = NULL;
    /* one batch holds up to 65,536 schedules; any seeded handle: every system gets a seed of its own; with
       --coherence the final states stay on the device for the check */
    int rc = batch_parse(&b, (const char *const *)&dir, 1, n, m);
    if (rc == DASH_OK) rc = batch_grow(&b, k ? k : 1, n);
    if (rc == DASH_OK) rc = batch_handle(&b, n, cs, m, dev, 1, coherence ? DASH_KEEP_STATE : 0, &h);
    if (rc == DASH_OK) {
        uint32_t total = 0, cap = 256;
        dash_outcome *o = NULL;
        CALL_WITH_ROOM(rc, o, cap, total,
                       weights ? dash_explore_micro(h, 0, s0, k, *weights, o, cap, &total)
                               : dash_explore(h, 0, s0, k, o, cap, &total));
        dash_coherence *c = NULL;
        if (rc == DASH_OK && coherence) {
            c = (dash_coherence *)malloc((total ? total : 1) * sizeof *c);
            rc = c ? dash_check_outcomes(h, 0, o, total, weights, c) : DASH_ENOMEM;
        }
        for (uint32_t i = 0; rc == DASH_OK && i < total && i < cap; i++) {
            printf("%016llx %llu %llu %u %x", (unsigned long long)o[i].digest, (unsigned long long)o[i].count,
                   (unsigned long long)o[i].seed, o[i].rounds, o[i].errors);
            if (c) printf(" %x", c[i].bits);
            printf("\n");
        }
        free(c);
        free(o);
    }
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    batch_free(&b);
    return rc;
}

/* --shrink OUTDIR: the directory's trace set cut down on the GPU (dash_shrink) to a 1-minimal one whose
   final state still has the coherence bits `bits` (0: the lowest bit of the source's own record) and no
   error bit the source does not have; written to OUTDIR as core_<n>.txt */
static int shrink_dir(const char *dir, unsigned n, unsigned cs, unsigned m, int dev, unsigned long long sched,
                      uint32_t bits, const char *out_dir) {
    batch b = {0};
    dash_t *h = NULL;
    uint64_t instr = 0;
    int rc = batch_parse(&b, (const char *const *)&dir, 1, n, m);
    if (rc == DASH_OK) { /* one system per candidate of the first round */
        const int C = dash_shrink_candidate(b.lens, n, 0, NULL, NULL, NULL);
        for (unsigned t = 0; t < n; t++) instr += b.lens[t];
        rc = batch_grow(&b, C > 0 ? (uint64_t)C : 1, n);
    }
    uint16_t *min_tr = (uint16_t *)calloc((size_t)n * b.stride, sizeof *min_tr); /* the result */
    uint32_t min_lens[DASH_MAX_PROCS] = {0};
    dash_shrink_step *steps = (dash_shrink_step *)malloc((instr ? instr : 1) * sizeof *steps);
    if (rc == DASH_OK && (!min_tr || !steps)) rc = DASH_ENOMEM;
    dash_coherence c = {0};
    uint32_t errors = 0, rounds = 0;
    if (rc == DASH_OK && (rc = batch_handle(&b, n, cs, m, dev, sched, DASH_KEEP_STATE, &h)) == DASH_OK &&
        (rc = dash_run(h, NULL)) == DASH_OK && (rc = dash_check_coherence(h, NULL)) == DASH_OK &&
        (rc = dash_read_coherence(h, 0, 1, &c)) == DASH_OK)
        rc = dash_read_results(h, 0, 1, NULL, NULL, &errors);
    if (rc == DASH_OK && c.bits == 0 && bits == 0) {
        printf("shrink: nothing to shrink (coherent)\n");
    } else if (rc == DASH_OK) {
        dash_shrink_goal goal = {bits ? bits : c.bits & (0u - c.bits), 0, ~errors, 0};
        dash_shrink_report rep;
        rc = dash_shrink(h, 0, sched, &goal, min_tr, b.stride, min_lens, steps, (uint32_t)instr, &rounds, &rep);
        if (rc == DASH_OK) rc = dash_write_dir(min_tr, b.stride, min_lens, n, out_dir);
        if (rc == DASH_OK) {
            for (uint32_t r = 0; r < rounds; r++)
                printf("shrink node=%u start=%u count=%u candidates=%u\n", steps[r].node, steps[r].start,
                       steps[r].count, steps[r].candidates);
            printf("shrunk instr=%llu->%llu rounds=%llu variants=%llu bits=0x%X\n",
                   (unsigned long long)rep.instr_before, (unsigned long long)rep.instr_after,
                   (unsigned long long)rep.rounds, (unsigned long long)rep.variants, goal.coh_all);
        } else if (rc == DASH_EIO) {
            fprintf(stderr, "cache_simulator: could not write %s\n", out_dir);
        }
    }
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    free(steps);
    free(min_tr);
    batch_free(&b);
    return rc;
}

/* dir, then the directories that the file `list` names, one per line: (*dirs)[0 .. *g), each the caller's to
   free; what could not be read is named on stderr */
static int dir_list_read(const char *dir, const char *list, unsigned n, char ***dirs_out, size_t *g_out) {
    FILE *f = fopen(list, "r");
    if (!f || n < 1 || n > DASH_MAX_PROCS) {
        fprintf(stderr, "Error: could not open %s\n", list);
        if (f) fclose(f);
        return f ? DASH_EINVAL : DASH_EIO;
    }
    size_t g = 1, gcap = 16;
    char **dirs = (char **)malloc(gcap * sizeof *dirs), line[4096];
    int rc = dirs ? DASH_OK : DASH_ENOMEM;
    if (dirs) dirs[0] = strdup(dir);
    while (rc == DASH_OK && fgets(line, sizeof line, f)) {
        line[strcspn(line, "\r\n")] = 0;
        if (!line[0]) continue;
        if (g == gcap) {
            char **grown = (char **)realloc(dirs, (gcap *= 2) * sizeof *dirs);
            if (!grown) rc = DASH_ENOMEM;
            else dirs = grown;
        }
        if (rc == DASH_OK && !(dirs[g++] = strdup(line))) rc = DASH_ENOMEM;
    }
    fclose(f);
    *dirs_out = dirs;
    *g_out = dirs ? g : 0;
    return rc;
}

static void dir_list_free(char **dirs, size_t g) {
    for (size_t s = 0; dirs && s < g; s++) free(dirs[s]);
    free(dirs);
}

/* --explore K / --explore-micro K with --sources FILE: the outcomes of several trace directories in one
   call (dash_explore_sources). dir is source 0; FILE lists the others, one per line. */
static int explore_sources_dirs(const char *dir, const char *list, unsigned n, unsigned cs, unsigned m, int dev,
                                unsigned long long k, unsigned long long s0, const uint64_t *weights, int coherence) {
    char **dirs = NULL;
    size_t g = 0;
    int rc = dir_list_read(dir, list, n, &dirs, &g);
    if (!dirs) return rc;
    /* a handle of up to 65,536 systems, at least one per source; any seeded handle: every system gets a
       seed of its own; the outcomes are classified from the final states of the passes */
    batch b = {0};
    dash_t *h = NULL;
    if (rc == DASH_OK) rc = batch_parse(&b, (const char *const *)dirs, g, n, m);
    if (rc == DASH_OK) rc = batch_grow(&b, k && g * k < 65536 ? g * k : 65536, n);
    if (rc == DASH_OK) rc = batch_handle(&b, n, cs, m, dev, 1, DASH_KEEP_STATE, &h);
    if (rc == DASH_OK) {
        uint64_t total = 0, cap = 4096;
        dash_outcome_ex *o = NULL;
        dash_source_summary *per = (dash_source_summary *)calloc(g, sizeof *per);
        CALL_WITH_ROOM(rc, o, cap, total,
                       per ? dash_explore_sources(h, g, s0, k, weights, 0, o, cap, &total, per, NULL) : DASH_ENOMEM);
        for (uint64_t i = 0; rc == DASH_OK && i < total && i < cap; i++) {
            printf("%u %016llx %llu %llu %u %x", o[i].source, (unsigned long long)o[i].o.digest,
                   (unsigned long long)o[i].o.count, (unsigned long long)o[i].o.seed, o[i].o.rounds, o[i].o.errors);
            if (coherence) printf(" %x", o[i].coh.bits);
            printf("\n");
        }
        for (size_t s = 0; rc == DASH_OK && s < g; s++)
            printf("source %zu %s outcomes=%u schedules=%llu incoherent=%llu\n", s, dirs[s], per[s].outcomes,
                   (unsigned long long)per[s].schedules, (unsigned long long)per[s].incoherent_schedules);
        free(per);
        free(o);
    }
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    batch_free(&b);
    dir_list_free(dirs, g);
    return rc;
}

/* --delays SPEC: t@r+len[,t@r+len..], up to four delays "node t sits out len rounds from round r on" (len
   a power of two up to 128, r up to 1022), or "-" for none, as a delay word (dash_set_system_delays) */
static int parse_delays(const char *text, uint64_t *word) {
    *word = DASH_DELAY_LOCKSTEP;
    if (!strcmp(text, "-")) return 0;
    for (unsigned s = 0; s < 4; s++) {
        unsigned t, r, len, e = 0;
        int used = 0;
        if (sscanf(text, "%u@%u+%u%n", &t, &r, &len, &used) != 3 || t >= DASH_MAX_PROCS || r > 1022u) return -1;
        while (e < 7 && (1u << e) < len) e++;
        if (len != 1u << e) return -1;
        *word = (*word & ~(0xFFFFull << (16 * s))) | (uint64_t)DASH_DELAY(t, e, r) << (16 * s);
        text += used;
        if (!*text) return 0;
        if (*text++ != ',') return -1;
    }
    return -1; /* a fifth delay */
}

/* a delay word in --delays' own spelling */
static void print_delays(uint64_t word) {
    int any = 0;
    for (unsigned s = 0; s < 4; s++) {
        const unsigned f = (unsigned)(word >> (16 * s)) & 0xFFFFu;
        if (f == DASH_DELAY_EMPTY) continue;
        printf("%s%u@%u+%u", any ? "," : "", f & 7u, f >> 6, 1u << ((f >> 3) & 7u));
        any = 1;
    }
    if (!any) printf("-");
}

/* --explore-delays D: the outcomes of every schedule within D delays of lockstep (dash_explore_delays) of
   dir and, with --sources FILE, of the directories FILE lists. starts == 0: the rounds of dir's own lockstep
   run, at most 1022. One line per outcome as --explore prints it (--sources: as with --sources), the seed
   column being the witness's schedule index, then the witness's delays as --delays takes them. */
static int explore_delays_dirs(const char *dir, const char *list, unsigned n, unsigned cs, unsigned m, int dev,
                               unsigned max_delays, unsigned starts, unsigned lens, int coherence) {
    char **dirs = NULL;
    size_t g = 1;
    int rc = DASH_OK;
    if (list) rc = dir_list_read(dir, list, n, &dirs, &g);
    if (list && !dirs) return rc;
    const char *const *names = list ? (const char *const *)dirs : &dir;
    batch b = {0};
    dash_t *h = NULL;
    dash_delay_space space = {starts, lens, max_delays, 0};
    uint64_t K = 0;
    if (rc == DASH_OK) rc = batch_parse(&b, names, g, n, m);
    if (rc == DASH_OK && !starts) { /* the lockstep run of dir alone */
        uint32_t rounds = 0;
        const uint64_t none = DASH_DELAY_LOCKSTEP;
        batch one = b;
        one.nsys = 1;
        if ((rc = batch_handle(&one, n, cs, m, dev, 1, 0, &h)) == DASH_OK &&
            (rc = dash_set_system_delays(h, &none, 1)) == DASH_OK && (rc = dash_run(h, NULL)) == DASH_OK)
            rc = dash_read_results(h, 0, 1, NULL, &rounds, NULL);
        if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
        dash_destroy(h);
        h = NULL;
        space.starts = rounds < 1 ? 1 : rounds > 1022 ? 1022 : rounds;
    }
    if (rc == DASH_OK && (rc = dash_delay_count(&space, n, &K)) != DASH_OK)
        fprintf(stderr, "cache_simulator: --explore-delays: D 0..4, --delay-starts 1..1023, --delay-lens 1..8\n");
    if (rc == DASH_OK) rc = batch_grow(&b, K < 65536 / g ? g * K : 65536, n);
    if (rc == DASH_OK) rc = batch_handle(&b, n, cs, m, dev, 1, DASH_KEEP_STATE, &h);
    if (rc == DASH_OK) {
        uint64_t total = 0, cap = 4096;
        dash_outcome_ex *o = NULL;
        dash_source_summary *per = (dash_source_summary *)calloc(g, sizeof *per);
        CALL_WITH_ROOM(rc, o, cap, total,
                       per ? dash_explore_delays(h, g, &space, 0, o, cap, &total, per, NULL) : DASH_ENOMEM);
        for (uint64_t i = 0; rc == DASH_OK && i < total && i < cap; i++) {
            uint64_t word = DASH_DELAY_LOCKSTEP;
            rc = dash_delay_word(&space, n, o[i].o.seed, &word);
            if (list) printf("%u ", o[i].source);
            printf("%016llx %llu %llu %u %x", (unsigned long long)o[i].o.digest, (unsigned long long)o[i].o.count,
                   (unsigned long long)o[i].o.seed, o[i].o.rounds, o[i].o.errors);
            if (coherence) printf(" %x", o[i].coh.bits);
            printf(" ");
            print_delays(word);
            printf("\n");
        }
        for (size_t s = 0; list && rc == DASH_OK && s < g; s++)
            printf("source %zu %s outcomes=%u schedules=%llu incoherent=%llu\n", s, names[s], per[s].outcomes,
                   (unsigned long long)per[s].schedules, (unsigned long long)per[s].incoherent_schedules);
        free(per);
        free(o);
    }
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    batch_free(&b);
    dir_list_free(dirs, list ? g : 0);
    return rc;
}

/* what shrink_jobs_out compares: the jobs' final sets, as dash_shrink_many returned them */
static struct {
    const uint16_t *tr;
    const uint32_t *lens;
    size_t row, n;
} set_cmp_ctx;

static int set_cmp(const void *a, const void *b) {
    const size_t i = *(const size_t *)a, j = *(const size_t *)b;
    const int c = memcmp(set_cmp_ctx.lens + i * set_cmp_ctx.n, set_cmp_ctx.lens + j * set_cmp_ctx.n,
                         set_cmp_ctx.n * sizeof *set_cmp_ctx.lens);
    return c ? c : memcmp(set_cmp_ctx.tr + i * set_cmp_ctx.row, set_cmp_ctx.tr + j * set_cmp_ctx.row,
                          set_cmp_ctx.row * sizeof *set_cmp_ctx.tr);
}

/* The jobs shrunk side by side (dash_shrink_many) on a loaded handle: job j is shown as source label[j]
   (with its seed when with_seed) and its minimal set goes to out_dir/<label[j]>/core_<n>.txt. Prints the
   jobs' "shrink" and "shrunk" lines and the closing line over `sources` sources, `coherent` of which gave
   no job. `stride` holds the longest source trace. */
static int shrink_jobs_out(dash_t *h, const dash_shrink_job *jobs, const uint64_t *label, size_t J, unsigned n,
                           size_t stride, uint64_t max_instr, int with_seed, size_t sources, size_t coherent,
                           const char *out_dir) {
    /* a job has at most as many winners as its source has instructions; the logs together stay below 256 MB */
    uint64_t cap = max_instr ? max_instr : 1;
    if (J && cap > (256u << 20) / (J * sizeof(dash_shrink_step))) cap = (256u << 20) / (J * sizeof(dash_shrink_step));
    uint16_t *tr = (uint16_t *)calloc((J ? J : 1) * n * stride, sizeof *tr);
    uint32_t *lens = (uint32_t *)calloc((J ? J : 1) * n, sizeof *lens);
    dash_shrink_step *steps = (dash_shrink_step *)malloc((J ? J : 1) * cap * sizeof *steps);
    dash_shrink_result *res = (dash_shrink_result *)calloc(J ? J : 1, sizeof *res);
    size_t *order = (size_t *)malloc((J ? J : 1) * sizeof *order);
    dash_shrink_many_report rep = {0};
    int rc = tr && lens && steps && res && order ? DASH_OK : DASH_ENOMEM;
    if (rc == DASH_OK && J) rc = dash_shrink_many(h, jobs, J, tr, stride, lens, steps, (uint32_t)cap, res, &rep);
    if (rc == DASH_OK && J && mkdir(out_dir, 0755) != 0 && errno != EEXIST) rc = DASH_EIO;
    size_t minimal = 0, distinct = 0;
    for (size_t j = 0; rc == DASH_OK && j < J; j++) {
        char seed[40] = "", sub[4200];
        if (with_seed) snprintf(seed, sizeof seed, " seed=%llu", (unsigned long long)jobs[j].seed);
        if (res[j].status != DASH_SHRINK_MINIMAL) {
            printf("source %llu:%s does not meet the goal (bits 0x%X errors 0x%X)\n", (unsigned long long)label[j], seed,
                   res[j].src_coh_bits, res[j].src_errors);
            continue;
        }
        for (uint32_t r = 0; r < res[j].rounds && r < cap; r++) {
            const dash_shrink_step *st = &steps[j * cap + r];
            printf("shrink source=%llu%s node=%u start=%u count=%u candidates=%u\n", (unsigned long long)label[j], seed,
                   st->node, st->start, st->count, st->candidates);
        }
        printf("shrunk source=%llu%s instr=%u->%u rounds=%u variants=%llu bits=0x%X\n", (unsigned long long)label[j], seed,
               res[j].instr_before, res[j].instr_after, res[j].rounds, (unsigned long long)res[j].variants,
               jobs[j].goal.coh_all);
        snprintf(sub, sizeof sub, "%s/%llu", out_dir, (unsigned long long)label[j]);
        rc = dash_write_dir(tr + j * n * stride, stride, lens + j * n, n, sub);
        order[minimal++] = j;
    }
    if (rc == DASH_OK) { /* the different minimal sets: lengths and words */
        set_cmp_ctx.tr = tr;
        set_cmp_ctx.lens = lens;
        set_cmp_ctx.row = n * stride;
        set_cmp_ctx.n = n;
        qsort(order, minimal, sizeof *order, set_cmp);
        for (size_t i = 0; i < minimal; i++) distinct += i == 0 || set_cmp(&order[i - 1], &order[i]) != 0;
        printf("shrunk sources=%zu minimal=%zu coherent=%zu distinct=%zu\n", sources, minimal, coherent, distinct);
    } else if (rc == DASH_EIO) {
        fprintf(stderr, "cache_simulator: could not write %s\n", out_dir);
    }
    free(order);
    free(res);
    free(steps);
    free(lens);
    free(tr);
    return rc;
}

/* the candidates of the first round over systems [0, g) of a batch, and their longest set in instructions */
static uint64_t batch_candidates(const batch *b, size_t g, unsigned n, uint64_t *max_instr) {
    uint64_t total = 0;
    *max_instr = 0;
    for (size_t s = 0; s < g; s++) {
        uint64_t instr = 0;
        const int C = dash_shrink_candidate(b->lens + s * n, n, 0, NULL, NULL, NULL);
        for (unsigned t = 0; t < n; t++) instr += b->lens[s * n + t];
        if (instr > *max_instr) *max_instr = instr;
        total += C > 0 ? (uint64_t)C : 0;
    }
    return total;
}

/* --shrink OUTDIR --sources FILE: one job per incoherent directory, dir first, then those FILE lists, all
   shrunk side by side (dash_shrink_many) under the goal shrink_dir gives a single directory */
static int shrink_sources_dirs(const char *dir, const char *list, unsigned n, unsigned cs, unsigned m, int dev,
                               unsigned long long sched, uint32_t bits, const char *out_dir) {
    char **dirs = NULL;
    size_t g = 0, J = 0;
    int rc = dir_list_read(dir, list, n, &dirs, &g);
    if (!dirs) return rc;
    batch b = {0};
    dash_t *h = NULL;
    uint64_t max_instr = 0;
    if (rc == DASH_OK) rc = batch_parse(&b, (const char *const *)dirs, g, n, m);
    if (rc == DASH_OK) { /* one system per candidate of the first round, over all directories */
        const uint64_t C = batch_candidates(&b, g, n, &max_instr);
        rc = batch_grow(&b, C > g ? C : g, n);
    }
    dash_coherence *c = (dash_coherence *)calloc(g, sizeof *c);
    uint32_t *errors = (uint32_t *)calloc(g, sizeof *errors);
    dash_shrink_job *jobs = (dash_shrink_job *)calloc(g, sizeof *jobs);
    uint64_t *label = (uint64_t *)calloc(g, sizeof *label);
    if (rc == DASH_OK && (!c || !errors || !jobs || !label)) rc = DASH_ENOMEM;
    /* every directory's own record under the schedule */
    if (rc == DASH_OK && (rc = batch_handle(&b, n, cs, m, dev, sched, DASH_KEEP_STATE, &h)) == DASH_OK &&
        (rc = dash_run(h, NULL)) == DASH_OK && (rc = dash_check_coherence(h, NULL)) == DASH_OK &&
        (rc = dash_read_coherence(h, 0, g, c)) == DASH_OK)
        rc = dash_read_results(h, 0, g, NULL, NULL, errors);
    for (size_t s = 0; rc == DASH_OK && s < g; s++) {
        if (c[s].bits == 0 && bits == 0) {
            printf("source %zu: nothing to shrink (coherent)\n", s);
            continue;
        }
        const dash_shrink_job job = {s, sched, {bits ? bits : c[s].bits & (0u - c[s].bits), 0, ~errors[s], 0}};
        label[J] = s;
        jobs[J++] = job;
    }
    if (rc == DASH_OK) rc = shrink_jobs_out(h, jobs, label, J, n, b.stride, max_instr, 0, g, g - J, out_dir);
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    free(label);
    free(jobs);
    free(errors);
    free(c);
    batch_free(&b);
    dir_list_free(dirs, g);
    return rc;
}

/* --explore K --coherence --shrink OUTDIR: the outcomes of K seeded round schedules of one directory, as
   --explore --coherence prints them, then one job per incoherent outcome: the directory under the outcome's
   witness seed, shrunk side by side (dash_shrink_many) with the lowest bit of the outcome's record as the
   goal and no error bit the outcome does not have. Job i is outcome i of the list. */
static int explore_shrink_dir(const char *dir, unsigned n, unsigned cs, unsigned m, int dev, unsigned long long k,
                              unsigned long long s0, const char *out_dir) {
    batch b = {0};
    dash_t *h = NULL;
    uint64_t max_instr = 0;
    int rc = batch_parse(&b, (const char *const *)&dir, 1, n, m);
    if (rc == DASH_OK) { /* a system per schedule and per candidate of the first round, whichever is more */
        const uint64_t C = batch_candidates(&b, 1, n, &max_instr);
        rc = batch_grow(&b, C > k ? C : (k ? k : 1), n);
    }
    if (rc == DASH_OK) rc = batch_handle(&b, n, cs, m, dev, 1, DASH_KEEP_STATE, &h);
    if (rc == DASH_OK) {
        uint32_t total = 0, cap = 256;
        dash_outcome *o = NULL;
        CALL_WITH_ROOM(rc, o, cap, total, dash_explore(h, 0, s0, k, o, cap, &total));
        dash_coherence *c = (dash_coherence *)malloc((total ? total : 1) * sizeof *c);
        dash_shrink_job *jobs = (dash_shrink_job *)calloc(total ? total : 1, sizeof *jobs);
        uint64_t *label = (uint64_t *)calloc(total ? total : 1, sizeof *label);
        if (rc == DASH_OK) rc = c && jobs && label ? dash_check_outcomes(h, 0, o, total, NULL, c) : DASH_ENOMEM;
        size_t J = 0;
        for (uint32_t i = 0; rc == DASH_OK && i < total; i++) {
            printf("%016llx %llu %llu %u %x %x\n", (unsigned long long)o[i].digest, (unsigned long long)o[i].count,
                   (unsigned long long)o[i].seed, o[i].rounds, o[i].errors, c[i].bits);
            if (c[i].bits == 0) continue;
            const dash_shrink_job job = {0, o[i].seed, {c[i].bits & (0u - c[i].bits), 0, ~o[i].errors, 0}};
            label[J] = i;
            jobs[J++] = job;
        }
        if (rc == DASH_OK && J > b.nsys) {
            fprintf(stderr, "cache_simulator: %zu incoherent outcomes on a batch of %llu systems\n", J,
                    (unsigned long long)b.nsys);
            rc = DASH_EINVAL;
        }
        if (rc == DASH_OK) rc = shrink_jobs_out(h, jobs, label, J, n, b.stride, max_instr, 1, total, total - J, out_dir);
        free(label);
        free(jobs);
        free(c);
        free(o);
    }
    if (rc != DASH_OK && h) fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    batch_free(&b);
    return rc;
}

typedef struct {
    unsigned n, cs, m, len, kind, locality;
    unsigned long long seed, sched;
    int dev, show;
    const char *out, *digests, *dump;
    int device_ingest, metrics, addr_metrics;
} bulk_opts;

static void print_stats(const dash_stats *st);

static int finish_bulk(dash_t *h, const bulk_opts *o, const dash_stats *st, uint64_t count, int dump_all) {
    int rc = DASH_OK;
    if (o->digests) rc = dash_write_digests(h, o->digests);
    if (rc == DASH_OK && (dump_all || o->dump)) {
        mkdir(o->out, 0755);
        const char *p = o->dump;
        for (uint64_t k = 0; rc == DASH_OK && (dump_all ? k < count : (p && *p)); k++) {
            uint64_t sys = dump_all ? k : strtoull(p, (char **)&p, 0);
            if (!dump_all && *p == ',') p++;
            char dir[4200];
            snprintf(dir, sizeof dir, "%s/%llu", o->out, (unsigned long long)sys);
            rc = dash_dump_system(h, sys, dir);
        }
    }
    if (rc != DASH_OK) fprintf(stderr, "%s\n", dash_last_error(h));
    if (o->show) print_stats(st);
    return rc;
}

/* the event log that holds every round of a finished run (st->rounds_max), for a second run of it */
static uint32_t log_rounds_of(const dash_stats *st) {
    return st->rounds_max ? (uint32_t)st->rounds_max : 4u;
}

static int run_batch_list(const char *list, const bulk_opts *o) {
    FILE *f = fopen(list, "r");
    if (!f) {
        fprintf(stderr, "Error: could not open %s\n", list);
        return DASH_EIO;
    }
    char **dirs = NULL, line[4096];
    uint64_t n = 0, cap = 0;
    while (fgets(line, sizeof line, f)) {
        size_t l = strcspn(line, "\r\n");
        line[l] = 0;
        if (!l || line[0] == '#') continue;
        if (n == cap) {
            cap = cap ? 2 * cap : 64;
            dirs = (char **)realloc(dirs, cap * sizeof *dirs);
        }
        dirs[n++] = strdup(line);
    }
    fclose(f);
    dash_cfg cfg = {0};
    cfg.num_procs = o->n;
    cfg.cache_size = o->cs;
    cfg.max_instr = o->m;
    cfg.flags = DASH_KEEP_STATE;
    cfg.num_systems = n;
    cfg.device = o->dev;
    cfg.schedule_seed = o->sched;
    dash_t *h = NULL;
    dash_stats st;
    int rc = n ? dash_create(&cfg, &h) : DASH_EINVAL;
    if (rc == DASH_OK &&
        (rc = o->device_ingest ? dash_load_dirs_device(h, (const char *const *)dirs, n)
                               : dash_load_dirs(h, (const char *const *)dirs, n)) == DASH_OK &&
        (rc = dash_run(h, &st)) == DASH_OK)
        rc = finish_bulk(h, o, &st, n, 1);
    else if (h)
        fprintf(stderr, "%s\n", dash_last_error(h));
    dash_destroy(h);
    if (rc == DASH_OK && (o->metrics || o->addr_metrics)) {  /* once more, with an event log of the rounds the run took */
        cfg.flags = 0;
        cfg.trace_events = log_rounds_of(&st);
        h = NULL;
        if ((rc = dash_create(&cfg, &h)) == DASH_OK && (rc = dash_load_dirs(h, (const char *const *)dirs, n)) == DASH_OK &&
            (rc = dash_run(h, NULL)) == DASH_OK) {
            if (o->metrics) rc = print_metrics(h, 0, o->n);
            if (rc == DASH_OK && o->addr_metrics) rc = print_addr_metrics(h, 0, o->n);
        }
        if (rc != DASH_OK) fprintf(stderr, "%s\n", h ? dash_last_error(h) : dash_last_error(NULL));
        dash_destroy(h);
    }
    for (uint64_t k = 0; k < n; k++) free(dirs[k]);
    free(dirs);
    return rc;
}

static int run_synthetic(uint64_t count, const bulk_opts *o) {
    dash_cfg cfg = {0};
    cfg.num_procs = o->n;
    cfg.cache_size = o->cs;
    cfg.max_instr = o->len;
    cfg.flags = o->dump ? DASH_KEEP_STATE : 0;
    cfg.num_systems = count;
    cfg.device = o->dev;
    cfg.schedule_seed = o->sched;
    dash_gen g = {0};
    g.seed = o->seed;
    g.kind = o->kind;
    g.locality = o->locality;
    g.len = o->len;
    dash_t *h = NULL;
    dash_stats st;
    int rc = dash_create(&cfg, &h);
    if (rc == DASH_OK && (rc = dash_generate(h, &g)) == DASH_OK && (rc = dash_run(h, &st)) == DASH_OK) {
        printf("%llu systems, %llu instructions, %.3f ms, %.4g instr/s\n", (unsigned long long)st.systems,
               (unsigned long long)st.instructions, st.kernel_ms, st.instructions / (st.kernel_ms * 1e-3));
        rc = finish_bulk(h, o, &st, count, 0);
    } else if (h) {
        fprintf(stderr, "%s\n", dash_last_error(h));
    }
    dash_destroy(h);
    if (rc == DASH_OK && (o->metrics || o->addr_metrics)) {  /* once more, with an event log of the rounds the run took */
        cfg.flags = 0;
        cfg.trace_events = log_rounds_of(&st);
        h = NULL;
        if ((rc = dash_create(&cfg, &h)) == DASH_OK && (rc = dash_generate(h, &g)) == DASH_OK &&
            (rc = dash_run(h, NULL)) == DASH_OK) {
            if (o->metrics) rc = print_metrics(h, 0, o->n);
            if (rc == DASH_OK && o->addr_metrics) rc = print_addr_metrics(h, 0, o->n);
        }
        if (rc != DASH_OK) fprintf(stderr, "%s\n", h ? dash_last_error(h) : dash_last_error(NULL));
        dash_destroy(h);
    }
    return rc;
}

int main(int argc, char *argv[]) {
    unsigned n = 4, cs = 4, m = 32;
    int dev = 0, show = 0, dbg_instr = 0, dbg_msg = 0, n_given = 0, device_ingest = 0;
    const char *out = ".", *dir = NULL, *batch = NULL, *digests = NULL, *dump = NULL, *rounds_file = NULL,
               *micro_file = NULL, *write_rounds_file = NULL, *write_micro_file = NULL, *weights_text = NULL,
               *sources_file = NULL, *shrink_out = NULL;
    uint32_t shrink_bits = 0;
    unsigned long long synth = 0, seed = 0x5EED, sched = 0, explore = 0, micro_seed = 0;
    int explore_given = 0, explore_micro = 0, micro_seed_given = 0, metrics = 0, addr_metrics = 0, coherence = 0;
    uint64_t weights = DASH_MICRO_UNIFORM, delay_word = DASH_DELAY_LOCKSTEP;
    const char *delays_text = NULL;
    unsigned explore_delays = 0, delay_starts = 0, delay_lens = 7;
    int explore_delays_given = 0;
    unsigned len = 4096, kind = DASH_GEN_UNIFORM;
    double loc = 0.5;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-n") && i + 1 < argc) n = (unsigned)atoi(argv[++i]), n_given = 1;
        else if (!strcmp(argv[i], "-c") && i + 1 < argc) cs = (unsigned)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) m = (unsigned)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
        else if (!strcmp(argv[i], "-d") && i + 1 < argc) dev = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s")) show = 1;
        else if (!strcmp(argv[i], "--debug-instr")) dbg_instr = 1;
        else if (!strcmp(argv[i], "--debug-msg")) dbg_msg = 1;
        else if (!strcmp(argv[i], "--metrics")) metrics = 1;
        else if (!strcmp(argv[i], "--addr-metrics")) addr_metrics = 1;
        else if (!strcmp(argv[i], "--coherence")) coherence = 1;
        else if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = argv[++i];
        else if (!strcmp(argv[i], "--device-ingest")) device_ingest = 1;
        else if (!strcmp(argv[i], "--synthetic") && i + 1 < argc) synth = strtoull(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--digests") && i + 1 < argc) digests = argv[++i];
        else if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
        else if (!strcmp(argv[i], "--len") && i + 1 < argc) len = (unsigned)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--schedule") && i + 1 < argc) sched = strtoull(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--rounds") && i + 1 < argc) rounds_file = argv[++i];
        else if (!strcmp(argv[i], "--micro") && i + 1 < argc) micro_file = argv[++i];
        else if (!strcmp(argv[i], "--write-rounds") && i + 1 < argc) write_rounds_file = argv[++i];
        else if (!strcmp(argv[i], "--explore") && i + 1 < argc) explore = strtoull(argv[++i], NULL, 0), explore_given = 1;
        else if (!strcmp(argv[i], "--explore-micro") && i + 1 < argc)
            explore = strtoull(argv[++i], NULL, 0), explore_given = explore_micro = 1;
        else if (!strcmp(argv[i], "--micro-seed") && i + 1 < argc) micro_seed = strtoull(argv[++i], NULL, 0), micro_seed_given = 1;
        else if (!strcmp(argv[i], "--weights") && i + 1 < argc) weights_text = argv[++i];
        else if (!strcmp(argv[i], "--sources") && i + 1 < argc) sources_file = argv[++i];
        else if (!strcmp(argv[i], "--delays") && i + 1 < argc) delays_text = argv[++i];
        else if (!strcmp(argv[i], "--explore-delays") && i + 1 < argc)
            explore_delays = (unsigned)strtoul(argv[++i], NULL, 0), explore_delays_given = 1;
        else if (!strcmp(argv[i], "--delay-starts") && i + 1 < argc) delay_starts = (unsigned)strtoul(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--delay-lens") && i + 1 < argc) delay_lens = (unsigned)strtoul(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--write-micro") && i + 1 < argc) write_micro_file = argv[++i];
        else if (!strcmp(argv[i], "--shrink") && i + 1 < argc) shrink_out = argv[++i];
        else if (!strcmp(argv[i], "--shrink-bits") && i + 1 < argc) shrink_bits = (uint32_t)strtoul(argv[++i], NULL, 0);
        else if (!strcmp(argv[i], "--locality") && i + 1 < argc) loc = atof(argv[++i]);
        else if (!strcmp(argv[i], "--kind") && i + 1 < argc) {
            const char *k = argv[++i];
            kind = !strcmp(k, "contention") ? DASH_GEN_CONTENTION : !strcmp(k, "locality") ? DASH_GEN_LOCALITY
                                                                                         : DASH_GEN_UNIFORM;
        }
        else if (!dir) dir = argv[i];
    }
    if (batch || synth) {
        if (synth && !n_given) n = 8; /* synthetic systems default to 8 nodes (BASELINE configs) */
        bulk_opts o = {n, cs, m, len, kind, (unsigned)(loc * 65536.0), seed, sched, dev, show, out, digests, dump,
                       device_ingest, metrics, addr_metrics};
        if (o.locality > 65536u) o.locality = 65536u;
        int rc = batch ? run_batch_list(batch, &o) : run_synthetic(synth, &o);
        return rc == DASH_OK ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    if (!dir) {
        fprintf(stderr, "Usage: %s <test_directory>\n", argv[0]); /* ref :128 */
        fprintf(stderr, "       %s <test_directory> --metrics   per-node miss, invalidation and wait metrics\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --addr-metrics   per-address traffic, sharers and sharing class\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --coherence   coherence invariants of the final state\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --shrink OUTDIR   a minimal trace set with the same broken state\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --shrink OUTDIR --sources LIST   the same for many directories at once\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --explore-delays D   every outcome within D delays of lockstep\n", argv[0]);
        fprintf(stderr, "       %s <test_directory> --delays t@r+len[,..]   lockstep but node t sits out len rounds from r on\n", argv[0]);
        return EXIT_FAILURE;
    }
    if (weights_text && parse_weights(weights_text, n, &weights) != 0) {
        fprintf(stderr, "cache_simulator: --weights: up to %u comma-separated weights of 0..31\n", n);
        return EXIT_FAILURE;
    }
    if (weights_text && !explore_micro && !micro_seed_given) {
        fprintf(stderr, "cache_simulator: --weights goes with --micro-seed or --explore-micro\n");
        return EXIT_FAILURE;
    }
    if (sources_file && !explore_given && !shrink_out && !explore_delays_given) {
        fprintf(stderr, "cache_simulator: --sources goes with --explore, --explore-micro, --explore-delays or --shrink\n");
        return EXIT_FAILURE;
    }
    if (delays_text && parse_delays(delays_text, &delay_word) != 0) {
        fprintf(stderr, "cache_simulator: --delays: up to four t@r+len, node t 0..7, round r 0..1022, len 1, 2, .., 128\n");
        return EXIT_FAILURE;
    }
    if ((delays_text || explore_delays_given) &&
        (sched || rounds_file || micro_file || micro_seed_given || write_rounds_file || write_micro_file ||
         explore_given || shrink_out || (delays_text && explore_delays_given))) {
        fprintf(stderr, "cache_simulator: --delays and --explore-delays are schedules of their own: no --schedule, "
                        "--rounds, --micro, --micro-seed, --write-rounds, --write-micro, --explore or --shrink\n");
        return EXIT_FAILURE;
    }
    if (explore_delays_given) {
        if (metrics || addr_metrics || dbg_instr || dbg_msg) {
            fprintf(stderr, "cache_simulator: --explore-delays takes no --metrics, --addr-metrics or --debug-*\n");
            return EXIT_FAILURE;
        }
        int rc = explore_delays_dirs(dir, sources_file, n, cs, m, dev, explore_delays, delay_starts, delay_lens,
                                     coherence);
        if (rc != DASH_OK) {
            const char *why = dash_last_error(NULL);
            fprintf(stderr, "cache_simulator: %s (%d)\n", why[0] ? why : "failed", rc);
        }
        return rc == DASH_OK ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    if (shrink_bits && !shrink_out) {
        fprintf(stderr, "cache_simulator: --shrink-bits goes with --shrink\n");
        return EXIT_FAILURE;
    }
    if (shrink_out) {
        /* with --explore K --coherence: one job per incoherent outcome; with --sources: one per directory */
        const int outcomes = explore_given && !explore_micro && coherence && !sources_file && !shrink_bits;
        if ((explore_given && !outcomes) || rounds_file || micro_file || micro_seed_given || write_rounds_file ||
            write_micro_file || metrics || addr_metrics || (coherence && !outcomes)) {
            fprintf(stderr, "cache_simulator: --shrink goes with --schedule, --shrink-bits and --sources, or with "
                            "--explore K --coherence [--schedule S0]\n");
            return EXIT_FAILURE;
        }
        int rc = outcomes       ? explore_shrink_dir(dir, n, cs, m, dev, explore, sched, shrink_out)
                 : sources_file ? shrink_sources_dirs(dir, sources_file, n, cs, m, dev, sched, shrink_bits, shrink_out)
                                : shrink_dir(dir, n, cs, m, dev, sched, shrink_bits, shrink_out);
        if (rc != DASH_OK) {
            const char *why = dash_last_error(NULL);
            fprintf(stderr, "cache_simulator: %s (%d)\n", why[0] ? why : "failed", rc);
        }
        return rc == DASH_OK ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    if (explore_given) {
        if (rounds_file || micro_file || write_rounds_file || write_micro_file || metrics || addr_metrics) {
            fprintf(stderr, "cache_simulator: --explore takes no --rounds, --micro, --write-rounds, --write-micro, "
                            "--metrics or --addr-metrics\n");
            return EXIT_FAILURE;
        }
        const unsigned long long s0 = explore_micro ? micro_seed : sched;
        const uint64_t *w = explore_micro ? &weights : NULL;
        int rc = sources_file ? explore_sources_dirs(dir, sources_file, n, cs, m, dev, explore, s0, w, coherence)
                              : explore_dir(dir, n, cs, m, dev, explore, s0, w, coherence);
        if (rc != DASH_OK) {
            const char *why = dash_last_error(NULL);
            fprintf(stderr, "cache_simulator: %s (%d)\n", why[0] ? why : "failed", rc);
        }
        return rc == DASH_OK ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    if (write_rounds_file && (rounds_file || micro_file)) {  /* the file would restate the seed, not the run */
        fprintf(stderr, "cache_simulator: --write-rounds goes with --schedule, not with --rounds or --micro\n");
        return EXIT_FAILURE;
    }
    if (micro_seed_given && (rounds_file || micro_file || sched || write_rounds_file)) {
        fprintf(stderr, "cache_simulator: --micro-seed is a schedule of its own: no --schedule, --rounds, --micro "
                        "or --write-rounds\n");
        return EXIT_FAILURE;
    }
    if (write_micro_file && !micro_seed_given) {
        fprintf(stderr, "cache_simulator: --write-micro goes with --micro-seed\n");
        return EXIT_FAILURE;
    }
    uint8_t *rounds = NULL;
    long nrounds = 0;
    if (rounds_file && micro_file) {  /* two schedules for one run: refuse rather than drop one */
        fprintf(stderr, "cache_simulator: --rounds and --micro are exclusive\n");
        return EXIT_FAILURE;
    }
    if (rounds_file && (nrounds = read_rounds(rounds_file, n, &rounds)) < 0) {
        fprintf(stderr, "cache_simulator: %s: not a round schedule for %u nodes\n", rounds_file, n);
        return EXIT_FAILURE;
    }
    if (micro_file && (nrounds = read_micro(micro_file, n, &rounds)) <= 0) {
        /* an empty micro-step schedule would fall through to a plain lockstep run */
        fprintf(stderr, "cache_simulator: %s: %s\n", micro_file,
                nrounds == 0 ? "empty micro-step schedule" : "not a micro-step schedule");
        free(rounds);
        return EXIT_FAILURE;
    }
    dash_stats st;
    const uint64_t mseed = micro_seed;
    int rc = (dbg_instr || dbg_msg || sched || rounds || write_rounds_file || micro_seed_given || metrics || addr_metrics ||
              coherence || delays_text)
                 ? simulate_traced(dir, n, cs, m, out, dev, dbg_instr, dbg_msg, sched, rounds, nrounds,
                                   micro_file != NULL, micro_seed_given ? &mseed : NULL, weights, write_micro_file,
                                   metrics, addr_metrics, coherence, delays_text ? &delay_word : NULL, &st)
                 : dash_simulate_dir(dir, n, cs, m, out, dev, &st);
    free(rounds);
    if (rc == DASH_OK && write_rounds_file &&
        (rc = write_rounds(write_rounds_file, sched, n, (uint32_t)st.rounds_max)) != DASH_OK)
        fprintf(stderr, "cache_simulator: could not write %s\n", write_rounds_file);
    if (rc != DASH_OK) {
        const char *why = dash_last_error(NULL);
        fprintf(stderr, "cache_simulator: %s (%d)\n", why[0] ? why : "failed", rc);
        return EXIT_FAILURE;
    }
    if (show) print_stats(&st);
    return st.err_bits ? 2 : EXIT_SUCCESS;
}

static void print_stats(const dash_stats *st) {
    fprintf(stderr, "rounds %llu instructions %llu errors 0x%llx dropped %llu\n",
            (unsigned long long)st->rounds_total, (unsigned long long)st->instructions,
            (unsigned long long)st->err_bits, (unsigned long long)st->dropped);
    for (int k = 0; k < DASH_NUM_TXN; k++)
        fprintf(stderr, "  %-15s %llu\n", txn_names[k], (unsigned long long)st->hist[k]);
}
