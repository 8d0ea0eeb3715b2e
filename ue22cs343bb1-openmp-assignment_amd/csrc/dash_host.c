/*
 * dash_host.c -- host boundary of libdash in C (no device code):
 *   trace ingest   = initializeProcessor's parse   (assignment.c:822-850)
 *   state init     = initializeProcessor's init    (assignment.c:806-821)
 *   dump           = printProcessorState           (assignment.c:853-905)
 *   digest         = 64-bit state digest, same spec as the kernel
 */
#define _POSIX_C_SOURCE 200809L
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "dash.h"

int dash_resolve_dir(const char *dir, char *resolved, size_t cap) {
    /* reference rule: tests/<dir>/core_<n>.txt relative to CWD (ref :824); BASELINE
       config 1 passes "tests/sample", which the reference rejects, so a directory
       that directly holds core_0.txt is accepted as well. */
    char probe[4096];
    struct stat st;
    if (!dir || !resolved || cap == 0) return DASH_EINVAL;
    snprintf(probe, sizeof probe, "tests/%s/core_0.txt", dir);
    if (stat(probe, &st) == 0) {
        if ((size_t)snprintf(resolved, cap, "tests/%s", dir) >= cap) return DASH_EINVAL;
        return DASH_OK;
    }
    snprintf(probe, sizeof probe, "%s/core_0.txt", dir);
    if (stat(probe, &st) == 0) {
        if ((size_t)snprintf(resolved, cap, "%s", dir) >= cap) return DASH_EINVAL;
        return DASH_OK;
    }
    if ((size_t)snprintf(resolved, cap, "tests/%s", dir) >= cap) return DASH_EINVAL;
    return DASH_EIO;
}

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

/* isspace in the C locale: what a blank in a scanf format and a conversion's leading skip take */
static int is_blank(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

/* sscanf "%hhx" as the C library reads it (tests/sscanf_ref.py holds it to that): blanks, an
   optional sign, then "0" with an optional x/X (consumed even when no hex digit follows: the 0
   is then the number), then hex digits; at least one digit in all. The number is an unsigned
   long that saturates (strtoul) before the cast to a byte: past ULONG_MAX it reads 0xFF, sign
   or not; otherwise a '-' negates it. */
static const char *scan_hhx(const char *p, unsigned *out) {
    while (is_blank((unsigned char)*p)) p++;
    int neg = 0, any = 0, over = 0;
    if (*p == '+' || *p == '-') neg = *p++ == '-';
    if (*p == '0') {
        any = 1;
        p++;
        if (*p == 'x' || *p == 'X') p++;
    }
    unsigned long v = 0;
    for (int d; (d = hexval((unsigned char)*p)) >= 0; p++) {
        over |= (v >> (sizeof v * 8 - 4)) != 0;
        v = (v << 4) | (unsigned long)d;
        any = 1;
    }
    if (!any) return NULL;
    *out = over ? 0xFFu : (unsigned)((neg ? 0ul - v : v) & 0xFFu);
    return p;
}

/* sscanf "%hhu": blanks, an optional sign, decimal digits (at least one; "0x5" reads 0 and
   stops at the x), saturating like %hhx -- out of reach inside a 19-byte record, where a WR
   leaves room for 15 digits. */
static const char *scan_hhu(const char *p, unsigned *out) {
    while (is_blank((unsigned char)*p)) p++;
    int neg = 0, over = 0;
    if (*p == '+' || *p == '-') neg = *p++ == '-';
    if (*p < '0' || *p > '9') return NULL;
    unsigned long v = 0;
    for (; *p >= '0' && *p <= '9'; p++) {
        const unsigned long d = (unsigned long)(*p - '0');
        over |= v > (~0ul - d) / 10ul;
        v = v * 10ul + d;
    }
    *out = over ? 0xFFu : (unsigned)((neg ? 0ul - v : v) & 0xFFu);
    return p;
}

int dash_parse_core_file(const char *path, uint32_t num_procs, uint32_t max_instr, uint16_t *out,
                         uint32_t *len) {
    if (!path || !len || (max_instr && !out)) return DASH_EINVAL;
    FILE *f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "Error: count not open file %s\n", path); /* ref :827, verbatim */
        return DASH_EIO;
    }
    char line[20]; /* ref :831: fgets(line, 20) -- long lines split into chunks */
    uint32_t n = 0;
    int rc = DASH_OK;
    while (n < max_instr && fgets(line, sizeof line, f)) {
        unsigned addr = 0, val = 0;
        const char *p;
        if (line[0] == 'R' && line[1] == 'D' && (p = scan_hhx(line + 2, &addr)) != NULL) {
            val = 0; /* ref :839 */
            (void)p;
            if ((addr >> 4) >= num_procs) { rc = DASH_EADDR; break; }
            out[n++] = (uint16_t)((addr << 8) | val);
        } else if (line[0] == 'W' && line[1] == 'R' && (p = scan_hhx(line + 2, &addr)) != NULL &&
                   scan_hhu(p, &val) != NULL) {
            if ((addr >> 4) >= num_procs) { rc = DASH_EADDR; break; }
            out[n++] = (uint16_t)(0x8000u | (addr << 8) | val);
        } else {
            /* the reference counts this line with an uninitialised instruction (ref :846) */
            rc = DASH_EPARSE;
            break;
        }
    }
    fclose(f);
    *len = n;
    return rc;
}

/* The inverse of dash_parse_core_file for a whole trace set, in the fixtures' own spelling. */
int dash_write_dir(const uint16_t *packed, uint64_t stride, const uint32_t *lens, uint32_t num_procs,
                   const char *out_dir) {
    if (!lens || !out_dir || num_procs < 1 || num_procs > DASH_MAX_PROCS) return DASH_EINVAL;
    for (uint32_t t = 0; t < num_procs; t++)
        if (lens[t] > stride || (lens[t] && !packed)) return DASH_EINVAL;
    if (mkdir(out_dir, 0777) != 0 && errno != EEXIST) return DASH_EIO;
    for (uint32_t t = 0; t < num_procs; t++) {
        char path[4200];
        if ((size_t)snprintf(path, sizeof path, "%s/core_%u.txt", out_dir, t) >= sizeof path) return DASH_EINVAL;
        FILE *f = fopen(path, "w");
        if (!f) return DASH_EIO;
        int bad = 0;
        for (uint32_t i = 0; i < lens[t]; i++) {
            const unsigned w = packed[t * stride + i], addr = (w >> 8) & 0x7Fu;
            bad |= ((w & 0x8000u) ? fprintf(f, "WR 0x%02X %u\n", addr, w & 0xFFu) : fprintf(f, "RD 0x%02X\n", addr)) < 0;
        }
        if (fclose(f) != 0 || bad) return DASH_EIO;
    }
    return DASH_OK;
}

void dash_init_node_state(dash_node_state *s, uint32_t node_id, uint32_t cache_size) {
    memset(s, 0, sizeof *s);
    for (uint32_t i = 0; i < DASH_MEM_SIZE; i++) {
        s->memory[i] = (uint8_t)(20u * node_id + i); /* ref :809 */
        s->dir_bitvector[i] = 0;
        s->dir_state[i] = 2; /* U */
    }
    for (uint32_t i = 0; i < cache_size && i < DASH_MAX_CACHE; i++) {
        s->cache_addr[i] = 0xFF;
        s->cache_value[i] = 0;
        s->cache_state[i] = 3; /* INVALID */
    }
}

int dash_dump_node(const dash_node_state *s, uint32_t id, uint32_t cache_size, char *buf,
                   size_t cap) {
    static const char *const cache_str[] = {"MODIFIED", "EXCLUSIVE", "SHARED", "INVALID"};
    static const char *const dir_str[] = {"EM", "S", "U"};
    if (!s || !buf || cache_size == 0 || cache_size > DASH_MAX_CACHE) return DASH_EINVAL;
    size_t n = 0;
    int w;
#define EMIT(...)                                                              \
    do {                                                                       \
        w = snprintf(buf + n, cap > n ? cap - n : 0, __VA_ARGS__);             \
        if (w < 0) return DASH_EINVAL;                                         \
        n += (size_t)w;                                                        \
    } while (0)
    EMIT("=======================================\n");
    EMIT(" Processor Node: %u\n", id);
    EMIT("=======================================\n\n");
    EMIT("-------- Memory State --------\n");
    EMIT("| Index | Address |   Value  |\n");
    EMIT("|----------------------------|\n");
    for (unsigned i = 0; i < DASH_MEM_SIZE; i++)
        EMIT("|  %3u  |  0x%02X   |  %5u   |\n", i, (id << 4) + i, (unsigned)s->memory[i]);
    EMIT("------------------------------\n\n");
    EMIT("------------ Directory State ---------------\n");
    EMIT("| Index | Address | State |    BitVector   |\n");
    EMIT("|------------------------------------------|\n");
    for (unsigned i = 0; i < DASH_MEM_SIZE; i++) {
        char bits[9]; /* "%08B" (ref :887) without relying on glibc >= 2.35 */
        for (int k = 0; k < 8; k++) bits[k] = (char)('0' + ((s->dir_bitvector[i] >> (7 - k)) & 1));
        bits[8] = '\0';
        EMIT("|  %3u  |  0x%02X   |  %2s   |   0x%s   |\n", i, (id << 4) + i,
             dir_str[s->dir_state[i] < 3 ? s->dir_state[i] : 2], bits);
    }
    EMIT("--------------------------------------------\n\n");
    EMIT("------------ Cache State ----------------\n");
    EMIT("| Index | Address | Value |    State    |\n");
    EMIT("|---------------------------------------|\n");
    for (unsigned i = 0; i < cache_size; i++)
        EMIT("|  %3u  |  0x%02X   |  %3u  |  %8s \t|\n", i, (unsigned)s->cache_addr[i],
             (unsigned)s->cache_value[i], cache_str[s->cache_state[i] & 3u]);
    EMIT("----------------------------------------\n\n");
#undef EMIT
    return n < cap ? (int)n : DASH_EINVAL;
}

int dash_dump_file(const dash_node_state *s, uint32_t id, uint32_t cache_size, const char *path) {
    char buf[8192];
    int n = dash_dump_node(s, id, cache_size, buf, sizeof buf);
    if (n < 0) return n;
    FILE *f = fopen(path, "w");
    if (!f) {
        printf("Error: Could not open file %s\n", path); /* ref :864 */
        return DASH_EIO;
    }
    size_t wr = fwrite(buf, 1, (size_t)n, f);
    int rc = fclose(f);
    return (wr == (size_t)n && rc == 0) ? DASH_OK : DASH_EIO;
}

static uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

int dash_format_event(const dash_event *e, char *buf, size_t cap) {
    if (!e || !buf) return DASH_EINVAL;
    int n;
    if (e->kind == DASH_EV_MSG) /* DEBUG_MSG (ref :180-181) */
        n = snprintf(buf, cap, "Processor %u msg from: %u, type: %u, address: 0x%02X\n", e->node,
                     (e->word >> 4) & 7u, e->word & 15u, (e->word >> 8) & 0x7Fu);
    else if (e->kind == DASH_EV_INSTR) /* DEBUG_INSTR (ref :650-651) */
        n = snprintf(buf, cap, "Processor %u: instr type=%c, address=0x%02X, value=%u\n", e->node,
                     (e->word & 0x8000u) ? 'W' : 'R', (e->word >> 8) & 0x7Fu, e->word & 0xFFu);
    else
        return DASH_EINVAL;
    return (n < 0 || (size_t)n >= cap) ? DASH_EINVAL : n;
}

uint64_t dash_digest_node(const dash_node_state *s, uint32_t node_id, uint32_t cache_size) {
    uint64_t h = 0x243F6A8885A308D3ULL ^ ((uint64_t)node_id << 56);
    for (int b = 0; b < DASH_MEM_SIZE; b++)
        h = fmix64(h ^ ((uint64_t)s->memory[b] | ((uint64_t)s->dir_bitvector[b] << 8) |
                        ((uint64_t)s->dir_state[b] << 16)));
    for (uint32_t i = 0; i < cache_size; i++)
        h = fmix64(h ^ ((uint64_t)s->cache_addr[i] | ((uint64_t)s->cache_value[i] << 8) |
                        ((uint64_t)s->cache_state[i] << 16) | (1ULL << 24)));
    return h;
}

/* The seeded schedule's round on the host: the same two hashes as the kernel's
   arb_word (csrc/dash_kernels.hip), written as a dash_set_schedule table. */

int dash_seed_schedule(uint64_t seed, uint32_t num_procs, uint32_t rounds, uint8_t *sched) {
    if (num_procs < 1 || num_procs > DASH_MAX_PROCS || !sched) return DASH_EINVAL;
    uint32_t P = 1;
    while (P < num_procs) P <<= 1;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t rk = seed ^ (r * 0x9E3779B97F4A7C15ULL);
        const uint64_t key = fmix64(rk), skey = fmix64(rk ^ 0xD1B54A32D192ED03ULL);
        const uint32_t A = ((uint32_t)key & (P - 1)) | 1u, Bc = (uint32_t)(key >> 8) & (P - 1);
        for (uint32_t t = 0; t < num_procs; t++) {
            uint8_t v = (uint8_t)((t * A + Bc) & (P - 1));
            if (seed == 0) v = (uint8_t)t; /* lockstep: every node steps, ascending sender order */
            else if (((skey >> (8 * t)) & 3u) == 0) v = DASH_SIT_OUT;
            sched[r * num_procs + t] = v;
        }
    }
    return DASH_OK;
}

/* The seeded micro-step schedule's pick (include/dash.h states the rule; the kernel's twin is
   micro_pick_lane in csrc/dash_kernels.hip). */
int dash_micro_pick(uint64_t seed, uint32_t round, uint32_t enabled, uint64_t weights, uint32_t num_procs) {
    if (num_procs < 1 || num_procs > DASH_MAX_PROCS || enabled == 0 || (enabled >> num_procs) != 0)
        return DASH_EINVAL;
    for (uint32_t t = 0; t < 8; t++)
        if (((weights >> (8 * t)) & 0xFFu) > 31u) return DASH_EINVAL;
    uint32_t W = 0;
    for (uint32_t t = 0; t < num_procs; t++)
        if ((enabled >> t) & 1u) W += (uint32_t)(weights >> (8 * t)) & 0xFFu;
    const int flat = W == 0; /* only weight-0 nodes are enabled: they count 1 each */
    if (flat) W = (uint32_t)__builtin_popcount(enabled);
    const uint64_t u = fmix64(seed ^ ((uint64_t)round * 0x9E3779B97F4A7C15ULL)) >> 32;
    const uint32_t x = (uint32_t)((u * W) >> 32);
    uint32_t acc = 0;
    for (uint32_t t = 0; t < num_procs; t++) {
        if (!((enabled >> t) & 1u)) continue;
        acc += flat ? 1u : (uint32_t)(weights >> (8 * t)) & 0xFFu;
        if (acc > x) return (int)t;
    }
    return DASH_EINVAL; /* not reached: x < W */
}

/* Which (source, seed) system k runs in one pass of dash_explore_sources, and whether it is counted
   (include/dash.h states the rule; the device's twin is fill_seeds in csrc/dash_outcomes.hip). */
int dash_explore_assign(uint64_t S, uint64_t G, uint64_t K, uint64_t F, uint64_t pass, uint64_t k,
                        uint32_t *source, uint64_t *seed, int *counted) {
    if (G < 1 || G > S || G > 0xFFFFFFFFull || K > UINT64_MAX - F || k >= S) return DASH_EINVAL;
    const uint64_t R = S / G;
    if (pass >= K / R + (K % R != 0)) return DASH_EINVAL;
    const uint64_t base = pass * R, row = k / G; /* base < K: no wrap */
    const uint64_t fresh = K - base < R ? K - base : R;
    const int is_counted = row < R && row < fresh;
    if (source) *source = (uint32_t)(k % G);
    if (seed) *seed = F + base + (is_counted ? row : row % fresh);
    if (counted) *counted = is_counted;
    return DASH_OK;
}

/* The coherence invariants of one system's final state (include/dash.h states them). One scan of
   the N x CS lines accumulates, per address, the count of copies, of owning copies, the holders,
   the smallest and largest value and the stale flag; one pass over the addresses forms the bits
   against the home's directory entry. */
int dash_check_states(const dash_node_state *nodes, uint32_t num_procs, uint32_t cache_size,
                      dash_coherence *out, uint32_t *addr_bits) {
    if (!nodes || !out || num_procs < 1 || num_procs > DASH_MAX_PROCS || cache_size < 1 ||
        cache_size > DASH_MAX_CACHE)
        return DASH_EINVAL;
    enum { A = DASH_MAX_PROCS * DASH_MEM_SIZE };
    uint8_t n[A] = {0}, own[A] = {0}, mask[A] = {0}, lo[A], hi[A] = {0}, stale[A] = {0};
    const uint32_t na = num_procs * DASH_MEM_SIZE;
    memset(lo, 0xFF, sizeof lo);
    for (uint32_t t = 0; t < num_procs; t++)
        for (uint32_t i = 0; i < cache_size; i++) {
            const uint32_t a = nodes[t].cache_addr[i], st = nodes[t].cache_state[i], v = nodes[t].cache_value[i];
            if (a >= na || st == 3) continue; /* another address, or INVALID */
            n[a]++;
            own[a] += st < 2; /* MODIFIED, EXCLUSIVE */
            mask[a] |= (uint8_t)(1u << t);
            if (v < lo[a]) lo[a] = (uint8_t)v;
            if (v > hi[a]) hi[a] = (uint8_t)v;
            if ((st == 1 || st == 2) && v != nodes[a >> 4].memory[a & 15]) stale[a] = 1;
        }
    out->bits = out->addrs = out->first_bits = 0;
    out->first_addr = 0xFFFFFFFFu;
    for (uint32_t a = 0; a < na; a++) {
        const uint32_t d = nodes[a >> 4].dir_state[a & 15], bv = nodes[a >> 4].dir_bitvector[a & 15];
        uint32_t b = 0;
        if (own[a] >= 1 && n[a] >= 2) b |= DASH_COH_SWMR;
        if (d == 2 && n[a] >= 1) b |= DASH_COH_DIR_U_HELD;
        if (d == 0 && !(n[a] == 1 && own[a] == 1)) b |= DASH_COH_DIR_EM;
        if (d == 1 && (own[a] >= 1 || n[a] == 0)) b |= DASH_COH_DIR_S;
        if (d != 2 && (mask[a] & ~bv)) b |= DASH_COH_LOST_SHARER;
        if (d != 2 && (bv & ~(uint32_t)mask[a])) b |= DASH_COH_STALE_SHARER;
        if (stale[a]) b |= DASH_COH_STALE_VALUE;
        if (n[a] >= 2 && lo[a] != hi[a]) b |= DASH_COH_VALUE_SPLIT;
        if (addr_bits) addr_bits[a] = b;
        if (!b) continue;
        if (!out->addrs) out->first_addr = a, out->first_bits = b;
        out->bits |= b;
        out->addrs++;
    }
    return DASH_OK;
}
