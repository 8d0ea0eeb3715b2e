/*
 * dash_text.c -- trace text in memory (pure C, no device): the rules of
 * dash_parse_core_file (dash_host.c; initializeProcessor's parse, assignment.c:822-849)
 * applied to a byte buffer, and the directory reader that gathers core_<n>.txt bytes into
 * one slab. dash_parse_core_text is the in-memory oracle of the device parser
 * (dash_ingest.hip): both restate the rules below.
 *
 * The rules are those of fgets(line, 20) + sscanf(line, "RD %hhx") / sscanf(line, "WR %hhx %hhu")
 * in the C library, as tested: tests/sscanf_ref.py calls the library's sscanf, and
 * tests/test_text_sscanf.py / test_gpu_text_sscanf.py hold the three parsers to it.
 *   Records   A record is up to 19 bytes and ends after a '\n'. A longer line continues as
 *             further records at 19-byte steps from the line's start. Trailing bytes without
 *             a final newline form a record; zero remaining bytes form none.
 *   NUL       A NUL byte ends the record's content (C-string scanning), not its extent.
 *   Cap       Reading stops once max_instr records are accepted; later text, bad text
 *             included, is never looked at. max_instr == 0 reads nothing. Hence only the
 *             first 19 * max_instr bytes of a file can matter.
 *   RD        "RD" followed by %hhx: a read, value 0 (ref :839).
 *   WR        "WR" followed by %hhx then %hhu: a write.
 *   Else      Any other record, an empty line included, is DASH_EPARSE at that record: so is
 *             every record in which sscanf would assign fewer fields than its format has.
 *   Blank     ' ' '\t' '\n' '\v' '\f' '\r' (isspace in the C locale). Any run of blanks, an
 *             empty one too, may stand before each number; none is needed ("RD12", "WR1-5").
 *   %hhx      Blanks. An optional '+' or '-'. Then "0" with an optional x/X, which is consumed
 *             even when no hex digit follows ("WR 0x 5" is address 0, value 5; "WR 0x-5" is
 *             address 0, value 251); then hex digits. At least one digit in all, the prefix's 0
 *             included. The number is an unsigned long: one that does not fit (17 significant
 *             hex digits where long has 64 bits) reads 0xFF, signed or not; otherwise '-'
 *             negates it, and the low byte is taken ("RD -0x10" is address 0xF0).
 *   %hhu      Blanks. An optional '+' or '-'. At least one decimal digit ("0x5" reads 0 and
 *             stops at the x; "- 5" and a lone sign fail). Saturation and negation as for %hhx;
 *             a record has no room for a decimal number that saturates.
 *   Trailing  Bytes after the numbers are ignored.
 *   Address   Checked after a successful parse: addr >> 4 >= num_procs is DASH_EADDR. A WR
 *             whose value fails to parse is DASH_EPARSE even with a bad address.
 *   First     The first failing record ends the file; *len = records accepted before it.
 */
#define _POSIX_C_SOURCE 200809L
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dash.h"
#include "dash_text.h"

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

/* as in dash_host.c; every scan stops at the record's terminating NUL.
   isspace in the C locale: what a blank in a scanf format and a conversion's leading skip take */
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

int dash_parse_core_text(const char *text, size_t length, uint32_t num_procs, uint32_t max_instr,
                         uint16_t *out, uint32_t *len) {
    if ((!text && length) || !len || (max_instr && !out)) return DASH_EINVAL;
    char line[20];
    uint32_t n = 0;
    size_t pos = 0;
    int rc = DASH_OK;
    while (n < max_instr && pos < length) {
        /* fgets(line, 20): up to 19 bytes, through the first '\n' */
        size_t k = 0;
        while (k < 19 && pos + k < length) {
            line[k] = text[pos + k];
            if (line[k++] == '\n') break;
        }
        line[k] = 0;
        pos += k;
        unsigned addr = 0, val = 0;
        const char *p;
        if (line[0] == 'R' && line[1] == 'D' && scan_hhx(line + 2, &addr) != NULL) {
            if ((addr >> 4) >= num_procs) { rc = DASH_EADDR; break; }
            out[n++] = (uint16_t)(addr << 8); /* value 0 (ref :839) */
        } else if (line[0] == 'W' && line[1] == 'R' && (p = scan_hhx(line + 2, &addr)) != NULL &&
                   scan_hhu(p, &val) != NULL) {
            if ((addr >> 4) >= num_procs) { rc = DASH_EADDR; break; }
            out[n++] = (uint16_t)(0x8000u | (addr << 8) | val);
        } else {
            rc = DASH_EPARSE;
            break;
        }
    }
    *len = n;
    return rc;
}

/* read() until n bytes or the end of the file; dst == NULL discards */
static uint64_t read_up_to(int fd, char *dst, uint64_t n) {
    char tmp[4096];
    uint64_t got = 0;
    while (got < n) {
        const uint64_t want = dst ? n - got : (n - got < sizeof tmp ? n - got : sizeof tmp);
        const ssize_t r = read(fd, dst ? dst + got : tmp, (size_t)(want < (1u << 30) ? want : (1u << 30)));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += (uint64_t)r;
    }
    return got;
}

int dashi_read_text_file(const char *path, uint64_t limit, char *dst, uint64_t room, uint64_t *got) {
    /* open + read rather than stdio: one system call per file and no buffer of its own */
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "Error: count not open file %s\n", path); /* ref :827, verbatim */
        return DASH_EIO;
    }
    int rc = DASH_OK;
    if (!dst) { /* measure: count what a read would return */
        *got = read_up_to(fd, NULL, limit);
    } else {
        const uint64_t n = read_up_to(fd, dst, limit < room ? limit : room);
        *got = n;
        if (n == room && room < limit) { /* more of the file's share may be left: say how much */
            const uint64_t more = read_up_to(fd, NULL, limit - n);
            if (more) {
                *got = n + more;
                rc = DASH_EINVAL;
            }
        }
    }
    close(fd);
    return rc;
}

int dash_read_dirs_text(const char *const *dirs, uint64_t n, uint32_t num_procs, uint32_t max_instr,
                        char *buf, uint64_t cap, uint64_t *offsets, uint32_t *lengths, uint64_t *need) {
    if ((!dirs && n) || !need || num_procs == 0) return DASH_EINVAL;
    const uint64_t limit = dash_text_limit(max_instr);
    if (limit > 0xFFFFFFFFull) return DASH_EINVAL;
    uint64_t pos = 0, end = 0;
    int rc = DASH_OK, fits = 1;
    char base[4096], path[4200];
    for (uint64_t k = 0; k < n && rc == DASH_OK; k++) {
        rc = dash_resolve_dir(dirs[k], base, sizeof base);
        for (uint32_t t = 0; rc == DASH_OK && t < num_procs; t++) {
            const uint64_t f = k * num_procs + t;
            pos = (end + 15u) & ~15ull; /* each file starts on a 16-byte boundary */
            uint64_t got = 0;
            snprintf(path, sizeof path, "%s/core_%u.txt", base, t);
            if (buf && fits && pos <= cap) {
                rc = dashi_read_text_file(path, limit, buf + pos, cap - pos, &got);
                if (rc == DASH_EINVAL) { /* buf is too small: go on measuring */
                    fits = 0;
                    rc = DASH_OK;
                }
            } else {
                if (buf) fits = 0;
                rc = dashi_read_text_file(path, limit, NULL, 0, &got);
            }
            if (rc != DASH_OK) break;
            if (offsets) offsets[f] = pos;
            if (lengths) lengths[f] = (uint32_t)got;
            end = pos + got;
        }
    }
    *need = end;
    if (rc != DASH_OK) return rc;
    return fits ? DASH_OK : DASH_EINVAL;
}
