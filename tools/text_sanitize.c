/*
 * text_sanitize.c -- sanitizer run (gcc ASan + UBSan) of csrc/dash_text.c, the in-memory
 * trace-text parser and the directory reader, next to csrc/dash_host.c's file parser:
 *   * dash_parse_core_text over exact-size heap copies of the corpus files (so a read one
 *     byte past a text is a heap-buffer-overflow), compared with dash_parse_core_file on the
 *     same bytes for several node counts and caps;
 *   * dash_read_dirs_text measuring, then reading into a heap buffer of exactly the measured
 *     size, one byte less (refused), and with a missing file.
 * Built and run by tests/test_text_sanitize.py, which writes the corpus.
 *
 * usage: text_sanitize CORPUS_DIR COUNT SCRATCH_DIR      (CORPUS_DIR/f<i>.txt, i < COUNT)
 */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "dash.h"

static int failures = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);              \
            fputc('\n', stderr);                       \
            failures++;                                \
        }                                              \
    } while (0)

/* the whole file in a heap block of exactly its size (NULL + 0 for an empty file) */
static char *slurp(const char *path, size_t *n) {
    FILE *f = fopen(path, "rb");
    *n = 0;
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    char *p = sz > 0 ? (char *)malloc((size_t)sz) : NULL;
    if (p && fread(p, 1, (size_t)sz, f) == (size_t)sz) *n = (size_t)sz;
    fclose(f);
    return p;
}

static void parse_corpus(const char *dir, int count) {
    static const uint32_t procs[] = {3, 4, 8}, caps[] = {0, 1, 32, 64};
    char path[4096];
    for (int i = 0; i < count; i++) {
        snprintf(path, sizeof path, "%s/f%d.txt", dir, i);
        size_t n;
        char *text = slurp(path, &n);
        for (unsigned a = 0; a < 3; a++)
            for (unsigned b = 0; b < 4; b++) {
                const uint32_t cap = caps[b];
                /* exact-size outputs too: a store past the cap is caught */
                uint16_t *w1 = (uint16_t *)malloc(sizeof(uint16_t) * (cap ? cap : 1));
                uint16_t *w2 = (uint16_t *)malloc(sizeof(uint16_t) * (cap ? cap : 1));
                uint32_t l1 = 0xFFFFFFFFu, l2 = 0xFFFFFFFEu;
                const int r1 = dash_parse_core_file(path, procs[a], cap, w1, &l1);
                const int r2 = dash_parse_core_text(text, n, procs[a], cap, w2, &l2);
                CHECK(r1 == r2 && l1 == l2, "%s N %u cap %u: file rc %d len %u, text rc %d len %u", path, procs[a],
                      cap, r1, l1, r2, l2);
                CHECK(l1 != l2 || memcmp(w1, w2, sizeof(uint16_t) * l1) == 0, "%s N %u cap %u: words differ", path,
                      procs[a], cap);
                free(w1);
                free(w2);
            }
        free(text);
    }
}

static void read_dirs(const char *corpus, int count, const char *scratch) {
    enum { N = 4, DIRS = 16, M = 8 };
    char path[4096], src[4096];
    const char *dirs[DIRS];
    static char names[DIRS][4096];
    for (int k = 0; k < DIRS; k++) {
        snprintf(names[k], sizeof names[k], "%s/d%d", scratch, k);
        mkdir(names[k], 0755);
        dirs[k] = names[k];
        for (int t = 0; t < N; t++) {
            snprintf(src, sizeof src, "%s/f%d.txt", corpus, (k * N + t) % count);
            size_t n;
            char *text = slurp(src, &n);
            snprintf(path, sizeof path, "%s/core_%d.txt", names[k], t);
            FILE *f = fopen(path, "wb");
            if (!f) { CHECK(0, "cannot write %s", path); free(text); return; }
            if (n) fwrite(text, 1, n, f);
            fclose(f);
            free(text);
        }
    }
    uint64_t off[DIRS * N], need = 0, need2 = 0;
    uint32_t len[DIRS * N];
    CHECK(dash_read_dirs_text(dirs, DIRS, N, M, NULL, 0, off, len, &need) == DASH_OK, "measure");
    char *buf = (char *)malloc(need ? need : 1);
    CHECK(dash_read_dirs_text(dirs, DIRS, N, M, buf, need, off, len, &need2) == DASH_OK && need2 == need,
          "read into exactly %llu bytes", (unsigned long long)need);
    for (int k = 0; k < DIRS; k++)
        for (int t = 0; t < N; t++) {
            snprintf(path, sizeof path, "%s/core_%d.txt", names[k], t);
            size_t n;
            char *text = slurp(path, &n);
            const size_t want = n < 19u * M ? n : 19u * M;
            const int f = k * N + t;
            CHECK(off[f] % 16 == 0 && len[f] == want && off[f] + len[f] <= need, "file %d: offset / length", f);
            CHECK(want == 0 || memcmp(buf + off[f], text, want) == 0, "file %d: bytes", f);
            /* and the gathered text parses like the file (the share covers max_instr records) */
            uint16_t w1[M], w2[M];
            uint32_t l1 = 0, l2 = 0;
            const int r1 = dash_parse_core_file(path, N, M, w1, &l1);
            const int r2 = dash_parse_core_text(buf + off[f], len[f], N, M, w2, &l2);
            CHECK(r1 == r2 && l1 == l2 && memcmp(w1, w2, sizeof(uint16_t) * l1) == 0, "file %d: parse of the share", f);
            free(text);
        }
    free(buf);
    if (need) {
        buf = (char *)malloc(need - 1 ? need - 1 : 1);
        CHECK(dash_read_dirs_text(dirs, DIRS, N, M, buf, need - 1, NULL, NULL, &need2) == DASH_EINVAL && need2 == need,
              "a buffer one byte short");
        free(buf);
    }
    snprintf(path, sizeof path, "%s/core_2.txt", names[DIRS - 1]);
    remove(path);
    CHECK(dash_read_dirs_text(dirs, DIRS, N, M, NULL, 0, NULL, NULL, &need2) == DASH_EIO, "missing core_2.txt");
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s CORPUS_DIR COUNT SCRATCH_DIR\n", argv[0]);
        return 2;
    }
    const int count = atoi(argv[2]);
    if (count <= 0) return 2;
    parse_corpus(argv[1], count);
    read_dirs(argv[1], count, argv[3]);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("text sanitizer run clean\n");
    return failures ? 1 : 0;
}
