// shrink_host_check.cpp -- test infrastructure (tests/test_shrink_spec.py builds and runs it, with the
// host sanitizers): the chunk arithmetic of a written row (csrc/dash_shrink.h: shrink_decode,
// variant_chunk) on the CPU against a plain deletion over arrays of instructions.
//
// For random bases in the engine's layout (node t's stream = nchunks 8-B chunks, garbage past its length)
// every candidate of the base -- or, for long bases, an evenly spaced sample of them with the last one --
// and the base itself (index C) are written chunk by chunk exactly as write_row's loop (csrc/dash_shrink.hip) does, and compared
// word for word with the deletion done the slow way. Streams sit in exactly-sized heap blocks, so a read
// outside [0, nchunks) of a stream is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dash_shrink.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int check_base(uint32_t N, uint32_t nchunks, const uint32_t* lens, uint64_t max_cands) {
    std::vector<uint2*> stream(N);
    for (uint32_t t = 0; t < N; t++) {
        stream[t] = (uint2*)malloc(sizeof(uint2) * nchunks);
        for (uint32_t q = 0; q < nchunks; q++) stream[t][q] = make_uint2((uint32_t)rnd(), (uint32_t)rnd());
    }
    auto instr = [&](uint32_t t, uint32_t i) {
        uint16_t w;
        memcpy(&w, (const char*)stream[t] + 2 * i, 2);
        return w;
    };
    dash::ShrinkCand none{};
    const uint64_t C = dash::shrink_decode(lens, N, ~0ull, none);
    int bad = 0;
    uint64_t prev_end = 0;
    uint32_t prev_node = 0;
    const uint64_t step = C > max_cands ? C / max_cands : 1;
    std::vector<uint64_t> cs;  // all of 0 .. C, or every step-th with the last candidate and C itself
    for (uint64_t c = 0; c < C; c += step) cs.push_back(c);
    if (C && cs.back() != C - 1) cs.push_back(C - 1);
    cs.push_back(C);
    for (const uint64_t c : cs) {
        if (bad) break;
        dash::ShrinkCand cand{0u, 0u, 0u};
        const uint64_t C2 = dash::shrink_decode(lens, N, c, cand);
        if (C2 != C) bad = printf("C differs at c=%llu\n", (unsigned long long)c);
        if (c == C) {  // past the last candidate: the base itself
            if (cand.count != 0) bad = printf("candidate C decodes\n");
        } else if (cand.count == 0 || cand.node >= N || cand.start + cand.count > lens[cand.node]) {
            bad = printf("candidate %llu out of its node\n", (unsigned long long)c);
        }
        if (step == 1 && c < C) {  // consecutive candidates of a level tile the node
            if (cand.node == prev_node && cand.start != 0 && cand.start != prev_end) bad = printf("gap at c=%llu\n", (unsigned long long)c);
            prev_end = cand.start + cand.count;
            prev_node = cand.node;
        }
        for (uint32_t t = 0; t < N && !bad; t++) {
            const uint32_t L = lens[t], cut = t == cand.node ? cand.count : 0u;
            std::vector<uint16_t> want(4 * (size_t)nchunks, 0);
            for (uint32_t i = 0, o = 0; i < L; i++)
                if (!(cut && i >= cand.start && i < cand.start + cut)) want[o++] = instr(t, i);
            for (uint32_t q = 0; q < nchunks && !bad; q++) {
                const uint64_t v = dash::variant_chunk(stream[t], nchunks, L, q, cand.start, cut);
                if (memcmp(&v, &want[4 * (size_t)q], 8) != 0)
                    bad = printf("c=%llu node %u chunk %u: %016llx\n", (unsigned long long)c, t, q, (unsigned long long)v);
            }
        }
    }
    for (uint32_t t = 0; t < N; t++) free(stream[t]);
    return bad;
}

int main() {
    int bad = 0;
    // every length 0..21 on a stream of exactly ceil(L / 4) chunks (at least one): all candidates
    for (uint32_t L = 0; L <= 21 && !bad; L++) {
        const uint32_t lens[2] = {L, (L * 7u) % 11u};
        bad = check_base(2, L > 8 ? (L + 3) / 4 : 3, lens, ~0ull);
        if (!bad) bad = check_base(2, 16, lens, ~0ull);
    }
    // random bases of 1..8 nodes
    for (int it = 0; it < 200 && !bad; it++) {
        const uint32_t N = 1 + (uint32_t)(rnd() % 8), nchunks = 16;
        uint32_t lens[8];
        for (uint32_t t = 0; t < N; t++) lens[t] = (uint32_t)(rnd() % 65);
        bad = check_base(N, nchunks, lens, ~0ull);
    }
    // long streams, sampled
    for (int it = 0; it < 6 && !bad; it++) {
        const uint32_t nchunks = 1040;
        uint32_t lens[8];
        for (uint32_t t = 0; t < 8; t++) lens[t] = (it == 0 || t == 0) ? 4096 : (uint32_t)(rnd() % 4097);
        bad = check_base(8, nchunks, lens, 300);
    }
    // the winner key orders candidates as the rule does: more deleted first, then the lower index
    if (!bad && !(dash::shrink_key(2, 9) > dash::shrink_key(1, 0) && dash::shrink_key(2, 3) > dash::shrink_key(2, 4) &&
                  dash::shrink_key_candidate(dash::shrink_key(5, 123456)) == 123456 && dash::shrink_key(1, 0xFFFFFFFEull) != 0))
        bad = printf("key order\n");
    printf(bad ? "FAILED\n" : "shrink host check ok\n");
    return bad ? 1 : 0;
}
