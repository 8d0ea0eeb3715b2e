// shrink_many_host_check.cpp -- test infrastructure (tests/test_shrink_many_spec.py builds and runs it, with
// the host sanitizers): the arithmetic the shrink engine's kernels share with the host
// (csrc/dash_shrink.h: many_find_job, many_assign) on the CPU against a plain loop over the jobs.
//
// For a vector of candidate counts and a handle size S, every system of every sub-pass -- and of one
// sub-pass past the last, where nothing is counted -- is assigned both ways (for the large vectors a sample
// of systems and sub-passes, with the first and last of each). The prefix sits in an
// exactly-sized heap block, so a read outside P[0 .. J] is an AddressSanitizer report. Covered: zeros at the
// ends and in the middle of the vector, T a multiple of S, one below and one above it, J == S, T == 0, and
// random vectors of up to 65,536 jobs (sampled).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dash_shrink.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// the rule of include/dash.h, the slow way: walk the jobs until g falls inside one
static bool plain_assign(const std::vector<uint64_t>& cands, uint64_t S, uint64_t pass, uint64_t k, uint64_t& job,
                         uint64_t& cand) {
    const uint64_t g = pass * S + k;
    uint64_t before = 0;
    for (uint64_t i = 0; i < cands.size(); i++) {
        if (g < before + cands[i]) {
            job = i;
            cand = g - before;
            return true;
        }
        before += cands[i];
    }
    job = k % cands.size();
    cand = 0;
    return false;
}

// every kstep-th system, with the last, of every pstep-th sub-pass, with the last and one more
static int check(const std::vector<uint64_t>& cands, uint64_t S, uint64_t kstep, uint64_t pstep = 1) {
    const uint64_t J = cands.size();
    uint64_t* P = (uint64_t*)malloc(sizeof(uint64_t) * (J + 1));
    P[0] = 0;
    for (uint64_t i = 0; i < J; i++) P[i + 1] = P[i] + cands[i];
    const uint64_t T = P[J], passes = (T + S - 1) / S;
    int bad = 0;
    uint64_t counted_total = 0;
    std::vector<uint64_t> ps, ks;
    for (uint64_t p = 0; p < passes; p += pstep) ps.push_back(p);
    if (passes && ps.back() != passes - 1) ps.push_back(passes - 1);
    ps.push_back(passes);
    for (uint64_t k = 0; k < S; k += kstep) ks.push_back(k);
    if (ks.back() != S - 1) ks.push_back(S - 1);
    for (const uint64_t p : ps) {
        for (const uint64_t k : ks) {
            if (bad) break;
            uint64_t j1 = ~0ull, c1 = ~0ull, j2 = ~0ull, c2 = ~0ull;
            const bool a = dash::many_assign(P, J, S, p, k, j1, c1), b = plain_assign(cands, S, p, k, j2, c2);
            if (a != b || j1 != j2 || c1 != c2)
                bad = printf("J=%llu S=%llu pass %llu system %llu: (%d, %llu, %llu), the plain loop (%d, %llu, %llu)\n",
                             (unsigned long long)J, (unsigned long long)S, (unsigned long long)p, (unsigned long long)k, a,
                             (unsigned long long)j1, (unsigned long long)c1, b, (unsigned long long)j2, (unsigned long long)c2);
            if (a && (j1 >= J || c1 >= cands[j1] || p == passes)) bad = printf("a counted system outside its job\n");
            if (a && dash::many_find_job(P, J, p * S + k) != j1) bad = printf("many_find_job differs from many_assign\n");
            counted_total += a;
        }
    }
    if (!bad && kstep == 1 && pstep == 1 && counted_total != T) bad = printf("%llu counted systems for T = %llu\n",
                                                             (unsigned long long)counted_total, (unsigned long long)T);
    free(P);
    return bad;
}

int main() {
    int bad = 0;
    // zeros at the ends and in the middle; T == 0
    const std::vector<std::vector<uint64_t>> small = {
        {0}, {5}, {0, 0, 0}, {0, 3, 0}, {3, 0, 0, 4}, {0, 0, 7, 0, 0, 1, 0}, {2, 2, 2, 2}, {1, 0, 1, 0, 1}, {0, 9}, {9, 0}};
    for (const auto& c : small)
        for (uint64_t S = c.size(); S <= c.size() + 9 && !bad; S++) bad = check(c, S, 1);  // J == S first
    // T a multiple of S, one below and one above it
    for (uint64_t S : {4ull, 7ull, 64ull, 600ull}) {
        for (int64_t d = -1; d <= 1 && !bad; d++) {
            std::vector<uint64_t> c = {S, 0, S + (uint64_t)(1 + d), 0, S - 1};  // T = 3 S + d
            bad = check(c, S, 1);
            if (!bad) bad = check({(uint64_t)(2 * S + d)}, S, 1);
        }
    }
    // J == S with every kind of count
    for (int it = 0; it < 50 && !bad; it++) {
        const uint64_t J = 1 + rnd() % 40;
        std::vector<uint64_t> c(J);
        for (auto& x : c) x = rnd() % 3 ? rnd() % 30 : 0;
        bad = check(c, J, 1);
    }
    // many jobs, as the late rounds have them (most stopped) and as the first round has them (thousands each)
    for (int it = 0; it < 8 && !bad; it++) {
        const uint64_t J = it == 0 ? 65536 : 1 + rnd() % 65536;
        std::vector<uint64_t> c(J);
        for (auto& x : c) x = it % 2 ? (rnd() % 8 ? 0 : rnd() % 64) : rnd() % 70000;
        bad = check(c, 65536, 9973, it % 2 ? 1 : 4001);
        if (!bad) bad = check(c, J, J / 5 + 1, it % 2 ? 3 : 40009);
    }
    printf(bad ? "FAILED\n" : "shrink many host check ok\n");
    return bad ? 1 : 0;
}
