// What a wave-uniform branch costs a wave on gfx950, taken and not taken (round 9).
// A dependent VALU/SALU stream in the round's mix (2 VALU : 1 SALU), four "rounds" per loop trip
// like sim_kernel's unrolled trip; each round ends in two wave-uniform tests of a value that is
// always zero, one guarding 4 and one guarding 50 never-executed instructions:
//   k_none    the tests alone (s_cmp), no branch: the baseline
//   k_taken   the cold code inline, each test a taken forward s_cbranch_scc1 over it (arm a)
//   k_fall    the cold code behind the loop, each test a not-taken s_cbranch_scc0 (arm b)
// Cost of a branch = (arm - baseline) / branches executed, as SIMD cycles at the 2.4-GHz clock
// limit: per wave at 4 waves per CU (one wave per SIMD: the latency a lone wave sees) and per
// SIMD at 18 waves per CU (4.5 waves per SIMD, the headline's occupancy: what the other waves
// do not hide).
// Build: hipcc --offload-arch=gfx950 -O3 branch_probe.hip -o branch_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

// 8 VALU + 4 SALU, each chain dependent on its own last result
#define CHUNK                                                                                 \
    "v_xor_b32 %0,%0,%8\n v_and_b32 %1,0x1234567,%1\n s_and_b64 s[42:43],s[42:43],s[44:45]\n" \
    "v_cndmask_b32 %2,%2,%8,s[42:43]\n v_lshrrev_b32 %3,3,%3\n s_or_b64 s[46:47],s[46:47],s[42:43]\n" \
    "v_cmp_eq_u32 s[44:45],%4,%8\n v_bfe_u32 %5,%5,3,5\n s_andn2_b64 s[42:43],s[46:47],s[44:45]\n" \
    "v_perm_b32 %6,%6,%8,%7\n v_add_u32 %7,%7,%8\n s_xor_b64 s[46:47],s[46:47],s[44:45]\n"
#define BODY CHUNK CHUNK CHUNK CHUNK  // one "round": 32 VALU + 16 SALU
#define C1 "v_xor_b32 %0,%1,%2\n"
#define C4 C1 C1 C1 C1
#define C10 C4 C4 C1 C1
#define C50 C10 C10 C10 C10 C10

#define ROUND_NONE(n) BODY "s_cmp_eq_u32 s40,0\n s_cmp_eq_u32 s41,0\n"
#define ROUND_TAKEN(n)                                          \
    BODY "s_cmp_eq_u32 s40,0\n s_cbranch_scc1 1" #n "%=f\n" C4   \
    "1" #n "%=:\n s_cmp_eq_u32 s41,0\n s_cbranch_scc1 2" #n "%=f\n" C50 "2" #n "%=:\n"
#define ROUND_FALL(n)                                                    \
    BODY "s_cmp_eq_u32 s40,0\n s_cbranch_scc0 3" #n "%=f\n 1" #n "%=:\n"  \
    "s_cmp_eq_u32 s41,0\n s_cbranch_scc0 4" #n "%=f\n 2" #n "%=:\n"
#define COLD_FALL(n) "3" #n "%=:\n" C4 "s_branch 1" #n "%=b\n 4" #n "%=:\n" C50 "s_branch 2" #n "%=b\n"

#define KERNEL(NAME, R, TAIL)                                                                         \
    __global__ __launch_bounds__(64) void NAME(uint32_t* out, int iters) {                            \
        uint32_t a0 = threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 ^ 9, a5 = a0 + 11, \
                 a6 = a0 * 13, a7 = a0 + 1;                                                           \
        uint32_t c = a0 ^ 0x55u;                                                                      \
        asm volatile("s_mov_b32 s40,0\n s_mov_b32 s41,0\n s_mov_b64 s[42:43],-1\n s_mov_b64 s[44:45],exec\n" \
                     "s_mov_b64 s[46:47],0\n s_mov_b32 s48,%9\n"                                      \
                     "0%=:\n" R(0) R(1) R(2) R(3)                                                     \
                     "s_sub_u32 s48,s48,1\n s_cmp_lg_u32 s48,0\n s_cbranch_scc1 0%=b\n"              \
                     "s_branch 9%=f\n" TAIL "9%=:\n"                                                  \
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) \
                     : "v"(c), "s"(iters)                                                             \
                     : "vcc", "scc", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48"); \
        out[blockIdx.x * 64 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                   \
    }

KERNEL(k_none, ROUND_NONE, "")
KERNEL(k_taken, ROUND_TAKEN, "")
KERNEL(k_fall, ROUND_FALL, COLD_FALL(0) COLD_FALL(1) COLD_FALL(2) COLD_FALL(3))

typedef void (*kfn)(uint32_t*, int);
static double run(kfn f, uint32_t* out, int wpc, int iters) {
    const int blocks = 256 * wpc;
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        hipLaunchKernelGGL(f, dim3(blocks), dim3(64), 0, 0, out, 100);
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(f, dim3(blocks), dim3(64), 0, 0, out, iters);
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return best;
}

int main() {
    uint32_t* out;
    if (hipMalloc(&out, 256 * 18 * 64 * 4) != hipSuccess) return 1;
    const int iters = 20000;                  // trips of 4 rounds, 2 tests per round
    const double nbr = 8.0 * iters;           // branches per wave in the branching arms
    printf("round = 32 VALU + 16 SALU + 2 wave-uniform tests; 4 rounds per trip, %d trips; best of 3\n", iters);
    for (int wpc : {4, 18}) {
        const double t0 = run(k_none, out, wpc, iters), ta = run(k_taken, out, wpc, iters),
                     tb = run(k_fall, out, wpc, iters);
        const double wps = wpc / 4.0;  // waves per SIMD
        // cycles of one SIMD per branch of one wave: elapsed cycles over the branches its waves ran
        const double ca = (ta - t0) * 1e-3 * 2.4e9 / (nbr * wps), cb = (tb - t0) * 1e-3 * 2.4e9 / (nbr * wps);
        printf("waves/CU %2d: none %8.3f ms  taken %8.3f ms  fall-through %8.3f ms | SIMD cycles(2.4GHz) per "
               "taken branch %.2f, per not-taken branch %.2f | round %.1f cycles\n",
               wpc, t0, ta, tb, ca, cb, t0 * 1e-3 * 2.4e9 / (4.0 * iters * wps));
    }
    return 0;
}
