// The tile primitives of the kernels in which a workgroup of 256 threads owns a tile of R batch rows (R = 16, 32 or 64) and every
// output is eight fma chains added pairwise: actor_critic.hip's backups and trpo.hip's fisher_seed_kernel.  The scheme itself is
// described at the top of actor_critic.hip.
#pragma once
#include <stddef.h>

#include "common.h"

constexpr int AC_THREADS = 256;
constexpr int AC_CHAINS = 8;                 // partial sums per output: input k goes to chain k mod 8
constexpr size_t AC_LDS_TWO = 64 * 1024;     // two workgroups per CU
constexpr size_t AC_LDS_LIMIT = 150 * 1024;  // one (the CU has 160 KiB)

inline int ac_up4(int x) { return (x + 3) & ~3; }

// Tile rows and LDS bytes at batch B: large batches take 64-row tiles (a weight chunk is staged once per 64 rows), small ones
// 16-row tiles (more workgroups); within a tile size, the plan that leaves room for a second workgroup on the CU comes first.
// plan(R, limit, min_nc) -> the dynamic LDS bytes of tiles of R rows within `limit` bytes with chunks of at least `min_nc` features,
// 0 when it does not fit.  -> the bytes of the first plan that fits (R: its rows), 0 when none does.
template <typename Plan>
size_t ac_choose_rows(int B, int& R, Plan&& plan) {
    for (R = B >= 16384 ? 64 : B >= 2048 ? 32 : 16; R >= 16; R >>= 1) {
        size_t lds = plan(R, AC_LDS_TWO, 64);
        if (lds == 0) lds = plan(R, AC_LDS_LIMIT, 16);
        if (lds != 0) return lds;
    }
    return 0;
}

// kernel<R> for the tile rows a plan chose:   rows_dispatch(R, [&]<int RR>() { launch_with_lds(kernel<RR>, ...); })
template <typename F>
void rows_dispatch(int R, F&& launch) {
    if (R == 64) launch.template operator()<64>();
    else if (R == 32) launch.template operator()<32>();
    else launch.template operator()<16>();
}

// The eight chains of an output, added pairwise (T: float, double or a vector of them, elementwise).
template <typename T>
__device__ __forceinline__ T chain_sum8(const T (&c)[AC_CHAINS]) {
    return ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
}

// One output of a head: eight double fma chains over the K hidden activations (input k in chain k mod 8, k ascending), added pairwise.
__device__ __forceinline__ double ac_head_dot(const float* xr, const float* wr, int K) {
    double c[AC_CHAINS];
#pragma unroll
    for (int i = 0; i < AC_CHAINS; ++i) c[i] = 0.0;
    const int K8 = K & ~(AC_CHAINS - 1);
    for (int k = 0; k < K8; k += AC_CHAINS) {
#pragma unroll
        for (int i = 0; i < AC_CHAINS; ++i) c[i] = fma((double)xr[k + i], (double)wr[k + i], c[i]);
    }
#pragma unroll
    for (int i = 0; i < AC_CHAINS - 1; ++i)
        if (K8 + i < K) c[i] = fma((double)xr[K8 + i], (double)wr[K8 + i], c[i]);
    return chain_sum8(c);
}
