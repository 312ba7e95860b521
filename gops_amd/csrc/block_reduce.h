// The deterministic sum (or minimum) over a batch that the loss kernels share, for workgroups of 256 threads.  The order is fixed
// and depends on the batch size only: every thread adds its own elements in index order; block_fold combines the 64 lanes of each
// wave with a butterfly (xor 32, 16, ... 1) and then the four waves as (w0 + w1) + (w2 + w3); with more than one block, every
// block parks its totals in global memory and draws a ticket (last_block), and the block that draws the last one reads the
// totals - block b in thread b - and folds them with the same block_fold, i.e. in block index order.  No block waits on another.
// grid_fold is that sequence for sums and what the kernels call; block_fold and last_block stand alone only in dsact.hip's mixed
// sum-and-minimum fold and in dw_gemm.hip's one-block sum.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// Up to here ONE block forms the sums (<= 32 elements per thread, no partials / ticket round); beyond it the kernels launch 64.
#define LOSS_ONE_BLOCK_MAX 8192

// What an entry point asks of the `stats` / state buffer it hands to these folds: the partial sums behind the results are doubles.
inline bool stats_aligned(const void* stats) { return (reinterpret_cast<uintptr_t>(stats) & 7) == 0; }

// s[i] <- the block's sum (MIN: minimum) of s[i], in every thread.  red: N rows of 4 doubles of LDS, reusable right after.
template <int N, bool MIN>
__device__ __forceinline__ void block_fold(double (&s)[N], double (*red)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double t = __shfl_xor(s[i], o);
            s[i] = MIN ? fmin(s[i], t) : s[i] + t;
        }
    }
    __syncthreads();   // (red may still be read by a previous call)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[i][threadIdx.x >> 6] = s[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i)
        s[i] = MIN ? fmin(fmin(red[i][0], red[i][1]), fmin(red[i][2], red[i][3])) : (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
}

// Publishes this block's partial values in row blockIdx.x of part[gridDim.x][stride] and draws a ticket; true in every thread of
// the block that drew the last one, which then holds in `v` the values of block threadIdx.x (zeros where there is no such block)
// and has left the ticket zero.  The ticket must be zero on entry; gridDim.x <= 256.
template <int N>
__device__ __forceinline__ bool last_block(double (&v)[N], double* part, int stride, unsigned* ticket, bool* last) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[stride * blockIdx.x + i] = v[i];
        __threadfence();
        *last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!*last) return false;
    __threadfence();
    const volatile double* vp = part;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = threadIdx.x < gridDim.x ? vp[stride * threadIdx.x + i] : 0.0;
    if (threadIdx.x == 0) *ticket = 0u;
    return true;
}

// The whole idiom for sums: s[i] <- the block's sums and, with more than one block, in the block that draws the last ticket the
// grid's.  True in the threads that hold the final sums: every thread of the one block, or of the last one.  red, part / stride /
// ticket, last: as block_fold's and last_block's (part and ticket are not touched by a grid of one block).
template <int N>
__device__ __forceinline__ bool grid_fold(double (&s)[N], double (*red)[4], double* part, int stride, unsigned* ticket, bool* last) {
    block_fold<N, false>(s, red);
    bool fin = gridDim.x == 1;
    if (!fin) {
        fin = last_block<N>(s, part, stride, ticket, last);
        if (fin) block_fold<N, false>(s, red);
    }
    return fin;
}
