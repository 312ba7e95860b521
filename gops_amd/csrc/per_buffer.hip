// The prioritized replay buffer (gops_amd/trainer/buffer/prioritized_replay_buffer.py, buffer_fused=True) in one launch per
// operation: gops_per_sample (draws -> leaves, weights and the gathered rows), gops_per_update (new priorities) and gops_per_fill
// (the leaves of freshly stored rows).  The trees are the buffer's own: float64, array layout, 2 N - 1 nodes, the leaf of slot i at
// i + N - 1, the children of p at 2 p + 1 and 2 p + 2; leaves sit on the last two levels, N = 1 is the root alone.
//
// per_sample_kernel splits the serial part of a sample from the wide part.  A workgroup of 256 threads owns PER_BLOCK_SAMPLES
// consecutive samples:
//   1. all threads copy the first 2^PER_STAGE_LEVELS - 1 nodes of the sum tree - contiguous in the array layout - into LDS;
//   2. one lane per sample descends: the first PER_STAGE_LEVELS steps read LDS, the rest are dependent 8-byte loads from global
//      memory; the lane forms the weight, stores idx and weight and leaves the row in LDS;
//   3. after one barrier a wave per sample copies the row of every key, lanes striding the row, 16 bytes per lane where the bases
//      and the width allow, 4 bytes otherwise.
// The arithmetic is the torch path's in float64, operation for operation, and none of it has the a * b + c form.
//
// per_update_kernel and per_fill_kernel are ONE workgroup each and level-synchronous: no workgroup ever waits for another.  The
// workgroup loops over its items, so neither B nor n is bounded by its size.
//   update: the indices are staged in LDS; item t writes its leaf only if no later item carries the same index (the last occurrence
//           wins: B^2 / 256 broadcast reads of LDS); then one round per level from the deepest up - in the round of depth d every
//           item whose leaf is at depth >= d recomputes the parent of its depth-d ancestor from both children, then a barrier.
//           Duplicated parents write equal values.  max_priority: block_reduce.h's fixed-order fold.
//   fill:   the leaves of a ring range are at most four contiguous index ranges (wrap-around x two leaf levels); each round
//           recomputes the parents [(lo - 1) / 2, (hi - 1) / 2] of the ranges of its level: about 2 n recomputations, not n D.
// After the root's round every touched ancestor is the recomputation from its final children, i.e. bit-equal to the torch path's.
#include <stdint.h>

#include "common.h"
#include "block_reduce.h"

namespace {

// Levels of the sum tree staged in LDS (2^L - 1 doubles: 16 KiB) and samples per workgroup: DESIGN.md section 4.19g, the measured choice
constexpr int PER_STAGE_LEVELS = 11;
constexpr int PER_BLOCK_SAMPLES = 16;
static_assert(PER_STAGE_LEVELS >= 1 && PER_STAGE_LEVELS <= 14, "2^L - 1 doubles of LDS");
static_assert(PER_BLOCK_SAMPLES >= 1 && PER_BLOCK_SAMPLES <= 256, "one lane per sample");
constexpr int PER_THREADS = 256;
constexpr int PER_MAX_CAPACITY = 1 << 29;   // tree indices are int32, and so is 2 node + 1 of every node

struct PerSampleParams {
    const double* sum;
    const double* mn;
    int N, size, B, staged;
    double beta;
    const double* u;
    int32_t* idx;
    float* weight;
    GopsPerGather g;
};

__device__ __forceinline__ int node_depth(int node) { return 31 - __clz(node + 1); }

// torch.minimum: a NaN on either side is the result
__device__ __forceinline__ double min_nan(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// Node p from both of its children: what a round of either kernel does to a parent (p has children: 2 p + 2 <= 2 N - 2).
__device__ __forceinline__ void recompute_parent(double* sum, double* mn, int p) {
    const int l = 2 * p + 1;
    sum[p] = sum[l] + sum[l + 1];
    mn[p] = min_nan(mn[l], mn[l + 1]);
}

// One row of one key, a wave: 16 bytes per lane where `vec`, else 4.
__device__ __forceinline__ void copy_row(const float* src, float* dst, int width, bool vec, int lane) {
    if (vec) {
        for (int k = lane * 4; k < width; k += 256) *reinterpret_cast<f32x4*>(dst + k) = *reinterpret_cast<const f32x4*>(src + k);
    } else {
        for (int k = lane; k < width; k += 64) dst[k] = src[k];
    }
}

__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(const PerSampleParams p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_top[];   // [staged], then the samples' rows: PER_BLOCK_SAMPLES ints
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nodes = 2 * p.N - 1, staged = p.staged;
    int* s_row = reinterpret_cast<int*>(s_top + staged);
    const int s0 = blockIdx.x * PER_BLOCK_SAMPLES, ns = min(PER_BLOCK_SAMPLES, p.B - s0);
    for (int i = tid; i < staged; i += PER_THREADS) s_top[i] = p.sum[i];
    __syncthreads();
    if (tid < ns) {
        const int i = s0 + tid;
        const double total = s_top[0];
        const double segment = total / (double)p.B;
        double value = ((double)i + p.u[i]) * segment;
        int node = 0;
        for (int left = 1; left < nodes; left = 2 * node + 1) {   // a node with a left child has a right one: 2 N - 1 is odd
            const double lsum = left < staged ? s_top[left] : p.sum[left];
            if (value <= lsum) {
                node = left;
            } else {
                value = value - lsum;
                node = left + 1;
            }
        }
        const double priority = node < staged ? s_top[node] : p.sum[node];
        const double sz = (double)p.size, nb = -p.beta;
        const double max_weight = pow(p.mn[0] / total * sz, nb);
        p.idx[i] = node;
        p.weight[i] = (float)(pow(priority / total * sz, nb) / max_weight);
        s_row[tid] = node - (p.N - 1);   // the descent ends at a node without children: N - 1 <= node <= 2 N - 2
    }
    __syncthreads();
    for (int s = wave; s < ns; s += PER_THREADS / 64) {
        const size_t row = (size_t)s_row[s], out = (size_t)(s0 + s);
        for (int k = 0; k < p.g.n_keys; ++k) {
            const int width = p.g.key[k].width;
            if (width == 0) continue;
            const float* src = p.g.key[k].src;
            float* dst = p.g.key[k].dst;
            const bool vec = (width & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
            copy_row(src + row * width, dst + out * width, width, vec, lane);
        }
    }
}

// The items of an update, staged: s_idx[t] = the leaf's tree index, or -1 for an index that is no leaf of this tree (such an item
// writes nothing and adds nothing to max_priority).
__global__ __launch_bounds__(PER_THREADS) void per_update_kernel(double* sum, double* mn, double* max_priority, int N, int B,
                                                                 const int32_t* idx, const void* priority, int priority_f64,
                                                                 double alpha, double epsilon) {
    // (no static LDS beside the dynamic block: launch_with_lds raises the kernel's dynamic limit to the whole 160 KiB)
    extern __shared__ __attribute__((aligned(16))) double s_red[];   // block_fold's 4 doubles, then the staged indices: B ints
    double (*red)[4] = reinterpret_cast<double (*)[4]>(s_red);
    int* s_idx = reinterpret_cast<int*>(s_red + 4);
    const int tid = threadIdx.x;
    const int nodes = 2 * N - 1;
    for (int t = tid; t < B; t += PER_THREADS) {
        const int node = idx[t];
        s_idx[t] = (node >= N - 1 && node < nodes) ? node : -1;
    }
    __syncthreads();
    bool any = false;
    double local = 0.0;
    for (int t = tid; t < B; t += PER_THREADS) {
        const int node = s_idx[t];
        if (node < 0) continue;
        const double pr = priority_f64 ? static_cast<const double*>(priority)[t] : (double)static_cast<const float*>(priority)[t];
        const double v = pow(pr + epsilon, alpha);
        local = any ? fmax(local, v) : v;
        any = true;
        bool last = true;
        for (int q = t + 1; q < B; ++q) last = last && s_idx[q] != node;
        if (last) {
            sum[node] = v;
            mn[node] = v;
        }
    }
    // the fold is block_fold's minimum, over -(this thread's largest new value); a thread without one brings +inf, i.e. a maximum of
    // -inf, which never wins against the stored max_priority
    double neg_max[1] = {any ? -local : __builtin_inf()};
    block_fold<1, true>(neg_max, red);   // (its barriers also publish the leaves to the rounds below)
    if (tid == 0) *max_priority = fmax(*max_priority, -neg_max[0]);
    const int deepest = node_depth(nodes - 1);
    for (int d = deepest; d >= 1; --d) {
        for (int t = tid; t < B; t += PER_THREADS) {
            const int node = s_idx[t];
            if (node < 0) continue;
            const int up = node_depth(node) - d;
            if (up >= 0) recompute_parent(sum, mn, (((node + 1) >> up) - 2) >> 1);   // the parent of the ancestor at depth d
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PER_THREADS) void per_fill_kernel(double* sum, double* mn, const double* max_priority, int N, int ptr, int n) {
    const int tid = threadIdx.x;
    const int nodes = 2 * N - 1;
    const double v = *max_priority;
    for (int j = tid; j < n; j += PER_THREADS) {
        const int node = (int)(((long long)ptr + j) % N) + N - 1;
        sum[node] = v;
        mn[node] = v;
    }
    __syncthreads();
    // the written leaves as tree-index ranges on ONE level each: the ring range is [ptr, ptr + n) cut at N, each piece cut where
    // the deepest level begins
    const int deepest = node_depth(nodes - 1), first_deep = (1 << deepest) - 1;
    int lo[4], hi[4], dep[4];
    const long long end = (long long)ptr + n;
    const int piece_lo[2] = {ptr + N - 1, N - 1};
    const int piece_hi[2] = {(int)(end < N ? end : N) + N - 2, (int)(end - N) + N - 2};   // (the second: empty unless end > N)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int a = piece_lo[k], b = piece_hi[k];
        lo[2 * k] = a; hi[2 * k] = min(b, first_deep - 1); dep[2 * k] = deepest - 1;   // (empty ranges have hi < lo)
        lo[2 * k + 1] = max(a, first_deep); hi[2 * k + 1] = b; dep[2 * k + 1] = deepest;
    }
    for (int d = deepest; d >= 1; --d) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (dep[r] != d || hi[r] < lo[r]) continue;
            const int plo = (lo[r] - 1) >> 1, phi = (hi[r] - 1) >> 1;
            for (int q = plo + tid; q <= phi; q += PER_THREADS) recompute_parent(sum, mn, q);
            lo[r] = plo; hi[r] = phi; dep[r] = d - 1;
        }
        __syncthreads();
    }
}

int check_trees(const void* sum, const void* mn, int32_t capacity) {
    if (!sum || !mn || capacity < 1) return GOPS_ERR_BAD_ARG;
    return capacity > PER_MAX_CAPACITY ? GOPS_ERR_UNSUPPORTED : GOPS_OK;
}

}  // namespace

extern "C" {

int gops_per_sample(const double* sum_tree, const double* min_tree, int32_t capacity, int32_t size, double beta, const double* u,
                    int32_t batch, const GopsPerGather* gather, int32_t* idx, float* weight, void* stream) {
    const int rc = check_trees(sum_tree, min_tree, capacity);
    if (rc != GOPS_OK) return rc;
    if (!u || !gather || !idx || !weight || batch < 1 || size < 1 || size > capacity) return GOPS_ERR_BAD_ARG;
    if (batch > GOPS_PER_MAX_BATCH || gather->n_keys > GOPS_PER_MAX_KEYS) return GOPS_ERR_UNSUPPORTED;
    if (gather->n_keys < 0) return GOPS_ERR_BAD_ARG;
    for (int k = 0; k < gather->n_keys; ++k) {
        const GopsPerKey& key = gather->key[k];
        if (key.width < 0 || (key.width > 0 && (!key.src || !key.dst))) return GOPS_ERR_BAD_ARG;
    }
    PerSampleParams p;
    p.sum = sum_tree, p.mn = min_tree, p.N = capacity, p.size = size, p.B = batch, p.beta = beta, p.u = u, p.idx = idx, p.weight = weight;
    const long long nodes = 2LL * capacity - 1, top = (1LL << PER_STAGE_LEVELS) - 1;
    p.staged = (int)(nodes < top ? nodes : top);
    p.g = *gather;
    launch_with_lds(per_sample_kernel, dim3((unsigned)((batch + PER_BLOCK_SAMPLES - 1) / PER_BLOCK_SAMPLES)), dim3(PER_THREADS),
                    (size_t)p.staged * sizeof(double) + PER_BLOCK_SAMPLES * sizeof(int), static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

int gops_per_update(double* sum_tree, double* min_tree, double* max_priority, int32_t capacity, const int32_t* idx, const void* priority,
                    int32_t priority_f64, int32_t batch, double alpha, double epsilon, void* stream) {
    const int rc = check_trees(sum_tree, min_tree, capacity);
    if (rc != GOPS_OK) return rc;
    if (!max_priority || !idx || !priority || batch < 1) return GOPS_ERR_BAD_ARG;
    if (batch > GOPS_PER_MAX_BATCH) return GOPS_ERR_UNSUPPORTED;
    launch_with_lds(per_update_kernel, dim3(1), dim3(PER_THREADS), 4 * sizeof(double) + (size_t)batch * sizeof(int), static_cast<hipStream_t>(stream), sum_tree,
                    min_tree, max_priority, (int)capacity, (int)batch, idx, priority, (int)(priority_f64 != 0), alpha, epsilon);
    return (int)hipGetLastError();
}

int gops_per_fill(double* sum_tree, double* min_tree, const double* max_priority, int32_t capacity, int32_t ptr, int32_t n, void* stream) {
    const int rc = check_trees(sum_tree, min_tree, capacity);
    if (rc != GOPS_OK) return rc;
    if (!max_priority || ptr < 0 || ptr >= capacity || n < 1 || n > capacity) return GOPS_ERR_BAD_ARG;
    launch_with_lds(per_fill_kernel, dim3(1), dim3(PER_THREADS), 0, static_cast<hipStream_t>(stream), sum_tree, min_tree, max_priority,
                    (int)capacity, (int)ptr, (int)n);
    return (int)hipGetLastError();
}

}  // extern "C"
