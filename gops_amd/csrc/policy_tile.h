// The policy MLP of a tile of GOPS_TILE rows inside a closed-loop kernel, stated once for the episode kernel (rollout_episode.hip,
// gops_episode_rollout) and the sampler kernel (rollout_sample.hip, gops_sample_rollout): the LDS plan, the once-per-launch staging
// of biases and weights, the hidden layers on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) and the head's dot
// products (16 lanes per row, DPP sum).  A workgroup of PT_THREADS = 256 threads (four waves) owns the tile; the kernels differ in
// what they do with the head's outputs and in the env phase around it.  Their discrete heads (gops_*_rollout_dis: an action table)
// read all outputs of a row through policy_tile_values and share the arg-max rule policy_tile_greedy.
#pragma once
#include <algorithm>

#include "common.h"

constexpr int PT_THREADS = 256;
constexpr size_t PT_LDS_LIMIT = 150 * 1024;   // dynamic LDS of one workgroup (the CU has 160 KiB)

struct PolicyTile {
    int nl, act, staged;
    int w16;                      // bit j: weight[j] is 16-byte aligned (the unstaged form may load it four floats at a time)
    int dims[GOPS_MAX_LAYERS + 1];
    const float* W[GOPS_MAX_LAYERS];
    const float* Bv[GOPS_MAX_LAYERS];
    int ldx;                      // row stride of an activation tile (floats)
    int ldw[GOPS_MAX_LAYERS];     // row stride of a staged weight image
    int w_off[GOPS_MAX_LAYERS];   // LDS offsets (floats)
    int b_off[GOPS_MAX_LAYERS];
    int flags_off;                // GOPS_TILE ints of per-row flags, the kernel's own
};

inline int pt_pad16(int x) { return (x + 15) & ~15; }

// LDS plan: two activation tiles, the biases, GOPS_TILE per-row flags, then - when everything fits - the weight images.  Returns the
// bytes, 0 when even the unstaged form does not fit (hidden widths beyond ~1100).
inline size_t policy_tile_plan(const GopsMlp& m, PolicyTile& p) {
    int maxd = 0;
    for (int j = 0; j < m.n_layers; ++j) maxd = std::max(maxd, pt_pad16(m.sizes[j]));
    p.ldx = maxd + 4;   // 4 mod 16: the 16 rows an MFMA operand read touches start in different banks
    size_t off = 2 * (size_t)GOPS_TILE * p.ldx;
    for (int j = 0; j < m.n_layers; ++j) { p.b_off[j] = (int)off; off += (size_t)pt_pad16(m.sizes[j + 1]); }
    p.flags_off = (int)off;
    off += GOPS_TILE;
    const size_t base = off;
    for (int j = 0; j < m.n_layers; ++j) {
        p.ldw[j] = pt_pad16(m.sizes[j]) + 4;
        p.w_off[j] = (int)off;
        off += (size_t)m.sizes[j + 1] * p.ldw[j];
    }
    p.staged = off * sizeof(float) <= PT_LDS_LIMIT;
    const size_t bytes = (p.staged ? off : base) * sizeof(float);
    return bytes <= PT_LDS_LIMIT ? bytes : 0;
}

// The network's shape and the live parameter tensors (read in place at every launch).
inline void policy_tile_bind(const GopsMlp& m, PolicyTile& p) {
    p.nl = m.n_layers, p.act = m.hidden_act, p.w16 = 0;
    for (int j = 0; j <= m.n_layers; ++j) p.dims[j] = m.sizes[j];
    for (int j = 0; j < m.n_layers; ++j) {
        p.W[j] = m.weight[j]; p.Bv[j] = m.bias[j];
        if ((reinterpret_cast<uintptr_t>(m.weight[j]) & 15) == 0) p.w16 |= 1 << j;
    }
}

// Once per launch: biases (and, staged, weights) into LDS.  The caller's barrier publishes them.
__device__ __forceinline__ void policy_tile_load(const PolicyTile& p, float* lds, int tid) {
    for (int j = 0; j < p.nl; ++j)
        for (int n = tid; n < p.dims[j + 1]; n += PT_THREADS) lds[p.b_off[j] + n] = p.Bv[j][n];
    if (p.staged) {
        for (int j = 0; j < p.nl; ++j) {
            const int K = p.dims[j], N = p.dims[j + 1], ldw = p.ldw[j];
            for (int idx = tid; idx < N * ldw; idx += PT_THREADS) {
                const int n = idx / ldw, k = idx - n * ldw;
                lds[p.w_off[j] + idx] = k < K ? p.W[j][(size_t)n * K + k] : 0.f;
            }
        }
    }
}

// The hidden layers of the tile whose (zero padded) input rows are in `xa`: all four waves, wave w the 16-feature tiles w, w + 4,
// ..; activations ping-pong between `xa` and `xb`.  Returns the tile the last hidden activations are in (published by a barrier).
__device__ __forceinline__ float* policy_tile_hidden(const PolicyTile& p, float* lds, float* xa, float* xb, int lane, int wave) {
    const int nl = p.nl, ldx = p.ldx;
    float* cur_x = xa;
    float* nxt_x = xb;
    for (int j = 0; j < nl - 1; ++j) {
        const int K = p.dims[j], N = p.dims[j + 1], kch = (K + 15) >> 4;
        const float* arow = cur_x + (lane & 15) * ldx + 4 * (lane >> 4);
        const int m0 = (lane >> 4) << 2;
        for (int nt = wave; nt < (N >> 4); nt += 4) {
            const int n = (nt << 4) + (lane & 15);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (p.staged) {
                const float* wrow = lds + p.w_off[j] + n * p.ldw[j] + 4 * (lane >> 4);
                for (int c = 0; c < kch; ++c) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 16 * c), b = *reinterpret_cast<const f32x4*>(wrow + 16 * c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc, 0, 0, 0);
                }
            } else if ((K & 15) == 0 && ((p.w16 >> j) & 1)) {   // rows of 64-byte multiples from a 16-byte aligned base: 16-byte loads
                const float* wrow = p.W[j] + (size_t)n * K + 4 * (lane >> 4);
                for (int c = 0; c < kch; ++c) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 16 * c), b = *reinterpret_cast<const f32x4*>(wrow + 16 * c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc, 0, 0, 0);
                }
            } else {   // the input layer of an unstaged net, or a weight view at a 4-byte offset: any width, guarded element loads
                const float* wrow = p.W[j] + (size_t)n * K;
                for (int c = 0; c < kch; ++c) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 16 * c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int k = 16 * c + 4 * (lane >> 4) + i;
                        const float b = k < K ? wrow[k] : 0.f;
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b, acc, 0, 0, 0);
                    }
                }
            }
            const float bn = lds[p.b_off[j] + n];
            act_dispatch(p.act, [&]<int ACT>() {
#pragma unroll
                for (int r = 0; r < 4; ++r) nxt_x[(m0 + r) * ldx + n] = act_fwd_t<ACT>(acc[r] + bn);
            });
        }
        __syncthreads();
        float* sw = cur_x; cur_x = nxt_x; nxt_x = sw;
    }
    return cur_x;
}

// The head's dot products of row m (16 lanes per row, `part` = lane within the row's group): y[a] = <x_m, W_out[row0 + a]> for
// a < n, without the bias, in every lane of the group.
__device__ __forceinline__ void policy_tile_head(const PolicyTile& p, const float* lds, const float* cur_x, int m, int part, int row0,
                                                 int n, float (&y)[GOPS_MAX_ACT]) {
    const int K = p.dims[p.nl - 1];
    const float* wo = p.staged ? lds + p.w_off[p.nl - 1] : p.W[p.nl - 1];
    const int ldo = p.staged ? p.ldw[p.nl - 1] : K;
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) {
        y[a] = 0.f;
        if (a < n) {
            float s = 0.f;
            for (int k = part; k < K; k += 16) s = fmaf(cur_x[m * p.ldx + k], wo[(row0 + a) * ldo + k], s);
            y[a] = row16_sum(s);
        }
    }
}

// The discrete heads (gops_sample_rollout_dis, gops_episode_rollout_dis): all n <= GOPS_DQN_MAX_ACTIONS raw outputs of row m WITH
// the bias (fp32), in every lane of the row's group - policy_tile_head in chunks of GOPS_MAX_ACT; y[a] = 0 for a >= n.  Every index
// below is a compile-time constant after unrolling: the array stays in registers.
__device__ __forceinline__ void policy_tile_values(const PolicyTile& p, const float* lds, const float* cur_x, int m, int part, int n,
                                                   float (&y)[GOPS_DQN_MAX_ACTIONS]) {
    const float* bo = lds + p.b_off[p.nl - 1];   // (pt_pad16(n) floats: a read below n's padding stays inside the plan)
#pragma unroll
    for (int c = 0; c < GOPS_DQN_MAX_ACTIONS; c += GOPS_MAX_ACT) {
        float yc[GOPS_MAX_ACT];
        policy_tile_head(p, lds, cur_x, m, part, c, n - c, yc);   // (n - c <= 0: no dot product is formed)
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) y[c + a] = c + a < n ? yc[a] + bo[c + a] : 0.f;
    }
}

// gops_dqn_backup's a_star rule: the LOWEST index among equal maxima; a NaN is the maximum (the first one), as for torch.max.
__device__ __forceinline__ int policy_tile_greedy(const float (&y)[GOPS_DQN_MAX_ACTIONS], int n) {
    float best = y[0];
    int idx = 0;
#pragma unroll
    for (int a = 1; a < GOPS_DQN_MAX_ACTIONS; ++a) {
        const float v = y[a];
        if (a < n && (v > best || (v != v && best == best))) best = v, idx = a;
    }
    return idx;
}

// The categorical head's draw from softmax(y[0 .. n)) by the inverse CDF of u0 in [0, 1), in double: the maximum (y[greedy]), the
// exponentials summed in index order, the threshold u0 S, the FIRST index whose cumulative sum exceeds it (n - 1 when rounding leaves
// none); `logp` = the log-softmax at the index.  As above every index is a compile-time constant after unrolling: y[] and z[] stay in
// registers.
__device__ __forceinline__ int policy_tile_categorical(const float (&y)[GOPS_DQN_MAX_ACTIONS], int n, int greedy, double u0, double& logp) {
    double mx = (double)y[0];
#pragma unroll
    for (int a = 1; a < GOPS_DQN_MAX_ACTIONS; ++a) mx = a == greedy ? (double)y[a] : mx;
    double z[GOPS_DQN_MAX_ACTIONS], S = 0.0;
#pragma unroll
    for (int a = 0; a < GOPS_DQN_MAX_ACTIONS; ++a) {
        z[a] = a < n ? exp((double)y[a] - mx) : 0.0;
        S += z[a];   // (index order; the zeros beyond n change nothing)
    }
    const double thr = u0 * S;
    double cum = 0.0, yi = 0.0;
    int index = n - 1;
    bool found = false;
#pragma unroll
    for (int a = 0; a < GOPS_DQN_MAX_ACTIONS; ++a) {
        cum += z[a];
        if (a < n && !found && thr < cum) index = a, found = true;
    }
#pragma unroll
    for (int a = 0; a < GOPS_DQN_MAX_ACTIONS; ++a) yi = a == index ? (double)y[a] : yi;
    logp = (yi - mx) - log(S);
    return index;
}
