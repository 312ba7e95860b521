// What the recurrent kernels share (rnn.hip: gops_rnn_forward / _backward; rollout_stack.hip: the closed loops under a recurrent
// policy): the MFMA step, the dense layer of a head on a tile in LDS, the activation pair, and the checks of a GopsRnn description.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

template <int ACT>
__device__ __forceinline__ void rnn_act_pair(float z, float& h, float& dh) {
    if constexpr (ACT == GOPS_ACT_GELU) {
        gelu_pair(z, h, dh);
    } else {
        h = act_fwd_t<ACT>(z);
        dh = act_bwd_t<ACT>(h, 0.f);
    }
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// [TB][K] = A [TB][K] (LDS) W^T, W [N][K] in torch layout streamed from L2; blocks of 16 output columns dealt to the waves.
// epi(acc, n, ok): acc[r] = element (row 4 g + r, column n); ok: n < N.
template <class Epi>
__device__ __forceinline__ void rnn_dense(const float* A, int lda, int K, const float* W, int N, int lane, int wave, Epi&& epi) {
    const int l15 = lane & 15, g = lane >> 4;
    for (int nt = wave; 16 * nt < N; nt += 4) {
        const int n = 16 * nt + l15;
        const bool ok = n < N;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < (K >> 4); ++c) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(A + l15 * lda + 16 * c + 4 * g);
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (ok) b = ld4(gptr(W) + (size_t)n * K + 16 * c + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = mfma4(a[i], b[i], acc);
        }
        epi(acc, n, ok);
    }
}

inline bool rnn_width_ok(int w) { return w >= 16 && w <= GOPS_RNN_MAX_HIDDEN && w % 16 == 0; }

// every check of the description: GOPS_OK, or the code the entry points refuse it with
inline int rnn_check(const GopsRnn& d, int B) {
    if (B < 1 || d.seq_len < 1 || d.n_heads < 1 || d.n_heads > GOPS_RNN_MAX_HEADS) return GOPS_ERR_BAD_ARG;
    if (!d.weight_ih || !d.weight_hh || !d.bias_ih || !d.bias_hh) return GOPS_ERR_BAD_ARG;
    for (int h = 0; h < d.n_heads; ++h) {
        const GopsMlp& m = d.head[h];
        if (m.n_layers < 1) return GOPS_ERR_BAD_ARG;
        if (m.n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_UNSUPPORTED;
        if (m.sizes[0] != d.hidden) return GOPS_ERR_BAD_ARG;
        for (int l = 0; l < m.n_layers; ++l)
            if (!m.weight[l] || !m.bias[l]) return GOPS_ERR_BAD_ARG;
    }
    if (d.seq_len > GOPS_RNN_MAX_SEQ || d.obs_dim < 1 || d.obs_dim > GOPS_RNN_MAX_OBS || !rnn_width_ok(d.hidden)) return GOPS_ERR_UNSUPPORTED;
    for (int h = 0; h < d.n_heads; ++h) {
        const GopsMlp& m = d.head[h];
        if (m.dtype != GOPS_DTYPE_F32 || m.hidden_act < GOPS_ACT_LINEAR || m.hidden_act > GOPS_ACT_TANH) return GOPS_ERR_UNSUPPORTED;
        for (int l = 1; l < m.n_layers; ++l)
            if (!rnn_width_ok(m.sizes[l])) return GOPS_ERR_UNSUPPORTED;
        if (m.sizes[m.n_layers] < 1 || m.sizes[m.n_layers] > GOPS_RNN_MAX_OUT) return GOPS_ERR_UNSUPPORTED;
    }
    return GOPS_OK;
}
