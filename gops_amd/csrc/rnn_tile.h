// What the recurrent kernels share (rnn.hip: gops_rnn_forward / _backward; rnn_dqn.hip: gops_rnn_dqn_step; rollout_stack.hip: the
// closed loops under a recurrent policy): the MFMA step, the dense layer of a head on a tile in LDS, the activation pair, the checks
// of a GopsRnn description - and, for the two batch kernels, the device description with its plan, the register-resident weights, one
// step of the recurrence and the heads (the forward's floating-point order is written once: rnn_load_regs / rnn_step / rnn_heads).
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

// ---- the batch kernels (rnn.hip, rnn_dqn.hip): device description, plan, and the forward's pieces --------------------------------
#define RNN_GRID_MAX 256                                      // workgroups (= slots) of the sweep

struct RnnHeadDev {
    int nl, act, yoff, pad_;
    int dims[GOPS_MAX_LAYERS + 1];
    const float* w[GOPS_MAX_LAYERS];   // torch layout [dims[l + 1]][dims[l]]
    const float* b[GOPS_MAX_LAYERS];
    float* sh[GOPS_MAX_LAYERS];        // stash of hidden layer l's activation [Bpad][dims[l + 1]] (l < nl - 1) ...
    float* sd[GOPS_MAX_LAYERS];        // ... and of act'(z)
    int off_w[GOPS_MAX_LAYERS], off_b[GOPS_MAX_LAYERS];   // floats from the start of a slot
};
struct RnnDev {
    int B, Bpad, L, O, O16, H, nheads, ny;
    int ldw, ldx;                      // LDS leading dims of the hidden / x tiles (floats)
    int off_wih, off_whh, off_b, P;    // slot layout, floats per slot
    int G, pad_;                       // slots
    const float *wih, *whh, *bih, *bhh;
    float* hst;                        // [L][Bpad][H]
    float* slots;                      // [G][P]
    RnnHeadDev head[GOPS_RNN_MAX_HEADS];
};

// x_t of the tile -> xs [TB][ldx], columns O .. O16 - 1 and rows beyond B zero; tid: 0 .. NTHREADS - 1, the thread among the four
// waves that carry the net
__device__ __forceinline__ void rnn_stage_x(const RnnDev& p, const float* x, int row0, int t, float* xs, int tid) {
    for (int idx = tid; idx < TB * p.O16; idx += NTHREADS) {
        const int m = idx / p.O16, o = idx - m * p.O16;
        float v = 0.f;
        if (row0 + m < p.B && o < p.O) v = gptr(x)[((size_t)(row0 + m) * p.L + t) * p.O + o];
        xs[m * p.ldx + o] = v;
    }
}

// the wave's blocks of W_hh and W_ih, and the summed bias of its columns: resident for all L steps (wave: 0 .. 3 among the net's four)
template <int NB>
struct RnnRegs {
    f32x4 whh[4 * NB][NB];
    float wih[GOPS_RNN_MAX_OBS / 4][NB], bias[NB];
};
template <int NB>
__device__ __forceinline__ void rnn_load_regs(const RnnDev& p, int wave, int lane, RnnRegs<NB>& w) {
    const int l15 = lane & 15, g = lane >> 4, H = p.H, nhb = H >> 4;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int nt = wave + 4 * j, n = 16 * nt + l15;
        const bool ok = nt < nhb;
        w.bias[j] = ok ? gptr(p.bih)[n] + gptr(p.bhh)[n] : 0.f;
#pragma unroll
        for (int c = 0; c < 4 * NB; ++c) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            w.whh[c][j] = (ok && c < nhb) ? ld4(gptr(p.whh) + (size_t)n * H + 16 * c + 4 * g) : z;
        }
#pragma unroll
        for (int kc = 0; kc < GOPS_RNN_MAX_OBS / 4; ++kc) {
            const int k = 4 * kc + g;
            w.wih[kc][j] = (ok && k < p.O) ? gptr(p.wih)[(size_t)n * p.O + k] : 0.f;
        }
    }
}

// Step t of the tile: h_{t+1} = tanh(x_t W_ih^T + h_t W_hh^T + b) from xs and hr (not read at t = 0: h_0 = 0) into hw and - `stash` -
// into row t of the stash.  One MFMA chain per block over k = O, then k = H, into the same accumulators.  The caller's barrier follows.
template <int NB>
__device__ __forceinline__ void rnn_step(const RnnDev& p, const RnnRegs<NB>& w, int t, int row0, const float* hr, float* hw,
                                         const float* xs, bool stash, int wave, int lane) {
    const int l15 = lane & 15, g = lane >> 4, H = p.H, nhb = H >> 4, ldw = p.ldw, ldx = p.ldx, nk = (p.O + 3) >> 2;
    if (wave >= nhb) return;
    f32x4 acc[NB] = {};
#pragma unroll
    for (int kc = 0; kc < GOPS_RNN_MAX_OBS / 4; ++kc)
        if (kc < nk) {
            const float a = xs[l15 * ldx + 4 * kc + g];
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = mfma4(a, w.wih[kc][j], acc[j]);
        }
    if (t > 0) {
#pragma unroll
        for (int c = 0; c < 4 * NB; ++c)
            if (c < nhb) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(hr + l15 * ldw + 16 * c + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[j] = mfma4(a[i], w.whh[c][j][i], acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int nt = wave + 4 * j, n = 16 * nt + l15;
        if (nt < nhb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const float v = tanhf(acc[j][r] + w.bias[j]);
                hw[row * ldw + n] = v;
                if (stash) gptr(p.hst)[((size_t)t * p.Bpad + row0 + row) * H + n] = v;
            }
        }
    }
}

// The heads on h_L = hidden tile (L & 1) of hb [3][TB][ldw]; the other two tiles take their hidden layers in turn.  A hidden layer's
// activation AND its derivative go to the stash (`stash`); the output layer is one masked 16-column block handed to
// out(head, acc, n, ok): acc[r] + bias = element (row 4 g + r, column n) of the head's output.  A workgroup barrier after every layer.
template <class Out>
__device__ __forceinline__ void rnn_heads(const RnnDev& p, float* hb, int row0, bool stash, int lane, int wave, Out&& out_epi) {
    const int g = lane >> 4, ldw = p.ldw, L = p.L;
    const float* hL = hb + (L & 1) * TB * ldw;
    float* const pp[2] = {hb + ((L & 1) ^ 1) * TB * ldw, hb + 2 * TB * ldw};
    for (int hd = 0; hd < p.nheads; ++hd) {
        const RnnHeadDev& hp = p.head[hd];
        const float* in = hL;
        for (int l = 0; l < hp.nl; ++l) {
            const int K = hp.dims[l], N = hp.dims[l + 1];
            const float* bl = hp.b[l];
            if (l + 1 < hp.nl) {
                float* out = (l & 1) ? pp[1] : pp[0];
                float *sh = hp.sh[l], *sd = hp.sd[l];
                act_dispatch(hp.act, [&]<int ACT>() {
                    rnn_dense(in, ldw, K, hp.w[l], N, lane, wave, [&](const f32x4& acc, int n, bool) {
                        const float bn = gptr(bl)[n];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * g + r;
                            float h, dh;
                            rnn_act_pair<ACT>(acc[r] + bn, h, dh);
                            out[row * ldw + n] = h;
                            if (stash) {
                                gptr(sh)[(size_t)(row0 + row) * N + n] = h;
                                gptr(sd)[(size_t)(row0 + row) * N + n] = dh;
                            }
                        }
                    });
                });
                in = out;
            } else {
                rnn_dense(in, ldw, K, hp.w[l], N, lane, wave, [&](const f32x4& acc, int n, bool ok) {
                    if (ok) out_epi(hp, acc, gptr(bl)[n], n);
                });
            }
            __syncthreads();
        }
    }
}

// ---- host: the plan of a checked description ---------------------------------------------------------------------------------------
struct RnnPlan {
    RnnDev dev;
    size_t bytes, lds_fwd, lds_bwd;
    int ntiles;
};

// the device description of a checked net: slot layout, LDS sizes and - with a workspace - the stash sections
inline RnnPlan rnn_plan(const GopsRnn& d, int B, void* ws) {
    RnnPlan pl = {};
    RnnDev& p = pl.dev;
    p.B = B; p.Bpad = (B + TB - 1) / TB * TB; p.L = d.seq_len; p.O = d.obs_dim; p.O16 = (d.obs_dim + 15) / 16 * 16; p.H = d.hidden;
    p.nheads = d.n_heads;
    p.wih = d.weight_ih; p.whh = d.weight_hh; p.bih = d.bias_ih; p.bhh = d.bias_hh;
    pl.ntiles = p.Bpad / TB;
    p.G = pl.ntiles < RNN_GRID_MAX ? pl.ntiles : RNN_GRID_MAX;
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto section = [&](size_t floats) {
        float* at = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += align256(floats * sizeof(float));
        return at;
    };
    p.hst = section((size_t)p.L * p.Bpad * p.H);
    int maxw = p.H, slot = 0;
    p.off_wih = slot; slot += p.H * p.O;
    p.off_whh = slot; slot += p.H * p.H;
    p.off_b = slot; slot += p.H;
    for (int h = 0; h < d.n_heads; ++h) {
        const GopsMlp& m = d.head[h];
        RnnHeadDev& hd = p.head[h];
        hd.nl = m.n_layers; hd.act = m.hidden_act; hd.yoff = p.ny;
        p.ny += m.sizes[m.n_layers];
        for (int l = 0; l <= m.n_layers; ++l) hd.dims[l] = m.sizes[l];
        for (int l = 0; l < m.n_layers; ++l) {
            hd.w[l] = m.weight[l]; hd.b[l] = m.bias[l];
            hd.off_w[l] = slot; slot += m.sizes[l + 1] * m.sizes[l];
            hd.off_b[l] = slot; slot += m.sizes[l + 1];
            if (l + 1 < m.n_layers) {
                maxw = m.sizes[l + 1] > maxw ? m.sizes[l + 1] : maxw;
                hd.sh[l] = section((size_t)p.Bpad * m.sizes[l + 1]);
                hd.sd[l] = section((size_t)p.Bpad * m.sizes[l + 1]);
            }
        }
    }
    p.P = slot;
    p.slots = section((size_t)p.G * p.P);
    p.ldw = maxw + 4; p.ldx = p.O16 + 4;
    pl.bytes = off;
    pl.lds_fwd = (size_t)(3 * TB * p.ldw + 2 * TB * p.ldx) * sizeof(float);
    pl.lds_bwd = (size_t)(4 * TB * p.ldw + TB * p.ldx) * sizeof(float);
    return pl;
}
