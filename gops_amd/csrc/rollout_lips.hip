// LipsNet policies (gops/apprfunc/lipsnet.py): an MLP f evaluated together with its input Jacobian J = df/dx and differentiated
// through it,  y = K(x) f(x) / (||J||_F + eps)  - include/gops_hip.h: gops_lips_workspace_bytes / _forward / _backward.
//
// Tangent propagation: a sample is 1 + n rows through the same layers - the primal row h and the n tangent rows T (T_0 = I_n):
//     z = W h + b,  U = W T,  h' = act(z),  T' = act'(z) * U           f = W_L h + b_L,  J = W_L T
// and the reverse pass walks the same rows back with one extra term on the primal delta:
//     G_U = act'(z) * G_T',   g_z = act'(z) g_h' + act''(z) sum_cols(G_T' * U),   g_h = W^T g_z,  G_T = W^T G_U
//     g_W = g_z h^T + G_U T^T,  g_b = g_z.
// Mapping: a workgroup owns a tile of NTS samples (NTS (1 + n) rows); activations / deltas of the current layer live in two LDS
// buffers, weights are read from L2 (every workgroup reads the same few KB), pre-activations (z, U) and deltas go to the workspace.
// One thread forms all 1 + n rows of one (sample, feature) pair, so act'(z) of the primal row is in a register when the tangent rows
// need it.  Weight gradients: a register-tiled fp32 GEMM over the stashed rows, split over row slabs whose partials are summed in a
// fixed order by the library's reduce kernel - no float atomics anywhere, results are bitwise reproducible.
// All arithmetic is fp32 fmaf chains with libm transcendentals (the 1e-5 bar of the tests is against a float64 evaluation).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "common.h"
#include "launchers.h"

#define LIPS_NT 256
#define LIPS_MAX_HIDDEN 3     // hidden layers of f
#define LIPS_MAX_KHIDDEN 2    // hidden layers of a local K net
#define LIPS_MAX_OBS 8
#define LIPS_MAX_WIDTH 256
#define LIPS_LDS_BUDGET (60 * 1024)
#define LIPS_DW_TILE 64
#define LIPS_DW_ROWS 16
#define LIPS_DW_MAX_JOBS 8
#define LIPS_DW_MAX_SLABS 64

struct LipsParams {
    int B, n, m, L, act, NTS, Wmax;
    int size[LIPS_MAX_HIDDEN + 2];          // n, hidden..., m
    const float* W[LIPS_MAX_HIDDEN + 1];
    const float* b[LIPS_MAX_HIDDEN + 1];
    int KL;                                 // hidden layers of the K net; 0: global K
    int ksize[LIPS_MAX_KHIDDEN + 2];        // n, hidden..., 1
    const float* KW[LIPS_MAX_KHIDDEN + 1];
    const float* Kb[LIPS_MAX_KHIDDEN + 1];
    const float* kscalar;
    float eps, lambda;
    int training, squash;
    float half[GOPS_MAX_ACT], mid[GOPS_MAX_ACT];
    const float* obs;
    const float* grad_action;
    float *action, *Kout, *Nout;
    // workspace
    float* Z[LIPS_MAX_HIDDEN];     // [B (1 + n)][width]: z (row 0 of a sample) and U (rows 1..n)
    float* D[LIPS_MAX_HIDDEN];     // deltas of the same rows
    float *FJ, *DO;                // [B (1 + n)][m]: f and the columns of J; their deltas
    float* ZK[LIPS_MAX_KHIDDEN];   // [B][width] pre-activations of the K net
    float* DK[LIPS_MAX_KHIDDEN];
    float *kpre, *dkpre, *Kws, *Nws, *y;   // [B], y [B][m]
};

// act3_t (common.h) for a run-time activation id
__device__ __forceinline__ void lips_act3(int act, float z, float& a, float& d1, float& d2) {
    act_dispatch(act, [&]<int ACT>() { act3_t<ACT>(z, a, d1, d2); });
}

// torch.nn.Softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float lips_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float lips_softplus_d(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }

// One hidden layer over the tile: NR rows per sample.  FIRST: the input is the observation tile X [NTS][LIPS_MAX_OBS] and the
// tangent rows start from the identity (U[c] = W[:, c]); else `in` is [NTS][NR][Win] in LDS, Win a multiple of 4.
// out [NTS][NR][Wout] (LDS) = (act(z), act'(z) U); Zg (global, the tile's first row) = (z, U) for the NVAL valid samples.
template <int NR, bool FIRST>
__device__ __forceinline__ void lips_layer_fwd(const float* in, int Win, const float* __restrict__ W, const float* __restrict__ bias,
                                               int Wout, int act, float* out, float* __restrict__ Zg, int NTS, int NVAL) {
    for (int it = threadIdx.x; it < NTS * Wout; it += LIPS_NT) {
        const int t = it / Wout, j = it - t * Wout;
        float acc[NR];
        acc[0] = bias[j];
#pragma unroll
        for (int r = 1; r < NR; ++r) acc[r] = 0.f;
        const float* w = W + (size_t)j * Win;
        if constexpr (FIRST) {
#pragma unroll
            for (int c = 0; c < LIPS_MAX_OBS; ++c) {
                if (c < Win) {
                    const float wc = w[c];
                    acc[0] = fmaf(wc, in[t * LIPS_MAX_OBS + c], acc[0]);
                    if (c + 1 < NR) acc[c + 1] = wc;
                }
            }
        } else {
            const float* x = in + (size_t)t * NR * Win;
            for (int k = 0; k < Win; k += 4) {
                const float4 wv = *reinterpret_cast<const float4*>(w + k);
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + r * Win + k);
                    acc[r] = fmaf(wv.x, xv.x, acc[r]);
                    acc[r] = fmaf(wv.y, xv.y, acc[r]);
                    acc[r] = fmaf(wv.z, xv.z, acc[r]);
                    acc[r] = fmaf(wv.w, xv.w, acc[r]);
                }
            }
        }
        float a, d1, d2;
        lips_act3(act, acc[0], a, d1, d2);
        float* o = out + (size_t)t * NR * Wout + j;
        o[0] = a;
#pragma unroll
        for (int r = 1; r < NR; ++r) o[r * Wout] = d1 * acc[r];
        if (t < NVAL) {
            float* zg = Zg + (size_t)t * NR * Wout + j;
#pragma unroll
            for (int r = 0; r < NR; ++r) zg[r * Wout] = acc[r];
        }
    }
}

// g_in [NTS][NR][Win] (LDS) = delta [NTS][NR][Wout] (LDS) times W [Wout][Win]; Wout a multiple of 4 or below 4
template <int NR>
__device__ __forceinline__ void lips_layer_bwd_x(const float* delta, int Wout, const float* __restrict__ W, int Win, float* gin, int NTS) {
    for (int it = threadIdx.x; it < NTS * Win; it += LIPS_NT) {
        const int t = it / Win, k = it - t * Win;
        float acc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] = 0.f;
        const float* d = delta + (size_t)t * NR * Wout;
        for (int j = 0; j < Wout; ++j) {
            const float w = W[(size_t)j * Win + k];
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = fmaf(w, d[r * Wout + j], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) gin[((size_t)t * NR + r) * Win + k] = acc[r];
    }
}

template <int N>
__global__ __launch_bounds__(LIPS_NT) void lips_fwd_kernel(const LipsParams p) {
    constexpr int NR = N + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NTS = p.NTS, tid = threadIdx.x, m = p.m;
    float* bufA = lds;
    float* bufB = bufA + NTS * NR * p.Wmax;
    float* X = bufB + NTS * NR * p.Wmax;          // [NTS][LIPS_MAX_OBS]
    float* FJs = X + NTS * LIPS_MAX_OBS;          // [NTS][NR][GOPS_MAX_ACT]
    float* Ks = FJs + NTS * NR * GOPS_MAX_ACT;    // [NTS] pre-softplus K
    const int b0 = blockIdx.x * NTS;
    const int NVAL = min(NTS, p.B - b0);
    for (int i = tid; i < NTS * LIPS_MAX_OBS; i += LIPS_NT) {
        const int t = i / LIPS_MAX_OBS, c = i - t * LIPS_MAX_OBS;
        X[i] = (t < NVAL && c < N) ? p.obs[(size_t)(b0 + t) * N + c] : 0.f;
    }
    __syncthreads();
    float *cur = bufA, *nxt = bufB;
    lips_layer_fwd<NR, true>(X, N, p.W[0], p.b[0], p.size[1], p.act, cur, p.Z[0] + (size_t)b0 * NR * p.size[1], NTS, NVAL);
    __syncthreads();
    for (int l = 1; l < p.L; ++l) {
        lips_layer_fwd<NR, false>(cur, p.size[l], p.W[l], p.b[l], p.size[l + 1], p.act, nxt, p.Z[l] + (size_t)b0 * NR * p.size[l + 1], NTS, NVAL);
        __syncthreads();
        float* s = cur; cur = nxt; nxt = s;
    }
    {   // output layer: f (row 0) and the columns of J (rows 1..n)
        const int Win = p.size[p.L];
        const float* WL = p.W[p.L];
        for (int it = tid; it < NTS * NR * m; it += LIPS_NT) {
            const int jo = it % m, tr = it / m, r = tr % NR, t = tr / NR;
            float acc = r == 0 ? p.b[p.L][jo] : 0.f;
            const float* x = cur + (size_t)tr * Win;
            const float* w = WL + (size_t)jo * Win;
            for (int k = 0; k < Win; ++k) acc = fmaf(w[k], x[k], acc);
            FJs[tr * GOPS_MAX_ACT + jo] = acc;
            if (t < NVAL) p.FJ[((size_t)(b0 + t) * NR + r) * m + jo] = acc;
        }
    }
    __syncthreads();
    if (p.KL > 0) {   // local K: a tanh MLP on the primal row only
        lips_layer_fwd<1, true>(X, N, p.KW[0], p.Kb[0], p.ksize[1], GOPS_ACT_TANH, bufA, p.ZK[0] + (size_t)b0 * p.ksize[1], NTS, NVAL);
        __syncthreads();
        cur = bufA; nxt = bufB;
        for (int l = 1; l < p.KL; ++l) {
            lips_layer_fwd<1, false>(cur, p.ksize[l], p.KW[l], p.Kb[l], p.ksize[l + 1], GOPS_ACT_TANH, nxt, p.ZK[l] + (size_t)b0 * p.ksize[l + 1], NTS, NVAL);
            __syncthreads();
            float* s = cur; cur = nxt; nxt = s;
        }
        const int Win = p.ksize[p.KL];
        if (tid < NTS) {
            float acc = p.Kb[p.KL][0];
            for (int k = 0; k < Win; ++k) acc = fmaf(p.KW[p.KL][k], cur[(size_t)tid * Win + k], acc);
            Ks[tid] = acc;
        }
    } else if (tid < NTS) {
        Ks[tid] = p.kscalar[0];
    }
    __syncthreads();
    if (tid < NVAL) {
        const int t = tid, b = b0 + t;
        float n2 = 0.f;
        for (int r = 1; r < NR; ++r)
            for (int jo = 0; jo < m; ++jo) { const float v = FJs[(t * NR + r) * GOPS_MAX_ACT + jo]; n2 = fmaf(v, v, n2); }
        const float nrm = sqrtf(n2), kpre = Ks[t], K = lips_softplus(kpre);
        const float s = K / (nrm + p.eps);
        for (int jo = 0; jo < m; ++jo) {
            const float y = s * FJs[t * NR * GOPS_MAX_ACT + jo];
            p.y[(size_t)b * m + jo] = y;
            p.action[(size_t)b * m + jo] = p.squash ? fmaf(p.half[jo], tanhf(y), p.mid[jo]) : y;
        }
        p.kpre[b] = kpre; p.Kws[b] = K; p.Nws[b] = nrm;
        if (p.Kout != nullptr) p.Kout[b] = K;
        if (p.Nout != nullptr) p.Nout[b] = nrm;
    }
}

template <int N>
__global__ __launch_bounds__(LIPS_NT) void lips_bwd_kernel(const LipsParams p) {
    constexpr int NR = N + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NTS = p.NTS, tid = threadIdx.x, m = p.m;
    float* G = lds;                               // adjoints of a layer's outputs (h', T')
    float* Dl = G + NTS * NR * p.Wmax;             // deltas of its pre-activations (z, U)
    float* DOs = Dl + NTS * NR * p.Wmax + NTS * LIPS_MAX_OBS;   // [NTS][NR][GOPS_MAX_ACT] (same layout as the forward's)
    float* dk = DOs + NTS * NR * GOPS_MAX_ACT;     // [NTS]
    const int b0 = blockIdx.x * NTS;
    const int NVAL = min(NTS, p.B - b0);
    if (tid < NTS) {
        const int t = tid, b = b0 + t;
        float gk = 0.f;
        if (t < NVAL) {
            const float K = p.Kws[b], nrm = p.Nws[b], den = nrm + p.eps;
            const float* fj = p.FJ + (size_t)b * NR * m;
            float gy[GOPS_MAX_ACT], c = 0.f;
            for (int jo = 0; jo < m; ++jo) {
                float g = p.grad_action[(size_t)b * m + jo];
                if (p.squash) {   // 1 - tanh^2 = sech^2 from one exponential: 1 - th * th loses its digits where the squash saturates
                    const float e = expf(-2.f * fabsf(p.y[(size_t)b * m + jo]));
                    g *= p.half[jo] * (4.f * e / ((1.f + e) * (1.f + e)));
                }
                gy[jo] = g;
                c = fmaf(g, fj[jo], c);
            }
            gk = c / den;
            if (p.training) gk += 2.f * p.lambda * K / (float)p.B;   // d(lambda mean K^2) / dK
            const float sJ = nrm > 0.f ? -K * c / (den * den) / nrm : 0.f;   // torch's subgradient of the norm at 0
            for (int jo = 0; jo < m; ++jo) {
                const float gf = K * gy[jo] / den;
                DOs[t * NR * GOPS_MAX_ACT + jo] = gf;
                p.DO[(size_t)b * NR * m + jo] = gf;
            }
            for (int r = 1; r < NR; ++r)
                for (int jo = 0; jo < m; ++jo) {
                    const float gj = sJ * fj[r * m + jo];
                    DOs[(t * NR + r) * GOPS_MAX_ACT + jo] = gj;
                    p.DO[((size_t)b * NR + r) * m + jo] = gj;
                }
            gk *= lips_softplus_d(p.kpre[b]);
            p.dkpre[b] = gk;
        } else {
            for (int i = 0; i < NR * GOPS_MAX_ACT; ++i) DOs[t * NR * GOPS_MAX_ACT + i] = 0.f;
        }
        dk[t] = gk;
    }
    __syncthreads();
    {   // through the output layer
        const int Win = p.size[p.L];
        const float* WL = p.W[p.L];
        for (int it = tid; it < NTS * Win; it += LIPS_NT) {
            const int t = it / Win, k = it - t * Win;
            float acc[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = 0.f;
            for (int jo = 0; jo < m; ++jo) {
                const float w = WL[(size_t)jo * Win + k];
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[r] = fmaf(w, DOs[(t * NR + r) * GOPS_MAX_ACT + jo], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) G[((size_t)t * NR + r) * Win + k] = acc[r];
        }
    }
    __syncthreads();
    for (int l = p.L - 1; l >= 0; --l) {
        const int Wl = p.size[l + 1];
        const float* Zg = p.Z[l] + (size_t)b0 * NR * Wl;
        float* Dg = p.D[l] + (size_t)b0 * NR * Wl;
        for (int it = tid; it < NTS * Wl; it += LIPS_NT) {
            const int t = it / Wl, j = it - t * Wl;
            float d[NR];
            if (t < NVAL) {
                const float* zg = Zg + (size_t)t * NR * Wl + j;
                const float* g = G + (size_t)t * NR * Wl + j;
                float a, d1, d2, s = 0.f;
                lips_act3(p.act, zg[0], a, d1, d2);
#pragma unroll
                for (int r = 1; r < NR; ++r) {
                    const float gt = g[r * Wl];
                    s = fmaf(gt, zg[r * Wl], s);
                    d[r] = d1 * gt;
                }
                d[0] = fmaf(d1, g[0], d2 * s);
                float* dg = Dg + (size_t)t * NR * Wl + j;
#pragma unroll
                for (int r = 0; r < NR; ++r) dg[r * Wl] = d[r];
            } else {
#pragma unroll
                for (int r = 0; r < NR; ++r) d[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) Dl[((size_t)t * NR + r) * Wl + j] = d[r];
        }
        __syncthreads();
        if (l > 0) {
            lips_layer_bwd_x<NR>(Dl, Wl, p.W[l], p.size[l], G, NTS);
            __syncthreads();
        }
    }
    if (p.KL > 0) {   // the K net: an ordinary reverse pass from d(loss)/d(pre-softplus K)
        {
            const int Win = p.ksize[p.KL];
            for (int it = tid; it < NTS * Win; it += LIPS_NT) {
                const int t = it / Win, k = it - t * Win;
                G[it] = p.KW[p.KL][k] * dk[t];
            }
        }
        __syncthreads();
        for (int l = p.KL - 1; l >= 0; --l) {
            const int Wl = p.ksize[l + 1];
            for (int it = tid; it < NTS * Wl; it += LIPS_NT) {
                const int t = it / Wl, j = it - t * Wl;
                float d = 0.f;
                if (t < NVAL) {
                    const float th = tanhf(p.ZK[l][(size_t)(b0 + t) * Wl + j]);
                    d = (1.f - th * th) * G[it];
                    p.DK[l][(size_t)(b0 + t) * Wl + j] = d;
                }
                Dl[it] = d;
            }
            __syncthreads();
            if (l > 0) {
                lips_layer_bwd_x<1>(Dl, Wl, p.KW[l], p.ksize[l], G, NTS);
                __syncthreads();
            }
        }
    }
}

// ---- weight gradients: g_W [Wout][Win] = sum_rows delta[row][:] (x) input[row][:], g_b = sum over primal rows of delta ---------
struct LipsDwJob {
    const float* D;       // [rows][Wout] deltas
    const float* Zp;      // [rows][Win] stash of the layer below (input = its activation), or null: the layer reads the observation
    const float* obs;     // [rows / NR][Win]
    float *pw, *pb;       // partials [slabs][Wout Win], [slabs][Wout]
    int Win, Wout, NR, act, rows;
};
struct LipsDwParams {
    LipsDwJob job[LIPS_DW_MAX_JOBS];
    int slab_samples;     // samples per row slab (a job's slab has slab_samples NR rows)
};

__global__ __launch_bounds__(LIPS_NT) void lips_dw_kernel(const LipsDwParams p) {
    __shared__ __attribute__((aligned(16))) float Dt[LIPS_DW_ROWS][LIPS_DW_TILE];
    __shared__ __attribute__((aligned(16))) float It[LIPS_DW_ROWS][LIPS_DW_TILE];
    const LipsDwJob& jb = p.job[blockIdx.z];
    const int Win = jb.Win, Wout = jb.Wout, NR = jb.NR;
    const int tk_n = max(1, (Win + LIPS_DW_TILE - 1) / LIPS_DW_TILE), tj_n = (Wout + LIPS_DW_TILE - 1) / LIPS_DW_TILE;
    if ((int)blockIdx.x >= tk_n * tj_n) return;
    const int tj = blockIdx.x / tk_n, tkk = blockIdx.x - tj * tk_n;
    const int j0 = tj * LIPS_DW_TILE, k0 = tkk * LIPS_DW_TILE;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int row_begin = blockIdx.y * p.slab_samples * NR;
    const int row_end = min(jb.rows, row_begin + p.slab_samples * NR);
    float acc[4][4], bacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bacc[i] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
    }
    for (int row0 = row_begin; row0 < row_end; row0 += LIPS_DW_ROWS) {
        for (int e = tid; e < LIPS_DW_ROWS * LIPS_DW_TILE; e += LIPS_NT) {
            const int rr = e / LIPS_DW_TILE, cc = e - rr * LIPS_DW_TILE, row = row0 + rr;
            float dv = 0.f, iv = 0.f;
            if (row < row_end) {
                const int smp = row / NR, r = row - smp * NR;
                if (j0 + cc < Wout) dv = jb.D[(size_t)row * Wout + j0 + cc];
                const int k = k0 + cc;
                if (k < Win) {
                    if (jb.Zp == nullptr) {
                        iv = r == 0 ? jb.obs[(size_t)smp * Win + k] : (k == r - 1 ? 1.f : 0.f);
                    } else {
                        float a, d1, d2;
                        lips_act3(jb.act, jb.Zp[(size_t)(row - r) * Win + k], a, d1, d2);
                        iv = r == 0 ? a : d1 * jb.Zp[(size_t)row * Win + k];
                    }
                }
            }
            Dt[rr][cc] = dv;
            It[rr][cc] = iv;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < LIPS_DW_ROWS; ++rr) {
            const float4 dv = *reinterpret_cast<const float4*>(&Dt[rr][ty * 4]);
            const float4 iv = *reinterpret_cast<const float4*>(&It[rr][tx * 4]);
            const float da[4] = {dv.x, dv.y, dv.z, dv.w}, ia[4] = {iv.x, iv.y, iv.z, iv.w};
            const bool primal = (row0 + rr) % NR == 0;   // (rows past row_end hold zeros)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (primal) bacc[i] += da[i];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(da[i], ia[q], acc[i][q]);
            }
        }
        __syncthreads();
    }
    float* pw = jb.pw + (size_t)blockIdx.y * Wout * Win;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = j0 + ty * 4 + i;
        if (j >= Wout) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + tx * 4 + q;
            if (k < Win) pw[(size_t)j * Win + k] = acc[i][q];
        }
        if (tkk == 0 && tx == 0 && jb.pb != nullptr) jb.pb[(size_t)blockIdx.y * Wout + j] = bacc[i];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static bool lips_width_ok(int w) { return w >= 16 && w <= LIPS_MAX_WIDTH && w % 16 == 0; }
static bool lips_act_ok(int a) { return a >= GOPS_ACT_RELU && a <= GOPS_ACT_TANH; }

static int lips_check(const GopsLipsNet& d, int B) {
    if (B < 1) return GOPS_ERR_BAD_ARG;
    const GopsMlp& f = d.mlp;
    if (f.n_layers < 2 || f.n_layers > LIPS_MAX_HIDDEN + 1) return GOPS_ERR_UNSUPPORTED;
    const int n = f.sizes[0], m = f.sizes[f.n_layers];
    if (n < 1 || n > LIPS_MAX_OBS || m < 1 || m > GOPS_MAX_ACT) return GOPS_ERR_UNSUPPORTED;
    if (!lips_act_ok(f.hidden_act) || f.dtype != GOPS_DTYPE_F32 || f.variant_flags != 0) return GOPS_ERR_UNSUPPORTED;
    for (int l = 1; l < f.n_layers; ++l)
        if (!lips_width_ok(f.sizes[l])) return GOPS_ERR_UNSUPPORTED;
    for (int l = 0; l < f.n_layers; ++l) {
        if (f.weight[l] == nullptr || f.bias[l] == nullptr) return GOPS_ERR_BAD_ARG;
        if (l > 0 && ((uintptr_t)f.weight[l] & 15) != 0) return GOPS_ERR_BAD_ARG;   // hidden-layer rows are read 16 bytes at a time
    }
    const GopsMlp& k = d.k_net;
    if (k.n_layers == 0) {
        if (d.k_scalar == nullptr) return GOPS_ERR_BAD_ARG;
    } else {
        if (k.n_layers < 2 || k.n_layers > LIPS_MAX_KHIDDEN + 1) return GOPS_ERR_UNSUPPORTED;
        if (k.sizes[0] != n || k.sizes[k.n_layers] != 1 || k.hidden_act != GOPS_ACT_TANH) return GOPS_ERR_UNSUPPORTED;
        if (k.dtype != GOPS_DTYPE_F32 || k.variant_flags != 0) return GOPS_ERR_UNSUPPORTED;
        for (int l = 1; l < k.n_layers; ++l)
            if (!lips_width_ok(k.sizes[l])) return GOPS_ERR_UNSUPPORTED;
        for (int l = 0; l < k.n_layers; ++l) {
            if (k.weight[l] == nullptr || k.bias[l] == nullptr) return GOPS_ERR_BAD_ARG;
            if (l > 0 && l < k.n_layers - 1 && ((uintptr_t)k.weight[l] & 15) != 0) return GOPS_ERR_BAD_ARG;
        }
    }
    if (!(d.eps >= 0.f)) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

struct LipsPlan {
    size_t Z[LIPS_MAX_HIDDEN], D[LIPS_MAX_HIDDEN], FJ, DO, ZK[LIPS_MAX_KHIDDEN], DK[LIPS_MAX_KHIDDEN], kpre, dkpre, Kws, Nws, y;
    size_t pw[LIPS_DW_MAX_JOBS], pb[LIPS_DW_MAX_JOBS];
    size_t bytes, lds;
    int NTS, Wmax, slabs, slab_samples, L, KL;
};

static LipsPlan lips_plan(const GopsLipsNet& d, int B) {
    LipsPlan pl;
    memset(&pl, 0, sizeof(pl));
    const GopsMlp &f = d.mlp, &k = d.k_net;
    const int n = f.sizes[0], m = f.sizes[f.n_layers], NR = n + 1;
    pl.L = f.n_layers - 1;
    pl.KL = k.n_layers > 0 ? k.n_layers - 1 : 0;
    int wmax = 16;
    for (int l = 1; l <= pl.L; ++l) wmax = f.sizes[l] > wmax ? f.sizes[l] : wmax;
    for (int l = 1; l <= pl.KL; ++l) wmax = k.sizes[l] > wmax ? k.sizes[l] : wmax;   // (the K net's layers pass through the same buffers)
    pl.Wmax = wmax;
    int NTS = 16;
    auto lds_of = [&](int tb) { return sizeof(float) * ((size_t)2 * tb * NR * wmax + (size_t)tb * LIPS_MAX_OBS + (size_t)tb * NR * GOPS_MAX_ACT + tb); };
    while (NTS > 1 && lds_of(NTS) > LIPS_LDS_BUDGET) NTS >>= 1;
    pl.NTS = NTS;
    pl.lds = lds_of(NTS);
    // row slabs of the weight-gradient GEMM: a function of the batch alone (fixed summation order)
    pl.slab_samples = (B + LIPS_DW_MAX_SLABS - 1) / LIPS_DW_MAX_SLABS;
    if (pl.slab_samples < 64) pl.slab_samples = 64;
    pl.slabs = (B + pl.slab_samples - 1) / pl.slab_samples;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += align256(floats * sizeof(float)); return o; };
    const size_t rows = (size_t)B * NR;
    for (int l = 0; l < pl.L; ++l) { pl.Z[l] = take(rows * f.sizes[l + 1]); pl.D[l] = take(rows * f.sizes[l + 1]); }
    pl.FJ = take(rows * m); pl.DO = take(rows * m);
    for (int l = 0; l < pl.KL; ++l) { pl.ZK[l] = take((size_t)B * k.sizes[l + 1]); pl.DK[l] = take((size_t)B * k.sizes[l + 1]); }
    pl.kpre = take(B); pl.dkpre = take(B); pl.Kws = take(B); pl.Nws = take(B); pl.y = take((size_t)B * m);
    int j = 0;
    for (int l = 0; l <= pl.L; ++l, ++j) { pl.pw[j] = take((size_t)pl.slabs * f.sizes[l] * f.sizes[l + 1]); pl.pb[j] = take((size_t)pl.slabs * f.sizes[l + 1]); }
    if (pl.KL > 0)
        for (int l = 0; l <= pl.KL; ++l, ++j) { pl.pw[j] = take((size_t)pl.slabs * k.sizes[l] * k.sizes[l + 1]); pl.pb[j] = take((size_t)pl.slabs * k.sizes[l + 1]); }
    else { pl.pw[j] = 0; pl.pb[j] = take(pl.slabs); }
    pl.bytes = off;
    return pl;
}

static LipsParams lips_params(const GopsLipsNet& d, int B, const LipsPlan& pl, void* ws) {
    LipsParams p;
    memset(&p, 0, sizeof(p));
    const GopsMlp &f = d.mlp, &k = d.k_net;
    p.B = B; p.n = f.sizes[0]; p.m = f.sizes[f.n_layers]; p.L = pl.L; p.act = f.hidden_act; p.NTS = pl.NTS; p.Wmax = pl.Wmax;
    for (int l = 0; l <= f.n_layers; ++l) p.size[l] = f.sizes[l];
    for (int l = 0; l < f.n_layers; ++l) { p.W[l] = f.weight[l]; p.b[l] = f.bias[l]; }
    p.KL = pl.KL;
    if (pl.KL > 0) {
        for (int l = 0; l <= k.n_layers; ++l) p.ksize[l] = k.sizes[l];
        for (int l = 0; l < k.n_layers; ++l) { p.KW[l] = k.weight[l]; p.Kb[l] = k.bias[l]; }
    }
    p.kscalar = d.k_scalar;
    p.eps = d.eps; p.lambda = d.lambda; p.training = d.training ? 1 : 0; p.squash = d.squash ? 1 : 0;
    for (int a = 0; a < GOPS_MAX_ACT; ++a) {   // (high - low) / 2 and (high + low) / 2 in fp32, as the module forms them
        p.half[a] = (d.act_high[a] - d.act_low[a]) / 2.f;
        p.mid[a] = (d.act_high[a] + d.act_low[a]) / 2.f;
    }
    char* w = static_cast<char*>(ws);
    auto at = [&](size_t o) { return reinterpret_cast<float*>(w + o); };
    for (int l = 0; l < pl.L; ++l) { p.Z[l] = at(pl.Z[l]); p.D[l] = at(pl.D[l]); }
    p.FJ = at(pl.FJ); p.DO = at(pl.DO);
    for (int l = 0; l < pl.KL; ++l) { p.ZK[l] = at(pl.ZK[l]); p.DK[l] = at(pl.DK[l]); }
    p.kpre = at(pl.kpre); p.dkpre = at(pl.dkpre); p.Kws = at(pl.Kws); p.Nws = at(pl.Nws); p.y = at(pl.y);
    return p;
}

template <int N> static void lips_launch_fwd(const LipsParams& p, int blocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(lips_fwd_kernel<N>, dim3(blocks), dim3(LIPS_NT), lds, s, p);
}
template <int N> static void lips_launch_bwd(const LipsParams& p, int blocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(lips_bwd_kernel<N>, dim3(blocks), dim3(LIPS_NT), lds, s, p);
}
#define LIPS_SWITCH_N(FN, ...)                  \
    switch (p.n) {                              \
        case 1: FN<1>(__VA_ARGS__); break;      \
        case 2: FN<2>(__VA_ARGS__); break;      \
        case 3: FN<3>(__VA_ARGS__); break;      \
        case 4: FN<4>(__VA_ARGS__); break;      \
        case 5: FN<5>(__VA_ARGS__); break;      \
        case 6: FN<6>(__VA_ARGS__); break;      \
        case 7: FN<7>(__VA_ARGS__); break;      \
        default: FN<8>(__VA_ARGS__); break;     \
    }

extern "C" {

size_t gops_lips_workspace_bytes(const GopsLipsNet* net, int32_t B) {
    if (!net || lips_check(*net, B) != GOPS_OK) return 0;
    return lips_plan(*net, B).bytes;
}

int gops_lips_forward(const GopsLipsNet* net, int32_t B, const float* obs, float* action, float* K, float* N, void* ws, size_t bytes,
                      void* stream) {
    if (net == nullptr) return GOPS_ERR_BAD_ARG;
    const GopsLipsNet& d = *net;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = lips_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (obs == nullptr || action == nullptr) return GOPS_ERR_BAD_ARG;
    const LipsPlan pl = lips_plan(d, B);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    LipsParams p = lips_params(d, B, pl, ws);
    p.obs = obs; p.action = action; p.Kout = K; p.Nout = N;
    const int blocks = (B + pl.NTS - 1) / pl.NTS;
    LIPS_SWITCH_N(lips_launch_fwd, p, blocks, pl.lds, s)
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

int gops_lips_backward(const GopsLipsNet* net, int32_t B, const float* obs, const float* grad_action, const GopsLipsGrad* grad, void* ws,
                       size_t bytes, void* stream) {
    if (net == nullptr || grad == nullptr) return GOPS_ERR_BAD_ARG;
    const GopsLipsNet& d = *net;
    const GopsLipsGrad& g = *grad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = lips_check(d, B);
    if (rc != GOPS_OK) return rc;
    if (obs == nullptr || grad_action == nullptr) return GOPS_ERR_BAD_ARG;
    const GopsMlp &f = d.mlp, &k = d.k_net;
    for (int l = 0; l < f.n_layers; ++l)
        if (g.mlp.weight[l] == nullptr || g.mlp.bias[l] == nullptr) return GOPS_ERR_BAD_ARG;
    for (int l = 0; l < k.n_layers; ++l)
        if (g.k_net.weight[l] == nullptr || g.k_net.bias[l] == nullptr) return GOPS_ERR_BAD_ARG;
    if (k.n_layers == 0 && g.k_scalar == nullptr) return GOPS_ERR_BAD_ARG;
    const LipsPlan pl = lips_plan(d, B);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    LipsParams p = lips_params(d, B, pl, ws);
    p.obs = obs; p.grad_action = grad_action;
    const int blocks = (B + pl.NTS - 1) / pl.NTS;
    LIPS_SWITCH_N(lips_launch_bwd, p, blocks, pl.lds, s)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;

    // weight gradients: one launch over every layer of both nets, then the fixed-order reduce of the slabs' partials
    LipsDwParams dw;
    memset(&dw, 0, sizeof(dw));
    dw.slab_samples = pl.slab_samples;
    char* w = static_cast<char*>(ws);
    auto at = [&](size_t o) { return reinterpret_cast<float*>(w + o); };
    const int NR = p.n + 1;
    int nj = 0, max_tiles = 1;
    auto tiles_of = [](int Win, int Wout) {
        const int tk = Win > 0 ? (Win + LIPS_DW_TILE - 1) / LIPS_DW_TILE : 1;
        return tk * ((Wout + LIPS_DW_TILE - 1) / LIPS_DW_TILE);
    };
    ReduceJobs rj_f, rj_k;
    memset(&rj_f, 0, sizeof(rj_f));
    memset(&rj_k, 0, sizeof(rj_k));
    for (int l = 0; l <= pl.L; ++l, ++nj) {
        LipsDwJob& jb = dw.job[nj];
        jb.Win = f.sizes[l]; jb.Wout = f.sizes[l + 1]; jb.NR = NR; jb.act = f.hidden_act; jb.rows = B * NR;
        jb.D = l < pl.L ? p.D[l] : p.DO;
        jb.Zp = l > 0 ? p.Z[l - 1] : nullptr;
        jb.obs = obs;
        jb.pw = at(pl.pw[nj]); jb.pb = at(pl.pb[nj]);
        const int t = tiles_of(jb.Win, jb.Wout);
        max_tiles = t > max_tiles ? t : max_tiles;
        reduce_jobs_add(rj_f, jb.pw, pl.slabs, 1, jb.Wout * jb.Win, jb.Wout * jb.Win, g.mlp.weight[l]);
        reduce_jobs_add(rj_f, jb.pb, pl.slabs, 1, jb.Wout, jb.Wout, g.mlp.bias[l]);
    }
    if (pl.KL > 0) {
        for (int l = 0; l <= pl.KL; ++l, ++nj) {
            LipsDwJob& jb = dw.job[nj];
            jb.Win = k.sizes[l]; jb.Wout = k.sizes[l + 1]; jb.NR = 1; jb.act = GOPS_ACT_TANH; jb.rows = B;
            jb.D = l < pl.KL ? p.DK[l] : p.dkpre;
            jb.Zp = l > 0 ? p.ZK[l - 1] : nullptr;
            jb.obs = obs;
            jb.pw = at(pl.pw[nj]); jb.pb = at(pl.pb[nj]);
            const int t = tiles_of(jb.Win, jb.Wout);
            max_tiles = t > max_tiles ? t : max_tiles;
            reduce_jobs_add(rj_k, jb.pw, pl.slabs, 1, jb.Wout * jb.Win, jb.Wout * jb.Win, g.k_net.weight[l]);
            reduce_jobs_add(rj_k, jb.pb, pl.slabs, 1, jb.Wout, jb.Wout, g.k_net.bias[l]);
        }
    } else {   // global K: the scalar's gradient is the "bias" sum of d(loss)/d(pre-softplus K) over the batch
        LipsDwJob& jb = dw.job[nj];
        jb.Win = 0; jb.Wout = 1; jb.NR = 1; jb.act = GOPS_ACT_LINEAR; jb.rows = B;
        jb.D = p.dkpre; jb.Zp = nullptr; jb.obs = obs; jb.pw = at(pl.pb[nj]); jb.pb = at(pl.pb[nj]);
        reduce_jobs_add(rj_k, jb.pb, pl.slabs, 1, 1, 1, g.k_scalar);
        ++nj;
    }
    hipLaunchKernelGGL(lips_dw_kernel, dim3(max_tiles, pl.slabs, nj), dim3(LIPS_NT), 0, s, dw);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = launch_reduce(rj_f, s)) != hipSuccess) return (int)e;
    e = launch_reduce(rj_k, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
