// Polynomial approximators (gops/apprfunc/poly.py) on the model rollout: one LANE per trajectory.
//
// A POLY policy is one Linear layer over a feature map of the observation (no hidden layer, no tanh squash); a POLY value is
// one Linear layer over the quadratic terms of the normalised observation.  At the shipped sizes (B = 64, a handful of
// parameters) a 16-row MFMA tile is the wrong shape: every lane walks ITS trajectory through the horizon with the per-lane
// model functions of env_models.h and the wrapper helpers of common.h, the weights are wave-uniform scalar loads, and the
// weight gradient is accumulated in registers across the horizon.
//
//   poly_fwd_kernel   features -> a = W phi (+ (t+1) column) (+ b) -> wrap_action -> wrapped model step, as env_step_kernel
//                     (aux_kernels.hip); sum_t gamma^t r_t (+ the optional tail (~done_H) gamma^H V(obs_H)).  With need_grad the
//                     observation each step starts from and its done flag are stashed as [t][i][B] / [t][B] (a wave's store is
//                     256 contiguous bytes).
//   poly_bwd_kernel   the same lane walks the horizon backwards: model adjoints recomputed from the stashed observation (the
//                     idpendulum sub-steps included), wrap_action_bwd, g_phi = W^T g_a, g_x += (d phi / d x)^T g_phi; dW += g_a phi
//                     in registers; per-block partial rows in a fixed order (wave butterfly, then the four waves in order).
//   reduce_partials_kernel (dw_gemm.hip) sums the blocks' rows in a fixed order: the gradient is bitwise reproducible.
//
// Instantiated per (env kind, obs_dim N, degree): each kernel carries only its own model's arithmetic.
// Bounds (template parameters, everything else is refused by the host code with GOPS_ERR_UNSUPPORTED): obs_dim N <= 6;
// degree 1 and 2 for every N, degree 3 for N <= 3 (F = N + N^2 + N^3 <= 39); act_dim <= GOPS_MAX_ACT.  The gradient registers are
// [GOPS_MAX_ACT][F + 2] (<= 176 floats at N = 6, degree 2).
#include <math.h>
#include <string.h>

#include "common.h"
#include "env_models.h"
#include "launchers.h"

#define POLY_THREADS 256

template <int N, int D>
__host__ __device__ constexpr int poly_feat_dim() { return D == 1 ? N : (D == 2 ? N + N * N : N + N * N + N * N * N); }
template <int N>
__host__ __device__ constexpr int poly_sym_dim() { return N * (N + 1) / 2; }

struct PolyParams {
    GopsEnv env;                 // padded (lq_pad_env)
    int B, H, A, fh, need_grad, tail, tail_unmasked, ldw;
    const float* W;              // [A][ldw], ldw = F + fh
    const float* b;              // [A] or null
    const float* Wv;             // tail value [1][N(N+1)/2]
    const float* bv;             // [1] or null
    const float* norm;           // [N] or null
    const float* obs;            // [B][N]
    const float* done;           // [B] or null
    const float* grad_v;         // backward: [B]
    float* v_pi;                 // [B]
    float* rewards;              // [H][B] or null
    float* final_obs;            // [B][N] or null
    float* final_done;           // [B] or null
    float* st_obs;               // [H + 1][N][B]
    float* st_done;              // [H + 1][B]
    float* part_w;               // [blocks][A * ldw]
    float* part_b;               // [blocks][A]
    float gpow[GOPS_MAX_HORIZON + 1];
};
static_assert(sizeof(PolyParams) <= 4000, "PolyParams outgrew the kernel-argument segment");

// ---- feature maps -----------------------------------------------------------------------------
// make_features (poly.py:30-49): degree k block = the k-fold outer product in n_matmul order, i-major; degree 3 = (x_i x_j) x_l.
template <int N, int D>
__device__ __forceinline__ void poly_features(const float (&x)[N], float (&phi)[poly_feat_dim<N, D>()]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) phi[k++] = x[i];
    if constexpr (D >= 2) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) phi[k++] = x[i] * x[j];
    }
    if constexpr (D >= 3) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float xij = x[i] * x[j];
#pragma unroll
                for (int l = 0; l < N; ++l) phi[k++] = xij * x[l];
            }
    }
}
// adjoint: g_x += (d phi / d x)^T g_phi
template <int N, int D>
__device__ __forceinline__ void poly_features_bwd(const float (&x)[N], const float (&gphi)[poly_feat_dim<N, D>()], float (&gx)[N]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) gx[i] += gphi[k++];
    if constexpr (D >= 2) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float g = gphi[k++];
                gx[i] += g * x[j];
                gx[j] += g * x[i];
            }
    }
    if constexpr (D >= 3) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float xij = x[i] * x[j];
                float gij = 0.f;
#pragma unroll
                for (int l = 0; l < N; ++l) {
                    const float g = gphi[k++];
                    gij += g * x[l];
                    gx[l] += g * xij;
                }
                gx[i] += gij * x[j];
                gx[j] += gij * x[i];
            }
    }
}
// create_features(obs * norm_matrix, 2) (poly.py:61-83): x_i x_j for i <= j, i-major
template <int N>
__device__ __forceinline__ float poly_value(const float* Wv, const float* bv, const float* norm, const float (&o)[N], float (&y)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = norm != nullptr ? o[i] * norm[i] : o[i];
    float v = 0.f;
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) v += Wv[k++] * (y[i] * y[j]);
    if (bv != nullptr) v += bv[0];
    return v;
}
// d V / d o into go (overwritten); y as poly_value left it
template <int N>
__device__ __forceinline__ void poly_value_bwd_x(const float* Wv, const float* norm, const float (&y)[N], float g, float (&go)[N]) {
    float gy[N];
#pragma unroll
    for (int i = 0; i < N; ++i) gy[i] = 0.f;
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i; j < N; ++j) {
            const float gk = g * Wv[k++];
            gy[i] += gk * y[j];
            gy[j] += gk * y[i];
        }
#pragma unroll
    for (int i = 0; i < N; ++i) go[i] = norm != nullptr ? gy[i] * norm[i] : gy[i];
}

// pre-wrapper actions of the policy at observation x, step t
template <int N, int D>
__device__ __forceinline__ void poly_policy(const PolyParams& p, const float (&phi)[poly_feat_dim<N, D>()], int t, float (&abar)[GOPS_MAX_ACT]) {
    constexpr int F = poly_feat_dim<N, D>();
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) {
        float acc = 0.f;
        if (a < p.A) {
            const float* w = p.W + a * p.ldw;
#pragma unroll
            for (int k = 0; k < F; ++k) acc += w[k] * phi[k];
            if (p.fh) acc += w[F] * (float)(t + 1);   // FiniteHorizonPolicy: virtual_t = step + 1, appended after the features
            if (p.b != nullptr) acc += p.b[a];
        }
        abar[a] = acc;
    }
}

// ---- forward rollout -----------------------------------------------------------------------------------------------------------
template <int ENV, int N, int D>
__global__ __launch_bounds__(POLY_THREADS) void poly_fwd_kernel(const PolyParams p) {
    constexpr int F = poly_feat_dim<N, D>();
    const int b = blockIdx.x * POLY_THREADS + threadIdx.x;
    if (b >= p.B) return;   // (no block-wide step in this kernel)
    const size_t B = (size_t)p.B;
    const bool nomask = p.env.no_mask_at_done != 0;
    float o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = p.obs[(size_t)b * N + i];
    bool dn = !nomask && p.done != nullptr && p.done[b] != 0.f;
    bool done_last = false;
    float v = 0.f;
#pragma unroll 1
    for (int t = 0; t < p.H; ++t) {
        if (p.need_grad) {
#pragma unroll
            for (int i = 0; i < N; ++i) p.st_obs[((size_t)t * N + i) * B + b] = o[i];
            p.st_done[(size_t)t * B + b] = dn ? 1.f : 0.f;
        }
        float phi[F], abar[GOPS_MAX_ACT], u[GOPS_MAX_ACT];
        poly_features<N, D>(o, phi);
        poly_policy<N, D>(p, phi, t, abar);
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) u[a] = a < p.A ? wrap_action(p.env, a, abar[a]) : 0.f;
        float on[N], r;
        bool done_m;
        state_model_step<ENV, N>(p.env, o, u, dn, on, r, done_m);
        float rr = dn ? 0.f : r;
        if (p.env.shaping) rr = (rr + p.env.reward_shift) * p.env.reward_scale;
        v += rr * p.gpow[t];
        if (p.rewards != nullptr) p.rewards[(size_t)t * B + b] = rr;
        dn = dn || (done_m && !nomask);
        done_last = done_m;
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = on[i];
    }
    // no MaskAtDoneModel: final_done (and the tail's mask) is the base model's done test on the last state
    const bool dH = nomask ? done_last : dn;
    if (p.tail) {
        float y[N];
        const float vt = poly_value<N>(p.Wv, p.bv, p.norm, o, y);
        v += ((p.tail_unmasked ? 1.f : (dH ? 0.f : 1.f)) * p.gpow[p.H]) * vt;
    }
    if (p.need_grad) {
#pragma unroll
        for (int i = 0; i < N; ++i) p.st_obs[((size_t)p.H * N + i) * B + b] = o[i];
        p.st_done[(size_t)p.H * B + b] = dH ? 1.f : 0.f;
    }
    p.v_pi[b] = v;
    if (p.final_obs != nullptr)
#pragma unroll
        for (int i = 0; i < N; ++i) p.final_obs[(size_t)b * N + i] = o[i];
    if (p.final_done != nullptr) p.final_done[b] = dH ? 1.f : 0.f;
}

// ---- backward sweep ------------------------------------------------------------------------------------------------------------
template <int ENV, int N, int D>
__global__ __launch_bounds__(POLY_THREADS) void poly_bwd_kernel(const PolyParams p) {
    constexpr int F = poly_feat_dim<N, D>();
    constexpr int FP = F + 2;   // features, (t+1) column, bias
    __shared__ float red[4 * GOPS_MAX_ACT * FP];
    const int b = blockIdx.x * POLY_THREADS + threadIdx.x;
    const bool valid = b < p.B;
    const size_t B = (size_t)p.B;
    float gw[GOPS_MAX_ACT][FP];
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a)
#pragma unroll
        for (int k = 0; k < FP; ++k) gw[a][k] = 0.f;
    if (valid) {
        const float gv = p.grad_v[b];
        float go[N], o[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { go[i] = 0.f; o[i] = p.st_obs[((size_t)p.H * N + i) * B + b]; }
        if (p.tail) {
            const bool dH = p.st_done[(size_t)p.H * B + b] != 0.f;
            const float gV = gv * ((p.tail_unmasked ? 1.f : (dH ? 0.f : 1.f)) * p.gpow[p.H]);
            float y[N];
            (void)poly_value<N>(p.Wv, p.bv, p.norm, o, y);
            poly_value_bwd_x<N>(p.Wv, p.norm, y, gV, go);
        }
#pragma unroll 1
        for (int t = p.H - 1; t >= 0; --t) {
#pragma unroll
            for (int i = 0; i < N; ++i) o[i] = p.st_obs[((size_t)t * N + i) * B + b];
            const bool dn = p.st_done[(size_t)t * B + b] != 0.f;
            float phi[F], abar[GOPS_MAX_ACT], u[GOPS_MAX_ACT];
            poly_features<N, D>(o, phi);
            poly_policy<N, D>(p, phi, t, abar);
#pragma unroll
            for (int a = 0; a < GOPS_MAX_ACT; ++a) u[a] = a < p.A ? wrap_action(p.env, a, abar[a]) : 0.f;
            float g_r = gv * p.gpow[t];   // adjoint of the shaped reward
            if (p.env.shaping) g_r *= p.env.reward_scale;
            float gu[GOPS_MAX_ACT], gx[N];
            state_model_step_bwd<ENV, N>(p.env, o, u, dn, g_r, go, gx, gu);
            float ga[GOPS_MAX_ACT], gphi[F];
#pragma unroll
            for (int a = 0; a < GOPS_MAX_ACT; ++a) ga[a] = a < p.A ? wrap_action_bwd(p.env, a, abar[a], gu[a]) : 0.f;
#pragma unroll
            for (int k = 0; k < F; ++k) gphi[k] = 0.f;
            const float tt = (float)(t + 1);
#pragma unroll
            for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                if (a < p.A) {
                    const float* w = p.W + a * p.ldw;
#pragma unroll
                    for (int k = 0; k < F; ++k) {
                        gphi[k] += w[k] * ga[a];
                        gw[a][k] += ga[a] * phi[k];
                    }
                    gw[a][F] += ga[a] * tt;
                    gw[a][F + 1] += ga[a];
                }
            }
            poly_features_bwd<N, D>(o, gphi, gx);
#pragma unroll
            for (int i = 0; i < N; ++i) go[i] = gx[i];
        }
    }
    // per-block partial rows, fixed order: butterfly inside each wave, then the four waves in order
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a)
#pragma unroll
        for (int k = 0; k < FP; ++k) wave_sum(gw[a][k], red, a * FP + k, GOPS_MAX_ACT * FP);
    __syncthreads();
    const int A = p.A, ldw = p.ldw;
    for (int e = threadIdx.x; e < A * FP; e += POLY_THREADS) {
        const int a = e / FP, k = e - a * FP;
        constexpr int S = GOPS_MAX_ACT * FP;
        const float s = (red[e] + red[S + e]) + (red[2 * S + e] + red[3 * S + e]);
        if (k < F || (k == F && p.fh)) p.part_w[(size_t)blockIdx.x * A * ldw + a * ldw + k] = s;
        else if (k == F + 1 && p.part_b != nullptr) p.part_b[(size_t)blockIdx.x * A + a] = s;
    }
}

// ---- POLY StateValue over a batch (INFADP's policy evaluation) -------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(POLY_THREADS) void poly_value_fwd_kernel(const float* Wv, const float* bv, const float* norm, int B,
                                                                      const float* obs, float* v) {
    const int b = blockIdx.x * POLY_THREADS + threadIdx.x;
    if (b >= B) return;
    float o[N], y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = obs[(size_t)b * N + i];
    v[b] = poly_value<N>(Wv, bv, norm, o, y);
}

template <int N>
__global__ __launch_bounds__(POLY_THREADS) void poly_value_bwd_kernel(const float* norm, int B, const float* obs, const float* grad_v,
                                                                      float* part_w, float* part_b) {
    constexpr int K = poly_sym_dim<N>();
    __shared__ float red[4 * (K + 1)];
    const int b = blockIdx.x * POLY_THREADS + threadIdx.x;
    float acc[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) acc[k] = 0.f;
    if (b < B) {
        const float g = grad_v[b];
        float y[N];
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = norm != nullptr ? obs[(size_t)b * N + i] * norm[i] : obs[(size_t)b * N + i];
        int k = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i; j < N; ++j) acc[k++] = g * (y[i] * y[j]);
        acc[K] = g;
    }
#pragma unroll
    for (int k = 0; k <= K; ++k) wave_sum(acc[k], red, k, K + 1);
    __syncthreads();
    const int e = threadIdx.x;
    if (e <= K) {
        const float s = (red[e] + red[(K + 1) + e]) + (red[2 * (K + 1) + e] + red[3 * (K + 1) + e]);
        if (e < K) part_w[(size_t)blockIdx.x * K + e] = s;
        else if (part_b != nullptr) part_b[blockIdx.x] = s;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

static int poly_blocks(int B) { return (B + POLY_THREADS - 1) / POLY_THREADS; }

// feature degree of a GopsMlp.hidden_act code, 0 = not a make_features code
static int poly_full_degree(int code) {
    return code == GOPS_POLY_FULL_1 ? 1 : code == GOPS_POLY_FULL_2 ? 2 : code == GOPS_POLY_FULL_3 ? 3 : 0;
}
static bool poly_shape_ok(int n, int deg) { return n >= 1 && n <= 6 && deg >= 1 && deg <= 3 && (deg < 3 || n <= 3); }
static int poly_feat_dim_rt(int n, int deg) { return deg == 1 ? n : deg == 2 ? n + n * n : n + n * n + n * n * n; }

// (n_layers = 1 alone does not make a POLY net: an RBF net of rollout_rbf.hip has it too, with a GOPS_RBF_* code)
bool poly_is_net(const GopsMlp& m) { return m.n_layers == 1 && (poly_full_degree(m.hidden_act) != 0 || m.hidden_act == GOPS_POLY_SYM_2); }

int poly_check_value(const GopsMlp& v, int obs_dim) {
    if (v.n_layers != 1 || v.hidden_act != GOPS_POLY_SYM_2) return GOPS_ERR_UNSUPPORTED;
    if (v.sizes[0] != obs_dim || v.sizes[1] != 1 || obs_dim < 1 || obs_dim > 6) return GOPS_ERR_UNSUPPORTED;
    if (v.sizes[2] != obs_dim * (obs_dim + 1) / 2) return GOPS_ERR_BAD_ARG;   // weight columns: the layout the kernels read
    if (v.weight[0] == nullptr) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

int poly_check_desc(const GopsRolloutDesc& d) {
    const int rc = state_model_check_desc(d);   // (env_models.h: shape, fp32, closed loop, the model envs of the per-lane step)
    if (rc != GOPS_OK) return rc;
    const GopsEnv& e = d.env;
    const int n = e.obs_dim;
    const GopsMlp& m = d.policy;
    const int deg = poly_full_degree(m.hidden_act);
    if (m.n_layers != 1 || deg == 0 || !poly_shape_ok(n, deg)) return GOPS_ERR_UNSUPPORTED;
    if (m.sizes[0] != n || m.sizes[1] != e.act_dim) return GOPS_ERR_UNSUPPORTED;
    // weight columns = features (+ the virtual_t column of a FiniteHorizonPolicy): a DetermPolicy in a finite-horizon rollout, or a
    // FiniteHorizonPolicy in an infinite-horizon one, would be read with the wrong row stride
    if (m.sizes[2] != poly_feat_dim_rt(n, deg) + (d.finite_horizon ? 1 : 0)) return GOPS_ERR_BAD_ARG;
    if (m.weight[0] == nullptr) return GOPS_ERR_BAD_ARG;
    if (d.tail_value) return poly_check_value(d.value, n);   // (a POLY policy with an MLP value, or the reverse: refused)
    return GOPS_OK;
}

struct PolyPlan {
    size_t obs, done, pw, pb, bytes;
    int blocks, ldw;
};
static PolyPlan poly_plan(const GopsRolloutDesc& d) {
    PolyPlan pl;
    const int n = d.env.obs_dim, A = d.env.act_dim, B = d.batch, H = d.horizon;
    pl.blocks = poly_blocks(B);
    pl.ldw = poly_feat_dim_rt(n, poly_full_degree(d.policy.hidden_act)) + (d.finite_horizon ? 1 : 0);
    size_t off = 0;
    pl.obs = off; off += align256((size_t)(H + 1) * n * B * sizeof(float));
    pl.done = off; off += align256((size_t)(H + 1) * B * sizeof(float));
    pl.pw = off; off += align256((size_t)pl.blocks * A * pl.ldw * sizeof(float));
    pl.pb = off; off += align256((size_t)pl.blocks * A * sizeof(float));
    pl.bytes = off;
    return pl;
}

extern "C" size_t gops_poly_rollout_workspace_bytes(const GopsRolloutDesc* desc) {
    if (!desc || poly_check_desc(*desc) != GOPS_OK) return 0;
    return poly_plan(*desc).bytes;
}

static PolyParams poly_params(const GopsRolloutDesc& d, const PolyPlan& pl, void* ws) {
    PolyParams p;
    memset(&p, 0, sizeof(p));
    p.env = d.env;
    lq_pad_env(p.env);
    p.B = d.batch; p.H = d.horizon; p.A = d.env.act_dim; p.fh = d.finite_horizon ? 1 : 0;
    p.need_grad = d.need_grad; p.tail = d.tail_value; p.tail_unmasked = d.tail_unmasked; p.ldw = pl.ldw;
    p.W = d.policy.weight[0]; p.b = d.policy.bias[0];
    if (d.tail_value) { p.Wv = d.value.weight[0]; p.bv = d.value.bias[0]; p.norm = d.value.weight[1]; }
    char* w = static_cast<char*>(ws);
    p.st_obs = reinterpret_cast<float*>(w + pl.obs);
    p.st_done = reinterpret_cast<float*>(w + pl.done);
    p.part_w = reinterpret_cast<float*>(w + pl.pw);
    p.part_b = reinterpret_cast<float*>(w + pl.pb);
    for (int t = 0; t <= p.H; ++t) p.gpow[t] = (float)pow(d.gamma, (double)t);   // gamma^t formed in double, then rounded
    return p;
}

template <template <int, int, int> class Launch>
static hipError_t poly_dispatch(int kind, int n, int deg, const PolyParams& p, hipStream_t s) {
    // one instantiation per (env kind, observation width, degree): the kernels carry only their own model's arithmetic
#define POLY_CASE(EE, NN, DD) if (kind == EE && n == NN && deg == DD) return Launch<EE, NN, DD>::run(p, s);
    POLY_CASE(GOPS_ENV_LQ, 1, 1) POLY_CASE(GOPS_ENV_LQ, 2, 1) POLY_CASE(GOPS_ENV_LQ, 3, 1)
    POLY_CASE(GOPS_ENV_LQ, 4, 1) POLY_CASE(GOPS_ENV_LQ, 5, 1) POLY_CASE(GOPS_ENV_LQ, 6, 1)
    POLY_CASE(GOPS_ENV_LQ, 1, 2) POLY_CASE(GOPS_ENV_LQ, 2, 2) POLY_CASE(GOPS_ENV_LQ, 3, 2)
    POLY_CASE(GOPS_ENV_LQ, 4, 2) POLY_CASE(GOPS_ENV_LQ, 5, 2) POLY_CASE(GOPS_ENV_LQ, 6, 2)
    POLY_CASE(GOPS_ENV_LQ, 1, 3) POLY_CASE(GOPS_ENV_LQ, 2, 3) POLY_CASE(GOPS_ENV_LQ, 3, 3)
    POLY_CASE(GOPS_ENV_IDPENDULUM, 6, 1) POLY_CASE(GOPS_ENV_IDPENDULUM, 6, 2)
    POLY_CASE(GOPS_ENV_CARTPOLE, 4, 1) POLY_CASE(GOPS_ENV_CARTPOLE, 4, 2)
    POLY_CASE(GOPS_ENV_PENDULUM, 3, 1) POLY_CASE(GOPS_ENV_PENDULUM, 3, 2) POLY_CASE(GOPS_ENV_PENDULUM, 3, 3)
#undef POLY_CASE
    return hipErrorInvalidValue;
}
template <int E, int N, int D> struct PolyFwd {
    static hipError_t run(const PolyParams& p, hipStream_t s) {
        hipLaunchKernelGGL((poly_fwd_kernel<E, N, D>), dim3(poly_blocks(p.B)), dim3(POLY_THREADS), 0, s, p);
        return hipGetLastError();
    }
};
template <int E, int N, int D> struct PolyBwd {
    static hipError_t run(const PolyParams& p, hipStream_t s) {
        hipLaunchKernelGGL((poly_bwd_kernel<E, N, D>), dim3(poly_blocks(p.B)), dim3(POLY_THREADS), 0, s, p);
        return hipGetLastError();
    }
};

extern "C" {

int gops_poly_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in_p, const GopsRolloutOut* out_p, void* ws, size_t bytes,
                              void* stream) {
    if (!desc || !in_p || !out_p) return GOPS_ERR_BAD_ARG;
    const GopsRolloutDesc& d = *desc;
    const GopsRolloutIn& in = *in_p;
    const GopsRolloutOut& out = *out_p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = poly_check_desc(d);
    if (rc != GOPS_OK) return rc;
    if (in.obs == nullptr || out.v_pi == nullptr) return GOPS_ERR_BAD_ARG;
    const PolyPlan pl = poly_plan(d);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    PolyParams p = poly_params(d, pl, ws);
    p.obs = in.obs; p.done = in.done;
    p.v_pi = out.v_pi; p.rewards = out.rewards; p.final_obs = out.final_obs; p.final_done = out.final_done;
    const hipError_t e = poly_dispatch<PolyFwd>(d.env.kind, d.env.obs_dim, poly_full_degree(d.policy.hidden_act), p, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

int gops_poly_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v, const GopsMlpGrad* grad,
                               void* ws, size_t bytes, void* stream) {
    if (!desc || !in || !grad) return GOPS_ERR_BAD_ARG;   // (`in` is not read: the forward stashed what the sweep needs)
    const GopsRolloutDesc& d = *desc;
    const GopsMlpGrad& g = *grad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = poly_check_desc(d);
    if (rc != GOPS_OK) return rc;
    if (!d.need_grad || grad_v == nullptr || g.weight[0] == nullptr) return GOPS_ERR_BAD_ARG;
    if ((d.policy.bias[0] != nullptr) != (g.bias[0] != nullptr)) return GOPS_ERR_BAD_ARG;
    const PolyPlan pl = poly_plan(d);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    PolyParams p = poly_params(d, pl, ws);
    p.grad_v = grad_v;
    if (d.policy.bias[0] == nullptr) p.part_b = nullptr;
    hipError_t e = poly_dispatch<PolyBwd>(d.env.kind, d.env.obs_dim, poly_full_degree(d.policy.hidden_act), p, s);
    if (e != hipSuccess) return (int)e;
    ReduceJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    const int A = d.env.act_dim;
    reduce_jobs_add(jobs, p.part_w, pl.blocks, 1, A * pl.ldw, A * pl.ldw, g.weight[0]);
    if (g.bias[0] != nullptr) reduce_jobs_add(jobs, p.part_b, pl.blocks, 1, A, A, g.bias[0]);
    e = launch_reduce(jobs, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

size_t gops_poly_value_workspace_bytes(const GopsMlp* value, int32_t B) {
    if (!value) return 0;
    const GopsMlp& v = *value;
    if (B < 1 || poly_check_value(v, v.sizes[0]) != GOPS_OK) return 0;
    const int K = v.sizes[0] * (v.sizes[0] + 1) / 2;
    return align256((size_t)poly_blocks(B) * K * sizeof(float)) + align256((size_t)poly_blocks(B) * sizeof(float));
}

int gops_poly_value_forward(const GopsMlp* value, int32_t B, const float* obs, float* out, void* stream) {
    if (!value) return GOPS_ERR_BAD_ARG;
    const GopsMlp& v = *value;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B < 1 || obs == nullptr || out == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = poly_check_value(v, v.sizes[0]);
    if (rc != GOPS_OK) return rc;
    const float *W = v.weight[0], *bv = v.bias[0], *nm = v.weight[1];
    const dim3 g(poly_blocks(B)), t(POLY_THREADS);
    switch (v.sizes[0]) {
        case 1: hipLaunchKernelGGL(poly_value_fwd_kernel<1>, g, t, 0, s, W, bv, nm, B, obs, out); break;
        case 2: hipLaunchKernelGGL(poly_value_fwd_kernel<2>, g, t, 0, s, W, bv, nm, B, obs, out); break;
        case 3: hipLaunchKernelGGL(poly_value_fwd_kernel<3>, g, t, 0, s, W, bv, nm, B, obs, out); break;
        case 4: hipLaunchKernelGGL(poly_value_fwd_kernel<4>, g, t, 0, s, W, bv, nm, B, obs, out); break;
        case 5: hipLaunchKernelGGL(poly_value_fwd_kernel<5>, g, t, 0, s, W, bv, nm, B, obs, out); break;
        default: hipLaunchKernelGGL(poly_value_fwd_kernel<6>, g, t, 0, s, W, bv, nm, B, obs, out); break;
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GOPS_OK : (int)e;
}

int gops_poly_value_backward(const GopsMlp* value, int32_t B, const float* obs, const float* grad_v, const GopsMlpGrad* grad, void* ws,
                             size_t bytes, void* stream) {
    if (!value || !grad) return GOPS_ERR_BAD_ARG;
    const GopsMlp& v = *value;
    const GopsMlpGrad& g = *grad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B < 1 || obs == nullptr || grad_v == nullptr || g.weight[0] == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = poly_check_value(v, v.sizes[0]);
    if (rc != GOPS_OK) return rc;
    if ((v.bias[0] != nullptr) != (g.bias[0] != nullptr)) return GOPS_ERR_BAD_ARG;
    const size_t need = gops_poly_value_workspace_bytes(value, B);
    if (ws == nullptr || bytes < need) return GOPS_ERR_WORKSPACE;
    const int n = v.sizes[0], K = n * (n + 1) / 2, nb = poly_blocks(B);
    float* pw = static_cast<float*>(ws);
    float* pb = g.bias[0] != nullptr ? reinterpret_cast<float*>(static_cast<char*>(ws) + align256((size_t)nb * K * sizeof(float))) : nullptr;
    const float* nm = v.weight[1];
    const dim3 gr(nb), t(POLY_THREADS);
    switch (n) {
        case 1: hipLaunchKernelGGL(poly_value_bwd_kernel<1>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
        case 2: hipLaunchKernelGGL(poly_value_bwd_kernel<2>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
        case 3: hipLaunchKernelGGL(poly_value_bwd_kernel<3>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
        case 4: hipLaunchKernelGGL(poly_value_bwd_kernel<4>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
        case 5: hipLaunchKernelGGL(poly_value_bwd_kernel<5>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
        default: hipLaunchKernelGGL(poly_value_bwd_kernel<6>, gr, t, 0, s, nm, B, obs, grad_v, pw, pb); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    ReduceJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    reduce_jobs_add(jobs, pw, nb, 1, K, K, g.weight[0]);
    if (pb != nullptr) reduce_jobs_add(jobs, pb, nb, 1, 1, 1, g.bias[0]);
    e = launch_reduce(jobs, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
