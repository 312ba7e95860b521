// Polynomial approximators (gops/apprfunc/poly.py) on the model rollout: one LANE per trajectory.
//
// A POLY policy is one Linear layer over a feature map of the observation (no hidden layer, no tanh squash); a POLY value is
// one Linear layer over the quadratic terms of the normalised observation.  At the shipped sizes (B = 64, a handful of
// parameters) a 16-row MFMA tile is the wrong shape: every lane walks ITS trajectory through the horizon with the per-lane
// model functions of env_models.h and the wrapper helpers of common.h, the weights are wave-uniform scalar loads, and the
// weight gradient is accumulated in registers across the horizon.
//
//   poly_fwd_kernel   the forward walk of lane_rollout.h with a = W phi (+ (t+1) column) (+ b) as its policy, and the optional
//                     tail (~done_H) gamma^H V(obs_H) on top of sum_t gamma^t r_t.
//   poly_bwd_kernel   the backward walk: g_phi = W^T g_a, g_x += (d phi / d x)^T g_phi; dW += g_a phi in registers; per-block
//                     partial rows in a fixed order (wave butterfly, then the four waves in order).
//   reduce_partials_kernel (dw_gemm.hip) sums the blocks' rows in a fixed order: the gradient is bitwise reproducible.
//
// Instantiated per (env kind, obs_dim N, degree): each kernel carries only its own model's arithmetic.
// Bounds (template parameters, everything else is refused by the host code with GOPS_ERR_UNSUPPORTED): obs_dim N <= 6;
// degree 1 and 2 for every N, degree 3 for N <= 3 (F = N + N^2 + N^3 <= 39); act_dim <= GOPS_MAX_ACT.  The gradient registers are
// [GOPS_MAX_ACT][F + 2] (<= 176 floats at N = 6, degree 2).
#include "lane_rollout.h"
#include "launchers.h"

template <int N, int D>
__host__ __device__ constexpr int poly_feat_dim() { return D == 1 ? N : (D == 2 ? N + N * N : N + N * N + N * N * N); }
template <int N>
__host__ __device__ constexpr int poly_sym_dim() { return N * (N + 1) / 2; }

struct PolyParams {
    GopsEnv env;                 // padded (lq_pad_env); the POLY kernels read it through the kernel argument
    int fh, tail, tail_unmasked, ldw;
    const float* W;              // [A][ldw], ldw = F + fh
    const float* b;              // [A] or null
    const float* Wv;             // tail value [1][N(N+1)/2]
    const float* bv;             // [1] or null
    const float* norm;           // [N] or null
    float* part_w;               // [blocks][A * ldw]
    float* part_b;               // [blocks][A]
    LaneParams l;                // last, as gpow[] was: ahead of the net's fields, poly_fwd_kernel<LQ, 2, 2> reserves a stack frame
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

// the features (a step's State of the walks) and the pre-wrapper actions of the policy at observation o, step t
template <int N, int D>
struct PolyStep {
    float phi[poly_feat_dim<N, D>()];
};
template <int N, int D>
__device__ __forceinline__ void poly_policy(const PolyParams& p, const float (&o)[N], int t, float (&phi)[poly_feat_dim<N, D>()],
                                            float (&abar)[GOPS_MAX_ACT]) {
    constexpr int F = poly_feat_dim<N, D>();
    poly_features<N, D>(o, phi);
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) {
        float acc = 0.f;
        if (a < p.l.A) {
            const float* w = p.W + a * p.ldw;
#pragma unroll
            for (int k = 0; k < F; ++k) acc += w[k] * phi[k];
            if (p.fh) acc += w[F] * (float)(t + 1);   // FiniteHorizonPolicy: virtual_t = step + 1, appended after the features
            if (p.b != nullptr) acc += p.b[a];
        }
        abar[a] = acc;
    }
}
// the tail's weight on V(obs_H): (~done_H) gamma^H, or gamma^H alone (tail_unmasked)
__device__ __forceinline__ float poly_tail_weight(const PolyParams& p, bool dH) {
    return (p.tail_unmasked ? 1.f : (dH ? 0.f : 1.f)) * p.l.gpow[p.l.H];
}

// ---- forward rollout -----------------------------------------------------------------------------------------------------------
template <int ENV, int N, int D>
__global__ __launch_bounds__(LANE_THREADS) void poly_fwd_kernel(const PolyParams p) {
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
    if (b >= p.l.B) return;   // (no block-wide step in this kernel)
    using Step = PolyStep<N, D>;
    LANE_FORWARD_LOOP(p.env, p.l, Step, (poly_policy<N, D>(p, o, t, st.phi, abar)))
    if (p.tail) {
        float y[N];
        const float vt = poly_value<N>(p.Wv, p.bv, p.norm, o, y);
        v += poly_tail_weight(p, dH) * vt;
    }
    LANE_FORWARD_FINISH(p.l)
}

// ---- backward sweep ------------------------------------------------------------------------------------------------------------
template <int ENV, int N, int D>
__global__ __launch_bounds__(LANE_THREADS) void poly_bwd_kernel(const PolyParams p) {
    constexpr int F = poly_feat_dim<N, D>();
    constexpr int FP = F + 2;   // features, (t+1) column, bias
    __shared__ float red[4 * GOPS_MAX_ACT * FP];
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
    float gw[GOPS_MAX_ACT][FP];
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a)
#pragma unroll
        for (int k = 0; k < FP; ++k) gw[a][k] = 0.f;
    if (b < p.l.B) {   // (every thread takes part in the block reduction below)
        lane_backward<ENV, N, PolyStep<N, D>>(
            p.env, p.l, b,
            [&](const float (&o)[N], int t, PolyStep<N, D>& st, float (&abar)[GOPS_MAX_ACT]) { poly_policy<N, D>(p, o, t, st.phi, abar); },
            [&](int t, const float (&o)[N], const PolyStep<N, D>& st, const float (&ga)[GOPS_MAX_ACT], float (&gx)[N]) {
                float gphi[F];
#pragma unroll
                for (int k = 0; k < F; ++k) gphi[k] = 0.f;
                const float tt = (float)(t + 1);
#pragma unroll
                for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                    if (a < p.l.A) {
                        const float* w = p.W + a * p.ldw;
#pragma unroll
                        for (int k = 0; k < F; ++k) {
                            gphi[k] += w[k] * ga[a];
                            gw[a][k] += ga[a] * st.phi[k];
                        }
                        gw[a][F] += ga[a] * tt;
                        gw[a][F + 1] += ga[a];
                    }
                }
                poly_features_bwd<N, D>(o, gphi, gx);
            },
            [&](float gv, float (&go)[N]) {
                if (p.tail) {
                    const size_t B = (size_t)p.l.B;
                    float o[N], y[N];
#pragma unroll
                    for (int i = 0; i < N; ++i) o[i] = p.l.st_obs[((size_t)p.l.H * N + i) * B + b];
                    const bool dH = p.l.st_done[(size_t)p.l.H * B + b] != 0.f;
                    const float gV = gv * poly_tail_weight(p, dH);
                    (void)poly_value<N>(p.Wv, p.bv, p.norm, o, y);
                    poly_value_bwd_x<N>(p.Wv, p.norm, y, gV, go);
                }
            });
    }
    // per-block partial rows, fixed order: butterfly inside each wave, then the four waves in order
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a)
#pragma unroll
        for (int k = 0; k < FP; ++k) wave_sum(gw[a][k], red, a * FP + k, GOPS_MAX_ACT * FP);
    __syncthreads();
    const int A = p.l.A, ldw = p.ldw;
    for (int e = threadIdx.x; e < A * FP; e += LANE_THREADS) {
        const int a = e / FP, k = e - a * FP;
        constexpr int S = GOPS_MAX_ACT * FP;
        const float s = (red[e] + red[S + e]) + (red[2 * S + e] + red[3 * S + e]);
        if (k < F || (k == F && p.fh)) p.part_w[(size_t)blockIdx.x * A * ldw + a * ldw + k] = s;
        else if (k == F + 1 && p.part_b != nullptr) p.part_b[(size_t)blockIdx.x * A + a] = s;
    }
}

// ---- POLY StateValue over a batch (INFADP's policy evaluation) -------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(LANE_THREADS) void poly_value_fwd_kernel(const float* Wv, const float* bv, const float* norm, int B,
                                                                      const float* obs, float* v) {
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
    if (b >= B) return;
    float o[N], y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = obs[(size_t)b * N + i];
    v[b] = poly_value<N>(Wv, bv, norm, o, y);
}

template <int N>
__global__ __launch_bounds__(LANE_THREADS) void poly_value_bwd_kernel(const float* norm, int B, const float* obs, const float* grad_v,
                                                                      float* part_w, float* part_b) {
    constexpr int K = poly_sym_dim<N>();
    __shared__ float red[4 * (K + 1)];
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
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
    LaneStash st;
    size_t pw, pb, bytes;
    int blocks, ldw;
};
static PolyPlan poly_plan(const GopsRolloutDesc& d) {
    PolyPlan pl;
    const int A = d.env.act_dim;
    pl.blocks = lane_blocks(d.batch);
    pl.ldw = poly_feat_dim_rt(d.env.obs_dim, poly_full_degree(d.policy.hidden_act)) + (d.finite_horizon ? 1 : 0);
    size_t off = lane_stash_plan(d, pl.st);
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
    lane_fill(d, ws, pl.st, p.env, p.l);
    p.fh = d.finite_horizon ? 1 : 0; p.tail = d.tail_value; p.tail_unmasked = d.tail_unmasked; p.ldw = pl.ldw;
    p.W = d.policy.weight[0]; p.b = d.policy.bias[0];
    if (d.tail_value) { p.Wv = d.value.weight[0]; p.bv = d.value.bias[0]; p.norm = d.value.weight[1]; }
    p.part_w = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.pw);
    p.part_b = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.pb);
    return p;
}

// the forward (FWD) or backward kernel of the description's (env kind, obs_dim, degree); degree 3 exists for N <= 3 (poly_shape_ok)
template <bool FWD>
static hipError_t poly_launch(const GopsRolloutDesc& d, const PolyParams& p, hipStream_t s) {
    const int deg = poly_full_degree(d.policy.hidden_act);
    return lane_dispatch(d.env.kind, d.env.obs_dim, [&]<int E, int N>() {
        const dim3 grid(lane_blocks(p.l.B));
        if (deg == 1) return lane_launch(FWD ? poly_fwd_kernel<E, N, 1> : poly_bwd_kernel<E, N, 1>, grid, s, p);
        if (deg == 2) return lane_launch(FWD ? poly_fwd_kernel<E, N, 2> : poly_bwd_kernel<E, N, 2>, grid, s, p);
        if constexpr (N <= 3)
            if (deg == 3) return lane_launch(FWD ? poly_fwd_kernel<E, N, 3> : poly_bwd_kernel<E, N, 3>, grid, s, p);
        return hipErrorInvalidValue;
    });
}

extern "C" {

int gops_poly_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out, void* ws, size_t bytes,
                              void* stream) {
    PolyParams p;
    const int rc = lane_forward_args(desc, in, out, ws, bytes, poly_check_desc, poly_plan, poly_params, p);
    if (rc != GOPS_OK) return rc;
    return lane_rc(poly_launch<true>(*desc, p, static_cast<hipStream_t>(stream)));
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
    p.l.grad_v = grad_v;   // (grad_final_obs stays null: the seed is the tail's adjoint, or zero)
    if (d.policy.bias[0] == nullptr) p.part_b = nullptr;
    hipError_t e = poly_launch<false>(d, p, s);
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
    return align256((size_t)lane_blocks(B) * K * sizeof(float)) + align256((size_t)lane_blocks(B) * sizeof(float));
}

int gops_poly_value_forward(const GopsMlp* value, int32_t B, const float* obs, float* out, void* stream) {
    if (!value) return GOPS_ERR_BAD_ARG;
    const GopsMlp& v = *value;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B < 1 || obs == nullptr || out == nullptr) return GOPS_ERR_BAD_ARG;
    const int rc = poly_check_value(v, v.sizes[0]);
    if (rc != GOPS_OK) return rc;
    const float *W = v.weight[0], *bv = v.bias[0], *nm = v.weight[1];
    return lane_rc(lane_dispatch_width(v.sizes[0], [&]<int N>() {
        return lane_launch(poly_value_fwd_kernel<N>, dim3(lane_blocks(B)), s, W, bv, nm, (int)B, obs, out);
    }));
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
    const int n = v.sizes[0], K = n * (n + 1) / 2, nb = lane_blocks(B);
    float* pw = static_cast<float*>(ws);
    float* pb = g.bias[0] != nullptr ? reinterpret_cast<float*>(static_cast<char*>(ws) + align256((size_t)nb * K * sizeof(float))) : nullptr;
    const float* nm = v.weight[1];
    hipError_t e = lane_dispatch_width(n, [&]<int N>() {
        return lane_launch(poly_value_bwd_kernel<N>, dim3(nb), s, nm, (int)B, obs, grad_v, pw, pb);
    });
    if (e != hipSuccess) return (int)e;
    ReduceJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    reduce_jobs_add(jobs, pw, nb, 1, K, K, g.weight[0]);
    if (pb != nullptr) reduce_jobs_add(jobs, pb, nb, 1, 1, 1, g.bias[0]);
    e = launch_reduce(jobs, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
