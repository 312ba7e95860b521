// GAUSS approximators (gops/apprfunc/gauss.py: radial basis functions) on the model rollout: one LANE per trajectory, as
// rollout_poly.hip, with the backward split in three because the feature map itself is trained.
//
//   y_a = sum_k w[a][k] phi_k + b[a],   phi_k = exp(-r_k / (2 |s_k|)),   r_k = sum_i (x_i - C[k][i])^2
//   DetermPolicy (GOPS_RBF_AFFINE): x = obs,              a = half y + mid
//   FiniteHorizonPolicy (GOPS_RBF_TANH): x = (obs, t + 1), a = half tanh(y) + mid      half / mid from GopsEnv.policy_low / _high
//
//   rbf_fwd_kernel         the forward walk of lane_rollout.h; its policy is a loop over the kernels k with C, s, w as wave-uniform
//                          loads (no phi[] array: y is accumulated directly), then the head.
//   rbf_sweep_kernel       the backward walk: y recomputed from the stash, the head's adjoint -> g_y, stored as [t][a][B]; g_x by
//                          one more loop over k.  No parameter-gradient registers: at K = 64, n = 7, A = 4 they would be 772 per lane.
//   rbf_param_grad_kernel  the parameter gradient is a plain sum over the H * B samples (t, b) of a function of
//                          (stashed obs, t + 1, g_y): grid = (sample blocks, kernel groups of RBF_GROUP), one lane per sample (a
//                          fixed stride over the samples beyond RBF_MAX_SAMPLE_BLOCKS blocks), n + 1 + A accumulators per kernel
//                          of the group in registers; wave butterfly, then the four waves in order, into per-block partial rows.
//   reduce_partials_kernel (dw_gemm.hip) sums the blocks' rows in a fixed order: the gradient is bitwise reproducible.
//
// No tail value in these kernels: INFADP composes it on the host from final_obs / grad_final_obs (algorithm/infadp.py).
// Bounds (everything else is refused by the host code): 1 <= K <= 64, obs_dim <= 6 (input width <= 7), out = act_dim <= GOPS_MAX_ACT.
#include "lane_rollout.h"
#include "launchers.h"

#define RBF_MAX_K 64
#define RBF_GROUP 8                  // kernels per block of the parameter-gradient launch: 8 * (7 + 1 + 4) + 4 accumulators
#define RBF_MAX_SAMPLE_BLOCKS 1024   // partial rows per gradient tensor at most; beyond it a lane adds several samples, in index order

struct RbfParams {
    GopsEnv env;                 // padded (lq_pad_env); the forward and the sweep read its LDS copy (lane_stage_env)
    LaneParams l;
    int K, nblk;
    const float* w;              // [A][K]
    const float* b;              // [A]
    const float* C;              // [K][NI], NI = obs_dim (+ 1: the virtual time, last)
    const float* s;              // sigma_square [K]
    float* st_gy;                // [H][A][B]
    float* part_w;               // [nblk][A * K]
    float* part_b;               // [nblk][A]
    float* part_C;               // [nblk][K * NI]
    float* part_s;               // [nblk][K]
};
static_assert(sizeof(RbfParams) <= 4000, "RbfParams outgrew the kernel-argument segment");

// ---- the net -------------------------------------------------------------------------------------------------------------------
// phi_k at input x (r: the squared distance to the centre, which the adjoint of sigma_square needs too)
template <int NI>
__device__ __forceinline__ float rbf_phi(const float* Ck, float s, const float (&x)[NI], float& r) {
    r = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const float d = x[i] - Ck[i];
        r += d * d;
    }
    return expf(-r / (2.f * fabsf(s)));
}

// the net's input at step t: the observation (+ virtual_t = t + 1)
template <int N, bool FH>
__device__ __forceinline__ void rbf_input(const float (&o)[N], int t, float (&x)[N + (FH ? 1 : 0)]) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = o[i];
    if constexpr (FH) x[N] = (float)(t + 1);
}

template <int NI>
__device__ __forceinline__ void rbf_net(const RbfParams& p, const float (&x)[NI], float (&y)[GOPS_MAX_ACT]) {
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) y[a] = a < p.l.A ? p.b[a] : 0.f;
#pragma unroll 1
    for (int k = 0; k < p.K; ++k) {
        float r;
        const float phi = rbf_phi<NI>(p.C + k * NI, p.s[k], x, r);
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a)
            if (a < p.l.A) y[a] += p.w[a * p.K + k] * phi;
    }
}

// the head: pre-wrapper action of output y, and the adjoint of y given the adjoint of that action
template <bool FH>
__device__ __forceinline__ float rbf_head(const GopsEnv& e, int a, float y) {
    const float half = (e.policy_high[a] - e.policy_low[a]) / 2.f, mid = (e.policy_high[a] + e.policy_low[a]) / 2.f;
    return half * (FH ? tanhf(y) : y) + mid;
}
template <bool FH>
__device__ __forceinline__ float rbf_head_bwd(const GopsEnv& e, int a, float y, float g) {
    const float half = (e.policy_high[a] - e.policy_low[a]) / 2.f;
    if constexpr (FH) {
        const float th = tanhf(y);
        return g * half * (1.f - th * th);
    }
    return g * half;
}

// the policy at observation o, step t: the net's input x and outputs y (a step's State of the walks), the pre-wrapper actions
template <int N, bool FH>
struct RbfStep {
    float x[N + (FH ? 1 : 0)], y[GOPS_MAX_ACT];
};
template <int N, bool FH>
__device__ __forceinline__ void rbf_policy(const RbfParams& p, const GopsEnv& env, const float (&o)[N], int t, RbfStep<N, FH>& st,
                                           float (&abar)[GOPS_MAX_ACT]) {
    rbf_input<N, FH>(o, t, st.x);
    rbf_net<N + (FH ? 1 : 0)>(p, st.x, st.y);
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) abar[a] = a < p.l.A ? rbf_head<FH>(env, a, st.y[a]) : 0.f;
}

// ---- forward rollout -----------------------------------------------------------------------------------------------------------
template <int ENV, int N, bool FH>
__global__ __launch_bounds__(LANE_THREADS) void rbf_fwd_kernel(const RbfParams p) {
    __shared__ unsigned s_env[sizeof(GopsEnv) / sizeof(unsigned)];
    const GopsEnv& env = lane_stage_env(p.env, s_env);
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
    if (b >= p.l.B) return;   // (no block-wide step after the staging)
    using Step = RbfStep<N, FH>;
    LANE_FORWARD_LOOP(env, p.l, Step, (rbf_policy<N, FH>(p, env, o, t, st, abar)))
    LANE_FORWARD_FINISH(p.l)   // (no tail value in these kernels)
}

// ---- backward sweep: adjoints of the observations, g_y of every step ---------------------------------------------------------------
template <int ENV, int N, bool FH>
__global__ __launch_bounds__(LANE_THREADS) void rbf_sweep_kernel(const RbfParams p) {
    constexpr int NI = N + (FH ? 1 : 0);
    __shared__ unsigned s_env[sizeof(GopsEnv) / sizeof(unsigned)];
    const GopsEnv& env = lane_stage_env(p.env, s_env);
    const int b = blockIdx.x * LANE_THREADS + threadIdx.x;
    if (b >= p.l.B) return;   // (no block-wide step after the staging)
    lane_backward<ENV, N, RbfStep<N, FH>>(
        env, p.l, b,
        [&](const float (&o)[N], int t, RbfStep<N, FH>& st, float (&abar)[GOPS_MAX_ACT]) { rbf_policy<N, FH>(p, env, o, t, st, abar); },
        [&](int t, const float (&)[N], const RbfStep<N, FH>& st, const float (&ga)[GOPS_MAX_ACT], float (&gx)[N]) {
            const float (&x)[NI] = st.x;
            float gy[GOPS_MAX_ACT];
#pragma unroll
            for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                gy[a] = a < p.l.A ? rbf_head_bwd<FH>(env, a, st.y[a], ga[a]) : 0.f;
                // (a row that is done has ga = 0, so g_y = 0: rbf_param_grad_kernel adds exact zeros for it without a test)
                if (a < p.l.A) p.st_gy[((size_t)t * p.l.A + a) * (size_t)p.l.B + b] = gy[a];
            }
            // g_x -= sum_k g_phi_k phi_k (x - C_k) / |s_k|  (observation inputs only: the time column takes no adjoint)
#pragma unroll 1
            for (int k = 0; k < p.K; ++k) {
                const float* Ck = p.C + k * NI;
                const float s = p.s[k];
                float r;
                const float phi = rbf_phi<NI>(Ck, s, x, r);
                float gphi = 0.f;
#pragma unroll
                for (int a = 0; a < GOPS_MAX_ACT; ++a)
                    if (a < p.l.A) gphi += p.w[a * p.K + k] * gy[a];
                const float c = gphi * phi / fabsf(s);
#pragma unroll
                for (int i = 0; i < N; ++i) gx[i] -= c * (x[i] - Ck[i]);
            }
        },
        [](float, float (&)[N]) {});   // (the seed is grad_final_obs alone)
}

// ---- parameter gradient: a sum over the H * B samples, RBF_GROUP kernels per block --------------------------------------------------
template <int N, bool FH>
__global__ __launch_bounds__(LANE_THREADS) void rbf_param_grad_kernel(const RbfParams p) {
    constexpr int NI = N + (FH ? 1 : 0);
    constexpr int G = RBF_GROUP;
    constexpr int PER = NI + 1 + GOPS_MAX_ACT;        // per kernel: g_C [NI], g_s, g_w [A]
    constexpr int NS = G * PER + GOPS_MAX_ACT;        // + g_b [A]
    __shared__ float red[4 * NS];
    const int k0 = blockIdx.y * G, K = p.K, A = p.l.A;
    float acc[G][PER], gb[GOPS_MAX_ACT];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int c = 0; c < PER; ++c) acc[j][c] = 0.f;
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) gb[a] = 0.f;
    const long long B = p.l.B, S = (long long)p.l.H * B, stride = (long long)gridDim.x * LANE_THREADS;
#pragma unroll 1
    for (long long smp = (long long)blockIdx.x * LANE_THREADS + threadIdx.x; smp < S; smp += stride) {
        const int t = (int)(smp / B);
        const size_t b = (size_t)(smp - (long long)t * B);
        float o[N], x[NI], gy[GOPS_MAX_ACT];
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = p.l.st_obs[((size_t)t * N + i) * (size_t)B + b];
        rbf_input<N, FH>(o, t, x);
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) {
            gy[a] = a < A ? p.st_gy[((size_t)t * A + a) * (size_t)B + b] : 0.f;
            gb[a] += gy[a];
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int k = k0 + j;
            if (k < K) {   // (wave-uniform)
                const float* Ck = p.C + k * NI;
                const float s = p.s[k];
                float r;
                const float phi = rbf_phi<NI>(Ck, s, x, r);
                float gphi = 0.f;
#pragma unroll
                for (int a = 0; a < GOPS_MAX_ACT; ++a) {
                    if (a < A) gphi += p.w[a * K + k] * gy[a];
                    acc[j][NI + 1 + a] += gy[a] * phi;
                }
                const float gp = gphi * phi;
                const float c = gp / fabsf(s);
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[j][i] += c * (x[i] - Ck[i]);
                acc[j][NI] += (s < 0.f ? -gp : gp) * r / (2.f * s * s);
            }
        }
    }
    // per-block partial rows, fixed order: butterfly inside each wave, then the four waves in order
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int c = 0; c < PER; ++c) wave_sum(acc[j][c], red, j * PER + c, NS);
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a) wave_sum(gb[a], red, G * PER + a, NS);
    __syncthreads();
    const size_t blk = blockIdx.x;
    for (int e = threadIdx.x; e < NS; e += LANE_THREADS) {
        const float sum = (red[e] + red[NS + e]) + (red[2 * NS + e] + red[3 * NS + e]);
        if (e < G * PER) {
            const int j = e / PER, c = e - j * PER, k = k0 + j;
            if (k >= K) continue;
            if (c < NI) p.part_C[blk * K * NI + k * NI + c] = sum;
            else if (c == NI) p.part_s[blk * K + k] = sum;
            else if (c - NI - 1 < A) p.part_w[blk * A * K + (c - NI - 1) * K + k] = sum;
        } else if (blockIdx.y == 0 && e - G * PER < A) {   // g_b: from group 0 only
            p.part_b[blk * A + (e - G * PER)] = sum;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

bool rbf_is_net(const GopsMlp& m) { return m.n_layers == 1 && (m.hidden_act == GOPS_RBF_AFFINE || m.hidden_act == GOPS_RBF_TANH); }

int rbf_check_desc(const GopsRolloutDesc& d) {
    const int rc = state_model_check_desc(d);   // (env_models.h: shape, fp32, closed loop, the model envs of the per-lane step)
    if (rc != GOPS_OK) return rc;
    if (d.tail_value) return GOPS_ERR_UNSUPPORTED;   // (the caller composes a tail from final_obs / grad_final_obs)
    const GopsMlp& m = d.policy;
    if (!rbf_is_net(m)) return GOPS_ERR_UNSUPPORTED;   // (a POLY or MLP net)
    const int n = d.env.obs_dim, fh = d.finite_horizon ? 1 : 0;
    if (m.sizes[2] < 1 || m.sizes[2] > RBF_MAX_K || m.sizes[1] != d.env.act_dim) return GOPS_ERR_UNSUPPORTED;
    if (m.sizes[0] < 1 || m.sizes[0] > GOPS_MAX_LQ_STATE + 1) return GOPS_ERR_UNSUPPORTED;
    // centre columns = observation (+ the virtual time of a FiniteHorizonPolicy), and the head that goes with them: a DetermPolicy in a
    // finite-horizon rollout, or a FiniteHorizonPolicy in an infinite-horizon one, would be read with the wrong row stride
    if (m.sizes[0] != n + fh || (m.hidden_act == GOPS_RBF_TANH) != (fh != 0)) return GOPS_ERR_BAD_ARG;
    if (m.weight[0] == nullptr || m.bias[0] == nullptr || m.weight[1] == nullptr || m.bias[1] == nullptr) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

struct RbfPlan {
    LaneStash st;
    size_t gy, pw, pb, pc, ps, bytes;
    int nblk, groups;
};
static RbfPlan rbf_plan(const GopsRolloutDesc& d) {
    RbfPlan pl;
    const int A = d.env.act_dim, B = d.batch, H = d.horizon, K = d.policy.sizes[2], NI = d.policy.sizes[0];
    const long long sb = ((long long)H * B + LANE_THREADS - 1) / LANE_THREADS;
    pl.nblk = (int)(sb < RBF_MAX_SAMPLE_BLOCKS ? sb : RBF_MAX_SAMPLE_BLOCKS);
    pl.groups = (K + RBF_GROUP - 1) / RBF_GROUP;
    size_t off = lane_stash_plan(d, pl.st);
    pl.gy = off; off += align256((size_t)H * A * B * sizeof(float));
    pl.pw = off; off += align256((size_t)pl.nblk * A * K * sizeof(float));
    pl.pb = off; off += align256((size_t)pl.nblk * A * sizeof(float));
    pl.pc = off; off += align256((size_t)pl.nblk * K * NI * sizeof(float));
    pl.ps = off; off += align256((size_t)pl.nblk * K * sizeof(float));
    pl.bytes = off;
    return pl;
}

static RbfParams rbf_params(const GopsRolloutDesc& d, const RbfPlan& pl, void* ws) {
    RbfParams p;
    memset(&p, 0, sizeof(p));
    lane_fill(d, ws, pl.st, p.env, p.l);
    p.K = d.policy.sizes[2]; p.nblk = pl.nblk;
    p.w = d.policy.weight[0]; p.b = d.policy.bias[0]; p.C = d.policy.weight[1]; p.s = d.policy.bias[1];
    char* w = static_cast<char*>(ws);
    p.st_gy = reinterpret_cast<float*>(w + pl.gy);
    p.part_w = reinterpret_cast<float*>(w + pl.pw);
    p.part_b = reinterpret_cast<float*>(w + pl.pb);
    p.part_C = reinterpret_cast<float*>(w + pl.pc);
    p.part_s = reinterpret_cast<float*>(w + pl.ps);
    return p;
}

// the forward (FWD) or sweep kernel of the description's (env kind, obs_dim, head)
template <bool FWD>
static hipError_t rbf_launch(const GopsRolloutDesc& d, const RbfParams& p, hipStream_t s) {
    return lane_dispatch(d.env.kind, d.env.obs_dim, [&]<int E, int N>() {
        const dim3 grid(lane_blocks(p.l.B));
        if (d.finite_horizon) return lane_launch(FWD ? rbf_fwd_kernel<E, N, true> : rbf_sweep_kernel<E, N, true>, grid, s, p);
        return lane_launch(FWD ? rbf_fwd_kernel<E, N, false> : rbf_sweep_kernel<E, N, false>, grid, s, p);
    });
}

extern "C" {

size_t gops_rbf_rollout_workspace_bytes(const GopsRolloutDesc* desc) {
    if (!desc || rbf_check_desc(*desc) != GOPS_OK) return 0;
    return rbf_plan(*desc).bytes;
}

int gops_rbf_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out, void* ws, size_t bytes,
                             void* stream) {
    RbfParams p;
    const int rc = lane_forward_args(desc, in, out, ws, bytes, rbf_check_desc, rbf_plan, rbf_params, p);
    if (rc != GOPS_OK) return rc;
    return lane_rc(rbf_launch<true>(*desc, p, static_cast<hipStream_t>(stream)));
}

int gops_rbf_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v, const GopsMlpGrad* grad,
                              const GopsRolloutAdjoint* adj, void* ws, size_t bytes, void* stream) {
    if (!desc || !in || !grad) return GOPS_ERR_BAD_ARG;   // (`in` is not read: the forward stashed what the sweep needs)
    const GopsRolloutDesc& d = *desc;
    const GopsMlpGrad& g = *grad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = rbf_check_desc(d);
    if (rc != GOPS_OK) return rc;
    if (!d.need_grad || grad_v == nullptr) return GOPS_ERR_BAD_ARG;
    if (g.weight[0] == nullptr || g.bias[0] == nullptr || g.weight[1] == nullptr || g.bias[1] == nullptr) return GOPS_ERR_BAD_ARG;
    if (adj != nullptr && adj->first_step_only != 0) return GOPS_ERR_UNSUPPORTED;
    const RbfPlan pl = rbf_plan(d);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    RbfParams p = rbf_params(d, pl, ws);
    p.l.grad_v = grad_v;
    if (adj != nullptr) { p.l.grad_final_obs = adj->grad_final_obs; p.l.grad_obs = adj->grad_obs; }
    hipError_t e = rbf_launch<false>(d, p, s);
    if (e != hipSuccess) return (int)e;
    e = lane_dispatch_width(d.env.obs_dim, [&]<int N>() {   // (the parameter gradient is independent of the env)
        const dim3 grid(p.nblk, pl.groups);
        return d.finite_horizon ? lane_launch(rbf_param_grad_kernel<N, true>, grid, s, p) : lane_launch(rbf_param_grad_kernel<N, false>, grid, s, p);
    });
    if (e != hipSuccess) return (int)e;
    ReduceJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    const int A = p.l.A, K = p.K, NI = d.policy.sizes[0];
    reduce_jobs_add(jobs, p.part_w, pl.nblk, 1, A * K, A * K, g.weight[0]);
    reduce_jobs_add(jobs, p.part_b, pl.nblk, 1, A, A, g.bias[0]);
    reduce_jobs_add(jobs, p.part_C, pl.nblk, 1, K * NI, K * NI, g.weight[1]);
    reduce_jobs_add(jobs, p.part_s, pl.nblk, 1, K, K, g.bias[1]);
    e = launch_reduce(jobs, s);
    return e == hipSuccess ? GOPS_OK : (int)e;
}

}  // extern "C"
