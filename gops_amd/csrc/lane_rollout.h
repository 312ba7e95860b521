// The one-LANE-per-trajectory model rollout, stated once for every approximator family that runs on it (POLY: rollout_poly.hip,
// GAUSS: rollout_rbf.hip).  A lane walks its trajectory through the horizon with the wrapped model step of env_models.h, stashes
// the observation and the done flag each step starts from, and walks back over the stash with the step's adjoint.  A family gives
// the policy between the two halves as callables and keeps its own net, parameter gradient and descriptor check:
//
//   State                       what the policy leaves for its adjoint within one step (features, net outputs): the walk declares
//                               it inside its step loop, which keeps the values' live ranges to the step
//   policy(o, t, st, abar)      the pre-wrapper actions abar[GOPS_MAX_ACT] at observation o, step t (zeros beyond act_dim)
//   adjoint(t, o, st, ga, gx)   ga: adjoint of abar; adds the policy's input adjoint to gx and keeps what it accumulates
//   (forward)                   between LANE_FORWARD_LOOP and LANE_FORWARD_FINISH: a terminal value added to v
//   tail(gv, go)                backward, before the loop: that value's adjoint written over the seed go
//
// The walks take the env description by reference and do not care where it lives: the kernel argument, or the LDS copy of
// lane_stage_env.  Host side: the stash plan, the shared kernel-argument fields, the forward entry points' common part, the launch
// and the two dispatches (over the (env kind, obs_dim) list of env_models.h, and over obs_dim alone).
#pragma once
#include <math.h>
#include <string.h>

#include "common.h"
#include "env_models.h"

#define LANE_THREADS 256

// the kernel-argument fields of every family, next to its `GopsEnv env` (padded: lq_pad_env) and its own net's fields
struct LaneParams {
    int B, H, A, need_grad;
    const float* obs;            // [B][N]
    const float* done;           // [B] or null
    const float* grad_v;         // backward: [B]
    const float* grad_final_obs; // backward: [B][N] or null
    float* grad_obs;             // backward: [B][N] or null
    float* v_pi;                 // [B]
    float* rewards;              // [H][B] or null
    float* final_obs;            // [B][N] or null
    float* final_done;           // [B] or null
    float* st_obs;               // [H + 1][N][B]  (a wave's store is 256 contiguous bytes)
    float* st_done;              // [H + 1][B]
    float gpow[GOPS_MAX_HORIZON + 1];
};

// The env description in LDS.  Read through the kernel argument its ~150 scalars are wave-uniform loads that the compiler hoists
// out of the step and kernel loops: more than the SGPR file holds (the pyth_lq kernels sat at its limit with 20 .. 110 scalar
// spills and a reserved stack frame).  From LDS they are broadcast reads with immediate offsets, as in the 64-row half kernels
// (common.h ENV_LDS_FLOATS).  Every thread of the block must call this (it holds a barrier).
__device__ __forceinline__ const GopsEnv& lane_stage_env(const GopsEnv& env, unsigned (&s_env)[sizeof(GopsEnv) / sizeof(unsigned)]) {
    const unsigned* src = reinterpret_cast<const unsigned*>(&env);
    for (int i = threadIdx.x; i < (int)(sizeof(GopsEnv) / sizeof(unsigned)); i += LANE_THREADS) s_env[i] = src[i];
    __syncthreads();
    return *reinterpret_cast<const GopsEnv*>(s_env);
}

// ---- forward walk of lane b < L.B: as env_step_kernel (aux_kernels.hip) per step; sum_t gamma^t r_t ------------------------------
// Two macros, not a function template: a walk that reads the shared fields through a reference compiles rbf_fwd_kernel<LQ, 6, affine>
// to 174 VGPRs (2 waves/SIMD), the same text on the kernel argument itself to the 168 (3 waves) it had.
//   read from the kernel's scope:   template parameters ENV, N; the lane index `int b` (< L.B)
//   arguments:                      ENVR the GopsEnv, L the kernel argument's LaneParams, STATE the step's record type (one token),
//                                   POLICY an expression (parenthesised) that fills `st` and `abar` from `o`, `t`
//   declared in the kernel's scope: LOOP: B, nomask, o[N], dn, done_last, v, dH (and, inside its loop only: t, st, abar, u, on, r,
//                                   done_m, rr); FINISH declares nothing and reads B, b, o, v, dH
// Between LOOP and FINISH a family may add a terminal value at `o` to `v`, masked by `dH`; it must not reuse the names above.
#define LANE_FORWARD_LOOP(ENVR, L, STATE, POLICY)                                                                                  \
    const size_t B = (size_t)L.B;                                                                                                  \
    const bool nomask = ENVR.no_mask_at_done != 0;                                                                                 \
    float o[N];                                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < N; ++i) o[i] = L.obs[(size_t)b * N + i];                                                 \
    bool dn = !nomask && L.done != nullptr && L.done[b] != 0.f;                                                                    \
    bool done_last = false;                                                                                                        \
    float v = 0.f;                                                                                                                 \
    _Pragma("unroll 1") for (int t = 0; t < L.H; ++t) {                                                                            \
        if (L.need_grad) {                                                                                                         \
            _Pragma("unroll") for (int i = 0; i < N; ++i) L.st_obs[((size_t)t * N + i) * B + b] = o[i];                            \
            L.st_done[(size_t)t * B + b] = dn ? 1.f : 0.f;                                                                         \
        }                                                                                                                          \
        STATE st;                                                                                                                  \
        float abar[GOPS_MAX_ACT], u[GOPS_MAX_ACT];                                                                                 \
        POLICY;                                                                                                                    \
        _Pragma("unroll") for (int a = 0; a < GOPS_MAX_ACT; ++a) u[a] = a < L.A ? wrap_action(ENVR, a, abar[a]) : 0.f;             \
        float on[N], r;                                                                                                            \
        bool done_m;                                                                                                               \
        state_model_step<ENV, N>(ENVR, o, u, dn, on, r, done_m);                                                                   \
        float rr = dn ? 0.f : r;                                                                                                   \
        if (ENVR.shaping) rr = (rr + ENVR.reward_shift) * ENVR.reward_scale;                                                       \
        v += rr * L.gpow[t];                                                                                                       \
        if (L.rewards != nullptr) L.rewards[(size_t)t * B + b] = rr;                                                               \
        dn = dn || (done_m && !nomask);                                                                                            \
        done_last = done_m;                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < N; ++i) o[i] = on[i];                                                                \
    }                                                                                                                              \
    /* no MaskAtDoneModel: final_done (and a tail's mask) is the base model's done test on the last state */                      \
    const bool dH = nomask ? done_last : dn;
#define LANE_FORWARD_FINISH(L)                                                                                                     \
    if (L.need_grad) {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < N; ++i) L.st_obs[((size_t)L.H * N + i) * B + b] = o[i];                              \
        L.st_done[(size_t)L.H * B + b] = dH ? 1.f : 0.f;                                                                           \
    }                                                                                                                              \
    L.v_pi[b] = v;                                                                                                                 \
    if (L.final_obs != nullptr)                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < N; ++i) L.final_obs[(size_t)b * N + i] = o[i];                                       \
    if (L.final_done != nullptr) L.final_done[b] = dH ? 1.f : 0.f;

// ---- backward walk of lane b < p.B over the stash: model adjoints recomputed from the stashed observation (the idpendulum
// sub-steps included); seeded with grad_final_obs (null: zeros), then with what `tail` writes over it -----------------------------
template <int ENV, int N, class State, class Policy, class Adjoint, class Tail>
__device__ __forceinline__ void lane_backward(const GopsEnv& env, const LaneParams& p, int b, Policy policy, Adjoint adjoint, Tail tail) {
    const size_t B = (size_t)p.B;
    const float gv = p.grad_v[b];
    float go[N], o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) go[i] = p.grad_final_obs != nullptr ? p.grad_final_obs[(size_t)b * N + i] : 0.f;
    tail(gv, go);
#pragma unroll 1
    for (int t = p.H - 1; t >= 0; --t) {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = p.st_obs[((size_t)t * N + i) * B + b];
        const bool dn = p.st_done[(size_t)t * B + b] != 0.f;
        State st;
        float abar[GOPS_MAX_ACT], u[GOPS_MAX_ACT];
        policy(o, t, st, abar);
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) u[a] = a < p.A ? wrap_action(env, a, abar[a]) : 0.f;
        float g_r = gv * p.gpow[t];   // adjoint of the shaped reward
        if (env.shaping) g_r *= env.reward_scale;
        float gu[GOPS_MAX_ACT], gx[N], ga[GOPS_MAX_ACT];
        state_model_step_bwd<ENV, N>(env, o, u, dn, g_r, go, gx, gu);
#pragma unroll
        for (int a = 0; a < GOPS_MAX_ACT; ++a) ga[a] = a < p.A ? wrap_action_bwd(env, a, abar[a], gu[a]) : 0.f;
        adjoint(t, o, st, ga, gx);
#pragma unroll
        for (int i = 0; i < N; ++i) go[i] = gx[i];
    }
    if (p.grad_obs != nullptr)
#pragma unroll
        for (int i = 0; i < N; ++i) p.grad_obs[(size_t)b * N + i] = go[i];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

static int lane_blocks(int B) { return (B + LANE_THREADS - 1) / LANE_THREADS; }
static int lane_rc(hipError_t e) { return e == hipSuccess ? GOPS_OK : (int)e; }

// the stash at the head of a family's workspace; returns the running offset, where the family appends its own rows
struct LaneStash {
    size_t obs, done;
};
static size_t lane_stash_plan(const GopsRolloutDesc& d, LaneStash& st) {
    const size_t n = d.env.obs_dim, B = d.batch, H = d.horizon;
    size_t off = 0;
    st.obs = off; off += align256((H + 1) * n * B * sizeof(float));
    st.done = off; off += align256((H + 1) * B * sizeof(float));
    return off;
}

// `env` and the shared fields of a kernel argument that the caller has zeroed (in / out / adjoint pointers: the entry points)
static void lane_fill(const GopsRolloutDesc& d, void* ws, const LaneStash& st, GopsEnv& env, LaneParams& l) {
    env = d.env;
    lq_pad_env(env);
    l.B = d.batch; l.H = d.horizon; l.A = d.env.act_dim; l.need_grad = d.need_grad;
    l.st_obs = reinterpret_cast<float*>(static_cast<char*>(ws) + st.obs);
    l.st_done = reinterpret_cast<float*>(static_cast<char*>(ws) + st.done);
    for (int t = 0; t <= l.H; ++t) l.gpow[t] = (float)pow(d.gamma, (double)t);   // gamma^t formed in double, then rounded
}

// A *_rollout_forward entry point up to its launch: the argument checks in their order, the family's kernel argument `p` with in /
// out wired.  `check`, `plan` (a record with `bytes`) and `params` are the family's own.
template <class Check, class Plan, class Params, class P>
static int lane_forward_args(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out, void* ws, size_t bytes,
                             Check check, Plan plan, Params params, P& p) {
    if (!desc || !in || !out) return GOPS_ERR_BAD_ARG;
    const int rc = check(*desc);
    if (rc != GOPS_OK) return rc;
    if (in->obs == nullptr || out->v_pi == nullptr) return GOPS_ERR_BAD_ARG;
    const auto pl = plan(*desc);
    if (ws == nullptr || bytes < pl.bytes) return GOPS_ERR_WORKSPACE;
    p = params(*desc, pl, ws);
    p.l.obs = in->obs; p.l.done = in->done;
    p.l.v_pi = out->v_pi; p.l.rewards = out->rewards; p.l.final_obs = out->final_obs; p.l.final_done = out->final_done;
    return GOPS_OK;
}

template <class... KA, class... A>
static hipError_t lane_launch(void (*kernel)(KA...), dim3 grid, hipStream_t s, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(LANE_THREADS), 0, s, args...);
    return hipGetLastError();
}

// f.operator()<ENV, N>() of the description's (env kind, obs_dim): one instantiation per pair of the list, so that a kernel carries
// only its own model's arithmetic
template <class F>
static hipError_t lane_dispatch(int kind, int n, F f) {
#define LANE_CASE(EE, NN) if (kind == EE && n == NN) return f.template operator()<EE, NN>();
    STATE_MODEL_CASES(LANE_CASE)
#undef LANE_CASE
    return hipErrorInvalidValue;
}
// f.operator()<N>() of an observation width alone
template <class F>
static hipError_t lane_dispatch_width(int n, F f) {
    static_assert(GOPS_MAX_LQ_STATE == 6, "one case per observation width");
    switch (n) {
        case 1: return f.template operator()<1>();
        case 2: return f.template operator()<2>();
        case 3: return f.template operator()<3>();
        case 4: return f.template operator()<4>();
        case 5: return f.template operator()<5>();
        case 6: return f.template operator()<6>();
        default: return hipErrorInvalidValue;
    }
}
