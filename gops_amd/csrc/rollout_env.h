// The env phase of the tile-form rollout kernels (rollout_fwd.hip, rollout_bwd.hip, rollout_h64.hip), stated once: the wrapper chain
// around the base models of env_models.h, its adjoint, and the bookkeeping every constrained / reference-tracking step repeats.
// Arithmetic only - values in, values out, in registers or through the pointers handed in; staging, thread mapping and barriers
// stay in the kernels.  env_step.h steps the same reference-point transform and done tests.
#pragma once
#include "common.h"
#include "env_models.h"

// ================================ policy head: de-squash and its adjoint ======================
// abar = sc th + of (th = tanh(head)), u = wrap_action(abar); `raw` (open_loop == 2): th IS the model action.
// NA: compile-time bound of the action loop; EXACT: the env has exactly NA actions (no run-time guard against A).
struct HeadAct { float sc[GOPS_MAX_ACT], abar[GOPS_MAX_ACT], u[GOPS_MAX_ACT]; };
template <int NA = GOPS_MAX_ACT, bool EXACT = false>
__device__ __forceinline__ HeadAct head_unsquash(const GopsEnv& env, const float* th, int A, bool raw) {
    HeadAct h = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        h.sc[a] = (env.policy_high[a] - env.policy_low[a]) / 2.f;
        h.abar[a] = h.sc[a] * th[a] + (env.policy_high[a] + env.policy_low[a]) / 2.f;
        h.u[a] = (EXACT || a < A) ? (raw ? th[a] : wrap_action(env, a, h.abar[a])) : 0.f;
    }
    return h;
}
// adjoint of the head output given the adjoint gu of the model action
__device__ __forceinline__ float head_unsquash_bwd(const GopsEnv& env, int a, float sc, float abar, float th, float gu, bool raw) {
    return raw ? gu : wrap_action_bwd(env, a, abar, gu) * sc * (1.f - th * th);
}
__device__ __forceinline__ float head_unsquash_bwd(const ActC& c, float abar, float th, float gu, bool raw) {   // staged constants
    return raw ? gu : wrap_action_bwd(c, abar, gu) * c.sc * (1.f - th * th);
}

// ================================ models whose observation is the state ========================
// pyth_lq (NS, NA: compile-time loop bounds, (4, 2) or the maxima), gym_cartpoleconti (4, 1), gym_pendulum (3, 1),
// gym_mountaincarconti (2, 1).
// EXACT (NS below the maximum): the dimensions ARE (NS, NA), no run-time guards against O / A.

// The wrapped forward step of row `xo` of the observation tile: un-scale, ActionRepeat's sub-steps with the initial done flag
// (GEN; else one step), freeze at done (MaskAtDone), re-scale, ClipObservation.  act: the row's wrapped actions.
template <int ENV, int NS, int NA, bool GEN>
__device__ __forceinline__ void obs_state_step(const GopsEnv& env, int O, int A, float* xo, const float* act, bool frozen,
                                               float& r, bool& done_m) {
    constexpr bool EXACT = NS < GOPS_MAX_LQ_STATE;
    float x[GOPS_MAX_LQ_STATE], xn[GOPS_MAX_LQ_STATE], u[GOPS_MAX_ACT];
#pragma unroll
    for (int i = 0; i < GOPS_MAX_LQ_STATE; ++i) { x[i] = (i < NS && (EXACT || i < O)) ? obs_unscale(env, i, xo[i]) : 0.f; xn[i] = 0.f; }
#pragma unroll
    for (int j = 0; j < GOPS_MAX_ACT; ++j) u[j] = (j < NA && (EXACT || j < A)) ? act[j] : 0.f;
    const int nrep = GEN ? env.repeat_num : 1;
    float rs = 0.f;
    for (int rep = 0; rep < nrep; ++rep) {
        if (rep > 0 && !frozen) {
#pragma unroll
            for (int i = 0; i < NS; ++i) x[i] = xn[i];
        }
        state_model_substep<ENV, NS, NA>(env, x, u, xn, r, done_m);
        rs = (GEN && !env.repeat_last_reward) ? rs + r : r;
    }
    r = rs;
    if (!frozen || env.clip_obs || env.scale_obs) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (EXACT || i < O) {
                const float v = obs_rescale(env, i, sel_reg(frozen, x[i], xn[i]));
                xo[i] = env.clip_obs ? clampf(v, env.obs_low[i], env.obs_high[i]) : v;
            }
    }
}

// Adjoint of that step without ActionRepeat.  x: the UNSCALED observation the step started from, u: its model actions, dn: its done
// flag, g_rm: the (masked) reward adjoint, Gin: the adjoint of the next observation (consumed).  -> gx: adjoint of the unscaled
// observation, gu: adjoint of the model actions.
template <int ENV, int NS, int NA>
__device__ __forceinline__ void obs_state_adjoint(const GopsEnv& env, int O, const float* x, const float (&u)[GOPS_MAX_ACT], bool dn,
                                                  float g_rm, float* Gin, float* gx, float* gu) {
    constexpr bool EXACT = NS < GOPS_MAX_LQ_STATE;
    if (env.clip_obs) {
        float xn[GOPS_MAX_LQ_STATE] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rdummy;
        bool ddummy;
        state_model_substep<ENV, NS, NA>(env, x, u, xn, rdummy, ddummy);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const float pre = obs_rescale(env, i, dn ? x[i] : xn[i]);   // what ClipObservation saw
            if ((EXACT || i < O) && !(pre >= env.obs_low[i] && pre <= env.obs_high[i])) Gin[i] = 0.f;
        }
    }
    if (env.scale_obs) {   // d(scaled next obs) / d(next obs) = scale
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (EXACT || i < O) Gin[i] *= env.obs_scale[i];
    }
    float gxn[GOPS_MAX_LQ_STATE];
#pragma unroll
    for (int i = 0; i < GOPS_MAX_LQ_STATE; ++i) {   // MaskAtDone: a finished trajectory's adjoint stays on its observation
        gxn[i] = (i < NS && !dn) ? Gin[i] : 0.f;
        gx[i] = (i < NS && dn) ? Gin[i] : 0.f;
    }
    state_model_backward<ENV, NS, NA>(env, x, u, gxn, g_rm, gx, gu);
}

// The end of every such adjoint: G row <- gx through the observation scaling, s_gy row <- gu through the head's squash.
template <int NS, int NA>
__device__ __forceinline__ void obs_state_adjoint_store(const GopsEnv& env, int O, int A, const float* gx, const float* gu, const HeadAct& h,
                                                        const float* th, bool raw, float* Grow, float* gyrow) {
    constexpr bool EXACT = NS < GOPS_MAX_LQ_STATE;
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (EXACT || i < O) Grow[i] = env.scale_obs ? gx[i] / env.obs_scale[i] : gx[i];   // d(obs / scale - shift) / d(obs)
#pragma unroll
    for (int a = 0; a < GOPS_MAX_ACT; ++a)
        gyrow[a] = (a < NA && (EXACT || a < A)) ? head_unsquash_bwd(env, a, h.sc[a], h.abar[a], th[a], gu[a], raw) : 0.f;
}

// ================================ pyth_idpendulum: the sub-step parking ========================
// One record per Euler sub-step, 24 floats: [0..5] the sub-step's input state, [6..11] s1 c1 s2 c2 s12 c12, [12..17] M^-1,
// [18..20] qdd, [21..23] unused.  The forward parks f32x4 records in global memory, the sweeps park floats in LDS.
#define IDP_REC 24
template <typename Q>   // Q: pointer to float, or to f32x4 (any address space): the same 24 slots, the unused ones zero
__device__ __forceinline__ void idp_park_store(Q d, const float* s, const IdpSub& w) {
    if constexpr (sizeof(d[0]) == sizeof(float)) {
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = s[i];
        d[6] = w.s1; d[7] = w.c1; d[8] = w.s2; d[9] = w.c2; d[10] = w.s12; d[11] = w.c12;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[12 + i] = w.inv[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[18 + i] = w.qdd[i];
    } else {
        d[0] = f32x4{s[0], s[1], s[2], s[3]};
        d[1] = f32x4{s[4], s[5], w.s1, w.c1};
        d[2] = f32x4{w.s2, w.c2, w.s12, w.c12};
        d[3] = f32x4{w.inv[0], w.inv[1], w.inv[2], w.inv[3]};
        d[4] = f32x4{w.inv[4], w.inv[5], w.qdd[0], w.qdd[1]};
        d[5] = f32x4{w.qdd[2], 0.f, 0.f, 0.f};
    }
}
__device__ __forceinline__ void idp_park_load(const float* pk, float* s, IdpSub& w) {
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = pk[i];
    w.s1 = pk[6]; w.c1 = pk[7]; w.s2 = pk[8]; w.c2 = pk[9]; w.s12 = pk[10]; w.c12 = pk[11];
#pragma unroll
    for (int i = 0; i < 6; ++i) w.inv[i] = pk[12 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w.qdd[i] = pk[18 + i];
}
// the five sub-steps from state s (left holding the state after the step), every sub-step parked in park[5][IDP_REC]
__device__ __forceinline__ void idp_park_step(const IdpConst& IC, float* s, float force, float* park) {
    float sn[6];
    IdpSub w;
#pragma unroll 1
    for (int k = 0; k < 5; ++k) {
        if (k == 0) idp_substep<true>(IC, s, force, 0.002f, sn, w);
        else idp_substep<false>(IC, s, force, 0.002f, sn, w);   // w.s1 .. w.c2 advanced at the end of the last trip
        idp_park_store(park + k * IDP_REC, s, w);
        idp_advance_trig(s, 0.002f, w, w);
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = sn[i];
    }
}
// adjoint of idp_reward w.r.t. the state s after the step, accumulated into g
__device__ __forceinline__ void idp_reward_bwd(const float* s, float gr, float* g) {
    g[1] += gr * (-10.f * s[1]);
    g[2] += gr * (-20.f * s[2]);
    g[3] += gr * (-1.f * s[3]);
    g[4] += gr * (-1.f * s[4]);
    g[5] += gr * (-2.f * s[5]);
}
// adjoint of the parked sub-step `pk`: g (adjoint of the state after it) -> adjoint of the state before it, gforce accumulated.
// (The callers walk k = 4 .. 0 with their own `#pragma unroll`: straight-line code in the sweeps' step, a loop under ActionRepeat.)
__device__ __forceinline__ void idp_park_substep_bwd(const IdpConst& IC, const float* pk, float* g, float& gforce) {
    IdpSub w;
    float sk[6];
    idp_park_load(pk, sk, w);
    idp_substep_bwd(IC, sk, 0.002f, w, g, gforce);
}
// adjoint of one whole step (five sub-steps, action a) at the state xi, recomputed through park[5][IDP_REC]: gn adjoint of the state
// after the step, gr adjoint of its reward -> gxo adjoint of xi, ga adjoint of the action (both overwritten)
__device__ __forceinline__ void idp_step_bwd_parked(const IdpConst& IC, const float* xi, float a, const float* gn, float gr, float* park,
                                                    float* gxo, float& ga) {
    float s[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { s[i] = xi[i]; gxo[i] = gn[i]; }
    idp_park_step(IC, s, 500.f * a, park);
    idp_reward_bwd(s, gr, gxo);
    float gforce = 0.f;
#pragma unroll 1
    for (int k = 4; k >= 0; --k) idp_park_substep_bwd(IC, park + k * IDP_REC, gxo, gforce);
    ga = 500.f * gforce + gr * (-2.f * a);
}

// ================================ constraint bookkeeping of one step ==========================
// Discounted sums of the exterior / linear / interior penalties, the feasibility flag and SPIL's products over a trajectory.
struct ConstraintSums {
    float ext = 0.f, lin = 0.f, itr = 0.f, feas = 1.f;
    float mul[GOPS_MAX_CONSTRAINT] = {1.f, 1.f, 1.f}, safe[GOPS_MAX_CONSTRAINT] = {1.f, 1.f, 1.f};
    // one step's constraint values c[0 .. n)
    __device__ __forceinline__ void add(const float* c, int n, float gpow) {
        float e2 = 0.f, e1 = 0.f, lg = 0.f;
#pragma unroll
        for (int k = 0; k < GOPS_MAX_CONSTRAINT; ++k) {
            if (k < n) {
                const float cp = fmaxf(c[k], 0.f), cm = fminf(c[k], 0.f);
                e2 += cp * cp;
                e1 += cp;
                lg += logf(-cm + 1e-8f);
                if (!(c[k] < 0.f)) feas = 0.f;
                float dlog;
                mul[k] *= spil_phi(c[k], dlog);
                if (!(c[k] <= 0.f)) safe[k] = 0.f;
            }
        }
        ext += e2 * gpow;
        lin += e1 * gpow;
        itr += lg * gpow;
    }
};
// d(loss)/d(c) of one constraint value of one step: g_ext / g_lin / g_int the adjoints of the three sums, g_mul = dL/dP_k * P_k of
// SPIL's product (d P_k / d c = P_k Phi'(c) / Phi(c)), g_step the adjoint handed in for this very value
__device__ __forceinline__ float constraint_grad(float c, float g_ext, float g_lin, float g_int, float gpow, float g_mul, float g_step) {
    float gck = g_ext * 2.f * fmaxf(c, 0.f) + (c > 0.f ? g_lin : 0.f);
    if (c < 0.f) gck += g_int * (-1.f / (-c + 1e-8f));
    gck *= gpow;
    float dlog;
    (void)spil_phi(c, dlog);
    gck += g_mul * dlog;
    gck += g_step;
    return gck;
}

// ================================ reference tracking ==========================================
// One reference point rp = (x, y, phi, u) in the ego frame of the state sn = (x, y, phi, u, ...); cn / snn = cos / sin(-phi).
struct EgoPoint { float x, y, phi, u; };
__device__ __forceinline__ EgoPoint ref_point_to_ego(const f32x4& rp, const float* sn, float cn, float snn) {
    const float dx = rp[0] - sn[0], dy = rp[1] - sn[1];
    EgoPoint e;
    e.x = dx * cn - dy * snn;
    e.y = dx * snn + dy * cn;
    e.phi = angle_normalize(rp[2] - sn[2]);
    e.u = rp[3] - sn[3];
    return e;
}
// done tests of the vehicle models on the tracking errors of the first reference point.  Macros, not functions: hipcc turns the
// inlined function into a branch-free form that costs the register-stationary forward kernels (256 VGPRs, no scratch) a spilled
// register; the expression in place keeps the short-circuit branches those kernels were tuned with.
#define VEH_DONE(xtf, ytf, ptf) ((fabsf(xtf) > 10.f) || (fabsf(ytf) > 10.f) || (fabsf(ptf) > 3.14159265358979323846f))
#define VEH2_DONE(dy, dphi) ((fabsf(dy) > 2.f) || (fabsf(dphi) > 3.14159265358979323846f))
