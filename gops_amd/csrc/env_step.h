// The single wrapped env step (one trajectory) and the reference-trajectory generator it evaluates (which the reference table of
// prologue.hip evaluates too): shared by env_step_kernel (aux_kernels.hip, gops_env_step) and the episode kernel (rollout_episode.hip, gops_episode_rollout), so that
// both step the SAME arithmetic, statement for statement.
#pragma once
#include "common.h"
#include "env_models.h"
#include "rollout_env.h"

// ---------------------------------------------------------------------------------------------
// Reference trajectories of pyth_veh3dofconti (ref_traj_model.py:26-232).  Every operation is
// rounded separately in fp32, in the reference's order (no FMA contraction): the heading is a
// 1 ms finite difference whose cancellation noise is part of the reference's result.
// ---------------------------------------------------------------------------------------------
// Transcendentals are evaluated in double and rounded once (common.h SINF_CR / COSF_CR), i.e. correctly rounded in fp32: the CPU
// reference (Sleef u10) is correctly rounded for almost every argument, so this minimises the
// number of points where a 1-ulp difference in x(t) is amplified ~1e3x by the finite difference.
// One rounding per operation, never fused (common.h rn_mul / rn_add / rn_sub)
#define RMUL(a, b) rn_mul((a), (b))
#define RADD(a, b) rn_add((a), (b))
#define RSUB(a, b) rn_sub((a), (b))

// `c` = GopsEnv.ref_c (include/gops_hip.h): the reference's path / speed parameters, folded on the host where the
// reference folds Python scalars.  With the default set every expression below rounds exactly like the constants the
// first version of this file had spelled out (x + 0.0f and 1.0f * x are exact).
__device__ __forceinline__ float ref_arc(const float* __restrict__ c, float t, int u_num) {
    if (u_num == 0) return RADD(RADD(RMUL(c[0], COSF_CR(RADD(RMUL(c[1], t), c[2]))), RMUL(c[3], t)), c[4]);
    if (u_num == 1) return RMUL(c[6], t);
    return 0.f;   // a speed id outside the registered set selects no profile: every mask of the reference's sum is false
}

__device__ __forceinline__ void ref_xy(const float* __restrict__ c, float t, int path, int u_num, float& x, float& y) {
    const float s = ref_arc(c, t, u_num);
    if (path == 0) {
        x = s;
        y = RMUL(c[7], SINF_CR(RADD(RMUL(c[8], t), c[9])));
    } else if (path == 1) {
        x = s;
        if (t <= c[10]) y = c[14];
        else if (t <= c[11]) y = RADD(RMUL(c[16], RSUB(t, c[10])), c[14]);
        else if (t <= c[12]) y = c[15];
        else if (t <= c[13]) y = RADD(RMUL(c[17], RSUB(t, c[12])), c[15]);
        else y = c[14];
    } else if (path == 2) {
        x = s;
        float sm = fmodf(t, c[18]);
        if (sm != 0.f && ((c[18] < 0.f) != (sm < 0.f))) sm += c[18];   // torch.remainder: sign of the divisor
        if (sm <= c[21]) y = RMUL(c[19], sm);
        else if (sm < c[18]) y = RMUL(c[20], RSUB(sm, c[18]));
        else y = 0.f;
    } else {
        const float q = s / c[22];
        x = RMUL(c[22], SINF_CR(q));
        y = RMUL(c[22], RSUB(COSF_CR(q), 1.0f));
    }
}

__device__ __forceinline__ f32x4 ref_point(const float* __restrict__ c, float t, int path, int u_num) {
    float x0, y0, x1, y1;
    ref_xy(c, t, path, u_num, x0, y0);
    ref_xy(c, RADD(t, 0.001f), path, u_num, x1, y1);
    const float phi = (float)atan2((double)RSUB(y1, y0), (double)RSUB(x1, x0));
    const float u = (u_num == 0) ? RADD(RMUL(c[5], SINF_CR(RADD(RMUL(c[1], t), c[2]))), c[3]) : (u_num == 1) ? c[6] : 0.f;
    f32x4 r = {x0, y0, phi, u};
    return r;
}

// The point (x, y, phi, u)(t) for the float ids the batches carry (info["path_num"], info["u_num"]).  Ids outside the registered
// sets behave like the reference's masked sums `sum_i (id == i) * f_i(t)` (ref_traj_model.py:54-84, 138-142): an unknown path
// selects nothing (zeros), an unknown speed profile leaves arc length and speed at zero under a known path.
__device__ __forceinline__ f32x4 ref_point_ids(const float* __restrict__ c, float t, float pn, float un) {
    const int path = (pn == 0.f) ? 0 : (pn == 1.f) ? 1 : (pn == 2.f) ? 2 : (pn == 3.f) ? 3 : -1;
    const int us = (un == 0.f) ? 0 : (un == 1.f) ? 1 : -1;
    if (path < 0) return f32x4{0.f, 0.f, 0.f, 0.f};
    return ref_point(c, t, path, us);
}

// ---------------------------------------------------------------------------------------------
// The step of a model whose observation is the state, from and to global memory: the wrapped model step (env_models.h:
// state_model_step), or - DATA environment, GopsEnv.data_env - ONE base-model step without MaskAtDone / ActionRepeat /
// ClipObservation, with the data env's own ending: pyth_lq (lq_base.py:224-239) is done when the NEXT state leaves the state
// bounds (clip_obs: they are finite) and pays -100 for it; gym_cartpoleconti (env_gym/gym_cartpoleconti.py:102-137) rewards 1
// also for the step that ends the episode; pyth_idpendulum's data env calls the model's Dynamics.
// ---------------------------------------------------------------------------------------------
template <int ENV, int N>
__device__ __forceinline__ void env_step_state_model(const GopsEnv& env, bool data, bool dn, const float* ob,
                                                     const float (&u)[GOPS_MAX_ACT], float* nob, float& r, bool& done_m) {
    const int n = ENV == GOPS_ENV_LQ ? env.obs_dim : N;
    float o[N], on[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = i < n ? ob[i] : 0.f;
    if (!data) {
        state_model_step<ENV, N>(env, o, u, dn, on, r, done_m, n);
    } else {
        float x[GOPS_MAX_LQ_STATE] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, xn[GOPS_MAX_LQ_STATE] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < n) x[i] = obs_unscale(env, i, o[i]);
        state_model_substep<ENV>(env, x, u, xn, r, done_m);
        r += 0.f;   // the wrapped step's sum over its one sub-step: a reward of -0 leaves as +0
#pragma unroll
        for (int i = 0; i < N; ++i) {
            on[i] = obs_rescale(env, i, xn[i]);
            if (ENV == GOPS_ENV_LQ && env.clip_obs && i < n && (xn[i] > env.obs_high[i] || xn[i] < env.obs_low[i])) done_m = true;
        }
        if (ENV == GOPS_ENV_LQ && done_m) r -= 100.f;
        if (ENV == GOPS_ENV_CARTPOLE) r = 1.f;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (i < n) nob[i] = on[i];
}

// ---------------------------------------------------------------------------------------------
// Single wrapped env-model step (pyth_base_model.py:59-67 contract) of trajectory `b`.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void env_step_one(const GopsEnv& env, int b, const GopsStepIO& io, float pdt) {
    const int O = env.obs_dim, A = env.act_dim;
    const bool data = env.data_env != 0;   // the DATA environment's step (include/gops_hip.h: GopsEnv.data_env)
    float u[GOPS_MAX_ACT] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < A; ++a) u[a] = wrap_action(env, a, io.action[(size_t)b * A + a]);
    const bool dn = !data && !env.no_mask_at_done && io.done != nullptr && io.done[b] != 0.f;   // (no MaskAtDoneModel: done flags ignored)
    float r = 0.f;
    bool done_m = false;
    const float* ob = io.obs + (size_t)b * O;
    float* nob = io.next_obs + (size_t)b * O;
    if (env.kind == GOPS_ENV_LQ) {
        env_step_state_model<GOPS_ENV_LQ, GOPS_MAX_LQ_STATE>(env, data, dn, ob, u, nob, r, done_m);
    } else if (env.kind == GOPS_ENV_CARTPOLE) {
        env_step_state_model<GOPS_ENV_CARTPOLE, 4>(env, data, dn, ob, u, nob, r, done_m);
    } else if (env.kind == GOPS_ENV_PENDULUM) {
        env_step_state_model<GOPS_ENV_PENDULUM, 3>(env, data, dn, ob, u, nob, r, done_m);
    } else if (env.kind == GOPS_ENV_MOUNTAINCAR) {
        env_step_state_model<GOPS_ENV_MOUNTAINCAR, 2>(env, data, dn, ob, u, nob, r, done_m);
    } else if (env.kind == GOPS_ENV_IDPENDULUM) {
        env_step_state_model<GOPS_ENV_IDPENDULUM, 6>(env, data, dn, ob, u, nob, r, done_m);
    } else if (env.kind == GOPS_ENV_MOBILEROBOT) {
        const MobConst MC = mob_const();
        float x[MOB_OBS], xn[MOB_OBS], c;
        for (int i = 0; i < MOB_OBS; ++i) x[i] = ob[i];
        const float nv = io.noise != nullptr ? io.noise[(size_t)b * 2 + 0] : 0.f;
        const float nw = io.noise != nullptr ? io.noise[(size_t)b * 2 + 1] : 0.f;
        MobStep w;
        if (data) mob_forward<true>(MC, x, u[0], u[1], nv, nw, xn, r, c, done_m, w);   // pyth_mobilerobot.py:108-152: headings clipped to +-pi
        else mob_forward(MC, x, u[0], u[1], nv, nw, xn, r, c, done_m, w);
        io.constraint[b] = c;   // of the model's new state, whatever `done` says
        for (int i = 0; i < MOB_OBS; ++i) {
            const float v = dn ? x[i] : xn[i];
            nob[i] = (env.clip_obs && !data) ? clampf(v, env.obs_low[i], env.obs_high[i]) : v;   // (the data env clips nothing)
        }
    } else if (env.kind == GOPS_ENV_VEH2DOF) {
        const Veh2Const C2 = veh2_const();
        const int P = env.pre_horizon;
        float s[4], sn[4], o4[4];
        for (int i = 0; i < 4; ++i) { s[i] = io.state[(size_t)b * 4 + i]; o4[i] = ob[i]; }
        r = veh2_reward(o4, u[0]);
        float sphi, cphi;
        sincosf(s[1], &sphi, &cphi);
        veh2_f_xu(C2, s, u[0], sphi, cphi, sn);
        const float nt = RADD(io.ref_time[b], 0.1f);
        const float pn = io.path_num[b], un = io.u_num[b];
        const f32x4 newp = io.ref_appended != nullptr ? reinterpret_cast<const f32x4*>(io.ref_appended)[b]
                                                      : ref_point_ids(env.ref_c, RADD(nt, pdt), pn, un);
        const float* rin = io.ref_points + (size_t)b * (P + 1) * 2;
        float* rout = io.next_ref_points + (size_t)b * (P + 1) * 2;
        for (int i = 0; i < P; ++i) { rout[2 * i] = rin[2 * (i + 1)]; rout[2 * i + 1] = rin[2 * (i + 1) + 1]; }
        rout[2 * P] = newp[1]; rout[2 * P + 1] = newp[2];
        const float o0 = sn[0] - rout[0], o1 = sn[1] - rout[1];
        done_m = VEH2_DONE(o0, o1);
        if (data && done_m) r -= 100.f;   // data env (pyth_veh2dofconti.py:179-219): the model's step, -100 at done
        if (dn) {
            for (int i = 0; i < O; ++i) nob[i] = ob[i];
        } else {
            nob[0] = o0; nob[1] = o1; nob[2] = sn[2]; nob[3] = sn[3];
            for (int i = 1; i <= P; ++i) nob[3 + i] = sn[0] - rout[2 * i];
        }
        for (int i = 0; i < 4; ++i) io.next_state[(size_t)b * 4 + i] = sn[i];
        io.next_ref_time[b] = nt;
        if (env.cstr_err && io.constraint != nullptr) io.constraint[b] = fabsf(o4[0]) - env.err_tol[0];   // of the observation it was called with
    } else if (env.kind == GOPS_ENV_VEH3DOFCONTI || env.kind == GOPS_ENV_VEH3DOF_SURR) {
        const bool surr = env.kind == GOPS_ENV_VEH3DOF_SURR;
        const VehConst VC = veh_const();
        const int P = env.pre_horizon;
        float s[6], sn[6], o6[6];
        for (int i = 0; i < 6; ++i) { s[i] = io.state[(size_t)b * 6 + i]; o6[i] = ob[i]; }
        VehStep w;
        sincosf(s[2], &w.sphi, &w.cphi);
        veh_f_xu(VC, s, u[0], u[1], sn, w);
        r = surr ? veh_reward_w(env.reward_w, o6, u[0], u[1]) : veh_reward(o6, u[0], u[1]);
        float pen_c = 0.f;
        if (surr && env.surr_penalty) {   // collision penalty on the current pose / current surrounding vehicle
            const float* s5 = io.surr_state + (size_t)b * env.n_surr * 5;
            const f32x4 cur = {s5[0], s5[1], s5[2], s5[3]};
            SurrCstr sc0;
            surr_constraint<false>(env, s[0], s[1], w.sphi, w.cphi, &cur, sc0);
            float dummy;
            pen_c = sc0.c[0];
            r -= surr_penalty(pen_c, dummy);
        }
        const float nt = RADD(io.ref_time[b], 0.1f);
        const float pn = io.path_num[b], un = io.u_num[b];
        const f32x4 newp = io.ref_appended != nullptr ? reinterpret_cast<const f32x4*>(io.ref_appended)[b]
                                                      : ref_point_ids(env.ref_c, RADD(nt, pdt), pn, un);
        const f32x4* rin = reinterpret_cast<const f32x4*>(io.ref_points) + (size_t)b * (P + 1);
        f32x4* rout = reinterpret_cast<f32x4*>(io.next_ref_points) + (size_t)b * (P + 1);
        float cn, snn;
        sincosf(-sn[2], &snn, &cn);
        for (int j = 0; j <= P; ++j) {
            const f32x4 rp = (j < P) ? rin[j + 1] : newp;
            rout[j] = rp;
            const EgoPoint e = ref_point_to_ego(rp, sn, cn, snn);
            if (j == 0) {
                if (data)   // pyth_veh3dofconti.py:263-271: world-frame offsets to the first reference point, 5 / 2 / pi
                    done_m = (fabsf(rp[0] - sn[0]) > 5.f) || (fabsf(rp[1] - sn[1]) > 2.f) || (fabsf(e.phi) > 3.14159265358979323846f);
                else
                    done_m = VEH_DONE(e.x, e.y, e.phi);
                if (!dn) { nob[0] = e.x; nob[1] = e.y; nob[2] = e.phi; nob[3] = e.u; nob[4] = sn[4]; nob[5] = sn[5]; }
            } else if (!dn) {
                float* d = nob + 6 + 4 * (j - 1);
                d[0] = e.x; d[1] = e.y; d[2] = e.phi; d[3] = e.u;
            }
        }
        if (data && done_m) r -= 100.f;   // :224-226
        if (surr) {   // pyth_veh3dofconti_surrcstr_model.py:84-95: surrounding vehicles step, relative obs, constraint (unmasked)
            f32x4 pts[GOPS_MAX_SURR];
            for (int i = 0; i < env.n_surr; ++i) {
                const float* s5 = io.surr_state + ((size_t)b * env.n_surr + i) * 5;
                const f32x4 cur = {s5[0], s5[1], s5[2], s5[3]};
                pts[i] = surr_next(cur, s5[4]);
                float* d5 = io.next_surr_state + ((size_t)b * env.n_surr + i) * 5;
                d5[0] = pts[i][0]; d5[1] = pts[i][1]; d5[2] = pts[i][2]; d5[3] = pts[i][3]; d5[4] = s5[4];
                if (!dn) {
                    float* d = nob + 6 + 4 * P + 4 * i;
                    if (env.surr_penalty) {   // ego frame of the CURRENT state
                        const float dx = pts[i][0] - s[0], dy = pts[i][1] - s[1];
                        d[0] = dx * w.cphi + dy * w.sphi; d[1] = -dx * w.sphi + dy * w.cphi;
                        d[2] = angle_normalize(pts[i][2] - s[2]); d[3] = pts[i][3] - s[3];
                    } else {
                        d[0] = pts[i][0] - sn[0]; d[1] = pts[i][1] - sn[1]; d[2] = pts[i][2] - sn[2]; d[3] = pts[i][3] - sn[3];
                    }
                }
            }
            SurrCstr sc;
            float sp, cp;
            sincosf(sn[2], &sp, &cp);
            surr_constraint<false>(env, sn[0], sn[1], sp, cp, pts, sc);
            if (env.surr_penalty) sc.c[0] = pen_c;   // info["constraint"] is filled before the info dict is updated (:131-139)
            if (env.cstr_err) { sc.c[0] = fabsf(o6[1]) - env.err_tol[0]; sc.c[1] = fabsf(o6[3]) - env.err_tol[1]; }   // current obs
            for (int k = 0; k < env.n_constraint; ++k) io.constraint[(size_t)b * env.n_constraint + k] = sc.c[k];
            if (env.surr_penalty) done_m = false;
        }
        if (dn) for (int i = 0; i < O; ++i) nob[i] = ob[i];
        for (int i = 0; i < 6; ++i) io.next_state[(size_t)b * 6 + i] = sn[i];
        io.next_ref_time[b] = nt;
    }
    float rr = dn ? 0.f : r;
    if (env.shaping) rr = (rr + env.reward_shift) * env.reward_scale;
    io.reward[b] = rr;
    io.next_done[b] = (dn || done_m) ? 1.f : 0.f;
}
