/*
 * gops_hip.h - C ABI of the MI355X-native GOPS ADP hot path (libgops_hip.so).
 *
 * Drop-in boundary for the reference's model-based ADP gradient loop.  Each entry point names
 * the reference interface it replaces (paths relative to the GOPS tree):
 *
 *   gops_rollout_forward   <- the H-step loop  `a = policy(o, t); o,r,d,info = envmodel.forward(...)`
 *                             of FHADP._compute_loss_policy      (gops/algorithm/fhadp.py:113-125)
 *                             and INFADP.__compute_loss_v/_policy (gops/algorithm/infadp.py:159-213),
 *                             i.e. MLP policy eval (gops/apprfunc/mlp.py:73-77,103-111), the wrapper
 *                             chain (gops/create_pkg/create_env_model.py:104-126) and the env models
 *                             pyth_lq / pyth_idpendulum / pyth_veh3dofconti
 *                             (gops/env/env_ocp/resources/lq_base.py:343-354,
 *                              gops/env/env_ocp/env_model/pyth_idpendulum_model.py:199-216,
 *                              gops/env/env_ocp/env_model/pyth_veh3dofconti_model.py:91-145).
 *   gops_rollout_backward  <- `loss.backward()` of the same functions (fhadp.py:108, infadp.py:143,151):
 *                             fills per-parameter gradients in torch nn.Linear layout.
 *   gops_rollout_backward_open_loop <- `loss.backward()` of FHADP2 (gops/algorithm/fhadp2.py:89) down to
 *                             the action sequence emitted by the single policy evaluation.
 *   gops_env_step          <- one wrapped `env_model.forward(obs, action, done, info)`
 *                             (gops/env/env_ocp/env_model/pyth_base_model.py:59-67), kept for
 *                             per-step consumers (gops/sys_simulator/opt_controller.py:240-300).
 *   gops_value_forward/backward <- `v = self.networks.v(o)` and its backward in INFADP PEV
 *                             (infadp.py:167,185; StateValue gops/apprfunc/mlp.py:327-329).
 *
 * Conventions: every buffer is caller-allocated DEVICE memory (fp32 unless noted); the library
 * allocates no device memory on the data path and keeps no per-call state, so calls on different
 * workspaces are re-entrant.  Process-wide state is limited to: the opt-in timing hook
 * (gops_profile_*: HIP events, mutex-guarded), the cached CU count of the device, a one-time
 * hipFuncSetAttribute per kernel, and - debug builds only - one counter buffer.  All work is enqueued on `stream`
 * (a hipStream_t passed as void*); no call synchronises.  Return value: 0 on success, a
 * negative GOPS_ERR_* code or a positive hipError_t otherwise; nothing throws across the ABI.
 */
#ifndef GOPS_HIP_H
#define GOPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define GOPS_HIP_ABI_VERSION 15

#define GOPS_MAX_LAYERS 5   /* Linear layers per MLP (<= 4 hidden + output) */
#define GOPS_MAX_ACT 4      /* action dimensions */
#define GOPS_MAX_LQ_STATE 6
#define GOPS_MAX_HORIZON 256
#define GOPS_TILE 16        /* trajectories per workgroup tile (MFMA M) */

enum { GOPS_OK = 0, GOPS_ERR_BAD_ARG = -1, GOPS_ERR_UNSUPPORTED = -2, GOPS_ERR_WORKSPACE = -3 };

/* env kinds: the three env models named by BASELINE.json + NONE (plain MLP batch evaluation) */
enum { GOPS_ENV_NONE = 0, GOPS_ENV_LQ = 1, GOPS_ENV_IDPENDULUM = 2, GOPS_ENV_VEH3DOFCONTI = 3,
       /* veh3dofconti + surrounding vehicles + constraint outputs: pyth_veh3dofconti_surrcstr_model.py:42-148 and
          pyth_veh3dofconti_detour_model.py:40-181 (the models behind FHADPExterior / Interior / Lagrangian) */
       GOPS_ENV_VEH3DOF_SURR = 4,
       /* gym-style models of the INFADP / MAC example scripts (obs == state, no info):
          gops/env/env_gym/env_model/gym_cartpoleconti_model.py:24-129 and gym_pendulum_model.py:26-115 */
       GOPS_ENV_CARTPOLE = 5, GOPS_ENV_PENDULUM = 6,
       /* pyth_veh2dofconti_model.py:24-174: lateral 2-DOF vehicle at constant speed tracking the reference path: state
          (y, phi, v, omega) [B,4], action steer, obs = (y - y_ref0, phi - phi_ref0, v, omega, y - y_ref_1 .. y - y_ref_P),
          info["ref_points"] [B, P+1, 2] = (y, phi) */
       GOPS_ENV_VEH2DOF = 7,
       /* pyth_mobilerobot_model.py:24-213 (the model of example_train/spil/spil_mlp_mobilerobot_{offserial,async}.py):
          obs == state [B,13] = ego (x, y, theta, v, w), tracking errors (e_y, e_theta, e_v), one obstacle robot
          (x, y, theta, v, w); action (v_cmd, w_cmd); dt = 0.2.  The ego follows its rate-limited, saturated commands, the
          obstacle its own (v, w) plus the noise draws handed in through GopsRolloutIn.noise / GopsStepIO.noise;
          info["constraint"] [B,1] = 0.89 - distance(obstacle', ego') of the NEW state (n_constraint = 1, unmasked);
          done = x' < -2 | |y'| > 4 | constraint > 0.15.  fp32 only; ClipObservation over all 13 columns. */
       GOPS_ENV_MOBILEROBOT = 8,
       /* gym_mountaincarconti_model.py:21-99 (additive, the version number stays 15): obs == state [B,2] = (pos, vel), one action in
          [-1, 1], observation bounds [-1.2, 0.6] x [-0.07, 0.07], no dt, no GopsEnv field beyond the common ones.  One step:
            vel' = clamp(vel + 0.0015 a - 0.0025 cos(3 pos), -0.07, 0.07);  pos' = clamp(pos + vel', -1.2, 0.6);
            vel' = 0 where pos' == -1.2 and vel' < 0 (behind the position update, which used the unzeroed vel');
            done = pos' >= 0.45 and vel' >= 0 on the NEXT state;  reward = 100 done - 0.1 a^2.
          Every operation rounds separately in the reference's order and the cosine is correctly rounded, so the clamps, the exact
          wall compare and the done test fall as in the reference.  Adjoint: clamps pass on their closed interval, the wall rule cuts
          the path into the returned vel' only (not vel' -> pos'), the indicator has no gradient, d reward / d a = -0.2 a.
          Takes every wrapper GOPS_ENV_PENDULUM takes (ScaleAction, ClipAction, ClipObservation, ScaleObservation, ShapingReward,
          ActionRepeat, MaskAtDone or none); the MLP rollouts (streamed kernels), the adjoint I/O of
          gops_rollout_backward_open_loop_adj, the POLY / RBF lane rollouts and gops_env_step.  fp32 only: GOPS_DTYPE_F16 is refused
          with GOPS_ERR_UNSUPPORTED (a half-precision plane cannot hold the 0.07 / 1.2 thresholds the branches compare against
          exactly); data_env = 1 likewise (no data-env restatement).  GOPS_ERR_BAD_ARG: obs_dim != 2, act_dim != 1, or an empty
          action range (min_action >= max_action or act_low > act_high, NaN included: ScaleAction would divide by zero and the NaN
          action would decide every branch). */
       GOPS_ENV_MOUNTAINCAR = 9 };
#define GOPS_MAX_SURR 4        /* surrounding vehicles */
#define GOPS_MAX_CONSTRAINT 3  /* constraint outputs per step */
#define GOPS_MAX_REPEAT 8      /* ActionRepeatModel: sub-steps per env step */
#define GOPS_MAX_CLIP_OBS 16   /* observation columns ClipObservationModel can act on */

/* hidden activations: gops/utils/common_utils.py:26-55 */
enum { GOPS_ACT_LINEAR = 0, GOPS_ACT_RELU = 1, GOPS_ACT_ELU = 2, GOPS_ACT_GELU = 3,
       GOPS_ACT_SELU = 4, GOPS_ACT_SIGMOID = 5, GOPS_ACT_TANH = 6 };
/* ABI v15: feature maps of a POLY net (gops/apprfunc/poly.py), in GopsMlp.hidden_act of a description with n_layers = 1.
 *   GOPS_POLY_FULL_d  make_features(obs, d) (:30-49): for k = 1..d the full k-fold outer product of the observation in n_matmul
 *                     order, i-major, duplicates included (degree 3: (x_i x_j) x_l): F = n + n^2 + .. + n^d features.
 *   GOPS_POLY_SYM_2   create_features(obs * norm_matrix, 2) (:61-83): x_i x_j for i <= j, i-major: n (n + 1) / 2 features. */
enum { GOPS_POLY_FULL_1 = 16, GOPS_POLY_FULL_2 = 17, GOPS_POLY_FULL_3 = 18, GOPS_POLY_SYM_2 = 24 };
/* Heads of an RBF net (gops/apprfunc/gauss.py), in GopsMlp.hidden_act of a description with n_layers = 1 (additive, the version
 * number stays 15): y = w phi(x) + b over K Gaussian kernels, then
 *   GOPS_RBF_AFFINE  DetermPolicy (:61-65): a = half y + mid, x = obs
 *   GOPS_RBF_TANH    FiniteHorizonPolicy (:85-93): a = half tanh(y) + mid, x = (obs, virtual_t = step + 1)
 * with half = (policy_high - policy_low) / 2 and mid = (policy_high + policy_low) / 2 of GopsEnv. */
enum { GOPS_RBF_AFFINE = 32, GOPS_RBF_TANH = 33 };

/* Arithmetic of the MLP contractions (BASELINE.json configs[4]: "fp16 MFMA MLP path").
 *   GOPS_DTYPE_F32: fp32 results at the 1e-4 parity bar (default).  NOT bit-level fp32 arithmetic where the plane-split
 *                   kernels run (gops_rollout_variant bits 0 / 2; every 256-wide net): weights, activations and deltas are
 *                   each carried as two IEEE-half planes x s = hi + lo / 2^11 (22 significant bits, fp32 has 24; s a power of
 *                   two - per 16 output features for weights, 2^-4 for forward activations, from max|delta| in the sweep),
 *                   a w = hi hi + (lo hi + hi lo) / 2^11 on three v_mfma_f32_16x16x32_f16 with fp32 accumulation; the large
 *                   weight-gradient GEMMs likewise (deltas scaled by the sweep's largest |delta_y|, saturated blocks redone exactly).
 *                   Forward range |activation| < 1.05e6: beyond it the launch's results are NaN (never silently wrong).
 *                   Measured distance to the reference on trained 256-wide networks 2e-6 .. 3e-5, at the level of the exact
 *                   fp32 kernels.  GOPS_VF_STREAMED_FP32 | GOPS_VF_DW_F32 in the descriptor's
 *                   variant_flags select v_mfma_f32_16x16x4_f32 (an fmaf chain) throughout.
 *   GOPS_DTYPE_F16: weights, hidden activations and deltas rounded to IEEE half, products accumulated
 *                   in fp32 by v_mfma_f32_16x16x32_f16; the activation stash is half (2 bytes/element).
 *                   Env model, wrapper chain, rewards, returns, observation / state adjoints, policy
 *                   head and every result stay fp32.  The backward pass runs on gradients scaled by a
 *                   power of two chosen from max|grad_v| on the device (deltas stay inside half's
 *                   range) and un-scales the parameter gradients; tolerance: DESIGN.md section 2. */
enum { GOPS_DTYPE_F32 = 0, GOPS_DTYPE_F16 = 1 };

/* An MLP in torch nn.Linear layout: layer j has weight [sizes[j+1]][sizes[j]] row-major and
 * bias [sizes[j+1]].  Hidden widths must be multiples of 16 (64 with GOPS_DTYPE_F16); the input width is arbitrary.
 * Weights and biases are always fp32 in memory; the F16 path rounds them when it packs them. */
typedef struct GopsMlp {
    int32_t n_layers;                      /* number of Linear layers, 2..GOPS_MAX_LAYERS */
    int32_t sizes[GOPS_MAX_LAYERS + 1];    /* in, hidden..., out */
    int32_t hidden_act;                    /* GOPS_ACT_* */
    int32_t dtype;                         /* GOPS_DTYPE_*: read by gops_value_forward / _backward only
                                              (a rollout takes GopsRolloutDesc.dtype for all its nets) */
    uint32_t variant_flags;                /* ABI v10: GOPS_VF_* for gops_value_* / gops_mlp_* calls (a rollout takes
                                              GopsRolloutDesc.variant_flags); 0 = the library's choice.  Occupies what was
                                              alignment padding in v9: offsets and size are unchanged */
    const float* weight[GOPS_MAX_LAYERS];  /* device pointers */
    const float* bias[GOPS_MAX_LAYERS];
} GopsMlp;

/* Gradients of one MLP, same shapes/layout as GopsMlp weight/bias (device, overwritten). */
typedef struct GopsMlpGrad {
    float* weight[GOPS_MAX_LAYERS];
    float* bias[GOPS_MAX_LAYERS];
} GopsMlpGrad;

/* The wrapped env model: base model constants + the wrapper chain built by create_env_model. */
typedef struct GopsEnv {
    int32_t kind;                 /* GOPS_ENV_* */
    int32_t obs_dim, act_dim;
    int32_t pre_horizon;          /* veh3dofconti: number of preview points P (obs_dim = 6+4P) */
    /* ScaleActionModel / ClipActionModel (scale_action.py:75-83, clip_action.py:34-36) */
    float min_action[GOPS_MAX_ACT], max_action[GOPS_MAX_ACT];
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];       /* base-model action bounds */
    /* tanh squash of the policy head (mlp.py:73-77): act_high_lim / act_low_lim buffers */
    float policy_low[GOPS_MAX_ACT], policy_high[GOPS_MAX_ACT];
    /* ClipObservationModel (clip_observation.py:38-40); +-inf = inactive */
    int32_t clip_obs;             /* 0: all bounds infinite (idpendulum, veh3dofconti) */
    float obs_low[GOPS_MAX_CLIP_OBS], obs_high[GOPS_MAX_CLIP_OBS];
    /* ShapingRewardModel (shaping_reward.py:84-88), applied outside MaskAtDone */
    int32_t shaping;
    float reward_scale, reward_shift;
    /* pyth_lq constants (lq_base.py:39-57): x' = inv_IA (x + dt B u), r = rs*(rsh - (Qx^2+Ru^2)) */
    float lq_inv_IA[GOPS_MAX_LQ_STATE * GOPS_MAX_LQ_STATE];    /* row-major n x n */
    float lq_B[GOPS_MAX_LQ_STATE * GOPS_MAX_ACT];              /* row-major n x m */
    float lq_Q[GOPS_MAX_LQ_STATE], lq_R[GOPS_MAX_ACT];
    float lq_dt, lq_reward_scale, lq_reward_shift;
    /* GOPS_ENV_VEH3DOF_SURR: obs_dim = 6 + 4 P + 4 n_surr; each surrounding vehicle follows its own kinematic
     * bicycle (x, y, phi, u, delta; SurrVehicleModel :28-39) independently of the policy; the observation appends
     * (x, y, phi, u)_surr - (x, y, phi, u)_ego per vehicle; constraint[0] = 2 r - min distance between the two ego
     * circles and the two circles of every surrounding vehicle (bicircle model, :98-148); n_constraint = 3 adds the road
     * boundary violations of the detour model (:143-151); the stage reward is
     * -(w[0] dx^2 + w[1] dy^2 + w[2] dphi^2 + w[3] du^2 + w[4] omega^2 + w[5] steer^2 + w[6] a_x^2 + w[7] v^2).
     * surr_penalty = 1 selects pyth_veh3dofconti_surrcstr_penalty_model.py:74-246 (one surrounding vehicle): the stage
     * reward also carries the collision penalty -15 (tanh(max(8 - 16 dis, 0) - 4) + 1), dis = min circle distance - 2 r,
     * evaluated on the CURRENT state; the appended observation is the NEXT surrounding-vehicle state in the ego frame of
     * the CURRENT state (x, y, phi rotated, u relative); the model never reports done; info["constraint"] (and the
     * constraint sums) are those of the CURRENT pose and carry no gradient (the model computes them on detached copies). */
    /* 1: no MaskAtDoneModel in the chain (mask_at_done.py:33-40): the model keeps stepping after its done test fired,
     * rewards are not zeroed (the raw model OptController drives, opt_controller.py:261-265; create_env_model(mask_at_done =
     * False), create_env_model.py:104-105).  The done flags handed in are ignored; final_done (and the mask of a tail
     * value) is the base model's done test on the LAST state.  Not for GOPS_ENV_VEH3DOF_SURR (final_done stays 0 there). */
    int32_t no_mask_at_done;
    int32_t n_surr, n_constraint, surr_penalty;
    float veh_length, veh_width, road_upper, road_lower;
    float reward_w[8];
    /* gops_env_step only (rollouts reject it): 1 = the step of the DATA environment the reference's samplers drive
     * (gops/env/env_ocp/pyth_veh3dofconti.py:195-271, resources/lq_base.py:209-231, pyth_idpendulum.py:71-87) instead
     * of the env MODEL's: same dynamics and stage reward, but the data env's termination tests (veh3dofconti: world-frame
     * |x - x_ref| > 5, |y - y_ref| > 2, |dphi| > pi; lq: next state outside the state bounds), a -100 terminal penalty
     * (veh3dofconti, lq), no observation clipping and no MaskAtDone (an episode that is done gets reset by the caller:
     * the `done` input is ignored).  GOPS_ENV_MOBILEROBOT (round 6; pyth_mobilerobot.py:108-152): the model's step with both new
     * headings clipped to +-pi, no terminal penalty. */
    int32_t data_env;
    /* ScaleObservationModel (gops/env/wrapper/scale_observation.py:74-119; create_env_model.py:115-118 puts it between
     * ShapingReward and ClipObservation): the observations the policy and the caller see are (obs + obs_shift) * obs_scale;
     * the model steps obs / obs_scale - obs_shift.  GOPS_ENV_LQ / _IDPENDULUM / _CARTPOLE / _PENDULUM / _MOUNTAINCAR only (obs_dim <= 8).  As in the
     * reference, ClipObservationModel then clips the SCALED observation with the model's own (unscaled) bounds. */
    int32_t scale_obs;
    float obs_scale[8], obs_shift[8];
    /* GOPS_ENV_VEH3DOF_SURR with cstr_err = 1: pyth_veh3dofconti_errcstr_model.py:22-55 - no surrounding vehicles
     * (n_surr = 0), n_constraint = 2: info["constraint"] = (|obs[1]| - err_tol[0], |obs[3]| - err_tol[1]) of the CURRENT
     * observation (lateral and speed tracking errors). */
    int32_t cstr_err;
    float err_tol[2];
    /* Reference-trajectory parameters of the veh3dofconti / veh2dofconti families (MultiRefTrajModel(path_para, u_para),
     * gops/env/env_ocp/resources/ref_traj_model.py:26-52; defaults ref_traj_data.py:18-37).  ref_custom = 0: the library
     * uses the default set.  ref_custom = 1: ref_c holds the constants, each folded in double on the host exactly where
     * the reference folds Python scalars and then rounded to fp32:
     *   [0] -A/omega  [1] omega  [2] phi  [3] b  [4] A/omega*cos(phi)  [5] A      sine speed profile
     *   [6] u                                                                   constant speed profile
     *   [7] A  [8] omega  [9] phi                                                sine path
     *   [10..13] t1..t4  [14] y1  [15] y2  [16] (y2-y1)/(t2-t1)  [17] (y1-y2)/(t4-t3)   double-lane path
     *   [18] T  [19] 2A/T  [20] -2A/T  [21] T/2                                  triangle path
     *   [22] r                                                                  circle path */
    int32_t ref_custom;
    float ref_c[24];
    /* ActionRepeatModel around MaskAtDoneModel (gops/create_pkg/create_env_model.py:104-107, gops/env/wrapper/
     * action_repeat.py:54-87): repeat_num >= 2 applies the masked base step repeat_num times to the advancing observation
     * with the INITIAL done flags; the rewards are summed (repeat_last_reward = 1: only the last one is returned), done is
     * the last sub-step's.  0 / 1 = no wrapper.  Supported for the models whose observation is the state (GOPS_ENV_LQ,
     * _IDPENDULUM, _CARTPOLE, _PENDULUM, _MOUNTAINCAR; the reference wrapper does not advance `info`), fp32, repeat_num <= GOPS_MAX_REPEAT. */
    int32_t repeat_num;
    int32_t repeat_last_reward;
} GopsEnv;

typedef struct GopsRolloutDesc {
    int32_t batch;            /* B trajectories */
    int32_t horizon;          /* H = pre_horizon (FHADP) or forward_step (INFADP) */
    int32_t finite_horizon;   /* 1: FiniteHorizonPolicy, time index t+1 appended to the input */
    int32_t need_grad;        /* 1: keep the activation stash for gops_rollout_backward */
    int32_t tail_value;       /* 1: v += (~done_H) gamma^H V(obs_H)   (infadp.py:182-184, 210) */
    int32_t open_loop;        /* 1: no policy evaluation inside the rollout - the pre-tanh head outputs of
                                 every step come from GopsRolloutIn.head_pre (FHADP2: one MLP evaluation
                                 emits all H actions, gops/algorithm/fhadp2.py:100-121); `policy` is ignored.
                                 2: as 1, but head_pre holds the MODEL ACTIONS themselves (no tanh squash, no
                                 ScaleAction / ClipAction): the shooting rollout of an optimal-control solver over
                                 the raw model, gops/sys_simulator/opt_controller.py:240-300; the backward returns
                                 d(loss)/d(action) */
    int32_t dtype;            /* GOPS_DTYPE_F32 (default) or GOPS_DTYPE_F16: arithmetic of the MLP contractions
                                 (hidden widths must then be multiples of 64) */
    int32_t tail_unmasked;    /* with tail_value: 1 = v += gamma^H V(obs_H) for finished trajectories too
                                 (SPIL's evaluation target, gops/algorithm/spil.py:208) */
    uint32_t variant_flags;   /* ABI v10: GOPS_VF_* bits - which kernel variants this rollout may NOT / must take.  0 = the
                                 library's choice (gops_rollout_variant reports it).  Part of the description: two callers
                                 in one process can choose differently, and forward / backward of one rollout must pass
                                 the same value */
    int32_t l2_warmup;        /* ABI v10: backward sweep's L2 warm-up of the next step's stash rows: 0 = library default,
                                 1 = off, 2 = all at the step top, 3 = spread over the step (tuning) */
    int32_t dw_workgroups;    /* ABI v10: target workgroup count of a weight-gradient GEMM, 0 = default (512) (tuning) */
    int32_t reserved0;
    double gamma;             /* discount; gamma^t is formed in double then rounded (fhadp.py:120) */
    GopsEnv env;
    GopsMlp policy;           /* out width = act_dim */
    GopsMlp value;            /* used iff tail_value (out width 1): INFADP's v_target */
} GopsRolloutDesc;

/* Batch inputs (the `data` dict of the algorithms). */
typedef struct GopsRolloutIn {
    const float* obs;         /* [B, obs_dim] */
    const float* done;        /* [B] 0/1 */
    const float* state;       /* veh3dofconti info["state"]      [B,6]      else NULL */
    const float* ref_points;  /* veh3dofconti info["ref_points"] [B,P+1,4]  else NULL */
    const float* path_num;    /* [B] */
    const float* u_num;       /* [B] */
    const float* ref_time;    /* [B] */
    const float* head_pre;    /* open_loop only: [B, H, act_dim] policy-head outputs BEFORE the tanh squash */
    const float* surr_state;  /* GOPS_ENV_VEH3DOF_SURR info["surr_state"] [B, n_surr, 5] (x, y, phi, u, delta) else NULL */
    const float* grad_constraint; /* gops_rollout_backward, GOPS_ENV_VEH3DOF_SURR: d(loss)/d(constraint_sums) [3, B]
                                 (rows as in GopsRolloutOut.constraint_sums); NULL = zeros */
    const float* grad_constraint_prod; /* gops_rollout_backward, GOPS_ENV_VEH3DOF_SURR: [n_constraint, B]
                                 d(loss)/d(P_k) * P_k for the products P_k of GopsRolloutOut.constraint_prods; NULL = zeros */
    const float* ref_appended; /* ABI v8, models with reference trajectories, or NULL: [B, H, 4] (x, y, phi, u) - the point the
                                 model APPENDS to info["ref_points"] at rollout step s (ref_traj_model.py:26-148 evaluated at
                                 ref_time + (s + 1) dt + P dt), supplied by the caller instead of evaluated by the library.
                                 Bit-parity mode: the reference's heading is a 1 ms finite difference in fp32 whose last-ulp
                                 behaviour depends on the host's libm; a caller that fills this tensor with the reference's own
                                 MultiRefTrajModel values gets observations identical to the reference's. */
    const float* noise;       /* ABI v9, GOPS_ENV_MOBILEROBOT, or NULL (= zeros): [H, B, 2] the obstacle robot's N(0, 0.03) / N(0, 0.02)
                                 draws of every rollout step, exactly what np.random.normal returns inside Robot.f_xu(.., "obs")
                                 (pyth_mobilerobot_model.py:143-167; the model adds 0.5 x draw to the obstacle's v / w).  Must stay
                                 valid until the backward call (d x' / d theta of the obstacle depends on it). */
    const float* grad_constraint_step; /* ABI v9, backward calls of the models with constraint outputs, or NULL (= zeros): [H, B, n_constraint]
                                 d(loss)/d(c_tk) for the per-step constraint values of GopsRolloutOut.constraints - a caller that needs
                                 the Jacobian of the constraint path (OptController's inequality constraints, gops/sys_simulator/
                                 opt_controller.py:178-206) replicates the trajectory once per row and seeds one unit entry each */
} GopsRolloutIn;

typedef struct GopsRolloutOut {
    float* v_pi;              /* [B] sum_t gamma^t r_t (+ tail); required */
    float* rewards;           /* [H,B] per-step (masked, shaped) rewards, or NULL */
    float* final_obs;         /* [B, obs_dim] or NULL */
    float* final_done;        /* [B] or NULL */
    float* final_state;       /* veh3dofconti [B,6] or NULL */
    /* Models with constraint outputs (GOPS_ENV_VEH3DOF_SURR, _VEH2DOF with cstr_err, _MOBILEROBOT), or NULL: [4, B] discounted sums over the rollout of the UNMASKED info["constraint"] c_t
     * (the algorithms read it regardless of `done`):
     *   row 0  sum_t gamma^t sum_k max(c_tk, 0)^2            (fhadp_exterior.py:64, fhadp_interior.py:66)
     *   row 1  sum_t gamma^t sum_k max(c_tk, 0)              (fhadp_lagrangian.py:66)
     *   row 2  sum_t gamma^t sum_k log(-min(c_tk, 0) + 1e-8) (fhadp_interior.py:65)
     *   row 3  1 if every c_tk < 0 (feasible trajectory, fhadp_interior.py:71) else 0 */
    float* constraint_sums;
    /* Same models, or NULL: [2 n_constraint, B] products over the rollout (gops/algorithm/spil.py:189-251):
     *   rows 0 .. n_constraint-1        P_k = prod_t Phi(c_tk),  Phi(y) = 1.07 / (1 + 0.0315 exp(clamp(y / 0.07, -10, 5)))
     *   rows n_constraint .. 2 n_c - 1  prod_t [c_tk <= 0]       (trajectory safe w.r.t. constraint k: 0 / 1) */
    float* constraint_prods;
    /* ABI v9, same models, or NULL: [H, B, n_constraint] the UNMASKED info["constraint"] the model returns at every step
     * (errcstr models: of the observation the step STARTS from; surrcstr / detour / mobilerobot: of the NEW state) */
    float* constraints;
} GopsRolloutOut;

int gops_hip_version(void);

/* Bytes of scratch `workspace` needed by forward(+backward) for this descriptor. */
size_t gops_rollout_workspace_bytes(const GopsRolloutDesc* desc);

int gops_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in,
                         const GopsRolloutOut* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Back-propagate d(loss)/d(v_pi[b]) = grad_v[b] through the stashed rollout into the policy
 * parameters (value/target parameters receive no gradient, as in the reference). */
int gops_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in,
                          const float* grad_v, const GopsMlpGrad* policy_grad,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Open-loop counterpart of gops_rollout_backward: d(loss)/d(head_pre) [B, H, act_dim] of a forward
 * run with desc->open_loop = 1 (the caller back-propagates it through its single MLP evaluation -
 * FiniteHorizonFullPolicy.forward_all_policy, gops/apprfunc/mlp.py:140-145). */
int gops_rollout_backward_open_loop(const GopsRolloutDesc* desc, const GopsRolloutIn* in,
                                    const float* grad_v, float* grad_head_pre,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Adjoints around a closed-loop rollout (ABI v5): what a caller needs to put a rollout in the middle of a larger
 * differentiable expression.  MPG's model return (gops/algorithm/mpg.py:340-353) is
 *     sum_t gamma^t r_t + gamma^H q1_target(o_H, policy(o_H))
 * where only step 0 acts through `policy`; later steps act through the frozen copy `policy4rollout` (same weights,
 * requires_grad False: gradients still flow through its INPUT).  The terminal term is evaluated by the caller
 * (gops_mlp_forward / gops_mlp_backward_x) and comes back as `grad_final_obs`.
 * Supported for the env kinds whose observation is the model state (GOPS_ENV_NONE, _LQ, _IDPENDULUM, _CARTPOLE,
 * _PENDULUM, _MOUNTAINCAR), fp32, tail_value = 0, closed loop. */
typedef struct GopsRolloutAdjoint {
    const float* grad_final_obs;  /* [B, obs_dim] d(loss)/d(final_obs) (GopsRolloutOut.final_obs); NULL = zeros */
    float* grad_obs;              /* out [B, obs_dim]: d(loss)/d(obs) of the initial observation; NULL = not wanted */
    int32_t first_step_only;      /* 1: parameter gradients only through the action of step 0 (mpg.py:343-349) */
    int32_t reserved;
} GopsRolloutAdjoint;
/* gops_rollout_backward with the adjoints above; policy_grad may be NULL (no parameter gradients wanted). */
int gops_rollout_backward_adj(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                              const GopsMlpGrad* policy_grad, const GopsRolloutAdjoint* adj,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Open-loop rollout with adjoint I/O (ABI v8): gops_rollout_backward_open_loop seeded with d(loss)/d(final_obs) and
 * returning d(loss)/d(obs) of the initial observation next to d(loss)/d(head_pre) - one collocation interval of
 * OptController (gops/sys_simulator/opt_controller.py:104-109, 196-215: the decision variables are the actions AND the
 * states at the control points; cost and transition-constraint Jacobians need both adjoints).  Same env kinds as
 * gops_rollout_backward_adj; adj->first_step_only is ignored. */
int gops_rollout_backward_open_loop_adj(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                                        float* grad_head_pre, const GopsRolloutAdjoint* adj,
                                        void* workspace, size_t workspace_bytes, void* stream);

/* One wrapped env-model step.  `action` is the raw (pre-wrapper) action [B, act_dim].  For
 * veh3dofconti the info tensors are updated into the next_* outputs (may alias the inputs
 * except ref_points). */
typedef struct GopsStepIO {
    const float* obs; const float* action; const float* done;
    const float* state; const float* ref_points; const float* path_num; const float* u_num;
    const float* ref_time;
    float* next_obs; float* reward; float* next_done;
    float* next_state; float* next_ref_points; float* next_ref_time;
    /* GOPS_ENV_VEH3DOF_SURR: info["surr_state"] [B, n_surr, 5] in / out, info["constraint"] [B, n_constraint] out */
    const float* surr_state; float* next_surr_state; float* constraint;
    const float* ref_appended;   /* ABI v8, or NULL: [B, 4] (veh2dofconti: (., y, phi, .)) the reference point this step appends,
                                    from the caller (see GopsRolloutIn.ref_appended) */
    const float* noise;          /* ABI v9, GOPS_ENV_MOBILEROBOT, or NULL (= zeros): [B, 2] this step's obstacle draws (GopsRolloutIn.noise) */
} GopsStepIO;
int gops_env_step(const GopsEnv* env, int32_t batch, const GopsStepIO* io, void* stream);

/* model.get_constraint(obs, info) (ABI v9; gops/env/env_ocp/env_model/pyth_base_model.py:69-75 - the hook OptController evaluates on
 * every state of its prediction, opt_controller.py:178-198): io->constraint [B, n_constraint] of the given io->obs (errcstr models:
 * pyth_veh3dofconti_errcstr_model.py:49-56, pyth_veh2dofconti_errcstr_model.py:47-51) or of the given io->state / io->surr_state
 * (pyth_veh3dofconti_surrcstr_model.py:98-148, _detour_model.py:102-151, _surrcstr_penalty_model.py:183-234).  Nothing else of
 * `io` is read or written.  GOPS_ERR_UNSUPPORTED for models that define no get_constraint. */
int gops_env_constraint(const GopsEnv* env, int32_t batch, const GopsStepIO* io, void* stream);

/* StateValue batch evaluation v = V(obs) with stash, and its backward into V's parameters. */
size_t gops_value_workspace_bytes(const GopsMlp* value, int32_t batch);
int gops_value_forward(const GopsMlp* value, int32_t batch, const float* obs, float* v,
                       void* workspace, size_t workspace_bytes, void* stream);
int gops_value_backward(const GopsMlp* value, int32_t batch, const float* obs, const float* grad_v,
                        const GopsMlpGrad* grad, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Batch evaluation of an MLP whose output layer has ANY width, and its backward into the parameters:
 * FiniteHorizonFullPolicy.pi (gops/apprfunc/mlp.py:114-145: obs -> hidden ... -> act_dim * pre_horizon, the single
 * evaluation of FHADP2, gops/algorithm/fhadp2.py:100-104) and `pre.backward(grad)` (:89).  y, grad_y: [batch, sizes[n_layers]]
 * row-major.  The hidden stack runs on the rollout kernels (GOPS_ENV_NONE tiles), the output layer on its own kernels;
 * mlp->dtype must be GOPS_DTYPE_F32. */
size_t gops_mlp_workspace_bytes(const GopsMlp* mlp, int32_t batch);
int gops_mlp_forward(const GopsMlp* mlp, int32_t batch, const float* x, float* y, void* workspace,
                     size_t workspace_bytes, void* stream);
int gops_mlp_backward(const GopsMlp* mlp, int32_t batch, const float* x, const float* grad_y,
                      const GopsMlpGrad* grad, void* workspace, size_t workspace_bytes, void* stream);
/* gops_mlp_backward that also returns d(loss)/d(x) [batch, sizes[0]] (ABI v5); `grad` may be NULL when only the input
 * adjoint is wanted: `q1(o, policy(o))` differentiated with respect to the action with frozen q parameters
 * (gops/algorithm/mpg.py:186-191,338) and the policy evaluated at the rollout's last observation (:352-354). */
int gops_mlp_backward_x(const GopsMlp* mlp, int32_t batch, const float* x, const float* grad_y,
                        const GopsMlpGrad* grad, float* grad_x, void* workspace, size_t workspace_bytes,
                        void* stream);

/* One Adam step (torch.optim.Adam defaults semantics: no weight decay, no amsgrad) over up to
 * GOPS_ADAM_MAX_TENSORS parameter tensors in ONE launch - replaces `self.networks.policy_optimizer.step()`
 * (gops/algorithm/fhadp.py:89, gops/algorithm/infadp.py:124).  The learning rate and the step count
 * live in DEVICE memory (`GopsAdamState`, caller-owned; initialise step = updates done so far,
 * beta1_pow = beta1^step, beta2_pow = beta2^step, ticket = 0): the kernel uses t = step + 1 for the
 * bias corrections and its last block stores the advanced state, so the call can be captured in a
 * HIP graph and replayed.  exp_avg / exp_avg_sq are updated in place.  Every gradient element is
 * multiplied by `grad_scale` as it is read (1/N after a SUM all-reduce over N data-parallel replicas:
 * the averaging costs no extra pass over the gradient buffer; set it to 1 otherwise). */
#define GOPS_ADAM_MAX_TENSORS 16
typedef struct GopsAdamTensors {
    int32_t n;
    int32_t reserved;
    int64_t numel[GOPS_ADAM_MAX_TENSORS];
    float* param[GOPS_ADAM_MAX_TENSORS];
    const float* grad[GOPS_ADAM_MAX_TENSORS];
    float* exp_avg[GOPS_ADAM_MAX_TENSORS];
    float* exp_avg_sq[GOPS_ADAM_MAX_TENSORS];
} GopsAdamTensors;
typedef struct GopsAdamState {   /* 48 bytes of device memory */
    double lr;
    int64_t step;
    double beta1_pow, beta2_pow;
    uint32_t ticket;
    uint32_t skipped_nonfinite;   /* ABI v13 (was `reserved`): gradient elements that were NOT finite and therefore took no step (parameter,
                                   * moments and - in a fused tail - Polyak target untouched), cumulative; the caller reads / clears it */
    double grad_scale;
} GopsAdamState;
int gops_adam_step(const GopsAdamTensors* tensors, GopsAdamState* state_dev, double beta1, double beta2,
                   double eps, void* stream);

/* ABI v12.  A single-process update - compute_gradient, then optimizer.step() (gops/algorithm/fhadp.py:87-90, infadp.py:101-104) - in
 * ONE call: gops_rollout_backward with what follows it folded into its last kernel, the split-K reduce that forms the final
 * gradients: the Adam step of gops_adam_step on every gradient element as it is formed (`adam`), and the loss mean of
 * gops_mean_loss in one more block of the same launch (`mean_x`; more than 8192 values: its own launch, still inside this call).
 * Element for element the arithmetic of the three separate calls (tests: bit-equal weights, moments and loss scalars); two
 * launches and their gaps less per update.  The gradients are written to policy_grad as well.  With GOPS_VF_BWD_PHASE_A only a tail
 * WITHOUT `adam` / `polyak` is accepted (round 6: the loss mean rides on phase A's reduce launch; a data-parallel update all-reduces
 * between gradient and optimizer step), never with GOPS_VF_BWD_PHASE_B, and not for open-loop rollouts. */
typedef struct GopsUpdateTail {
    const GopsAdamTensors* adam;   /* NULL: no optimizer step.  grad[i] must be one of policy_grad's tensors with numel[i] its element
                                    * count, and EVERY tensor of policy_grad must appear (a parameter without its step is a bug) */
    GopsAdamState* adam_state;     /* device memory, as for gops_adam_step */
    double beta1, beta2, eps;
    const float* mean_x;           /* NULL: no loss mean; else mean_n device values (the forward's v_pi) */
    int32_t mean_n;
    int32_t reserved;
    double mean_scale;             /* mean_stats[0] = mean_scale * mean(x), mean_stats[1] = mean(x) */
    float* mean_stats;             /* GOPS_LOSS_STATS_FLOATS floats, as for gops_mean_loss */
    const GopsAdamTensors* polyak; /* NULL: no target-network averaging; else the table of gops_polyak_update (param[i] = target tensor,
                                    * grad[i] = online tensor) for the network `adam` steps: every online tensor must be one of adam's
                                    * param[] - the target element is averaged with the NEW parameter value right where Adam forms it
                                    * (infadp.py:124-133 after :104), same two roundings as gops_polyak_update.  Needs `adam` */
    double polyak_tau;
} GopsUpdateTail;
int gops_rollout_backward_update(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                                 const GopsMlpGrad* policy_grad, const GopsUpdateTail* tail,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The same for a value / MLP batch: gops_value_backward with the tail (INFADP's policy-evaluation update: Adam step of the value
 * net + Polyak step of its target in the launch that forms the gradients; tail->mean_x is usually NULL there - gops_value_loss
 * has to run BEFORE the backward, it produces grad_v). */
int gops_value_backward_update(const GopsMlp* value, int32_t batch, const float* obs, const float* grad_v,
                               const GopsMlpGrad* grad, const GopsUpdateTail* tail,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ABI v11.  Polyak averaging of a target network, every tensor in one launch - replaces the two passes of
 * gops/algorithm/infadp.py:124-133 (`p_targ.mul_(1 - tau); p_targ.add_(tau * p)`), same roundings per element.
 * Table: param[i] = target tensor i (updated in place), grad[i] = online tensor i, numel[i]; the moment slots are ignored. */
int gops_polyak_update(const GopsAdamTensors* tensors, double tau, void* stream);

/* ABI v11.  The scalars (and the loss gradient) the algorithms form from a batch of values, one launch, no host sync:
 *   gops_value_loss:  stats[0] = mean((v - target)^2), stats[1] = mean(v), grad[i] = (2 / n) (v[i] - target[i]) (grad may be NULL)
 *                     - `loss_v = ((v - backup) ** 2).mean()` and `torch.mean(v)` of gops/algorithm/infadp.py:172-173 and
 *                     d(loss_v) / d(v);
 *   gops_mean_loss:   stats[0] = scale * mean(x), stats[1] = mean(x) - `-v_pi.mean()` (infadp.py:213, fhadp.py:123) with scale = -1.
 * `stats` is 8-byte aligned device memory of GOPS_LOSS_STATS_FLOATS floats, ALL ZERO before the first call: behind the two
 * results it holds the blocks' partial sums and a ticket counter that every call leaves zero again; sums are formed in double
 * in a fixed order (run-to-run reproducible). */
#define GOPS_LOSS_STATS_FLOATS 260
int gops_value_loss(const float* v, const float* target, int32_t n, float* grad, float* stats, void* stream);
int gops_mean_loss(const float* x, int32_t n, double scale, float* stats, void* stream);

/* ABI v15.  POLY approximators (gops/apprfunc/poly.py: DetermPolicy, FiniteHorizonPolicy, StateValue) on the model rollout, one lane per
 * trajectory (csrc/rollout_poly.hip).  A POLY net is a GopsMlp with n_layers = 1 (which the MLP entry points reject):
 *   sizes[0] = obs_dim, sizes[1] = out width (act_dim for a policy, 1 for a value), sizes[2] = columns of weight[0] (F, plus 1 for a
 *   FiniteHorizonPolicy; checked against desc->finite_horizon: GOPS_ERR_BAD_ARG otherwise), hidden_act = GOPS_POLY_*,
 *   weight[0] = [out][F (+1)] row-major (+1: FiniteHorizonPolicy's virtual_t = step + 1 column AFTER the features; the rollout
 *   takes it when desc->finite_horizon = 1), bias[0] = [out] or NULL (add_bias), weight[1] = norm_matrix [obs_dim] or NULL (value only);
 *   GopsMlpGrad.weight[0] / bias[0] likewise.
 * No tanh squash: the raw linear output goes into ScaleAction / ClipAction.  The rollout is that of gops_rollout_forward / _backward for
 * GOPS_ENV_LQ (obs_dim <= 6), _IDPENDULUM, _CARTPOLE, _PENDULUM and _MOUNTAINCAR with every wrapper those take (MaskAtDone or none, ClipObservation,
 * ShapingReward, ScaleObservation, ActionRepeat); policy degree 1 or 2 for every obs_dim, degree 3 for obs_dim <= 3; the tail value
 * (tail_value, tail_unmasked) must be a GOPS_POLY_SYM_2 net.  fp32 only (GOPS_DTYPE_F16 refused), closed loop only, variant_flags 0.
 * Anything else - an MLP policy or value in the description, another env kind - returns GOPS_ERR_UNSUPPORTED.
 * The weight gradient is summed over trajectories in a fixed order (per-block partial rows, then one reduce launch): bitwise
 * reproducible run to run. */
size_t gops_poly_rollout_workspace_bytes(const GopsRolloutDesc* desc);
int gops_poly_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int gops_poly_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                               const GopsMlpGrad* policy_grad, void* workspace, size_t workspace_bytes, void* stream);
/* POLY StateValue (GOPS_POLY_SYM_2) over a batch: v [batch] = V(obs [batch, obs_dim]) and its backward into the parameters
 * (INFADP's policy evaluation; gops_value_loss / gops_adam_step / gops_polyak_update take the tensors as they are). */
size_t gops_poly_value_workspace_bytes(const GopsMlp* value, int32_t batch);
int gops_poly_value_forward(const GopsMlp* value, int32_t batch, const float* obs, float* v, void* stream);
int gops_poly_value_backward(const GopsMlp* value, int32_t batch, const float* obs, const float* grad_v,
                             const GopsMlpGrad* grad, void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15).  GAUSS approximators (gops/apprfunc/gauss.py: DetermPolicy,
 * FiniteHorizonPolicy over radial basis functions) on the model rollout, one lane per trajectory (csrc/rollout_rbf.hip).  An RBF net is
 * a GopsMlp with n_layers = 1 and hidden_act = GOPS_RBF_* (the MLP and POLY entry points reject it):
 *   sizes = (in_dim, out_dim, K): in_dim = obs_dim for GOPS_RBF_AFFINE, obs_dim + 1 for GOPS_RBF_TANH (the virtual time is the LAST
 *   input; checked with the head against desc->finite_horizon: GOPS_ERR_BAD_ARG otherwise), out_dim = act_dim, 1 <= K <= 64;
 *   weight[0] = w [out][K], bias[0] = b [out], weight[1] = C [K][in_dim], bias[1] = sigma_square [K], all required;
 *   GopsMlpGrad uses the same four slots, all required.
 *   phi_k = exp(-|x - C_k|^2 / (2 |sigma_square_k|)), y = w phi + b; the head's limits are GopsEnv.policy_low / policy_high.
 * Env models, wrappers and the other limits are those of gops_poly_rollout_*: fp32, closed loop, variant_flags 0.  desc->tail_value
 * must be 0 (GOPS_ERR_UNSUPPORTED): a caller composes a terminal value from GopsRolloutOut.final_obs / final_done and hands its
 * adjoint back as adj->grad_final_obs.  `adj` may be NULL; grad_final_obs and grad_obs are honoured, first_step_only must be 0
 * (GOPS_ERR_UNSUPPORTED).  The backward is three launches - the sweep (adjoints of the observations, g_y of every
 * step), the parameter gradient as a sum over the horizon * batch samples, the fixed-order sum of its per-block rows: bitwise
 * reproducible run to run. */
size_t gops_rbf_rollout_workspace_bytes(const GopsRolloutDesc* desc);
int gops_rbf_rollout_forward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const GopsRolloutOut* out,
                             void* workspace, size_t workspace_bytes, void* stream);
int gops_rbf_rollout_backward(const GopsRolloutDesc* desc, const GopsRolloutIn* in, const float* grad_v,
                              const GopsMlpGrad* policy_grad, const GopsRolloutAdjoint* adj,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): RPI's policy evaluation (gops/algorithm/rpi.py local_update) as ONE
 * launch of one workgroup, one lane per batch row (csrc/rollout_rpi.hip).  Up to `max_steps` gradient steps on the weights of a
 * POLY StateValue of degree 2 (F = S (S + 1) / 2 weights in create_features order; the bias takes no gradient), each with its env
 * step under the target weights' action / adversary pair, the Hamiltonian loss mean|h| and its gradient, an Adam step, the held-out
 * Hamiltonian norm and the reference's continue test |after| > 0.88 |before|.  Sums are formed in a fixed order: results are bitwise
 * reproducible.
 * The env kinds are an enum of their own: no rollout entry point accepts these models. */
enum { GOPS_RPI_ENV_OSCILLATOR = 1, GOPS_RPI_ENV_AIRCRAFT = 2, GOPS_RPI_ENV_SUSPENSION = 3 };   /* state_dim S = 2, 3, 4 */
#define GOPS_RPI_MAX_BATCH 1024          /* lanes of the one workgroup */
#define GOPS_RPI_MAX_STEPS (1 << 20)
/* `consts`: GOPS_RPI_CONST_COUNT floats in HOST memory, read at the call */
enum {
    GOPS_RPI_C_GAMMA_ATTE = 0, GOPS_RPI_C_DT = 1, GOPS_RPI_C_R = 2,   /* disturbance attenuation, Euler step, control weight */
    GOPS_RPI_C_ACT_LOW = 3, GOPS_RPI_C_ACT_HIGH = 4, GOPS_RPI_C_ADV_LOW = 5, GOPS_RPI_C_ADV_HIGH = 6,   /* the model's action / adversary bounds */
    GOPS_RPI_C_SCALE_ACT_LOW = 7, GOPS_RPI_C_SCALE_ACT_HIGH = 8, GOPS_RPI_C_SCALE_ADV_LOW = 9, GOPS_RPI_C_SCALE_ADV_HIGH = 10,   /* ScaleAction's min_action / max_action per column */
    GOPS_RPI_C_ACTION_SCALE = 11, GOPS_RPI_C_CLIP_ACTION = 12,   /* wrapper switches, 0 or 1 (they act on the Hamiltonian's pair only) */
    GOPS_RPI_C_Q = 13,           /* [4] diagonal of the state weight */
    GOPS_RPI_C_THRESHOLD = 17,   /* [4] |x_i| beyond which a lane is done */
    GOPS_RPI_C_NORM = 21,        /* [4] the value net's norm_matrix */
    GOPS_RPI_CONST_COUNT = 32
};
/* The state block (device memory, persists from call to call, written by the caller before the first one), in floats:
 *   [0, 10) Adam exp_avg, [10, 20) exp_avg_sq, [20] Adam step count (a float: exact to 2^24 steps, where it stops advancing -
 *   the bias corrections it feeds are exactly 1 long before), up to GOPS_RPI_STATE_HEADER reserved (zero);
 *   then x [S][batch] (lane states, column-major), count [batch] (steps since construction: the counter the time-limit test reads),
 *   shown [batch] (the counter the algorithm assigns at a reset; -1 = not assigned yet).
 * gops_rpi_state_bytes: its size; 0 for an unknown env kind or batch outside 1 .. GOPS_RPI_MAX_BATCH. */
#define GOPS_RPI_STATE_HEADER 32
size_t gops_rpi_state_bytes(int32_t env_kind, int32_t batch);
/* weights [F] (device, stepped in place), target_weights [F], max_step [batch] (time limit per lane),
 * reset_pool [max_steps + 1][S][batch] (entry 0: the held-out set; entry 1 + i: the reset draw of step i),
 * result [4] (device): steps taken, last loss, norm_before, norm_after; trace [max_steps][2] (loss, norm_after per step) or NULL.
 * batch > GOPS_RPI_MAX_BATCH or an unknown env kind: GOPS_ERR_UNSUPPORTED, nothing is launched; max_steps outside
 * 1 .. GOPS_RPI_MAX_STEPS or a NULL pointer: GOPS_ERR_BAD_ARG; state_bytes too small: GOPS_ERR_WORKSPACE. */
int gops_rpi_evaluate(int32_t env_kind, int32_t batch, int32_t max_steps, const float* consts, float* weights,
                      const float* target_weights, const float* max_step, const float* reset_pool, void* state, size_t state_bytes,
                      double lr, double beta1, double beta2, double eps, float* result, float* trace, void* stream);

/* ABI v15, additive entry points (the version number stays 15): the same policy evaluation for an MLP value net
 * (csrc/rollout_rpi_mlp.hip), again ONE launch of one workgroup; batch rows are processed in tiles of 64.  `value` and `target`
 * describe nets of the same shape: S -> H1 [-> H2] -> 1 with a linear output, one or two hidden layers, widths multiples of 16 and at
 * most 64, hidden_act GOPS_ACT_ELU / _GELU / _TANH / _SIGMOID, GOPS_DTYPE_F32, sizes[0] = the model's state dimension.  Per step:
 * dV/dx of the TARGET net by a reverse pass (action / adversary pair), the value net's forward pass with a tangent along f
 * (h = U + dV/dx . f), the reverse pass over it seeded with sign(h) / batch, an Adam step on every weight and hidden bias (the
 * output bias has no gradient), the held-out norm, the 0.88 test.  All products are fp32 fmaf chains; sums have a fixed order:
 * results are bitwise reproducible.  The weights and hidden biases are stepped IN PLACE through the pointers of `value`.
 * The state block, in floats (P = parameter count of the net, output bias included):
 *   [0] Adam step count (a float, as above), up to GOPS_RPI_STATE_HEADER reserved (zero);
 *   x [S][batch], count [batch], shown [batch] as for gops_rpi_evaluate;
 *   exp_avg [P], exp_avg_sq [P] in torch's parameters() order (weight then bias of each Linear layer, row-major; the output
 *   bias's slots stay as they are);
 *   scratch [S + 1][batch] (the held-out set's f and U, rewritten by every call).
 * gops_rpi_mlp_state_bytes: its size; 0 for anything unsupported.
 * consts (GOPS_RPI_C_NORM unused), max_step, reset_pool, result and trace as for gops_rpi_evaluate.
 * An unsupported net (also: target of another shape), env kind or batch > GOPS_RPI_MAX_BATCH: GOPS_ERR_UNSUPPORTED, nothing is
 * launched; max_steps outside 1 .. GOPS_RPI_MAX_STEPS, batch < 1 or a NULL pointer: GOPS_ERR_BAD_ARG; state_bytes too small:
 * GOPS_ERR_WORKSPACE. */
size_t gops_rpi_mlp_state_bytes(int32_t env_kind, int32_t batch, const GopsMlp* value);
int gops_rpi_mlp_evaluate(int32_t env_kind, int32_t batch, int32_t max_steps, const float* consts, const GopsMlp* value,
                          const GopsMlp* target, const float* max_step, const float* reset_pool, void* state, size_t state_bytes,
                          double lr, double beta1, double beta2, double eps, float* result, float* trace, void* stream);

/* ABI v15, additive entry points (the version number stays 15): whole closed-loop EVALUATION episodes in one launch
 * (csrc/rollout_episode.hip) - the loop of Evaluator.run_an_episode (gops/trainer/evaluator.py:45-86): a_t = policy(obs_t) (a
 * FiniteHorizonPolicy - sizes[0] = obs_dim + 1 - always gets virtual_t = 1, the default the reference evaluator calls it with), the
 * tanh squash / act limits, then one DATA-env step (gops_env_step with GopsEnv.data_env = 1: the same device function), until the
 * first `done` or `max_steps`.  Rewards are the data env's own; env->shaping is honoured as gops_env_step honours it.
 * Episodes run in tiles of GOPS_TILE per workgroup; the MLP contractions are exact fp32 (v_mfma_f32_16x16x4_f32) whatever
 * policy->variant_flags says; weights are read in place from the tensors `policy` points to.  No host sync, no device allocation.
 *   init:  obs [E, obs_dim] and, for the vehicle families, state / ref_points / path_num / u_num / ref_time as gops_env_step takes
 *          them: the per-episode initial condition (read only; every other field is ignored).  The appended reference point is
 *          evaluated in the kernel (strict host points - ref_appended - are out of scope for evaluation).
 *   out:   ret [E] = sum of the rewards up to and including the step that ends the episode (summed in double, rounded once),
 *          length [E] = steps taken, terminated [E] = 1 when `done` ended the episode, 0 when it reached max_steps;
 *          trace_obs [E][max_steps][obs_dim], trace_act [E][max_steps][act_dim] (the policy's output, before ScaleAction /
 *          ClipAction), trace_rew [E][max_steps]: optional (NULL), rows beyond `length` are left untouched.
 * Accepted: GOPS_ENV_LQ, _IDPENDULUM, _CARTPOLE, _VEH3DOFCONTI, _VEH2DOF (without cstr_err) with data_env = 1 and repeat_num <= 1;
 * MLP policies with 2 .. GOPS_MAX_LAYERS layers, hidden widths multiples of 16 (up to ~1100: two activation tiles must fit in LDS),
 * every GOPS_ACT_*, GOPS_DTYPE_F32; weight tensors at any 4-byte alignment (16-byte loads are taken only where the pointer allows).
 * GOPS_ERR_UNSUPPORTED: any other env kind (mobilerobot draws noise per step, the constrained
 * vehicle models, GOPS_ENV_PENDULUM and _MOUNTAINCAR have no data-env restatement), POLY nets (n_layers = 1), GOPS_DTYPE_F16.  GOPS_ERR_BAD_ARG:
 * data_env = 0, shapes that do not match the env kind, NULL pointers.  GOPS_ERR_WORKSPACE: workspace_bytes too small.
 * gops_episode_workspace_bytes: 0 for a description gops_episode_rollout rejects. */
struct GopsEpisodeOut {
    float* ret; int32_t* length; float* terminated;
    float* trace_obs; float* trace_act; float* trace_rew;
};
typedef struct GopsEpisodeOut GopsEpisodeOut;
size_t gops_episode_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t episodes, int32_t max_steps);
int gops_episode_rollout(const GopsEnv* env, const GopsMlp* policy, int32_t episodes, int32_t max_steps, const GopsStepIO* init,
                         const GopsEpisodeOut* out, void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): a whole sample() of the device samplers in one launch
 * (csrc/rollout_sample.hip) - `steps` = T times the loop body of DeviceEnvSampler._step_once for `n_envs` = N environment
 * instances: policy, exploration head, one env step (gops_env_step's own device function), the stored transition row, episode
 * bookkeeping and the re-seeding of finished instances.  Instances run in tiles of GOPS_TILE per workgroup, the MLP contractions
 * are exact fp32 (v_mfma_f32_16x16x4_f32) as in gops_episode_rollout; weights are read in place.  No host sync, no device
 * allocation, no atomics; no workgroup reads what another wrote, so a row does not depend on the tiling.
 *   desc->head, with y the policy's raw output, eps = noise[t][i] and (lo, hi) = env->policy_low / policy_high:
 *     GOPS_SAMPLE_DETERM      y [A]:   act = (hi - lo) / 2 tanh(y) + (hi + lo) / 2 + noise_std eps, logp = 0;
 *     GOPS_SAMPLE_GAUSS       y [2A] = (mean, raw log std): ls = clamp(raw, min_log_std, max_log_std), act = mean + exp(ls) eps,
 *                             logp = sum_a(-eps_a^2 / 2 - ls_a - log sqrt(2 pi));
 *     GOPS_SAMPLE_TANH_GAUSS  u as for GAUSS, act = (hi - lo) / 2 tanh(u) + (hi + lo) / 2, logp = the Gaussian's at u
 *                             - sum_a log(1 + 1e-6 - tanh(u_a)^2) - sum_a log((hi_a - lo_a) / 2)  (TanhGaussDistribution).
 *     Every head is formed in double and rounded once per stored value.
 *   noise: [T, N, A] standard normals - the kernel draws nothing: a launch is a pure function of its inputs.
 *   state (read AND written): obs [N, obs_dim]; for the vehicle families state / ref_points / path_num / u_num / ref_time as
 *     gops_env_step takes them; t [N] int32 steps into the running episode; reset_count [N] int32 resets since the pool was drawn.
 *   pool: desc->pool_rows = R reset states per instance, [R, N, ...] for obs and each info tensor (read only).
 *   Per step: the row of (obs_t, info_t) is stored, the head gives act_t / logp_t, the env step gives rew, done, obs2 and the
 *     next_* info; t_i += 1; over = done != 0 || t_i >= max_episode_steps.  Where `over`, instance i continues from pool row
 *     [reset_count[i] % R][i], reset_count[i] += 1 and t_i = 0; else from (obs2, next info).  The rule needs nothing from another
 *     instance; an instance that resets more than R times between refreshes of the pool revisits its rows (defined behaviour).
 *   out, time-major [T, N, ...], a tile's rows contiguous: obs, act, rew, done, obs2, logp; each info tensor and its next_ twin
 *     (vehicle families; ignored otherwise); time_limited = over && done == 0; end = over, 1 at t = T - 1.
 * Accepted: GOPS_ENV_LQ, _IDPENDULUM, _CARTPOLE, _VEH3DOFCONTI, _VEH2DOF (without cstr_err) with data_env = 1; GOPS_ENV_PENDULUM and
 * _MOUNTAINCAR with data_env = 0 (they have no data-env restatement); repeat_num <= 1; MLP policies as gops_episode_rollout accepts
 * them, sizes[0] = obs_dim, out_dim = A (DETERM) or 2A (the Gaussian heads), A <= GOPS_MAX_ACT, GOPS_DTYPE_F32.
 * GOPS_ERR_UNSUPPORTED, nothing launched: any other env kind or data_env value (mobilerobot draws obstacle noise per step, the
 * constrained vehicle models), POLY nets (n_layers = 1), time-augmented policies (sizes[0] = obs_dim + 1), GOPS_DTYPE_F16, hidden
 * widths outside the episode kernel's.  GOPS_ERR_BAD_ARG: NULL pointers, steps < 1, n_envs < 1, pool_rows < 1,
 * max_episode_steps < 1, an unknown head, an output width that is not the head's (an odd one for the Gaussian heads), shapes that
 * do not match the env kind.  GOPS_ERR_WORKSPACE: workspace_bytes < GOPS_SAMPLE_WORKSPACE_BYTES (the kernel stages nothing there:
 * the outputs are its step buffers; the section is reserved so that a later kernel may).
 * gops_sample_workspace_bytes: 0 for a description gops_sample_rollout rejects. */
#define GOPS_SAMPLE_DETERM 0
#define GOPS_SAMPLE_GAUSS 1
#define GOPS_SAMPLE_TANH_GAUSS 2
#define GOPS_SAMPLE_WORKSPACE_BYTES 256
struct GopsSampleDesc {
    int32_t head, max_episode_steps, pool_rows, reserved;
    double noise_std, min_log_std, max_log_std;
};
typedef struct GopsSampleDesc GopsSampleDesc;
struct GopsSampleState {
    float* obs; float* state; float* ref_points; float* path_num; float* u_num; float* ref_time;
    int32_t* t; int32_t* reset_count;
};
typedef struct GopsSampleState GopsSampleState;
struct GopsSamplePool {
    const float* obs; const float* state; const float* ref_points; const float* path_num; const float* u_num; const float* ref_time;
};
typedef struct GopsSamplePool GopsSamplePool;
struct GopsSampleOut {
    float* obs; float* act; float* rew; float* done; float* obs2; float* logp; float* time_limited; float* end;
    float* state; float* next_state; float* ref_points; float* next_ref_points; float* path_num; float* next_path_num;
    float* u_num; float* next_u_num; float* ref_time; float* next_ref_time;
};
typedef struct GopsSampleOut GopsSampleOut;
size_t gops_sample_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t n_envs, int32_t steps);
int gops_sample_rollout(const GopsEnv* env, const GopsMlp* policy, const GopsSampleDesc* desc, int32_t n_envs, int32_t steps,
                        const GopsSampleState* state, const GopsSamplePool* pool, const float* noise, const GopsSampleOut* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): the same launch with a DISCRETE action set (DQN, discrete TRPO) -
 * gops_sample_rollout_dis takes what gops_sample_rollout takes, plus `dis`; state, pool, out, the per-step books and the resets are
 * gops_sample_rollout's, word for word (one kernel body).  desc->head, noise_std, min_log_std and max_log_std are ignored.
 *   dis->action_table [act_num, A], device memory, row-major (read only): the action the env is stepped with for each index;
 *   dis->act_num = n, 2 .. GOPS_DQN_MAX_ACTIONS; the policy's output width must be n;
 *   dis->env_act [T, N, A] (required output): the table row applied at each step, env_act[t][i] = action_table[index] bit for bit;
 *   out->act is [T, N, 1] here: the chosen index as a float (what the samplers store for a discrete action);
 *   noise: [T, N, 2] UNIFORMS in [0, 1), (u0, u1) per row - the kernel still draws nothing: a launch is a pure function of its inputs.
 *   dis->head, with y [n] the policy's raw outputs (fp32, bias added in fp32) and greedy = the LOWEST index attaining max y - a NaN
 *   counts as the maximum, the first one wins: gops_dqn_backup's a_star rule, torch.argmax's on finite values:
 *     GOPS_SAMPLE_EPS_GREEDY   y = action values: explore = (double)u0 < epsilon, uniform = min((int)((double)u1 * n), n - 1),
 *                              index = explore ? uniform : greedy, logp = 0;
 *     GOPS_SAMPLE_CATEGORICAL  y = logits, formed in double: m = y[greedy], z_k = exp(y_k - m), S = z_0 + .. + z_{n-1} in index
 *                              order; index = the smallest k with u0 * S < z_0 + .. + z_k, else n - 1;
 *                              logp = (y_index - m) - log S, rounded once (the log-softmax at the index); epsilon must be 0.
 *     No tanh squash, no act limits: the env lane steps with env_act as gops_env_step's `action`.
 * Accepted: the env kinds and policies of gops_sample_rollout with sizes[n_layers] = n.  GOPS_ERR_UNSUPPORTED, nothing launched:
 * act_num outside 2 .. GOPS_DQN_MAX_ACTIONS and whatever gops_sample_rollout returns it for.  GOPS_ERR_BAD_ARG, nothing launched: a
 * NULL action_table or env_act, an unknown head (the continuous heads included), an output width other than act_num, epsilon
 * outside [0, 1] (a NaN included), a nonzero epsilon with GOPS_SAMPLE_CATEGORICAL, and gops_sample_rollout's own cases.
 * GOPS_ERR_WORKSPACE as for gops_sample_rollout.  gops_sample_rollout itself keeps rejecting every head above
 * GOPS_SAMPLE_TANH_GAUSS.  gops_sample_dis_workspace_bytes: 0 for a description gops_sample_rollout_dis rejects. */
#define GOPS_SAMPLE_EPS_GREEDY 3
#define GOPS_SAMPLE_CATEGORICAL 4
struct GopsSampleDis {
    const float* action_table;
    int32_t act_num, head;
    double epsilon;
    float* env_act;
};
typedef struct GopsSampleDis GopsSampleDis;
size_t gops_sample_dis_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t act_num, int32_t n_envs, int32_t steps);
int gops_sample_rollout_dis(const GopsEnv* env, const GopsMlp* policy, const GopsSampleDesc* desc, const GopsSampleDis* dis,
                            int32_t n_envs, int32_t steps, const GopsSampleState* state, const GopsSamplePool* pool, const float* noise,
                            const GopsSampleOut* out, void* workspace, size_t workspace_bytes, void* stream);

/* The greedy head of the evaluator over a DISCRETE action set: gops_episode_rollout with a_t = action_table[greedy(y)], y [act_num]
 * the policy's raw outputs and `greedy` as above - the mode() of ValueDiracDistribution (an ActionValueDis' values) and of
 * CategoricalDistribution (a StochaPolicyDis' logits), which the reference evaluator acts with.  No tanh squash, no act limits.
 * action_table [act_num, A] in device memory (read only); trace_act is [E][max_steps][1]: the index as a float.  Everything else -
 * init, out, the env kinds, the policies (sizes[n_layers] = act_num), the workspace - as gops_episode_rollout.
 * GOPS_ERR_UNSUPPORTED: act_num outside 2 .. GOPS_DQN_MAX_ACTIONS and gops_episode_rollout's cases; GOPS_ERR_BAD_ARG: a NULL
 * action_table, an output width other than act_num and gops_episode_rollout's cases.  Nothing is launched on a refusal.
 * gops_episode_dis_workspace_bytes: 0 for a description gops_episode_rollout_dis rejects. */
size_t gops_episode_dis_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t act_num, int32_t episodes, int32_t max_steps);
int gops_episode_rollout_dis(const GopsEnv* env, const GopsMlp* policy, const float* action_table, int32_t act_num, int32_t episodes,
                             int32_t max_steps, const GopsStepIO* init, const GopsEpisodeOut* out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): the evaluator over a STOCHASTIC policy - gops_episode_rollout with
 * a_t = the mode() of the policy's action distribution.  The policy stack has output width 2A, y = (mean [A], raw log std [A]) as
 * gops_sample_rollout's Gaussian heads take it; the action is formed from the mean half alone (the log-std rows are part of the
 * stack and of no dot product), with (lo, hi) = env->policy_low / policy_high as for gops_episode_rollout's squash:
 *     GOPS_SAMPLE_GAUSS       a = clamp(mean, lo, hi)                          (GaussDistribution.mode; a NaN mean stays a NaN)
 *     GOPS_SAMPLE_TANH_GAUSS  a = (hi - lo) / 2 tanh(mean) + (hi + lo) / 2     (TanhGaussDistribution.mode)
 * in fp32.  trace_act is [E][max_steps][A]: that action.  Everything else - init, out, the env kinds, the data-env step, the books,
 * the workspace, one kernel body - as gops_episode_rollout.  GOPS_ERR_BAD_ARG, nothing launched: any other head, an output width
 * other than 2A (A and odd widths included) and gops_episode_rollout's cases; GOPS_ERR_UNSUPPORTED and GOPS_ERR_WORKSPACE as for
 * gops_episode_rollout (the workspace is tested after everything else).  gops_episode_rollout itself keeps refusing a 2A-wide stack.
 * gops_episode_mode_workspace_bytes: 0 for a description gops_episode_rollout_mode rejects. */
size_t gops_episode_mode_workspace_bytes(const GopsEnv* env, const GopsMlp* policy, int32_t head, int32_t episodes, int32_t max_steps);
int gops_episode_rollout_mode(const GopsEnv* env, const GopsMlp* policy, int32_t head, int32_t episodes, int32_t max_steps,
                              const GopsStepIO* init, const GopsEpisodeOut* out, void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): LipsNet policies (gops/apprfunc/lipsnet.py DetermPolicy) - an MLP f
 * evaluated together with its input Jacobian J = df/dx and differentiated through it (csrc/rollout_lips.hip):
 *     y = K(x) f(x) / (||J||_F + eps),   action = y   or, with `squash`,   (high - low) / 2 tanh(y) + (high + low) / 2,
 * K(x) = softplus(*k_scalar) (global: k_net.n_layers = 0) or softplus(k_net(x)) (local: a tanh MLP obs -> 1, hidden_act GOPS_ACT_TANH).
 * A sample is 1 + obs_dim rows through the layers of f (the primal row and the obs_dim tangent columns); the backward walks them
 * back with the second derivative of the activation on the primal delta.  fp32 fmaf arithmetic throughout; weight gradients are
 * per-slab partials summed in a fixed order: results are bitwise reproducible.  softplus has torch's threshold of 20; relu'(0) = 0.
 * Bounds (GOPS_ERR_UNSUPPORTED outside): obs_dim <= 8, act_dim <= GOPS_MAX_ACT, 1..3 hidden layers in `mlp`, `k_net` global or 1..2
 * hidden layers, hidden widths multiples of 16 up to 256, hidden_act GOPS_ACT_RELU .. GOPS_ACT_TANH, GOPS_DTYPE_F32, variant_flags 0.
 * Hidden-layer weight tensors must be 16-byte aligned (GOPS_ERR_BAD_ARG).
 *   gops_lips_forward:  obs [B, obs_dim] -> action [B, act_dim]; K [B] and N [B] (= ||J||_F) are optional outputs (NULL).  Keeps the
 *                       stash of the backward in `workspace`.
 *   gops_lips_backward: grad_action [B, act_dim] -> the gradient of every tensor of `mlp` and of `k_net` / `k_scalar` (overwritten),
 *                       after a forward call with the same description, batch, obs and workspace.  With `training` = 1 the
 *                       gradient of the regular loss lambda mean_b K(x_b)^2 (the reference's backward pre-hook in training mode)
 *                       is part of it: 2 lambda K_b / B on K's adjoint of every row.
 * gops_lips_workspace_bytes: 0 for a description the entry points reject. */
struct GopsLipsNet {
    GopsMlp mlp;                 /* f: sizes = obs_dim, hidden..., act_dim */
    GopsMlp k_net;               /* local K; n_layers = 0: global K */
    const float* k_scalar;       /* global K: device pointer to the scalar parameter */
    float eps, lambda;
    int32_t training;
    int32_t squash;
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];   /* the squash bounds (act_low_lim / act_high_lim buffers) */
};
typedef struct GopsLipsNet GopsLipsNet;
struct GopsLipsGrad {
    GopsMlpGrad mlp;
    GopsMlpGrad k_net;
    float* k_scalar;
};
typedef struct GopsLipsGrad GopsLipsGrad;
size_t gops_lips_workspace_bytes(const GopsLipsNet* net, int32_t batch);
int gops_lips_forward(const GopsLipsNet* net, int32_t batch, const float* obs, float* action, float* K, float* N,
                      void* workspace, size_t workspace_bytes, void* stream);
int gops_lips_backward(const GopsLipsNet* net, int32_t batch, const float* obs, const float* grad_action, const GopsLipsGrad* grad,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ABI v15, additive entry points (the version number stays 15): the no-grad half of a DDPG / TD3 update (csrc/actor_critic.hip).
 *
 * gops_ac_backup: the whole Bellman backup of gops/algorithm/ddpg.py:149-151 and td3.py:166-183 in ONE launch, forward only:
 *     a2     = (high - low) / 2 tanh(policy(obs2)) + (high + low) / 2          (DetermPolicy.forward, squash_low / squash_high)
 *     a2     = clamp(a2 + clamp(xi * target_noise, -noise_clip, noise_clip), act_low, act_high)      (`smooth` = 1: TD3)
 *     q_targ = q[i]([obs2, a2]),  i < n_q;   n_q = 2 takes the minimum                (the concatenation exists in LDS only)
 *     backup = rew * reward_scale + gamma * (1 - done) * q_targ
 * `policy` / `q[i]` are the TARGET networks; xi [B, act_dim] are unit-normal draws supplied by the caller (read iff `smooth`).
 * A workgroup of 256 threads owns a tile of 16, 32 or 64 batch rows (by batch size and LDS plan); the three networks are
 * evaluated one after the other on that tile, weights staged through LDS in chunks of output features, every output eight fp32 fmaf
 * chains (input k in chain k mod 8, k ascending) added pairwise with the bias added last; the output layers, the squash, the clamps,
 * the minimum and the backup are formed in double (the hyper-parameters are doubles, as Python holds them) and rounded to fp32 once,
 * where a2 - the critics' input -, q_targ and backup are stored: the results are bitwise reproducible and do not depend on
 * the tile size.  Nothing is stashed; no global scratch beyond the one section below.
 * Accepted (gops_ac_backup_workspace_bytes returns 0 otherwise, gops_ac_backup GOPS_ERR_UNSUPPORTED): 1 .. 3 hidden layers per
 * network (n_layers 2 .. 4), hidden widths multiples of 16 up to 256, every GOPS_ACT_*, GOPS_DTYPE_F32, variant_flags 0,
 * act_dim <= GOPS_MAX_ACT, obs_dim + act_dim <= 64; policy: obs_dim -> .. -> act_dim, q[i]: obs_dim + act_dim -> .. -> 1.
 * GOPS_ERR_BAD_ARG: n_q outside 1 .. 2, shapes of the three networks that do not fit together, NULL pointers, batch < 1.
 * The workspace is one 256-byte section (no contents today: the kernel keeps no state in global memory; the argument is part of
 * the call so that a later kernel may stage there without an ABI change); workspace_bytes below it: GOPS_ERR_WORKSPACE.
 * Outputs: backup [B]; a2 [B, act_dim] and q_targ [n_q, B] are optional (NULL). */
struct GopsAcBackup {
    GopsMlp policy;
    GopsMlp q[2];
    int32_t n_q;                 /* 1: DDPG, 2: TD3 (minimum of the two) */
    int32_t smooth;              /* 1: target-policy smoothing (TD3) */
    float squash_low[GOPS_MAX_ACT], squash_high[GOPS_MAX_ACT];   /* the policy's act_low_lim / act_high_lim buffers */
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];         /* the algorithm's action limits: clamp after the noise */
    double target_noise, noise_clip, reward_scale, gamma;
};
typedef struct GopsAcBackup GopsAcBackup;
size_t gops_ac_backup_workspace_bytes(const GopsAcBackup* desc, int32_t batch);
int gops_ac_backup(const GopsAcBackup* desc, int32_t batch, const float* obs2, const float* rew, const float* done,
                   const float* xi, float* backup, float* a2, float* q_targ, void* workspace, size_t workspace_bytes,
                   void* stream);
/* gops_ac_critic_loss: the critic losses of the same update in one launch.  q [n_q, B] (row i: critic i on the batch), backup [B],
 * weight [B] or NULL (prioritized replay's importance weights; NULL = ones):
 *     seed [n_q, B] = (2 / B) weight (q_i - backup)        d(loss_i) / d(q_i), loss_i = mean(weight (q_i - backup)^2)
 *     abs_err [B]   = |q_0 - backup|                       the new priorities (NULL: not wanted)
 *     stats[0] = loss_0, stats[1] = loss_1 (0 for n_q = 1), stats[2] = mean(q_0), stats[3] = loss_0 + loss_1 (fp32 sum)
 * `stats`: 8-byte aligned device memory of GOPS_AC_LOSS_STATS_FLOATS floats, ALL ZERO before the first call (behind the four
 * results: the blocks' partial sums and a ticket the call leaves zero again), as for gops_value_loss; sums in double, in a fixed
 * order that depends on B only.  A `stats` pointer that is not 8-byte aligned: GOPS_ERR_BAD_ARG. */
#define GOPS_AC_LOSS_STATS_FLOATS 392
int gops_ac_critic_loss(const float* q, const float* backup, const float* weight, int32_t n_q, int32_t batch, float* seed,
                        float* abs_err, float* stats, void* stream);

/* ABI v15, additive entry points (the version number stays 15): DSAC-T (gops/algorithm/dsact.py; csrc/actor_critic.hip, csrc/dsact.hip).
 * All fp32, fixed summation order, bitwise reproducible; no kernel waits on another workgroup.
 *
 * gops_soft_backup: the whole no-grad target of dsact.py:237-313 in ONE launch, forward only, nothing stashed.  Per batch row:
 *     (mean, log_std) = policy(obs2)                      the TARGET StochaPolicy's raw stack, 2 * act_dim linear outputs
 *     u      = mean + exp(clamp(log_std, min_log_std, max_log_std)) * eps_next
 *     a2     = half * tanh(u) + mid,   half = (act_high - act_low) / 2,  mid = (act_high + act_low) / 2
 *     logp   = sum_a [Normal(mean, std).log_prob(u) - log(1 + 1e-6 - tanh(u)^2) - log(half)]
 *     (m_i, s_i) = (q[i]([obs2, a2])[0], softplus(q[i]([obs2, a2])[1]))    softplus with torch's threshold of 20; i = 1, 2
 *     q_next = min(m_1, m_2);   q_next_sample = m_1 < m_2 ? m_1 + clamp(z_1, -3, 3) s_1 : m_2 + clamp(z_2, -3, 3) s_2
 *     target_q        = rew + (1 - done) gamma (q_next - alpha logp)
 *     target_q_sample = rew + (1 - done) gamma (q_next_sample - alpha logp)
 * eps_next [B, act_dim] and z_next [2, B] are unit-normal draws supplied by the caller.  alpha: `log_alpha` (a device pointer to one
 * float; the kernel forms exp itself) when it is not NULL, else the double `alpha`.  Tiles, staging and the eight fmaf chains are
 * gops_ac_backup's; the heads, the squash, the log-probability, softplus, the minimum and the targets are formed in double and rounded
 * once where they are stored (a2 - the critics' input - included).  One thread per (row, action dimension) forms that dimension's
 * mean and log std.  Accepted shapes as for gops_ac_backup, with policy: obs_dim -> .. -> 2 * act_dim, q[i]: obs_dim + act_dim -> .. -> 2;
 * the same return codes and the same 256-byte workspace section.
 * Outputs: target_q [B], target_q_sample [B]; optional (NULL): a2 [B, act_dim], logp [B], q_targ [2, B, 2] = (m_i, s_i). */
struct GopsSoftBackup {
    GopsMlp policy;
    GopsMlp q[2];
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];   /* the policy's act_low_lim / act_high_lim buffers */
    double min_log_std, max_log_std, gamma, alpha;
    const float* log_alpha;                                /* device memory, or NULL: use `alpha` */
};
typedef struct GopsSoftBackup GopsSoftBackup;
size_t gops_soft_backup_workspace_bytes(const GopsSoftBackup* desc, int32_t batch);
int gops_soft_backup(const GopsSoftBackup* desc, int32_t batch, const float* obs2, const float* rew, const float* done,
                     const float* eps_next, const float* z_next, float* target_q, float* target_q_sample, float* a2, float* logp,
                     float* q_targ, void* workspace, size_t workspace_bytes, void* stream);
/* gops_dsact_critic_loss: the critic losses of dsact.py:243-251, 284-313 and their gradient seeds.  qraw [2, B, 2]: the ONLINE critics'
 * raw head outputs (q_i, raw_i) on the data, std_i = softplus(raw_i); target_q, target_q_sample [B] from gops_soft_backup.
 *     state->mean_std[i] <- mean(std_i)                                            first call (state->initialised == 0)
 *                           (1 - tau_b) state->mean_std[i] + tau_b mean(std_i)     later calls;   rounded to fp32, then used below
 *     bound_i = q_i + clamp(target_q_sample - q_i, -3 mean_std_i, 3 mean_std_i)
 *     loss_i  = (mean_std_i^2 + 0.1) mean(-(target_q - q_i) / (std_i^2 + 0.1) q_i - ((q_i - bound_i)^2 - std_i^2) / (std_i^3 + 0.1) std_i)
 *     seed [2, B, 2] = d(loss_1 + loss_2) / d(q_i, raw_i): q_i and std_i standing alone are live, every other occurrence is detached
 *                      (the reference's pattern); the raw column carries softplus' derivative sigmoid(raw_i)
 *     stats[0] = loss_1 + loss_2 (fp32 sum), [1], [2] = mean(q_i), [3], [4] = mean(std_i), [5], [6] = min(std_i),
 *     stats[7], [8] = mean_std_i, [9], [10] = loss_i
 * The seeds need the batch mean of std before they can be formed: up to 8192 rows one workgroup does both phases in ONE launch;
 * larger batches take TWO launches of 64 workgroups (moments and state, then seeds and losses).
 * `state`: zero before the first update.  `stats`: 8-byte aligned, GOPS_DSACT_STATS_FLOATS floats, ALL ZERO before the first call
 * (partial sums and a ticket the call leaves zero again, as for gops_ac_critic_loss); otherwise GOPS_ERR_BAD_ARG. */
struct GopsDsactState {
    float mean_std[2];
    uint32_t initialised;
    uint32_t reserved;
};
typedef struct GopsDsactState GopsDsactState;
#define GOPS_DSACT_STATS_FLOATS 800
int gops_dsact_critic_loss(const float* qraw, const float* target_q, const float* target_q_sample, int32_t batch, double tau_b,
                           GopsDsactState* state, float* seed, float* stats, void* stream);
/* gops_tanh_gauss_forward / _backward: StochaPolicy's sampling head (TanhGaussDistribution.rsample) and its reverse.
 * head [B, 2 * act_dim] = (mean, log_std) raw, eps [B, act_dim] unit-normal draws:
 *     act [B, act_dim], logp [B] as a2 / logp of gops_soft_backup;
 *     stats[0] = mean(logp), [1] = mean(tanh(mean)), [2] = mean(std), [3] = -(mean(logp) + target_entropy) = d loss_alpha / d log_alpha
 * backward: g_act [B, act_dim], g_logp [B] -> g_head [B, 2 * act_dim]; the log_std column is zero outside [min_log_std, max_log_std].
 * `stats`: 8-byte aligned, GOPS_TANH_GAUSS_STATS_FLOATS floats, all zero before the first call.  act_dim outside 1 .. GOPS_MAX_ACT,
 * NULL pointers, batch < 1: GOPS_ERR_BAD_ARG. */
struct GopsTanhGauss {
    int32_t act_dim;
    int32_t reserved;
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];
    double min_log_std, max_log_std;
};
typedef struct GopsTanhGauss GopsTanhGauss;
#define GOPS_TANH_GAUSS_STATS_FLOATS 800
int gops_tanh_gauss_forward(const GopsTanhGauss* desc, int32_t batch, const float* head, const float* eps, double target_entropy,
                            float* act, float* logp, float* stats, void* stream);
int gops_tanh_gauss_backward(const GopsTanhGauss* desc, int32_t batch, const float* head, const float* eps, const float* g_act,
                             const float* g_logp, float* g_head, void* stream);

/* ABI v15, additive entry points (the version number stays 15): SAC and DSAC (gops/algorithm/sac.py, dsac.py; csrc/actor_critic.hip,
 * csrc/dsact.hip).
 *
 * gops_soft_q_backup: the whole no-grad target of sac.py:214-223 / dsac.py:199-252 in ONE launch, forward only, nothing stashed.
 * a2 and logp per batch row exactly as in gops_soft_backup (clamp of log_std, u = mean + std eps_next, squash, log-probability), then
 *     distri = 0:  backup = rew + (1 - done) gamma (min_i q[i]([obs2, a2]) - alpha logp)              n_q = 2: SAC; n_q = 1: no minimum
 *     distri = 1:  (m, s) = (q[0](..)[0], softplus(q[0](..)[1]))   softplus with torch's threshold of 20;   n_q = 1: DSAC
 *                  backup = rew + (1 - done) gamma (m + clamp(z_next, -3, 3) s - alpha logp)
 * distri = 1 with n_q = 2 is gops_soft_backup's case: GOPS_ERR_UNSUPPORTED (and 0 workspace bytes).  z_next [B] is read iff `distri`;
 * NULL then: GOPS_ERR_BAD_ARG.  `policy` is whichever policy the algorithm evaluates at obs2 (SAC: the online one).
 * Tiles, staging, chains, doubles and the policy head are gops_soft_backup's; results are bitwise reproducible and do not depend on the
 * tile size.  Accepted shapes as for gops_soft_backup, with q[i]: obs_dim + act_dim -> .. -> 1 (distri = 0) or 2 (distri = 1); the
 * same return codes and the same 256-byte workspace section; n_q outside 1 .. 2 or distri outside 0 .. 1: GOPS_ERR_BAD_ARG.
 * Outputs: backup [B]; optional (NULL): a2 [B, act_dim], logp [B], q_targ - [n_q, B] for distri = 0, [B, 2] = (m, s) for distri = 1. */
struct GopsSoftQBackup {
    GopsMlp policy;              /* obs_dim -> .. -> 2 * act_dim, raw (mean, log_std) */
    GopsMlp q[2];
    int32_t n_q;                 /* 1 or 2 */
    int32_t distri;              /* 0: q[i] -> 1 output (ActionValue); 1: q[i] -> 2 outputs (mean, softplus std) */
    float act_low[GOPS_MAX_ACT], act_high[GOPS_MAX_ACT];
    double min_log_std, max_log_std, gamma, alpha;
    const float* log_alpha;      /* device, or NULL: use alpha */
};
typedef struct GopsSoftQBackup GopsSoftQBackup;
size_t gops_soft_q_backup_workspace_bytes(const GopsSoftQBackup* desc, int32_t batch);
int gops_soft_q_backup(const GopsSoftQBackup* desc, int32_t batch, const float* obs2, const float* rew, const float* done,
                       const float* eps_next, const float* z_next, float* backup, float* a2, float* logp, float* q_targ, void* workspace,
                       size_t workspace_bytes, void* stream);
/* gops_dsac_critic_loss: DSAC's critic loss (dsac.py:235-252) and its gradient seeds.  qraw [B, 2]: the ONLINE critic's raw head on
 * the data, q = qraw[:, 0], sd = softplus(qraw[:, 1]); target_q [B] from gops_soft_q_backup.
 *     td_bound = 3 mean(sd) (rounded to fp32, then used);   target_q_bound = q + clamp(target_q - q, -td_bound, td_bound)
 *     bound != 0:  loss = mean((q - target_q)^2 / (2 sd^2) + (q - target_q_bound)^2 / (2 sd^2) + log sd)
 *                  the first term live in q (its sd detached), the second and third live in sd (their q detached)
 *     bound == 0:  loss = mean(-Normal(q, sd).log_prob(target_q)), live in both
 *     seed [B, 2] = d loss / d(q, raw); the raw column carries softplus' derivative sigmoid(raw)
 *     stats[0] = loss, [1] = mean(q), [2] = mean(sd), [3] = td_bound
 * Up to 8192 rows one workgroup in ONE launch; larger batches TWO launches of 64 workgroups (moments, then seeds and loss).
 * `stats`: 8-byte aligned, GOPS_DSAC_STATS_FLOATS floats, ALL ZERO before the first call (partial sums and a ticket the call leaves
 * zero again); otherwise, and for NULL pointers or batch < 1, GOPS_ERR_BAD_ARG. */
#define GOPS_DSAC_STATS_FLOATS 264
int gops_dsac_critic_loss(const float* qraw, const float* target_q, int32_t batch, int32_t bound, float* seed, float* stats,
                          void* stream);

/* ABI v15, additive entry points (the version number stays 15): PPO (gops/algorithm/ppo.py, gops/trainer/sampler/on_sampler.py;
 * csrc/ppo.hip).  fp32 in and out, arithmetic in double, one rounding per stored value, sums in the fixed order of the batch size.
 *
 * gops_ppo_loss: the losses of ppo.py:167-240 and their gradient seeds for one minibatch of `batch` = M rows, A = act_dim.
 *   head_new [M, 2A]: the ONLINE StochaPolicy's RAW stack output (mean, log_std); ls = clamp(log_std, min_log_std, max_log_std),
 *   std = exp(ls) are formed here.  v_new [M], act [M, A], logp_old [M], adv [M], ret [M], val_old [M];
 *   logits_old [M, 2A] = (mean_old, std_old) as policy(obs) returned them before the update.
 *   hyper (device, 5 floats): clip, value_clip, c_kl, c_v, c_ent - read by the kernel, so a schedule may change them under a graph.
 *     logp_new = sum_a (-(act - mean)^2 / (2 std^2) - ls - log sqrt(2 pi));   ratio = exp(logp_new - logp_old)
 *     sur      = min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv)
 *     l1 = (v_new - ret)^2;  vc = val_old + clamp(v_new - val_old, -value_clip, value_clip);  l2 = (vc - ret)^2
 *     value_loss = loss_value_clip ? max(l1, l2) : l1
 *     entropy  = sum_a (0.5 + log sqrt(2 pi) + ls)
 *     kl       = sum_a (ls - log std_old + (std_old^2 + (mean_old - mean)^2) / (2 std^2) - 0.5)          KL(N(old) || N(new))
 *     loss_surrogate = -mean(sur);  loss_value = mean(value_loss), divided by 6 std(ret) (unbiased, over the M rows) iff loss_value_norm
 *     loss_total = loss_surrogate + c_kl mean(kl) + c_v loss_value - c_ent mean(entropy)
 *   seed_head [M, 2A] = d loss_total / d head_new (the log_std column through the exp; exactly 0 where log_std lies outside the clamp),
 *   seed_v [M] = d loss_total / d v_new, under torch's tie rules:
 *     surrogate: -(1/M) adv ratio d logp_new where ratio adv <= clamp(ratio) adv, else 0 (inside the clip both are the same number and
 *       clamp passes its gradient on the closed interval, so min's half-and-half split adds up to the whole);
 *     value: (2 c_v / M)(v_new - ret) / norm where l1 >= l2 or |v_new - val_old| <= value_clip, else 0.
 *   stats[0 .. 5] = loss_total, loss_surrogate, loss_value, mean(entropy), mean(kl), mean(|ratio - 1| > clip); behind them 6 std(ret),
 *   the blocks' partial sums and a ticket: GOPS_PPO_STATS_FLOATS floats, 8-byte aligned, ALL ZERO before the first call; the call leaves
 *   the ticket zero.  loss_value_norm: up to 8192 rows one workgroup in ONE launch, larger minibatches TWO launches of 64 workgroups
 *   (moments of ret, then seeds and sums); without it one launch at every size.
 *   GOPS_ERR_BAD_ARG: a NULL pointer, batch < 1, act_dim outside 1 .. GOPS_MAX_ACT, a misaligned `stats`, batch < 2 with loss_value_norm. */
struct GopsPpoLoss {
    int32_t act_dim;
    int32_t loss_value_clip;
    int32_t loss_value_norm;
    int32_t reserved;
    double min_log_std, max_log_std;
};
typedef struct GopsPpoLoss GopsPpoLoss;
#define GOPS_PPO_STATS_FLOATS 656
#define GOPS_PPO_HYPER_FLOATS 8
int gops_ppo_loss(const GopsPpoLoss* desc, int32_t batch, const float* head_new, const float* v_new, const float* act, const float* logp_old,
                  const float* adv, const float* ret, const float* val_old, const float* logits_old, const float* hyper, float* seed_head,
                  float* seed_v, float* stats, void* stream);
/* gops_adv_normalize: out[i] = (adv[i] - mean(adv)) / (std(adv) + eps), std unbiased (ppo.py:123-125); `out` may be `adv`.
 * stats[0] = mean, [1] = std; GOPS_ADV_STATS_FLOATS floats, 8-byte aligned, all zero before the first call.  One launch up to 8192
 * elements, two launches of 64 workgroups beyond.  GOPS_ERR_BAD_ARG: a NULL pointer, n < 2, a misaligned `stats`. */
#define GOPS_ADV_STATS_FLOATS 264
int gops_adv_normalize(const float* adv, int32_t n, double eps, float* out, float* stats, void* stream);
/* gops_gae: value targets and generalised advantages (on_sampler.py:168-187) of n_envs environments over `steps` = T steps, arrays
 * time-major [T, n_envs]; one lane per environment walks backwards:
 *     at a step with end != 0 (the last of a segment: terminated, timed out) and at t = T - 1:
 *         next_v = val_next (1 - done), the carried gae restarts at 0;     elsewhere next_v = val[t + 1]
 *     delta = rew + gamma next_v - val;   gae = delta + gamma gae_lambda gae;   ret = gae + val;   adv = gae
 * in double, stored as float.  GOPS_ERR_BAD_ARG: a NULL pointer, steps < 1, n_envs < 1. */
int gops_gae(const float* rew, const float* val, const float* val_next, const float* done, const float* end, int32_t steps, int32_t n_envs,
             double gamma, double gae_lambda, float* ret, float* adv, void* stream);

/* ABI v15, additive entry points (the version number stays 15): TRPO (gops/algorithm/trpo.py; csrc/trpo.hip).
 *
 * At theta = theta_old the Hessian of mean_i KL(pi_theta(.|o_i) || pi_old(.|o_i)) is its Gauss-Newton term alone (the KL's gradient
 * with respect to the head vanishes there):   H v = (1/B) sum_i J_i^T M_i J_i v,   J_i the Jacobian of the policy's RAW head
 * (mean, raw log std) [2A] of row i with respect to the parameters,   M_i = diag(1 / sigma_a^2, m_a),   m_a = 2 where the raw log std
 * lies in [min_log_std, max_log_std], 0 outside.  One product is gops_gauss_fisher_seed followed by gops_mlp_backward with its
 * result as grad_y.
 *
 * gops_gauss_fisher_seed: seed [B, 2A] = (1/B) M_i (J_i v) for x [B, in] - the parameter-tangent forward fused with the metric.
 *   `tangent`: v in GopsMlpGrad's layout (read only): weight[j] [out_j, in_j], bias[j] [out_j].  The primal is recomputed here; no
 *   stash is read or written, and no workspace is needed.  Accepted nets: fp32, 1 .. 3 hidden layers of widths that are multiples of 16
 *   up to 256, in <= 64, an even output width 2A with A <= GOPS_MAX_ACT, every hidden activation; GOPS_ERR_UNSUPPORTED otherwise.  A
 *   row's result does not depend on the batch size.
 * gops_trpo_surrogate: from the RAW heads head_new, head_old [M, 2A] (clamped and exponentiated here; they may be the same array),
 *   act [M, A], adv [M]:
 *     stats[0] = mean(exp(logp_new - logp_old) adv),   stats[1] = mean(KL(N(new) || N(old))),
 *     ((int32_t*)stats)[2] = stats[0] > 0 && stats[1] < hyper[0]   (hyper: device, hyper[0] = delta; the line search's verdict),
 *     seed_head [M, 2A] = d stats[0] / d head_new (the log-std column exactly 0 outside the clamp), unless seed_head is NULL.
 *   With head_old == head_new the ratio is exactly 1 and the KL exactly 0.  stats: GOPS_TRPO_STATS_FLOATS floats, 8-byte aligned, all
 *   zero before the first call (partial sums and a ticket behind the results).  One workgroup up to 8192 rows, 64 beyond.
 * gops_cg_init / _step / _finish: `_conjugate_gradient` (trpo.py:226-267) for (H + damping I) x = g on flat fp32 vectors of n
 *   elements, every scalar in the device state block, so that the host reads nothing between two products:
 *     init:   x = 0, r = p = g, r_dot = r.r, done = all(|r| <= atol)   (allclose against zero: rtol multiplies |0|), counters = 0
 *     step:   calls += 1; if done: nothing else.  Otherwise, with Ap the UNDAMPED product H p:
 *             Ap += damping p;  alpha = r_dot / (p.Ap + 1e-8);  x += alpha p;  r -= alpha Ap;  iterations += 1;
 *             done = all(|r| <= atol);  if not done: beta = r_dot' / (r_dot + 1e-8), p = r + beta p;   r_dot = r_dot'
 *     finish: g_x = g.x;  scale = sqrt(2 hyper[0] / (g_x + 1e-8));  step = scale x     (hyper[0] = delta, as above)
 *   Dots are doubles in the fixed order of the element count; elements are formed in double and rounded once.  Up to
 *   GOPS_CG_ONE_BLOCK_MAX elements one workgroup does a whole call in one launch; beyond, a step is three launches of 64 workgroups
 *   (init one, finish two).  The state block must be all zero before the first gops_cg_init.
 *   GOPS_ERR_BAD_ARG: a NULL pointer, n < 1, a state block that is not 8-byte aligned. */
struct GopsCgState {
    double r_dot;         /* r.r of the current residual */
    double p_ap;          /* p.(H + damping I) p of the last step */
    double alpha, beta;   /* of the last step */
    double g_x, scale;    /* gops_cg_finish */
    int32_t done;         /* 1 once all(|r| <= atol) */
    int32_t calls;        /* gops_cg_step calls since gops_cg_init */
    int32_t iterations;   /* of them, the ones that updated x and r: where the reference's loop returns */
    int32_t ticket;       /* scratch: zero between launches */
    double part[128];     /* scratch: 64 workgroups' two partial sums */
};
typedef struct GopsCgState GopsCgState;
#define GOPS_CG_STATE_FLOATS 272
#define GOPS_CG_ONE_BLOCK_MAX 8192
#define GOPS_TRPO_STATS_FLOATS 264
#define GOPS_TRPO_HYPER_FLOATS 4
int gops_gauss_fisher_seed(const GopsMlp* policy, const GopsMlpGrad* tangent, int32_t batch, const float* x, double min_log_std,
                           double max_log_std, float* seed, void* stream);
int gops_trpo_surrogate(int32_t act_dim, int32_t batch, double min_log_std, double max_log_std, const float* head_new, const float* head_old,
                        const float* act, const float* adv, const float* hyper, float* seed_head, float* stats, void* stream);
int gops_cg_init(const float* g, float* x, float* r, float* p, int32_t n, double atol, GopsCgState* state, void* stream);
int gops_cg_step(float* p, float* Ap, float* x, float* r, int32_t n, double damping, double atol, GopsCgState* state, void* stream);
int gops_cg_finish(const float* g, const float* x, float* step, int32_t n, const float* hyper, GopsCgState* state, void* stream);

/* ABI v15, additive entry points (the version number stays 15): DQN (gops/algorithm/dqn.py; csrc/actor_critic.hip).
 *
 * gops_dqn_backup: the whole no-grad half of dqn.py:138-140 in ONE launch, forward only, nothing stashed.  Per batch row:
 *     q_targ [act_num] = q(obs2)                       the TARGET ActionValueDis' stack, act_num linear outputs
 *     a_star = argmax_a q_targ[a]                      the LOWEST index among bit-equal maxima
 *     backup = rew * reward_scale + gamma * (1 - done) * q_targ[a_star]
 * Tiles, staging and the eight fp32 fmaf chains of the hidden layers are gops_ac_backup's; the act_num head outputs are the same
 * chains in double - thread (row, g) forms outputs g, g + 256 / R, .. and parks them in LDS, thread (row, 0) takes the maximum over
 * the doubles in index order - and every stored value is rounded once: the results are bitwise reproducible and a row's result
 * depends neither on the batch size nor on the tile size.  (Rounding is monotone: q_targ[row, a_star] is the row's maximum of the
 * stored fp32 values as well.)
 * Accepted (gops_dqn_backup_workspace_bytes returns 0 otherwise, gops_dqn_backup GOPS_ERR_UNSUPPORTED): act_num 2 ..
 * GOPS_DQN_MAX_ACTIONS, obs_dim <= 64, q: obs_dim -> .. -> act_num as gops_ac_backup accepts a network.  GOPS_ERR_BAD_ARG: NULL
 * obs2 / rew / done / backup, batch < 1, a network whose output width is not act_num.  The same 256-byte workspace section as
 * gops_ac_backup; workspace_bytes below it: GOPS_ERR_WORKSPACE.
 * Outputs: backup [B]; optional (NULL): q_targ [B, act_num], a_star [B] (int32). */
#define GOPS_DQN_MAX_ACTIONS 16
struct GopsDqnBackup {
    GopsMlp q;                   /* the TARGET network: obs_dim -> .. -> act_num */
    int32_t act_num;
    int32_t reserved;
    double reward_scale, gamma;
};
typedef struct GopsDqnBackup GopsDqnBackup;
size_t gops_dqn_backup_workspace_bytes(const GopsDqnBackup* desc, int32_t batch);
int gops_dqn_backup(const GopsDqnBackup* desc, int32_t batch, const float* obs2, const float* rew, const float* done, float* backup,
                    float* q_targ, int32_t* a_star, void* workspace, size_t workspace_bytes, void* stream);
/* gops_dqn_loss: the seam between the forward and the backward of the live network in one launch.  q_all [B, act_num]: the ONLINE
 * network on obs (gops_mlp_forward's output); act [B]: the replay buffer's float column, the index by truncation towards zero (as
 * `a.to(torch.long)`); backup [B]; weight [B] or NULL (prioritized replay's importance weights; NULL = ones).  q_sel = q_all[b, act[b]]:
 *     seed [B, act_num] = (2 / B) weight (q_sel - backup) in column act[b], an explicit 0 in every other (the DENSE seed of the output
 *                         layer, for gops_mlp_backward)
 *     abs_err [B]       = |q_sel - backup|                                                      (NULL: not wanted)
 *     stats[0] = mean(weight (q_sel - backup)^2), stats[1] = mean(q_sel), stats[2] = the number of rows whose index lies outside
 *     [0, act_num) - such a row (a NaN index included) gets an all-zero seed row and abs_err 0, adds nothing to the sums (the means
 *     still divide by B) and reads and writes nothing outside its own row.
 * `stats`: 8-byte aligned device memory of GOPS_DQN_LOSS_STATS_FLOATS floats, ALL ZERO before the first call (behind the results:
 * the blocks' partial sums and a ticket the call leaves zero again), as for gops_ac_critic_loss; sums in double, in a fixed order
 * that depends on B only (one block up to 8192 rows, else 64 blocks folded by the last one).
 * GOPS_ERR_BAD_ARG: NULL q_all / act / backup / seed / stats, batch < 1, act_num < 1, a misaligned `stats`. */
#define GOPS_DQN_LOSS_STATS_FLOATS 392
int gops_dqn_loss(const float* q_all, const float* act, const float* backup, const float* weight, int32_t act_num, int32_t batch,
                  float* seed, float* abs_err, float* stats, void* stream);

/* ABI v15, additive entry points (the version number stays 15): TRPO on discrete actions - a categorical policy (StochaPolicyDis) over
 * n = act_num action indices, p = softmax(logits) (csrc/trpo.hip).  The Gauss-Newton form of the KL's Hessian above holds with J_i
 * the Jacobian of the n LOGITS of row i and M_i = diag(p_i) - p_i p_i^T, the softmax Fisher metric.
 *
 * gops_cat_fisher_seed: seed [B, n] = (1/B) (diag(p) - p p^T) (J v), n = policy->sizes[n_layers], for x [B, in]; `tangent` as for
 *   gops_gauss_fisher_seed, and the hidden layers are that kernel's tangent forward (one kernel, the head is its template parameter).
 *   Head, per row, in double: the logits z_k and their tangents u_k = W t + V h + c are the eight-chain dots of the Gaussian head,
 *   parked in LDS - thread (row, g) forms k = g, g + 256 / R, .. -; then in index order
 *       m = max_k z_k,  e_k = exp(z_k - m),  S = sum_k e_k,  p_k = e_k / S,  pu = sum_k p_k u_k,   seed[k] = (float)(p_k (u_k - pu) / B).
 *   Every stored value is rounded once; a row's bits depend neither on the batch size (beyond the 1 / B) nor on the tile rows; a second
 *   launch gives the same bits; no atomics.  Accepted: fp32, 1 .. 3 hidden layers of widths that are multiples of 16 up to 256,
 *   in <= 64, 2 <= n <= GOPS_DQN_MAX_ACTIONS, every hidden activation; GOPS_ERR_UNSUPPORTED otherwise.  GOPS_ERR_BAD_ARG: a NULL
 *   pointer (a tangent slice included), batch < 1.
 * gops_cat_trpo_surrogate: logits_new, logits_old [M, n] (they may be the same array), act [M] the float index column (the index by
 *   truncation towards zero, as in gops_dqn_loss), adv [M].  Per row, in double:
 *       lse = m + log(sum_k exp(z_k - m)),  logp_k = z_k - lse   (new and old),   p_new,k = exp(z_new,k - m_new) / S_new,
 *       ratio = exp(logp_new[a] - logp_old[a]),   kl = sum_k p_new,k (logp_new,k - logp_old,k)   in index order: KL(new || old),
 *       seed_head [M, n]: seed_head[i, k] = (float)((1/M) adv_i ratio_i ((k == a) - p_new,k)), unless seed_head is NULL.
 *     stats[0] = mean surrogate, stats[1] = mean KL, ((int32_t*)stats)[2] = stats[0] > 0 && stats[1] < hyper[0] on the stored fp32
 *     values, ((int32_t*)stats)[3] = the number of rows whose index lies outside [0, n), a NaN index included.  Such a row adds nothing
 *     to either sum (the means still divide by M), gets an all-zero seed row, and reads and writes nothing outside its own row.
 *   With logits_old == logits_new the ratio is exactly 1 and the KL exactly 0.  The KL has no special case for a zero probability: a
 *   p_new,k that underflows to 0 contributes 0, and logp_old is finite for finite logits - torch's kl_divergence returns inf where
 *   q = 0 in fp32; this does not.  stats: gops_trpo_surrogate's layout and size (GOPS_TRPO_STATS_FLOATS floats, 8-byte aligned, all
 *   zero before the first call: the partial sums, the ticket and the running count of bad rows behind the results, left zero again).
 *   One workgroup up to 8192 rows, 64 beyond.  GOPS_ERR_BAD_ARG: a NULL pointer (seed_head excepted), batch < 1, act_num < 1, a
 *   misaligned `stats`; GOPS_ERR_UNSUPPORTED: act_num outside 2 .. GOPS_DQN_MAX_ACTIONS. */
int gops_cat_fisher_seed(const GopsMlp* policy, const GopsMlpGrad* tangent, int32_t batch, const float* x, float* seed, void* stream);
int gops_cat_trpo_surrogate(int32_t act_num, int32_t batch, const float* logits_new, const float* logits_old, const float* act,
                            const float* adv, const float* hyper, float* seed_head, float* stats, void* stream);

/* Which kernels a rollout description runs on this device (ABI v8; for benchmarks / profiles, no launch):
 * bit 0 (GOPS_VARIANT_SPLIT): the register-stationary kernels with plane-split contractions - hidden-layer weights,
 *        activations and deltas as two half planes each (22 bits), 3 f16 MFMAs (16x16x32) per 32-deep block, fp32
 *        accumulation and results (GOPS_DTYPE_F32 above);
 * bit 1 (GOPS_VARIANT_STATIONARY_F32): the register-stationary kernels on exact fp32 MFMAs;
 * bit 2 (GOPS_VARIANT_STREAMED_SPLIT_FWD, ABI v9): the FORWARD rollout on the streamed plane-split kernel (any number of
 *        256-wide hidden layers, weight planes streamed from L2, tail value net included - except that the tail value net of a
 *        relu / selu launch that keeps a gradient is evaluated with exact fp32 products); the backward sweep of such a
 *        launch runs on the streamed plane-split sweep where its LDS image fits twice per CU, else on the streamed fp32-MFMA kernel;
 * bit 3 (GOPS_VARIANT_HALF_TILE64, ABI v10): GOPS_DTYPE_F16 on the 64-trajectory-tile kernels (rollout_h64.hip);
 * none: the streamed kernels (exact fp32 MFMAs, or half-precision MFMAs for GOPS_DTYPE_F16).
 * Negative: a GOPS_ERR_* code for a description the library rejects. */
/* GopsRolloutDesc.variant_flags / GopsMlp.variant_flags (ABI v10; replaces the process-environment knobs of v9).  ABI v14
 * retired the bits 0x20, 0x40, 0x80, 0x200 and 0x80000 .. 0x800000: a description that carries a bit outside GOPS_VF_ALL is
 * rejected (GOPS_ERR_BAD_ARG). */
#define GOPS_VF_NO_STATIONARY_SPLIT 0x1u     /* not the register-stationary plane-split kernels */
#define GOPS_VF_NO_STREAMED_SPLIT_FWD 0x2u   /* not the streamed plane-split forward */
#define GOPS_VF_NO_STREAMED_SPLIT_BWD 0x4u   /* not the streamed plane-split sweep */
#define GOPS_VF_NO_STREAMED_SPLIT_VALUE 0x8u /* value / MLP batches (GOPS_ENV_NONE) on the fp32-MFMA kernels */
#define GOPS_VF_STREAMED_FP32 0x10u          /* the plain streamed exact-fp32 kernels: no stationary weights, no planes */
#define GOPS_VF_SPLIT_TAIL_MULTI 0x100u      /* stationary plane-split kernels also for tail + more tiles than CUs */
#define GOPS_VF_NO_NARROW_LDS 0x400u         /* narrow policies on the streamed fp32 kernels: hidden-layer weights from L2 every step, not LDS-resident (A/B) */
#define GOPS_VF_NO_NARROW_N64 0x800u         /* obs-64-64-act policies on the generic narrow kernels, not the ones written out for that shape (A/B, identical results) */
#define GOPS_VF_DW_EXACT 0x10000u            /* weight-gradient GEMM: exact three-plane bf16 split */
#define GOPS_VF_DW_F32 0x20000u              /*   fp32-MFMA GEMM */
#define GOPS_VF_DW_NO_GUARD 0x40000u         /*   test knob: no exact redo of saturated blocks */
#define GOPS_VF_NO_FUSED_DW0 0x4000000u      /*   GOPS_DTYPE_F16, 64-row kernels: the first layer's gradient by its GEMM, not inside the sweep (A/B) */
/* A backward call in two halves, so that a data-parallel caller can put the all-reduce of the gradients that are ready
 * first on a side stream while the rest is still being formed (gops_amd/trainer/grad_sync.py):
 *   PHASE_A: sweep, output layer's gradient and every hidden layer's EXCEPT the first one's (reduced and final in the caller's
 *            buffers when the call's work completes); PHASE_B (same description, same workspace, after PHASE_A): the first
 *            hidden layer's weight gradient + bias from the stash PHASE_A left.  Neither / both bits: the whole backward. */
#define GOPS_VF_BWD_PHASE_A 0x1000000u
#define GOPS_VF_BWD_PHASE_B 0x2000000u
#define GOPS_VF_ALL (GOPS_VF_NO_STATIONARY_SPLIT | GOPS_VF_NO_STREAMED_SPLIT_FWD | GOPS_VF_NO_STREAMED_SPLIT_BWD | \
                     GOPS_VF_NO_STREAMED_SPLIT_VALUE | GOPS_VF_STREAMED_FP32 | GOPS_VF_SPLIT_TAIL_MULTI | GOPS_VF_NO_NARROW_LDS | \
                     GOPS_VF_NO_NARROW_N64 | GOPS_VF_DW_EXACT | GOPS_VF_DW_F32 | GOPS_VF_DW_NO_GUARD | GOPS_VF_NO_FUSED_DW0 | \
                     GOPS_VF_BWD_PHASE_A | GOPS_VF_BWD_PHASE_B)   /* ABI v14: every bit a description may carry */

#define GOPS_VARIANT_SPLIT 1
#define GOPS_VARIANT_STATIONARY_F32 2
#define GOPS_VARIANT_STREAMED_SPLIT_FWD 4
#define GOPS_VARIANT_HALF_TILE64 8   /* ABI v10: GOPS_DTYPE_F16 on the 64-trajectory-tile kernels (GOPS_ENV_LQ / _NONE, 256-wide nets) */
int gops_rollout_variant(const GopsRolloutDesc* desc);

/* Which kernel the weight-gradient stage runs for ONE layer (host only: no launch, no device; for tests): dW[N][K] =
 * delta^T * input over S stash rows (S = samples padded to whole 16-row tiles, times the horizon), Kp = K padded to 16.
 *   f16: GOPS_DTYPE_F16 stash;  scaled: the launch has a delta scale (grad_v is the backward call's one gradient source - the
 *   hidden layers of gops_value_backward / gops_rollout_backward; 0 for gops_mlp_backward);  vflags: GOPS_VF_DW_* bits;
 *   dw_workgroups: GopsRolloutDesc.dw_workgroups (0 = default; gops_mlp_backward's output layer always plans with 0).
 * out = {kernel (GOPS_DW_*), split-K slabs, 32-sample chunks per slab (64-sample for f16), launched workgroups - the grid
 * comes in whole groups of 8 slabs, the surplus workgroups return at once}.  GOPS_OK or GOPS_ERR_BAD_ARG. */
enum { GOPS_DW_NONE = 0, GOPS_DW_SPEC = 1, GOPS_DW_RING_H2 = 2, GOPS_DW_RING_EXACT = 3, GOPS_DW_SKINNY = 4, GOPS_DW_FM4_BF3 = 5,
       GOPS_DW_FM4_F32 = 6, GOPS_DW_FM2_BF3 = 7, GOPS_DW_FM2_F32 = 8, GOPS_DW_F16 = 9 };
int gops_dw_plan_query(int32_t N, int32_t K, int32_t Kp, int64_t S, int32_t f16, int32_t scaled, uint32_t vflags,
                       int32_t dw_workgroups, int32_t out[4]);

/* ABI v15, additive entry points (the version number stays 15): batched shooting MPC - `batch` independent box-constrained problems
 * min f_b(x), lo <= x <= hi, of n = control points x act_dim variables each, solved side by side by a limited-memory BFGS with history
 * m whose every scalar lives in ONE device state block, so that the host reads nothing between two cost evaluations
 * (csrc/mpc_lbfgs.hip).  The caller evaluates cost and gradient of all rows at x_trial (one open-loop rollout forward and backward)
 * and hands them to gops_mpc_step, which writes the next x_trial.
 *
 * State block, gops_mpc_state_bytes(batch, n, m) bytes (0 for arguments the entry points refuse), 8-byte aligned:
 *     double  [batch][GOPS_MPC_SCALARS + m]    f, f_prev, alpha, dphi, gamma, rho[m]
 *     int32_t [batch][GOPS_MPC_COUNTERS]       status (GOPS_MPC_*), iterations, evaluations, line-search count, ring head, ring count
 *     float   lo [n'], hi [n']                 n' = n rounded up to even
 *     float   [batch][GOPS_MPC_VECTORS + 2 m][n]   x, g (accepted), x_prev, g_prev, d, x_trial, s[m], y[m]
 *   a problem's vectors are consecutive rows of n floats: the lanes that work on it read contiguous memory.
 * gops_mpc_init: x = x_trial = clamp(x0, lo, hi) (also written to the x_trial argument), everything else of the block cleared
 *   (gamma = 1), every status GOPS_MPC_RUNNING; lo, hi are copied into the block.
 * gops_mpc_step: f [batch], g [batch, n] = cost and gradient at the x_trial the previous call (or gops_mpc_init) wrote.  For every
 *   row whose status is GOPS_MPC_RUNNING (the others are left untouched, their x_trial row rewritten as their accepted x):
 *     evaluations += 1.  f or any g not finite: status = GOPS_MPC_NONFINITE.
 *     First call after init: the point is accepted without a test and without a pair.  Otherwise the Armijo test
 *         f <= f_acc + c1 dphi,   dphi = g_acc . (x_trial - x) the directional derivative along the PROJECTED step.
 *     Fails: line-search count += 1; when it reaches max_ls: status = GOPS_MPC_LINE_SEARCH; else alpha *= shrink,
 *         x_trial = clamp(x + alpha d), dphi again.
 *     Holds: s = x_trial - x, y = g - g_acc (rounded to float); the pair enters the ring (rho = 1 / s.y, gamma = s.y / y.y) unless
 *         s.y <= curv_eps y.y (the curvature test of scipy's L-BFGS-B).  x_prev, g_prev, f_prev <- the accepted point; the trial point
 *         becomes the accepted one; iterations += 1, line-search count = 0.
 *         max |x - clamp(x - g)| <= pgtol: status = GOPS_MPC_CONVERGED_PG;
 *         else f_prev - f <= ftol max(|f_prev|, |f|, 1): status = GOPS_MPC_CONVERGED_F    (not on the first call).
 *         Still running: d = - H g by the two-loop recursion over the ring on the FREE variables (free: not on a bound with
 *         the gradient pointing outward; fixed variables get d = 0; initial matrix gamma I; rho of the unrestricted pairs);
 *         with an empty ring d = - g on the free variables and alpha = min(1, 1 / |d|), else alpha = 1;
 *         x_trial = clamp(x + alpha d).
 *     Whenever a trial point is formed with dphi >= 0 and a non-empty ring, the ring is dropped (count = 0) and the trial point
 *     is formed again along the projected steepest descent as above.
 *   hyper: DEVICE memory, GOPS_MPC_HYPER_FLOATS floats read by the kernel - {c1, shrink, max_ls, pgtol, ftol, curv_eps, 0, 0} - so a
 *   change of tolerances does not invalidate a captured graph.
 * gops_mpc_finish: x [batch, n], f [batch], status [batch], iterations [batch] <- the accepted point of every row.
 * One launch per call.  A sub-group of W lanes owns a problem: W = 64 for n > 64, else the smallest of 4, 8, 16, 32 with 2 W >= n.
 * Every dot product is a fixed-order sum in double (own elements in index order, then an xor butterfly), there are no atomics and
 * every stored value is rounded once: a repeated call gives the same bits, and a row's bits depend neither on batch nor on its index.
 * GOPS_ERR_BAD_ARG: a NULL pointer, batch < 1, n < 1, m < 1, m > GOPS_MPC_MAX_HISTORY, a state block that is not 8-byte aligned;
 * then GOPS_ERR_UNSUPPORTED: n > GOPS_MPC_MAX_DIM; then GOPS_ERR_WORKSPACE: state_bytes < gops_mpc_state_bytes(batch, n, m) - all
 * before any HIP call. */
#define GOPS_MPC_MAX_DIM 256
#define GOPS_MPC_MAX_HISTORY 8
#define GOPS_MPC_HYPER_FLOATS 8
#define GOPS_MPC_SCALARS 5
#define GOPS_MPC_COUNTERS 8
#define GOPS_MPC_VECTORS 6
enum { GOPS_MPC_RUNNING = 0, GOPS_MPC_CONVERGED_PG = 1, GOPS_MPC_CONVERGED_F = 2, GOPS_MPC_LINE_SEARCH = 3, GOPS_MPC_NONFINITE = 4 };
size_t gops_mpc_state_bytes(int32_t batch, int32_t n, int32_t m);
int gops_mpc_init(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, const float* x0, const float* lo, const float* hi,
                  float* x_trial, void* stream);
int gops_mpc_step(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, const float* f, const float* g, float* x_trial,
                  const float* hyper, void* stream);
int gops_mpc_finish(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, float* x, float* f, int32_t* status,
                    int32_t* iterations, void* stream);

/* ABI v15, additive entry point (the version number stays 15): the receding-horizon hand-over between two solves of a closed loop,
 * one launch.  Per row, with x, status, iterations, evaluations the values gops_mpc_finish reports and A = act_dim, n = n_cp A:
 *     action [batch, A]  <- x[0 : A], the first control point; 0 for a frozen row
 *     x0                 =  (x[A : n], x[n - A : n]): the first control point dropped, the last repeated (n_cp = 1: x0 = x)
 *     the row's block    <- what gops_mpc_init leaves for x0: x = x_trial = clamp(x0, lo, hi) with the bounds of the block (also
 *                           written to the x_trial argument), every other vector, scalar and counter cleared, gamma = 1, status
 *                           GOPS_MPC_RUNNING - or GOPS_MPC_FROZEN for a frozen row, which gops_mpc_step then leaves untouched
 *     record [batch][4]  :  [0] <- the status read (GOPS_MPC_FROZEN for a frozen row); for a row that is not frozen
 *                           [1] += iterations, [2] += evaluations, [3] += 1 (the caller clears the record before an episode)
 * frozen [batch]: non-zero = the row's episode has ended.  The block must have been initialised by gops_mpc_init (it holds lo, hi).
 * Same sub-group layout as the other kernels; every source element is read before any is written; copies and a clamp only.
 * GOPS_ERR_BAD_ARG: a NULL pointer, batch < 1, n outside 1 .. GOPS_MPC_MAX_DIM, m outside 1 .. GOPS_MPC_MAX_HISTORY, act_dim < 1,
 * n % act_dim != 0, a state block that is not 8-byte aligned, state_bytes != gops_mpc_state_bytes(batch, n, m) - before any HIP call. */
#define GOPS_MPC_FROZEN 5
int gops_mpc_advance(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, int32_t act_dim, const float* frozen,
                     float* action, int32_t* record, float* x_trial, void* stream);

/* ABI v15, additive entry points (the version number stays 15): path constraints c_tk(x) <= 0 of the batched shooting MPC by an
 * augmented Lagrangian around gops_mpc_step, per row and with no host read.  With t = 0 .. H - 1 the steps whose constraint value
 * depends on the plan and k = 0 .. n_c - 1, the inner problem the L-BFGS minimises between two multiplier updates is
 *     f_al(x) = f(x) + (1 / (2 rho)) sum_{t,k} (max(0, lambda_tk + rho c_tk(x))^2 - lambda_tk^2)        (Rockafellar's form),
 * whose gradient is that of f plus the constraint Jacobian applied to the seed max(0, lambda_tk + rho c_tk).
 * Layouts: c and seed [H, batch, n_c] (GopsRolloutOut.constraints / GopsRolloutIn.grad_constraint_step), lambda [batch, H, n_c]
 * (a row's multipliers contiguous), rho, viol, viol_prev, f, f_al [batch], outer [batch][GOPS_MPC_AL_COUNTERS] int32:
 * {outer status (GOPS_MPC_AL_*), outer iterations, evaluations of the inner solves already re-armed, 0}.
 * al_hyper: DEVICE memory, GOPS_MPC_AL_HYPER_FLOATS floats {rho0, growth, rho_max, shrink_target, cstr_tol, max_outer, lambda_tol, 0}.
 *
 * gops_mpc_al_eval (csrc/mpc_constraint.hip), one launch: f_al, seed and viol = max_{t,k} max(0, c_tk) of every row from c, lambda,
 *   rho and the rollout cost f (f_al must not be f).  One wave per row: lane l adds the terms j = t n_c + k = l, l + 64, .. in index
 *   order in double, then an xor butterfly - a fixed order that depends on neither batch nor the row.  A c that is not finite makes
 *   f_al NaN (gops_mpc_step then reports GOPS_MPC_NONFINITE); the seed of a NaN c is NaN; viol passes over a NaN.
 *   GOPS_ERR_BAD_ARG: a NULL pointer, batch < 1, H outside 1 .. GOPS_MPC_AL_MAX_H, n_c outside 1 .. GOPS_MAX_CONSTRAINT - before any
 *   HIP call.
 * gops_mpc_al_update (csrc/mpc_lbfgs.hip), one launch: the outer step.  c, viol: those of the row's ACCEPTED point.  Only a row whose
 *   inner status is GOPS_MPC_CONVERGED_PG, _CONVERGED_F or _LINE_SEARCH and whose outer status is GOPS_MPC_AL_RUNNING is touched
 *   (GOPS_MPC_RUNNING, _NONFINITE and _FROZEN rows are left alone):
 *     lambda_tk <- max(0, lambda_tk + rho c_tk) (formed in double, rounded once); change = max_{t,k} |new - old|;
 *     unless viol <= shrink_target viol_prev: rho <- min(rho growth, rho_max);   viol_prev <- viol;   outer iterations += 1;
 *     viol <= cstr_tol and change <= lambda_tol rho (rho before its growth; change / rho = max |max(c_tk, - lambda_tk / rho)|, the
 *       complementarity measure in the units of c): outer status GOPS_MPC_AL_CONVERGED;
 *     else outer iterations == max_outer: GOPS_MPC_AL_MAX_OUTER;
 *     else the row's L-BFGS block is re-armed for the new objective: status GOPS_MPC_RUNNING, ring count, ring head, line-search
 *       count and f_prev cleared (pairs and costs of the old objective are stale), the block's evaluations moved into outer[2] and
 *       cleared - so the next gops_mpc_step accepts x with its new cost and gradient untested, as after gops_mpc_init; x, iterations kept.
 *   GOPS_ERR_BAD_ARG: a NULL pointer, batch < 1, n outside 1 .. GOPS_MPC_MAX_DIM, m outside 1 .. GOPS_MPC_MAX_HISTORY, H outside
 *   1 .. GOPS_MPC_AL_MAX_H, n_c outside 1 .. GOPS_MAX_CONSTRAINT, a state block that is not 8-byte aligned, state_bytes !=
 *   gops_mpc_state_bytes(batch, n, m) - before any HIP call.
 * gops_mpc_al_advance (csrc/mpc_lbfgs.hip), two launches: gops_mpc_advance with its arguments and refusals, then per row that is not
 *   frozen: lambda_out_t = lambda_in_{t + shift} (t + shift < H), 0 from there on (shift = env steps of one control interval);
 *   record[2] += outer[2]; rho = rho0; viol_prev = +inf; outer cleared.  Frozen rows: lambda_out = lambda_in, nothing else written.
 *   Out of place: lambda_in != lambda_out.  GOPS_ERR_BAD_ARG additionally: a NULL pointer, lambda_in == lambda_out, H or n_c as
 *   above, shift < 1 - before any HIP call. */
#define GOPS_MPC_AL_HYPER_FLOATS 8
#define GOPS_MPC_AL_COUNTERS 4
#define GOPS_MPC_AL_MAX_H 65536
enum { GOPS_MPC_AL_RUNNING = 0, GOPS_MPC_AL_CONVERGED = 1, GOPS_MPC_AL_MAX_OUTER = 2 };
int gops_mpc_al_eval(int32_t batch, int32_t H, int32_t n_c, const float* c, const float* lambda, const float* rho, const float* f,
                     float* f_al, float* seed, float* viol, void* stream);
int gops_mpc_al_update(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, int32_t H, int32_t n_c, const float* c,
                       float* lambda, float* rho, const float* viol, float* viol_prev, int32_t* outer, const float* al_hyper, void* stream);
int gops_mpc_al_advance(void* state, size_t state_bytes, int32_t batch, int32_t n, int32_t m, int32_t act_dim, const float* frozen,
                        float* action, int32_t* record, float* x_trial, int32_t H, int32_t n_c, int32_t shift, const float* lambda_in,
                        float* lambda_out, float* rho, float* viol_prev, int32_t* outer, const float* al_hyper, void* stream);

/* Timing hook for bench.py: average duration in ms of the named internal kernel over the
 * launches recorded since the last reset (HIP events on the launch stream).  kernel ids:
 * 0 = forward rollout, 1 = backward sweep, 2 = weight-gradient GEMMs (+ reduce) of gops_rollout_*;
 * 3, 4, 5 = the same three of gops_value_forward / _backward (plain MLP batches, INFADP's V(o)). */
void gops_profile_enable(int32_t on);
void gops_profile_reset(void);
int gops_profile_read(int32_t kernel_id, double* avg_ms, int64_t* launches);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GOPS_HIP_H */
