"""ctypes binding of libgops_hip.so (C ABI: include/gops_hip.h).

PyTorch is used only for device memory and streams: every call passes raw device pointers of
caller-owned tensors plus the current HIP stream.  There is NO CPU or eager-PyTorch fallback:
if the shared library is missing, or a shape is unsupported, the call raises.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# GOPS_HIP_LIB: another build of the same library (the phase-counter build `make -C gops_amd/csrc dbg`)
LIB_PATH = os.environ.get("GOPS_HIP_LIB") or os.path.join(_HERE, "libgops_hip.so")

MAX_LAYERS, MAX_ACT, MAX_LQ, TILE = 5, 4, 6, 16
ENV_NONE, ENV_LQ, ENV_IDP, ENV_VEH, ENV_VEH_SURR, ENV_CARTPOLE, ENV_PENDULUM, ENV_VEH2DOF, ENV_MOBILEROBOT = 0, 1, 2, 3, 4, 5, 6, 7, 8
ENV_MOUNTAINCAR = 9
STATE_OBS_ENV_KINDS = (ENV_LQ, ENV_IDP, ENV_CARTPOLE, ENV_PENDULUM, ENV_MOUNTAINCAR)   # the models whose observation is the state
DATA_ENV_KINDS = (ENV_LQ, ENV_IDP, ENV_VEH, ENV_CARTPOLE, ENV_VEH2DOF, ENV_MOBILEROBOT)   # the models whose data env gops_env_step restates
MAX_CLIP_OBS = 16
# std of the obstacle robot's per-step (v, w) noise draws (pyth_mobilerobot_model.py:141-147, std_type["obs"])
MOBILEROBOT_NOISE_STD = (0.03, 0.02)
MAX_SURR = 4
MAX_REPEAT = 8   # GOPS_MAX_REPEAT
ACT_IDS = {"linear": 0, "relu": 1, "elu": 2, "gelu": 3, "selu": 4, "sigmoid": 5, "tanh": 6}
# GopsMlp.hidden_act of a POLY net (ABI v15): make_features(obs, d) for d = 1, 2, 3 and create_features(obs * norm_matrix, 2)
POLY_FULL = {1: 16, 2: 17, 3: 18}
POLY_SYM_2 = 24
# GopsMlp.hidden_act of an RBF net (gops/apprfunc/gauss.py): DetermPolicy's affine head, FiniteHorizonPolicy's tanh head (GOPS_RBF_*)
RBF_AFFINE, RBF_TANH = 32, 33
# RPI's policy evaluation (gops_rpi_evaluate): env kinds of its own and the layout of its constant table (GOPS_RPI_* of gops_hip.h)
RPI_ENV_OSCILLATOR, RPI_ENV_AIRCRAFT, RPI_ENV_SUSPENSION = 1, 2, 3
(RPI_C_GAMMA_ATTE, RPI_C_DT, RPI_C_R, RPI_C_ACT_LOW, RPI_C_ACT_HIGH, RPI_C_ADV_LOW, RPI_C_ADV_HIGH, RPI_C_SCALE_ACT_LOW,
 RPI_C_SCALE_ACT_HIGH, RPI_C_SCALE_ADV_LOW, RPI_C_SCALE_ADV_HIGH, RPI_C_ACTION_SCALE, RPI_C_CLIP_ACTION) = range(13)
RPI_C_Q, RPI_C_THRESHOLD, RPI_C_NORM, RPI_CONST_COUNT = 13, 17, 21, 32
RPI_MAX_BATCH, RPI_MAX_STEPS, RPI_STATE_HEADER = 1024, 1 << 20, 32
DTYPE_IDS = {"fp32": 0, "f32": 0, "float32": 0, "fp16": 1, "f16": 1, "float16": 1, "half": 1}


def dtype_id(name) -> int:
    """GOPS_DTYPE_* of an `mlp_dtype` setting ("fp32" default; "fp16" = half-precision MFMA contractions)."""
    if name is None:
        return 0
    try:
        return DTYPE_IDS[str(name).lower()]
    except KeyError:
        raise RuntimeError(f"unknown mlp_dtype {name!r}: expected 'fp32' or 'fp16'") from None

_fp = C.POINTER(C.c_float)


class GopsMlp(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("sizes", C.c_int32 * (MAX_LAYERS + 1)),
                ("hidden_act", C.c_int32), ("dtype", C.c_int32), ("variant_flags", C.c_uint32),
                ("weight", C.c_void_p * MAX_LAYERS), ("bias", C.c_void_p * MAX_LAYERS)]


class GopsMlpGrad(C.Structure):
    _fields_ = [("weight", C.c_void_p * MAX_LAYERS), ("bias", C.c_void_p * MAX_LAYERS)]


class GopsEnv(C.Structure):
    _fields_ = [("kind", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32),
                ("pre_horizon", C.c_int32),
                ("min_action", C.c_float * MAX_ACT), ("max_action", C.c_float * MAX_ACT),
                ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT),
                ("policy_low", C.c_float * MAX_ACT), ("policy_high", C.c_float * MAX_ACT),
                ("clip_obs", C.c_int32), ("obs_low", C.c_float * MAX_CLIP_OBS), ("obs_high", C.c_float * MAX_CLIP_OBS),
                ("shaping", C.c_int32), ("reward_scale", C.c_float), ("reward_shift", C.c_float),
                ("lq_inv_IA", C.c_float * (MAX_LQ * MAX_LQ)), ("lq_B", C.c_float * (MAX_LQ * MAX_ACT)),
                ("lq_Q", C.c_float * MAX_LQ), ("lq_R", C.c_float * MAX_ACT),
                ("lq_dt", C.c_float), ("lq_reward_scale", C.c_float), ("lq_reward_shift", C.c_float),
                ("no_mask_at_done", C.c_int32), ("n_surr", C.c_int32), ("n_constraint", C.c_int32), ("surr_penalty", C.c_int32),
                ("veh_length", C.c_float), ("veh_width", C.c_float),
                ("road_upper", C.c_float), ("road_lower", C.c_float), ("reward_w", C.c_float * 8),
                ("data_env", C.c_int32), ("scale_obs", C.c_int32), ("obs_scale", C.c_float * 8), ("obs_shift", C.c_float * 8),
                ("cstr_err", C.c_int32), ("err_tol", C.c_float * 2),
                ("ref_custom", C.c_int32), ("ref_c", C.c_float * 24),
                ("repeat_num", C.c_int32), ("repeat_last_reward", C.c_int32)]


class GopsRolloutDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("horizon", C.c_int32), ("finite_horizon", C.c_int32),
                ("need_grad", C.c_int32), ("tail_value", C.c_int32), ("open_loop", C.c_int32),
                ("dtype", C.c_int32), ("tail_unmasked", C.c_int32), ("variant_flags", C.c_uint32), ("l2_warmup", C.c_int32),
                ("dw_workgroups", C.c_int32), ("reserved0", C.c_int32), ("gamma", C.c_double), ("env", GopsEnv), ("policy", GopsMlp),
                ("value", GopsMlp)]


# GopsRolloutDesc.variant_flags / GopsMlp.variant_flags (include/gops_hip.h, ABI v10): kernel-variant selection is part of the
# description - no process-global state.  DEFAULT_VARIANT_FLAGS is what `Rollout` / `make_mlp` use when the caller passes none
# (tests patch it to steer the algorithm classes).
VF_NO_STATIONARY_SPLIT, VF_NO_STREAMED_SPLIT_FWD, VF_NO_STREAMED_SPLIT_BWD, VF_NO_STREAMED_SPLIT_VALUE = 0x1, 0x2, 0x4, 0x8
VF_STREAMED_FP32, VF_SPLIT_TAIL_MULTI, VF_NO_NARROW_LDS, VF_NO_NARROW_N64 = 0x10, 0x100, 0x400, 0x800
VF_DW_EXACT, VF_DW_F32, VF_DW_NO_GUARD = 0x10000, 0x20000, 0x40000
VF_BWD_PHASE_A, VF_BWD_PHASE_B, VF_NO_FUSED_DW0 = 0x1000000, 0x2000000, 0x4000000   # a backward in two halves (overlapped gradient all-reduce, trainer/grad_sync.py)
DEFAULT_VARIANT_FLAGS = 0
# gops_dw_plan_query's kernel ids (include/gops_hip.h GOPS_DW_*: csrc/dw_plan.h DwKernel)
(DW_NONE, DW_SPEC, DW_RING_H2, DW_RING_EXACT, DW_SKINNY, DW_FM4_BF3, DW_FM4_F32, DW_FM2_BF3, DW_FM2_F32, DW_F16) = range(10)
DW_KERNEL_NAMES = ("None", "Spec", "RingH2", "RingExact", "Skinny", "Fm4Bf3", "Fm4F32", "Fm2Bf3", "Fm2F32", "F16")


class GopsRolloutIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "done", "state", "ref_points", "path_num", "u_num",
                                          "ref_time", "head_pre", "surr_state", "grad_constraint", "grad_constraint_prod",
                                          "ref_appended", "noise", "grad_constraint_step")]


class GopsRolloutOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("v_pi", "rewards", "final_obs", "final_done", "final_state", "constraint_sums",
                                          "constraint_prods", "constraints")]


ADAM_MAX = 16


class GopsRolloutAdjoint(C.Structure):
    _fields_ = [("grad_final_obs", C.c_void_p), ("grad_obs", C.c_void_p), ("first_step_only", C.c_int32),
                ("reserved", C.c_int32)]


class GopsAdamTensors(C.Structure):
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("numel", C.c_int64 * ADAM_MAX),
                ("param", C.c_void_p * ADAM_MAX), ("grad", C.c_void_p * ADAM_MAX),
                ("exp_avg", C.c_void_p * ADAM_MAX), ("exp_avg_sq", C.c_void_p * ADAM_MAX)]


class GopsUpdateTail(C.Structure):   # ABI v12: gops_rollout_backward_update
    _fields_ = [("adam", C.POINTER(GopsAdamTensors)), ("adam_state", C.c_void_p), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("mean_x", C.c_void_p), ("mean_n", C.c_int32), ("reserved", C.c_int32),
                ("mean_scale", C.c_double), ("mean_stats", C.c_void_p), ("polyak", C.POINTER(GopsAdamTensors)), ("polyak_tau", C.c_double)]


class GopsStepIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "action", "done", "state", "ref_points", "path_num",
                                          "u_num", "ref_time", "next_obs", "reward", "next_done",
                                          "next_state", "next_ref_points", "next_ref_time",
                                          "surr_state", "next_surr_state", "constraint", "ref_appended", "noise")]


class GopsLipsNet(C.Structure):   # gops_lips_forward / _backward
    _fields_ = [("mlp", GopsMlp), ("k_net", GopsMlp), ("k_scalar", C.c_void_p), ("eps", C.c_float), ("lam", C.c_float),
                ("training", C.c_int32), ("squash", C.c_int32), ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT)]


class GopsLipsGrad(C.Structure):
    _fields_ = [("mlp", GopsMlpGrad), ("k_net", GopsMlpGrad), ("k_scalar", C.c_void_p)]


class GopsEpisodeOut(C.Structure):   # gops_episode_rollout
    _fields_ = [(k, C.c_void_p) for k in ("ret", "length", "terminated", "trace_obs", "trace_act", "trace_rew")]


SAMPLE_DETERM, SAMPLE_GAUSS, SAMPLE_TANH_GAUSS = 0, 1, 2   # include/gops_hip.h: GOPS_SAMPLE_*
SAMPLE_WORKSPACE_BYTES = 256                             # include/gops_hip.h: GOPS_SAMPLE_WORKSPACE_BYTES
SAMPLE_INFO_KEYS = ("state", "ref_points", "path_num", "u_num", "ref_time")


class GopsSampleDesc(C.Structure):   # gops_sample_rollout
    _fields_ = [("head", C.c_int32), ("max_episode_steps", C.c_int32), ("pool_rows", C.c_int32), ("reserved", C.c_int32),
                ("noise_std", C.c_double), ("min_log_std", C.c_double), ("max_log_std", C.c_double)]


class GopsSampleState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs",) + SAMPLE_INFO_KEYS + ("t", "reset_count")]


class GopsSamplePool(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs",) + SAMPLE_INFO_KEYS]


class GopsSampleOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "act", "rew", "done", "obs2", "logp", "time_limited", "end")
                + tuple(p + k for k in SAMPLE_INFO_KEYS for p in ("", "next_"))]


SAMPLE_EPS_GREEDY, SAMPLE_CATEGORICAL = 3, 4   # include/gops_hip.h: GOPS_SAMPLE_EPS_GREEDY / _CATEGORICAL (gops_sample_rollout_dis)


class GopsSampleDis(C.Structure):   # gops_sample_rollout_dis
    _fields_ = [("action_table", C.c_void_p), ("act_num", C.c_int32), ("head", C.c_int32), ("epsilon", C.c_double),
                ("env_act", C.c_void_p)]


class GopsAcBackup(C.Structure):   # gops_ac_backup
    _fields_ = [("policy", GopsMlp), ("q", GopsMlp * 2), ("n_q", C.c_int32), ("smooth", C.c_int32),
                ("squash_low", C.c_float * MAX_ACT), ("squash_high", C.c_float * MAX_ACT),
                ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT),
                ("target_noise", C.c_double), ("noise_clip", C.c_double), ("reward_scale", C.c_double), ("gamma", C.c_double)]


class GopsDqnBackup(C.Structure):   # gops_dqn_backup
    _fields_ = [("q", GopsMlp), ("act_num", C.c_int32), ("reserved", C.c_int32), ("reward_scale", C.c_double), ("gamma", C.c_double)]


class GopsSoftBackup(C.Structure):   # gops_soft_backup
    _fields_ = [("policy", GopsMlp), ("q", GopsMlp * 2), ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT),
                ("min_log_std", C.c_double), ("max_log_std", C.c_double), ("gamma", C.c_double), ("alpha", C.c_double),
                ("log_alpha", C.c_void_p)]


class GopsSoftQBackup(C.Structure):   # gops_soft_q_backup
    _fields_ = [("policy", GopsMlp), ("q", GopsMlp * 2), ("n_q", C.c_int32), ("distri", C.c_int32),
                ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT),
                ("min_log_std", C.c_double), ("max_log_std", C.c_double), ("gamma", C.c_double), ("alpha", C.c_double),
                ("log_alpha", C.c_void_p)]


class GopsTanhGauss(C.Structure):   # gops_tanh_gauss_forward / _backward
    _fields_ = [("act_dim", C.c_int32), ("reserved", C.c_int32), ("act_low", C.c_float * MAX_ACT), ("act_high", C.c_float * MAX_ACT),
                ("min_log_std", C.c_double), ("max_log_std", C.c_double)]


class GopsPpoLoss(C.Structure):   # gops_ppo_loss
    _fields_ = [("act_dim", C.c_int32), ("loss_value_clip", C.c_int32), ("loss_value_norm", C.c_int32), ("reserved", C.c_int32),
                ("min_log_std", C.c_double), ("max_log_std", C.c_double)]


def _signatures():
    """name -> (restype, argtypes) of every symbol of include/gops_hip.h (argtypes None: not declared to ctypes)."""
    P, vp, i32, sz, f64, rc = C.POINTER, C.c_void_p, C.c_int32, C.c_size_t, C.c_double, C.c_int
    desc, rin, rout, mlp, grad, env, io = (P(t) for t in (GopsRolloutDesc, GopsRolloutIn, GopsRolloutOut, GopsMlp, GopsMlpGrad, GopsEnv,
                                                          GopsStepIO))
    tail, adj, tensors, lips = P(GopsUpdateTail), P(GopsRolloutAdjoint), P(GopsAdamTensors), P(GopsLipsNet)
    return {
        "gops_hip_version": (rc, None),
        "gops_rollout_workspace_bytes": (sz, [desc]),
        "gops_rollout_forward": (rc, [desc, rin, rout, vp, sz, vp]),
        "gops_rollout_backward": (rc, [desc, rin, vp, grad, vp, sz, vp]),
        "gops_rollout_backward_open_loop": (rc, [desc, rin, vp, vp, vp, sz, vp]),
        "gops_rollout_backward_adj": (rc, [desc, rin, vp, grad, adj, vp, sz, vp]),
        "gops_rollout_backward_open_loop_adj": (rc, [desc, rin, vp, vp, adj, vp, sz, vp]),
        "gops_rollout_backward_update": (rc, [desc, rin, vp, grad, tail, vp, sz, vp]),
        "gops_rollout_variant": (rc, [desc]),
        "gops_dw_plan_query": (rc, [i32, i32, i32, C.c_int64, i32, i32, C.c_uint32, i32, P(i32)]),
        "gops_env_step": (rc, [env, i32, io, vp]),
        "gops_env_constraint": (rc, [env, i32, io, vp]),
        "gops_value_workspace_bytes": (sz, [mlp, i32]),
        "gops_value_forward": (rc, [mlp, i32, vp, vp, vp, sz, vp]),
        "gops_value_backward": (rc, [mlp, i32, vp, vp, grad, vp, sz, vp]),
        "gops_value_backward_update": (rc, [mlp, i32, vp, vp, grad, tail, vp, sz, vp]),
        "gops_mlp_workspace_bytes": (sz, [mlp, i32]),
        "gops_mlp_forward": (rc, [mlp, i32, vp, vp, vp, sz, vp]),
        "gops_mlp_backward": (rc, [mlp, i32, vp, vp, grad, vp, sz, vp]),
        "gops_mlp_backward_x": (rc, [mlp, i32, vp, vp, grad, vp, vp, sz, vp]),
        "gops_adam_step": (rc, [tensors, vp, f64, f64, f64, vp]),
        "gops_polyak_update": (rc, [tensors, f64, vp]),
        "gops_value_loss": (rc, [vp, vp, i32, vp, vp, vp]),
        "gops_mean_loss": (rc, [vp, i32, f64, vp, vp]),
        "gops_poly_rollout_workspace_bytes": (sz, [desc]),
        "gops_poly_rollout_forward": (rc, [desc, rin, rout, vp, sz, vp]),
        "gops_poly_rollout_backward": (rc, [desc, rin, vp, grad, vp, sz, vp]),
        "gops_poly_value_workspace_bytes": (sz, [mlp, i32]),
        "gops_poly_value_forward": (rc, [mlp, i32, vp, vp, vp]),
        "gops_poly_value_backward": (rc, [mlp, i32, vp, vp, grad, vp, sz, vp]),
        "gops_rbf_rollout_workspace_bytes": (sz, [desc]),
        "gops_rbf_rollout_forward": (rc, [desc, rin, rout, vp, sz, vp]),
        "gops_rbf_rollout_backward": (rc, [desc, rin, vp, grad, adj, vp, sz, vp]),
        "gops_rpi_state_bytes": (sz, [i32, i32]),
        "gops_rpi_evaluate": (rc, [i32, i32, i32, _fp, vp, vp, vp, vp, vp, sz, f64, f64, f64, f64, vp, vp, vp]),
        "gops_rpi_mlp_state_bytes": (sz, [i32, i32, mlp]),
        "gops_rpi_mlp_evaluate": (rc, [i32, i32, i32, _fp, mlp, mlp, vp, vp, vp, sz, f64, f64, f64, f64, vp, vp, vp]),
        "gops_episode_workspace_bytes": (sz, [env, mlp, i32, i32]),
        "gops_episode_rollout": (rc, [env, mlp, i32, i32, io, P(GopsEpisodeOut), vp, sz, vp]),
        "gops_sample_workspace_bytes": (sz, [env, mlp, i32, i32]),
        "gops_sample_rollout": (rc, [env, mlp, P(GopsSampleDesc), i32, i32, P(GopsSampleState), P(GopsSamplePool), vp, P(GopsSampleOut),
                                     vp, sz, vp]),
        "gops_sample_dis_workspace_bytes": (sz, [env, mlp, i32, i32, i32]),
        "gops_sample_rollout_dis": (rc, [env, mlp, P(GopsSampleDesc), P(GopsSampleDis), i32, i32, P(GopsSampleState), P(GopsSamplePool),
                                         vp, P(GopsSampleOut), vp, sz, vp]),
        "gops_episode_dis_workspace_bytes": (sz, [env, mlp, i32, i32, i32]),
        "gops_episode_rollout_dis": (rc, [env, mlp, vp, i32, i32, i32, io, P(GopsEpisodeOut), vp, sz, vp]),
        "gops_episode_mode_workspace_bytes": (sz, [env, mlp, i32, i32, i32]),
        "gops_episode_rollout_mode": (rc, [env, mlp, i32, i32, i32, io, P(GopsEpisodeOut), vp, sz, vp]),
        "gops_lips_workspace_bytes": (sz, [lips, i32]),
        "gops_lips_forward": (rc, [lips, i32, vp, vp, vp, vp, vp, sz, vp]),
        "gops_lips_backward": (rc, [lips, i32, vp, vp, P(GopsLipsGrad), vp, sz, vp]),
        "gops_ac_backup_workspace_bytes": (sz, [P(GopsAcBackup), i32]),
        "gops_ac_backup": (rc, [P(GopsAcBackup), i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gops_ac_critic_loss": (rc, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "gops_soft_backup_workspace_bytes": (sz, [P(GopsSoftBackup), i32]),
        "gops_soft_backup": (rc, [P(GopsSoftBackup), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gops_dsact_critic_loss": (rc, [vp, vp, vp, i32, f64, vp, vp, vp, vp]),
        "gops_tanh_gauss_forward": (rc, [P(GopsTanhGauss), i32, vp, vp, f64, vp, vp, vp, vp]),
        "gops_tanh_gauss_backward": (rc, [P(GopsTanhGauss), i32, vp, vp, vp, vp, vp, vp]),
        "gops_soft_q_backup_workspace_bytes": (sz, [P(GopsSoftQBackup), i32]),
        "gops_soft_q_backup": (rc, [P(GopsSoftQBackup), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gops_dsac_critic_loss": (rc, [vp, vp, i32, i32, vp, vp, vp]),
        "gops_ppo_loss": (rc, [P(GopsPpoLoss), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gops_adv_normalize": (rc, [vp, i32, f64, vp, vp, vp]),
        "gops_gae": (rc, [vp, vp, vp, vp, vp, i32, i32, f64, f64, vp, vp, vp]),
        "gops_gauss_fisher_seed": (rc, [mlp, grad, i32, vp, f64, f64, vp, vp]),
        "gops_trpo_surrogate": (rc, [i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gops_cat_fisher_seed": (rc, [mlp, grad, i32, vp, vp, vp]),
        "gops_cat_trpo_surrogate": (rc, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gops_cg_init": (rc, [vp, vp, vp, vp, i32, f64, vp, vp]),
        "gops_cg_step": (rc, [vp, vp, vp, vp, i32, f64, f64, vp, vp]),
        "gops_cg_finish": (rc, [vp, vp, vp, i32, vp, vp, vp]),
        "gops_mpc_state_bytes": (sz, [i32, i32, i32]),
        "gops_mpc_init": (rc, [vp, sz, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gops_mpc_step": (rc, [vp, sz, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gops_mpc_finish": (rc, [vp, sz, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gops_mpc_advance": (rc, [vp, sz, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gops_mpc_al_eval": (rc, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gops_mpc_al_update": (rc, [vp, sz, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gops_mpc_al_advance": (rc, [vp, sz, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "gops_dqn_backup_workspace_bytes": (sz, [P(GopsDqnBackup), i32]),
        "gops_dqn_backup": (rc, [P(GopsDqnBackup), i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gops_dqn_loss": (rc, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "gops_profile_enable": (rc, [i32]),
        "gops_profile_reset": (rc, []),
        "gops_profile_read": (rc, [i32, P(f64), P(C.c_int64)]),
    }


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
_lib = None


def lib() -> C.CDLL:
    """Load libgops_hip.so; fails loudly (no fallback) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C gops_amd/csrc`). The HIP rollout has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        _lib = l
    return _lib


def dw_plan_query(N: int, K: int, S: int, *, Kp: Optional[int] = None, f16=False, scaled=False, vflags: int = 0,
                  dw_workgroups: int = 0) -> Dict[str, int]:
    """`gops_dw_plan_query` (host only): the kernel (DW_*), split-K slabs, chunks per slab and launched grid of one layer's
    weight-gradient GEMM dW[N][K] over S stash rows."""
    out = (C.c_int32 * 4)()
    kp = (K + 15) // 16 * 16 if Kp is None else Kp
    check(lib().gops_dw_plan_query(N, K, kp, S, int(bool(f16)), int(bool(scaled)), vflags, dw_workgroups, out), "gops_dw_plan_query")
    return dict(kernel=out[0], splits=out[1], chunks_per_split=out[2], grid=out[3])


_ERR = {-1: "GOPS_ERR_BAD_ARG", -2: "GOPS_ERR_UNSUPPORTED", -3: "GOPS_ERR_WORKSPACE"}


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {_ERR.get(rc, 'hipError_t ' + str(rc))}")


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "need contiguous fp32 device tensor"
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = float(v)


def _fill_mlp(m: GopsMlp, weights, biases, act: str) -> GopsMlp:
    m.n_layers = len(weights)
    if weights:
        m.sizes[0] = weights[0].shape[1]
    for j, (w, b) in enumerate(zip(weights, biases)):
        m.sizes[j + 1] = w.shape[0]
        m.weight[j], m.bias[j] = _ptr(w), _ptr(b)
    m.hidden_act = ACT_IDS[act]
    return m


def make_mlp(weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], act: str, dtype=None,
             variant_flags: Optional[int] = None) -> GopsMlp:
    """`dtype` ("fp32" / "fp16") and `variant_flags` (VF_*) only matter for `ValueNet` / `Mlp` batches; a `Rollout` takes its
    own for all nets."""
    m = GopsMlp()
    m.dtype = dtype_id(dtype)
    m.variant_flags = DEFAULT_VARIANT_FLAGS if variant_flags is None else variant_flags
    if not 2 <= len(weights) <= MAX_LAYERS:
        raise RuntimeError(f"MLP with {len(weights)} Linear layers is outside the HIP path (2..{MAX_LAYERS})")
    _fill_mlp(m, weights, biases, act)
    m._keep = (list(weights), list(biases))   # the struct holds raw pointers: keep the tensors alive
    return m


def make_mlp_grad(gw: Sequence[torch.Tensor], gb: Sequence[torch.Tensor]) -> GopsMlpGrad:
    g = GopsMlpGrad()
    for j, (w, b) in enumerate(zip(gw, gb)):
        g.weight[j] = _ptr(w)
        g.bias[j] = _ptr(b)
    return g


def make_env(kind: int, obs_dim: int, act_dim: int, *, act_low, act_high, min_action=-1.0, max_action=1.0,
             policy_low=None, policy_high=None, obs_low=None, obs_high=None, pre_horizon: int = 0,
             reward_scale: Optional[float] = None, reward_shift: Optional[float] = None,
             lq: Optional[Dict] = None, data_env: bool = False, surr: Optional[Dict] = None,
             obs_scale=None, obs_shift=None, ref_c=None, repeat_num: Optional[int] = None, sum_reward: bool = True,
             mask_at_done: bool = True, n_constraint: Optional[int] = None) -> GopsEnv:
    """Constants of the wrapped env model (create_env_model.py:86-128) as a C struct.  `data_env=True` (for
    `env_step` only): the DATA environment's termination tests / terminal penalty instead of the model's; obs_low /
    obs_high are then the data env's state bounds (pyth_lq) and are NOT applied as a clip."""
    e = GopsEnv()
    e.data_env = int(bool(data_env))
    e.no_mask_at_done = int(not mask_at_done)   # create_env_model(mask_at_done=False): no MaskAtDoneModel in the chain
    if repeat_num is not None:   # ActionRepeatModel (repeat_num = 1 is the identity wrapper)
        e.repeat_num, e.repeat_last_reward = int(repeat_num), int(not sum_reward)
    if ref_c is not None:   # custom path_para / u_para of the reference trajectories (resources/ref_traj_params.py)
        assert len(ref_c) == 24
        e.ref_custom = 1
        _fill(e.ref_c, [float(v) for v in ref_c])
    if obs_scale is not None or obs_shift is not None:   # ScaleObservationModel: obs seen = (obs + shift) * scale
        if obs_dim > 8:
            raise RuntimeError("obs_scale / obs_shift: observation dimension > 8 is not supported by the HIP env models")

        def bo(v, default):
            v = torch.as_tensor(default if v is None else v, dtype=torch.float32).reshape(-1)
            if v.numel() not in (1, obs_dim):
                raise RuntimeError(f"obs_scale / obs_shift must be scalars or have {obs_dim} entries")
            return (v.expand(obs_dim) if v.numel() == 1 else v).tolist() + [0.0] * (8 - obs_dim)
        e.scale_obs = 1
        _fill(e.obs_scale, bo(obs_scale, 1.0)); _fill(e.obs_shift, bo(obs_shift, 0.0))
        for i in range(obs_dim, 8):
            e.obs_scale[i] = 1.0
    if surr is not None:   # ENV_VEH_SURR: surrounding vehicles, constraint geometry, reward weights
        e.n_surr, e.n_constraint = int(surr["n_surr"]), int(surr["n_constraint"])
        e.veh_length, e.veh_width = float(surr["veh_length"]), float(surr["veh_width"])
        e.road_upper, e.road_lower = float(surr.get("road_upper", 0.0)), float(surr.get("road_lower", 0.0))
        e.surr_penalty = int(bool(surr.get("penalty", False)))
        if surr.get("err_tol") is not None:   # pyth_veh3dofconti_errcstr: constraints on the tracking errors of the observation
            e.cstr_err = 1
            _fill(e.err_tol, [float(v) for v in surr["err_tol"]])
        _fill(e.reward_w, list(surr["reward_w"]) + [0.0] * (8 - len(surr["reward_w"])))
    e.kind, e.obs_dim, e.act_dim, e.pre_horizon = kind, obs_dim, act_dim, pre_horizon
    if n_constraint is not None:
        e.n_constraint = int(n_constraint)
    A = act_dim

    def bc(v):
        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        return (v.expand(A) if v.numel() == 1 else v).tolist()

    _fill(e.min_action, bc(min_action)); _fill(e.max_action, bc(max_action))
    _fill(e.act_low, bc(act_low)); _fill(e.act_high, bc(act_high))
    _fill(e.policy_low, bc(-1.0 if policy_low is None else policy_low))
    _fill(e.policy_high, bc(1.0 if policy_high is None else policy_high))
    finite = False
    if obs_low is not None:
        lo = torch.as_tensor(obs_low, dtype=torch.float32).reshape(-1)
        hi = torch.as_tensor(obs_high, dtype=torch.float32).reshape(-1)
        finite = bool(torch.isfinite(lo).any() or torch.isfinite(hi).any())
        if finite:
            if obs_dim > (MAX_CLIP_OBS if kind == ENV_MOBILEROBOT else 8):
                raise RuntimeError("finite observation bounds are only supported for obs_dim <= 8 (pyth_lq, gym models) "
                                   "and for pyth_mobilerobot")
            _fill(e.obs_low, lo.tolist()); _fill(e.obs_high, hi.tolist())
    e.clip_obs = 1 if finite else 0
    e.shaping = 1 if (reward_scale is not None or reward_shift is not None) else 0
    e.reward_scale = 1.0 if reward_scale is None else float(reward_scale)
    e.reward_shift = 0.0 if reward_shift is None else float(reward_shift)
    if lq is not None:
        n, m = obs_dim, act_dim
        _fill(e.lq_inv_IA, torch.as_tensor(lq["inv_IA"], dtype=torch.float32).reshape(n * n).tolist())
        _fill(e.lq_B, torch.as_tensor(lq["B"], dtype=torch.float32).reshape(n * m).tolist())
        _fill(e.lq_Q, torch.as_tensor(lq["Q"], dtype=torch.float32).tolist())
        _fill(e.lq_R, torch.as_tensor(lq["R"], dtype=torch.float32).tolist())
        e.lq_dt = float(lq["dt"])
        e.lq_reward_scale = float(lq.get("reward_scale", 1.0))
        e.lq_reward_shift = float(lq.get("reward_shift", 0.0))
    return e


def has_constraints(env: GopsEnv) -> bool:
    """Models whose rollout returns constraint sums / products (and whose env step fills info["constraint"])."""
    return env.kind in (ENV_VEH_SURR, ENV_MOBILEROBOT) or (env.kind == ENV_VEH2DOF and env.cstr_err != 0)


def mobilerobot_noise(shape, device) -> torch.Tensor:
    """The obstacle robot's noise draws of `shape` = (..., 2): N(0, 0.03) for v, N(0, 0.02) for w - what
    np.random.normal hands Robot.f_xu(.., "obs") every step (pyth_mobilerobot_model.py:141-167), drawn on the device."""
    n = torch.randn(*shape, dtype=torch.float32, device=device)
    n[..., 0] *= MOBILEROBOT_NOISE_STD[0]   # (scalar kernel arguments: no host-to-device copy, so a HIP-graph capture of the
    n[..., 1] *= MOBILEROBOT_NOISE_STD[1]   #  caller stays legal and every replay draws fresh numbers from the captured generator)
    return n


def _rollout_desc(env: GopsEnv, policy: Optional[GopsMlp], value: Optional[GopsMlp], *, batch, horizon, gamma, finite_horizon,
                  need_grad, tail_unmasked) -> GopsRolloutDesc:
    """The fields `Rollout` and `PolyRollout` fill alike."""
    d = GopsRolloutDesc()
    d.batch, d.horizon, d.finite_horizon = batch, horizon, int(finite_horizon)
    d.need_grad, d.tail_value, d.gamma = int(need_grad), int(value is not None), float(gamma)
    d.tail_unmasked = int(bool(tail_unmasked))   # SPIL's evaluation target: the terminal value is not masked at done
    d.env = env
    if policy is not None:
        d.policy = policy
    if value is not None:
        d.value = value
    return d


def _rollout_workspace(ro, bytes_fn, refusal: str, device):
    """`ro.device` and `ro.workspace`, sized by the library for `ro.desc`; a descriptor it refuses raises `refusal`."""
    nbytes = bytes_fn(C.byref(ro.desc))
    if nbytes == 0:
        raise RuntimeError(refusal)
    ro.device = device or torch.device("cuda", torch.cuda.current_device())
    ro.workspace = torch.empty(nbytes, dtype=torch.uint8, device=ro.device)


def _rebind_nets(ro, policy: GopsMlp, value: Optional[GopsMlp]):
    if policy is not ro._mlps[0]:
        ro.desc.policy = policy
    if value is not None and value is not ro._mlps[1]:
        ro.desc.value = value
    ro._mlps = (policy, value if value is not None else ro._mlps[1])


def _rollout_outputs(ro, want_rewards, want_final):
    """(GopsRolloutOut, result dict) with v_pi and, on request, rewards [H, B] and final_obs [B, O] / final_done [B]."""
    d, dev = ro.desc, ro.device
    out = GopsRolloutOut()
    res = {"v_pi": torch.empty(d.batch, dtype=torch.float32, device=dev)}
    out.v_pi = _ptr(res["v_pi"])
    if want_rewards:
        res["rewards"] = torch.empty(d.horizon, d.batch, dtype=torch.float32, device=dev)
        out.rewards = _ptr(res["rewards"])
    if want_final:
        res["final_obs"] = torch.empty(d.batch, d.env.obs_dim, dtype=torch.float32, device=dev)
        res["final_done"] = torch.empty(d.batch, dtype=torch.float32, device=dev)
        out.final_obs, out.final_done = _ptr(res["final_obs"]), _ptr(res["final_done"])
    return out, res


class Rollout:
    """One configured horizon rollout (forward + backward) bound to caller-owned tensors.

    The workspace (activation stash, packed weights, reference table, split-K partials) is a
    single torch uint8 tensor sized by `gops_rollout_workspace_bytes` and reused across calls.
    """

    def __init__(self, env: GopsEnv, policy: Optional[GopsMlp], *, batch: int, horizon: int, gamma: float,
                 finite_horizon: bool, need_grad: bool = True, value: Optional[GopsMlp] = None,
                 device: Optional[torch.device] = None, dtype=None, raw_actions: bool = False,
                 tail_unmasked: bool = False, variant_flags: Optional[int] = None, l2_warmup: int = 0, dw_workgroups: int = 0):
        """`policy=None` selects the open-loop mode: `forward(data, head_pre=...)` takes the pre-tanh
        policy-head outputs of all steps [B, H, act_dim] and `backward_open_loop` returns their gradient.
        `dtype`: "fp32" (default: fp32 results at the 1e-4 bar, plane-split MFMAs where they apply) or "fp16" (half-precision
        MFMA contractions and stash).  `variant_flags`: VF_* bits (GopsRolloutDesc.variant_flags), None = DEFAULT_VARIANT_FLAGS."""
        d = self.desc = _rollout_desc(env, policy, value, batch=batch, horizon=horizon, gamma=gamma, finite_horizon=finite_horizon,
                                      need_grad=need_grad, tail_unmasked=tail_unmasked)
        d.dtype = dtype_id(dtype)
        d.variant_flags = DEFAULT_VARIANT_FLAGS if variant_flags is None else variant_flags
        d.l2_warmup, d.dw_workgroups = int(l2_warmup), int(dw_workgroups)
        # raw_actions (open loop only): `head_pre` holds the model's actions themselves (GopsRolloutDesc.open_loop = 2)
        d.open_loop = (2 if raw_actions else 1) if policy is None else 0
        self._mlps = (policy, value)
        _rollout_workspace(self, lib().gops_rollout_workspace_bytes,
                           "gops_rollout_workspace_bytes: descriptor rejected (unsupported shape for the HIP path)", device)
        self._in = GopsRolloutIn()
        self._keep = None

    def set_policy(self, policy: GopsMlp, value: Optional[GopsMlp] = None):
        """Rebind the networks (their storage moved, or a new GopsMlp was built for them)."""
        _rebind_nets(self, policy, value)

    def forward(self, data: Dict[str, torch.Tensor], *, want_rewards=False, want_final=False,
                head_pre: Optional[torch.Tensor] = None, want_constraints=False):
        d = self.desc
        B, H = d.batch, d.horizon
        i = self._in
        if d.open_loop:
            assert head_pre is not None and tuple(head_pre.shape) == (B, H, d.env.act_dim)
            i.head_pre = _ptr(head_pre)
            self._head_pre = head_pre
        i.obs, i.done = _ptr(data["obs"]), _ptr(data.get("done"))
        if d.env.kind in (ENV_VEH, ENV_VEH_SURR, ENV_VEH2DOF):
            for k in ("state", "ref_points", "path_num", "u_num", "ref_time"):
                setattr(i, k, _ptr(data[k]))
        if d.env.kind == ENV_VEH_SURR:
            i.surr_state = _ptr(data.get("surr_state"))   # (None for the errcstr model: no surrounding vehicles)
        # bit-parity mode (GopsRolloutIn.ref_appended): the reference's own appended reference points [B, H, 4]
        i.ref_appended = _ptr(data.get("ref_appended"))
        self._keep = dict(data)
        self._last_phase = None   # (a new forward invalidates a pending backward phase A)
        if d.env.kind == ENV_MOBILEROBOT:   # the obstacle's draws of this rollout [H, B, 2] (a caller may hand in its own)
            noise = data.get("noise")
            if noise is None:
                noise = mobilerobot_noise((H, B, 2), self.device)
            assert tuple(noise.shape) == (H, B, 2) and noise.dtype == torch.float32 and noise.is_contiguous()
            self._keep["noise"] = noise
            i.noise = _ptr(noise)   # the kernels (and a later backward) read these tensors: keep them alive
        out, res = _rollout_outputs(self, want_rewards, want_final)
        if want_final:
            if d.env.kind in (ENV_VEH, ENV_VEH_SURR, ENV_VEH2DOF):
                res["final_state"] = torch.empty(B, 4 if d.env.kind == ENV_VEH2DOF else 6, dtype=torch.float32, device=self.device)
                out.final_state = _ptr(res["final_state"])
        if has_constraints(d.env):   # [4, B]: sum c+^2, sum c+, sum log(-c- + eps), feasible  (discounted, unmasked)
            res["constraint_sums"] = torch.empty(4, B, dtype=torch.float32, device=self.device)
            out.constraint_sums = _ptr(res["constraint_sums"])
            # [2 n_c, B]: prod_t Phi(c_tk) and prod_t [c_tk <= 0] per constraint k (SPIL)
            nc = d.env.n_constraint
            res["constraint_prods"] = torch.empty(2 * nc, B, dtype=torch.float32, device=self.device)
            out.constraint_prods = _ptr(res["constraint_prods"])
            if want_constraints:   # [H, B, n_c]: the unmasked info["constraint"] of every step
                res["constraints"] = torch.empty(H, B, nc, dtype=torch.float32, device=self.device)
                out.constraints = _ptr(res["constraints"])
        check(lib().gops_rollout_forward(C.byref(d), C.byref(i), C.byref(out), self.workspace.data_ptr(),
                                         self.workspace.numel(), _stream()), "gops_rollout_forward")
        return res

    def backward(self, grad_v: torch.Tensor, grad_w: List[torch.Tensor], grad_b: List[torch.Tensor],
                 grad_constraint: Optional[torch.Tensor] = None, grad_constraint_prod: Optional[torch.Tensor] = None,
                 grad_constraint_step: Optional[torch.Tensor] = None, phase: Optional[str] = None,
                 tail: Optional["GopsUpdateTail"] = None):
        """`grad_constraint` (models with constraint outputs): d(loss)/d(constraint_sums rows 0..2), [3, B];
        `grad_constraint_prod`: d(loss)/d(P_k) * P_k for the Phi-products P_k = constraint_prods[k], [n_constraint, B];
        `grad_constraint_step`: d(loss)/d(per-step constraint values), [H, B, n_constraint].
        `phase`: None = the whole backward; "a" = sweep + every gradient except the first hidden layer's, "b" (after "a", same
        arguments) = the first hidden layer's (GOPS_VF_BWD_PHASE_A / _B): lets a data-parallel trainer start the all-reduce of the
        gradients that are ready first while the rest is being formed.
        `tail` (ABI v12, `gops_rollout_backward_update`; with `phase="a"` only a loss-mean tail): the Adam step and / or the loss mean of a single-process
        update, folded into the launch that forms the final gradients (`HipAdam.begin_fused`, `make_update_tail`)."""
        if tail is not None and phase is not None and (phase != "a" or tail.adam or tail.polyak):
            raise ValueError("Rollout.backward: only a loss-mean tail can ride on half a backward, and only on phase 'a'")
        if phase == "b":
            # phase B reuses the inputs (and the delta stash) phase A left in this workspace: it must follow one, directly
            if getattr(self, "_last_phase", None) != "a":
                raise RuntimeError("Rollout.backward(phase='b') must directly follow backward(phase='a') of the same rollout")
            self._last_phase = "b"
            return self._backward_call(grad_v, make_mlp_grad(grad_w, grad_b), VF_BWD_PHASE_B)
        self._last_phase = phase
        g = make_mlp_grad(grad_w, grad_b)
        self._in.grad_constraint = _ptr(grad_constraint)
        self._in.grad_constraint_prod = _ptr(grad_constraint_prod)
        self._in.grad_constraint_step = _ptr(grad_constraint_step)
        self._grad_c = (grad_constraint, grad_constraint_prod, grad_constraint_step)
        self._backward_call(grad_v, g, VF_BWD_PHASE_A if phase == "a" else 0, tail)

    def _backward_call(self, grad_v, g, phase_bits, tail=None):
        flags = self.desc.variant_flags
        self.desc.variant_flags = flags | phase_bits
        try:
            if tail is not None:
                check(lib().gops_rollout_backward_update(C.byref(self.desc), C.byref(self._in), _ptr(grad_v), C.byref(g), C.byref(tail),
                                                         self.workspace.data_ptr(), self.workspace.numel(), _stream()),
                      "gops_rollout_backward_update")
            else:
                check(lib().gops_rollout_backward(C.byref(self.desc), C.byref(self._in), _ptr(grad_v), C.byref(g),
                                                  self.workspace.data_ptr(), self.workspace.numel(), _stream()),
                      "gops_rollout_backward")
        finally:
            self.desc.variant_flags = flags


    def backward_adj(self, grad_v: torch.Tensor, grad_w: Optional[List[torch.Tensor]] = None,
                     grad_b: Optional[List[torch.Tensor]] = None, *, grad_final_obs: Optional[torch.Tensor] = None,
                     want_grad_obs: bool = False, first_step_only: bool = False) -> Optional[torch.Tensor]:
        """`gops_rollout_backward_adj`: the sweep seeded with d(loss)/d(final_obs), optionally returning
        d(loss)/d(obs) of the initial observation; `first_step_only`: parameter gradients through the action of step 0
        only (MPG's model return, mpg.py:340-353).  `grad_w is None`: no parameter gradients."""
        d = self.desc
        self._in.grad_constraint = self._in.grad_constraint_prod = self._in.grad_constraint_step = None   # (no stale seeds of an earlier call)
        adj = GopsRolloutAdjoint()
        adj.grad_final_obs = _ptr(grad_final_obs)
        g_obs = torch.empty(d.batch, d.env.obs_dim, dtype=torch.float32, device=self.device) if want_grad_obs else None
        adj.grad_obs = _ptr(g_obs)
        adj.first_step_only = int(bool(first_step_only))
        g = make_mlp_grad(grad_w, grad_b) if grad_w is not None else None
        check(lib().gops_rollout_backward_adj(C.byref(d), C.byref(self._in), _ptr(grad_v), C.byref(g) if g is not None else None,
                                              C.byref(adj), self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_rollout_backward_adj")
        return g_obs

    def backward_open_loop_adj(self, grad_v: torch.Tensor, grad_final_obs: Optional[torch.Tensor] = None):
        """`gops_rollout_backward_open_loop_adj`: (d(loss)/d(head_pre) [B, H, act_dim], d(loss)/d(obs) [B, obs_dim]) of the last
        open-loop forward, the sweep seeded with d(loss)/d(final_obs) (models whose observation is the state)."""
        d = self.desc
        self._in.grad_constraint = self._in.grad_constraint_prod = self._in.grad_constraint_step = None
        g = torch.empty(d.batch, d.horizon, d.env.act_dim, dtype=torch.float32, device=self.device)
        g_obs = torch.empty(d.batch, d.env.obs_dim, dtype=torch.float32, device=self.device)
        adj = GopsRolloutAdjoint()
        adj.grad_final_obs, adj.grad_obs, adj.first_step_only = _ptr(grad_final_obs), _ptr(g_obs), 0
        check(lib().gops_rollout_backward_open_loop_adj(C.byref(d), C.byref(self._in), _ptr(grad_v), _ptr(g), C.byref(adj),
                                                        self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_rollout_backward_open_loop_adj")
        return g, g_obs

    def backward_open_loop(self, grad_v: torch.Tensor, grad_constraint_step: Optional[torch.Tensor] = None) -> torch.Tensor:
        """d(loss)/d(head_pre) [B, H, act_dim] of the last open-loop forward; `grad_constraint_step` [H, B, n_constraint]:
        d(loss)/d(per-step constraint values) (GopsRolloutIn.grad_constraint_step)."""
        d = self.desc
        self._in.grad_constraint = self._in.grad_constraint_prod = None
        self._in.grad_constraint_step = _ptr(grad_constraint_step)
        self._grad_cs = grad_constraint_step
        g = torch.empty(d.batch, d.horizon, d.env.act_dim, dtype=torch.float32, device=self.device)
        check(lib().gops_rollout_backward_open_loop(C.byref(d), C.byref(self._in), _ptr(grad_v), _ptr(g),
                                                    self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_rollout_backward_open_loop")
        return g


def make_poly(weight: torch.Tensor, bias: Optional[torch.Tensor], feature_code: int,
              norm_matrix: Optional[torch.Tensor] = None) -> GopsMlp:
    """`GopsMlp` of a POLY net (ABI v15): n_layers = 1, sizes = (obs_dim, out width, weight columns), hidden_act = a POLY_*
    feature-map code, weight[0] = the Linear weight [out][F (+1)], bias[0] = its bias or NULL, weight[1] = norm_matrix [obs_dim] or
    NULL (value).  The library checks the column count against the feature map and the rollout's finite_horizon."""
    m = GopsMlp()
    m.n_layers = 1
    m.hidden_act = int(feature_code)
    m.weight[0], m.bias[0] = _ptr(weight), _ptr(bias)
    m.weight[1] = _ptr(norm_matrix)
    m.sizes[1], m.sizes[2] = weight.shape[0], weight.shape[1]
    m._keep = (weight, bias, norm_matrix)
    return m


def _poly_grad(grad_w: torch.Tensor, grad_b: Optional[torch.Tensor]) -> GopsMlpGrad:
    g = GopsMlpGrad()
    g.weight[0], g.bias[0] = _ptr(grad_w), _ptr(grad_b)
    return g


class _LaneRollout:
    """What the lane rollouts (csrc/lane_rollout.h) share here: the refusals, the descriptor and workspace set-up, `forward`.  A
    subclass names its family, net and three library functions (`_fns`), and keeps `_prepare_nets`, `set_policy` and `backward`."""
    _family = _net = _entry = _fns = None

    def __init__(self, env: GopsEnv, policy: GopsMlp, value: Optional[GopsMlp], *, batch, horizon, gamma, finite_horizon, need_grad,
                 tail_unmasked, device, dtype, variant_flags):
        name, fam = type(self).__name__, self._family
        if dtype_id(dtype) != 0:
            raise RuntimeError(f"{name}: {fam} approximators run in fp32 only (mlp_dtype fp16 is an MLP setting)")
        if variant_flags:
            raise RuntimeError(f"{name}: no kernel variants on the {fam} path (variant_flags {variant_flags:#x})")
        self._prepare_nets(env, policy, value)
        self.desc = _rollout_desc(env, policy, value, batch=batch, horizon=horizon, gamma=gamma, finite_horizon=finite_horizon,
                                  need_grad=need_grad, tail_unmasked=tail_unmasked)
        self._mlps = (policy, value)
        _rollout_workspace(self, self._fns(lib())[0], f"{self._entry}_workspace_bytes: descriptor rejected ({self._net} net, env model "
                           f"or wrapper outside the HIP {fam} path)", device)
        self._in = GopsRolloutIn()

    def _prepare_nets(self, env, policy, value):
        """What a family writes into its nets; called after the refusals, so that a refused construction changes nothing."""

    def forward(self, data: Dict[str, torch.Tensor], *, want_rewards=False, want_final=False):
        d, i = self.desc, self._in
        i.obs, i.done = _ptr(data["obs"]), _ptr(data.get("done"))
        self._keep = dict(data)
        out, res = _rollout_outputs(self, want_rewards, want_final)
        check(self._fns(lib())[1](C.byref(d), C.byref(i), C.byref(out), self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              self._entry + "_forward")
        return res

    def _backward(self, grad_v, g: GopsMlpGrad, *adj):
        check(self._fns(lib())[2](C.byref(self.desc), C.byref(self._in), _ptr(grad_v), C.byref(g), *adj, self.workspace.data_ptr(),
                             self.workspace.numel(), _stream()), self._entry + "_backward")


class PolyRollout(_LaneRollout):
    """`Rollout`'s call surface for a POLY policy (and POLY tail value): `gops_poly_rollout_forward / _backward`, one lane per
    trajectory (csrc/rollout_poly.hip).  `backward(grad_v, [grad_weight], [grad_bias or None])` - the lists hold the one Linear
    layer's gradient tensors, as `grad_buffers` / `poly_grad_buffers` hand them out.  No phases, no fused update tail: a POLY net
    has one or two tensors."""
    _family, _net, _entry = "POLY", "POLY", "gops_poly_rollout"
    _fns = staticmethod(lambda L: (L.gops_poly_rollout_workspace_bytes, L.gops_poly_rollout_forward, L.gops_poly_rollout_backward))

    def __init__(self, env: GopsEnv, policy: GopsMlp, *, batch: int, horizon: int, gamma: float, finite_horizon: bool,
                 need_grad: bool = True, value: Optional[GopsMlp] = None, device: Optional[torch.device] = None,
                 tail_unmasked: bool = False, dtype=None, variant_flags: Optional[int] = None):
        """`dtype` must be fp32 and `variant_flags` empty: the POLY kernels have no other arithmetic and no variants."""
        super().__init__(env, policy, value, batch=batch, horizon=horizon, gamma=gamma, finite_horizon=finite_horizon,
                         need_grad=need_grad, tail_unmasked=tail_unmasked, device=device, dtype=dtype, variant_flags=variant_flags)

    def _prepare_nets(self, env, policy, value):   # a POLY GopsMlp learns its input width here (make_poly has only the weight's shape)
        for net in filter(None, (policy, value)):
            net.sizes[0] = env.obs_dim

    def set_policy(self, policy: GopsMlp, value: Optional[GopsMlp] = None):
        self._prepare_nets(self.desc.env, policy, value)
        _rebind_nets(self, policy, value)

    def backward(self, grad_v: torch.Tensor, grad_w: List[torch.Tensor], grad_b: List[Optional[torch.Tensor]], **kw):
        if any(v is not None for v in kw.values()):
            raise NotImplementedError(f"PolyRollout.backward: {sorted(k for k, v in kw.items() if v is not None)} "
                                      "do not apply to a POLY rollout")
        self._backward(grad_v, _poly_grad(grad_w[0], grad_b[0] if grad_b else None))


def make_rbf(w: torch.Tensor, b: torch.Tensor, C: torch.Tensor, sigma_square: torch.Tensor, head_code: int) -> GopsMlp:
    """`GopsMlp` of an RBF net (gops_rbf_rollout_*): n_layers = 1, sizes = (in_dim, out_dim, K), hidden_act = RBF_AFFINE / RBF_TANH,
    weight[0] = w [1, out, K], bias[0] = b [1, out, 1], weight[1] = C [1, K, in_dim], bias[1] = sigma_square [1, K] (the module's
    own storage: contiguous, so the leading 1 and the trailing 1 change nothing).  The library checks in_dim and the head against
    the env's obs_dim and the rollout's finite_horizon."""
    for t in (w, b, C, sigma_square):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("make_rbf: the four parameter tensors must be contiguous fp32")
    K, in_dim, out = C.shape[-2], C.shape[-1], w.shape[-2]
    if w.shape[-1] != K or sigma_square.numel() != K or b.numel() != out:
        raise RuntimeError(f"make_rbf: shapes w {tuple(w.shape)}, b {tuple(b.shape)}, C {tuple(C.shape)}, sigma_square "
                           f"{tuple(sigma_square.shape)} do not describe one RBF net")
    m = GopsMlp()
    m.n_layers = 1
    m.hidden_act = int(head_code)
    m.sizes[0], m.sizes[1], m.sizes[2] = in_dim, out, K
    m.weight[0], m.bias[0], m.weight[1], m.bias[1] = _ptr(w), _ptr(b), _ptr(C), _ptr(sigma_square)
    m._keep = (w, b, C, sigma_square)
    return m


class RbfRollout(_LaneRollout):
    """`PolyRollout`'s call surface for a GAUSS policy: `gops_rbf_rollout_forward / _backward`, one lane per trajectory
    (csrc/rollout_rbf.hip).  `backward(grad_v, grads)`: `grads` holds the four gradient tensors in `state_dict` order (C,
    sigma_square, w, b).  No tail value (a caller composes it from `final_obs` and hands `grad_final_obs` back), no phases, no fused
    update tail."""
    _family, _net, _entry = "GAUSS", "RBF", "gops_rbf_rollout"
    _fns = staticmethod(lambda L: (L.gops_rbf_rollout_workspace_bytes, L.gops_rbf_rollout_forward, L.gops_rbf_rollout_backward))

    def __init__(self, env: GopsEnv, policy: GopsMlp, *, batch: int, horizon: int, gamma: float, finite_horizon: bool,
                 need_grad: bool = True, device: Optional[torch.device] = None, dtype=None, variant_flags: Optional[int] = None):
        """`dtype` must be fp32 and `variant_flags` empty: the RBF kernels have no other arithmetic and no variants."""
        super().__init__(env, policy, None, batch=batch, horizon=horizon, gamma=gamma, finite_horizon=finite_horizon,
                         need_grad=need_grad, tail_unmasked=False, device=device, dtype=dtype, variant_flags=variant_flags)

    def set_policy(self, policy: GopsMlp, value=None):
        if value is not None:
            raise NotImplementedError("RbfRollout: no tail value inside the RBF rollout")
        _rebind_nets(self, policy, None)

    def backward(self, grad_v: torch.Tensor, grads: Sequence[torch.Tensor], grad_final_obs: Optional[torch.Tensor] = None,
                 grad_obs: Optional[torch.Tensor] = None):
        """`grad_final_obs` [B, obs_dim]: d(loss)/d(final_obs), None = zeros; `grad_obs` [B, obs_dim]: filled with d(loss)/d(obs)."""
        g_C, g_s, g_w, g_b = grads
        g = GopsMlpGrad()
        g.weight[0], g.bias[0], g.weight[1], g.bias[1] = _ptr(g_w), _ptr(g_b), _ptr(g_C), _ptr(g_s)
        adj = GopsRolloutAdjoint()
        adj.grad_final_obs, adj.grad_obs, adj.first_step_only = _ptr(grad_final_obs), _ptr(grad_obs), 0
        self._adj_keep = (grad_final_obs, grad_obs)
        self._backward(grad_v, g, C.byref(adj))


class PolyValueNet:
    """`ValueNet`'s call surface for a POLY StateValue (`gops_poly_value_forward / _backward`)."""

    def __init__(self, value: GopsMlp, batch: int, obs_dim: int, device: Optional[torch.device] = None):
        value.sizes[0] = obs_dim
        self.mlp, self.batch, self.obs_dim = value, batch, obs_dim
        nbytes = lib().gops_poly_value_workspace_bytes(C.byref(value), batch)
        if nbytes == 0:
            raise RuntimeError("gops_poly_value_workspace_bytes: unsupported POLY value network for the HIP path")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def set_net(self, value: GopsMlp):
        value.sizes[0] = self.obs_dim
        self.mlp = value

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        v = torch.empty(self.batch, dtype=torch.float32, device=self.device)
        check(lib().gops_poly_value_forward(C.byref(self.mlp), self.batch, _ptr(obs), _ptr(v), _stream()), "gops_poly_value_forward")
        return v

    def backward(self, obs: torch.Tensor, grad_v: torch.Tensor, grad_w, grad_b, tail=None):
        if tail is not None:
            raise NotImplementedError("PolyValueNet.backward: no fused update tail on the POLY path")
        g = _poly_grad(grad_w[0], grad_b[0] if grad_b else None)
        check(lib().gops_poly_value_backward(C.byref(self.mlp), self.batch, _ptr(obs), _ptr(grad_v), C.byref(g),
                                             self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_poly_value_backward")


def _small_mlp(weights, biases, act: str) -> GopsMlp:
    """A LipsNet's nets: zero Linear layers (the global K) up to MAX_LAYERS; the module keeps the tensors alive."""
    if len(weights) > MAX_LAYERS:
        raise RuntimeError(f"MLP with {len(weights)} Linear layers is outside the HIP path")
    return _fill_mlp(GopsMlp(), weights, biases, act)


class LipsPolicy:
    """A LipsNet DetermPolicy (gops_amd/apprfunc/lipsnet.py) on the tangent-propagation kernels: `gops_lips_workspace_bytes /
    _forward / _backward` (csrc/rollout_lips.hip).  The parameters of `module` are read in place; call `refresh()` after they moved
    (`.to(device)`, `load_state_dict` keeps the storage).  `forward(obs, training)` -> (action [B, m], K [B], N [B]) and keeps the
    stash; `backward(grad_action)` overwrites the gradient buffers (`grads()`: one tensor per parameter in `parameters()` order -
    mlp, then K - views into one flat buffer, installed as the parameters' `.grad`)."""

    def __init__(self, module, batch: int, device: Optional[torch.device] = None):
        self.module, self.batch = module, int(batch)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.refresh()
        nbytes = lib().gops_lips_workspace_bytes(C.byref(self.net), self.batch)
        if nbytes == 0:
            raise RuntimeError("gops_lips_workspace_bytes: descriptor rejected (LipsNet outside the HIP path: obs_dim <= 8, act_dim <= 4, "
                               "1..3 hidden layers, K net global or 1..2 hidden layers, widths multiples of 16 up to 256)")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._obs = None

    def refresh(self):
        pol = self.module
        lin = pol.pi.linear_layers()
        klin = pol.pi.K.linear_layers()
        key = tuple(p.data_ptr() for p in pol.parameters())
        if getattr(self, "_key", None) == key:
            return
        self._key = key
        d = self.net = GopsLipsNet()
        d.mlp = _small_mlp([l.weight.data for l in lin], [l.bias.data for l in lin], pol._hidden_activation)
        d.k_net = _small_mlp([l.weight.data for l in klin], [l.bias.data for l in klin], "tanh")
        d.k_scalar = None if klin else _ptr(pol.pi.K.K.data)
        d.eps, d.lam = float(pol.pi.eps), float(pol.pi.loss_lambda)
        d.squash = int(pol.squash_action)
        # (more than MAX_ACT actions: the library rejects the description, gops_lips_workspace_bytes = 0)
        _fill(d.act_low, pol.act_low_lim.detach().float().cpu().reshape(-1).tolist()[:MAX_ACT])
        _fill(d.act_high, pol.act_high_lim.detach().float().cpu().reshape(-1).tolist()[:MAX_ACT])
        self._grads = None

    def grads(self) -> List[torch.Tensor]:
        params = list(self.module.parameters())
        if self._grads is None or any(p.grad is None or p.grad.data_ptr() != g.data_ptr() for p, g in zip(params, self._grads)):
            flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=self.device)
            off, self._grads = 0, []
            for p in params:
                p.grad = flat[off:off + p.numel()].view_as(p)
                self._grads.append(p.grad)
                off += p.numel()
            self.module._flat_grad = flat
            g = self._g = GopsLipsGrad()
            n_lin = len(self.module.pi.linear_layers())
            for j in range(n_lin):
                g.mlp.weight[j], g.mlp.bias[j] = _ptr(self._grads[2 * j]), _ptr(self._grads[2 * j + 1])
            rest = self._grads[2 * n_lin:]
            if self.module.pi.K.linear_layers():
                for j in range(len(rest) // 2):
                    g.k_net.weight[j], g.k_net.bias[j] = _ptr(rest[2 * j]), _ptr(rest[2 * j + 1])
            else:
                g.k_scalar = rest[0].data_ptr()
        return self._grads

    def forward(self, obs: torch.Tensor, training: bool = False):
        """`training`: the backward that follows carries the regular loss's gradient (lips_auto_adjust in training mode)."""
        self.refresh()
        B, m = self.batch, self.net.mlp.sizes[self.net.mlp.n_layers]
        if tuple(obs.shape) != (B, self.net.mlp.sizes[0]) or obs.device != self.device:   # (_ptr: fp32, contiguous, on a GPU)
            raise RuntimeError(f"LipsPolicy.forward: obs {tuple(obs.shape)} on {obs.device}, expected {(B, self.net.mlp.sizes[0])} on {self.device}")
        self.net.training = int(bool(training) and self.module.pi.lips_auto_adjust)
        act = torch.empty(B, m, dtype=torch.float32, device=self.device)
        K = torch.empty(B, dtype=torch.float32, device=self.device)
        N = torch.empty(B, dtype=torch.float32, device=self.device)
        check(lib().gops_lips_forward(C.byref(self.net), B, _ptr(obs), _ptr(act), _ptr(K), _ptr(N), self.workspace.data_ptr(),
                                      self.workspace.numel(), _stream()), "gops_lips_forward")
        self._obs = obs
        return act, K, N

    def backward(self, grad_action: torch.Tensor) -> List[torch.Tensor]:
        if self._obs is None:
            raise RuntimeError("LipsPolicy.backward before forward")
        m = self.net.mlp.sizes[self.net.mlp.n_layers]
        if tuple(grad_action.shape) != (self.batch, m) or grad_action.device != self.device:
            raise RuntimeError(f"LipsPolicy.backward: grad_action {tuple(grad_action.shape)} on {grad_action.device}, expected "
                               f"{(self.batch, m)} on {self.device}")
        grads = self.grads()
        check(lib().gops_lips_backward(C.byref(self.net), self.batch, _ptr(self._obs), _ptr(grad_action), C.byref(self._g),
                                       self.workspace.data_ptr(), self.workspace.numel(), _stream()), "gops_lips_backward")
        return grads


class _RpiState:
    """What both RPI evaluators own: the constant table, the device state block (`state`: a header, then the lanes' states
    column-major, the time-limit counters and the counters the algorithm assigns; it persists from one call to the next) and the
    result tensor."""

    def __init__(self, env_kind: int, batch: int, state_dim: int, consts, device, state_bytes: int, refusal: str):
        self.kind, self.batch, self.state_dim = int(env_kind), int(batch), int(state_dim)
        self.consts = (C.c_float * RPI_CONST_COUNT)(*[float(v) for v in consts])
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        if state_bytes == 0:
            raise RuntimeError(refusal)
        self.state = torch.zeros(state_bytes // 4, dtype=torch.float32, device=self.device)
        self.result = torch.zeros(4, dtype=torch.float32, device=self.device)

    def lanes(self) -> torch.Tensor:
        """[state_dim, B] view of the lanes' states."""
        return self.state[RPI_STATE_HEADER:RPI_STATE_HEADER + self.state_dim * self.batch].view(self.state_dim, self.batch)

    def counters(self) -> torch.Tensor:
        """[2, B] view: the time-limit counter of each lane, then the counter the algorithm assigns at a reset."""
        o = RPI_STATE_HEADER + self.state_dim * self.batch
        return self.state[o:o + 2 * self.batch].view(2, self.batch)

    def _check(self, pool, max_steps, trace):
        assert tuple(pool.shape) == (max_steps + 1, self.state_dim, self.batch)
        assert trace is None or trace.numel() >= 2 * max_steps


class RpiEvaluator(_RpiState):
    """RPI's policy evaluation of one `local_update` as ONE launch (`gops_rpi_evaluate`, csrc/rollout_rpi.hip): up to `max_steps`
    gradient steps on the value weights, each with its env step, Hamiltonian, Adam step, held-out Hamiltonian norm and 0.88 test.
    The header of the state block holds the Adam moments and step count."""

    def __init__(self, env_kind: int, batch: int, state_dim: int, consts, device: Optional[torch.device] = None):
        super().__init__(env_kind, batch, state_dim, consts, device, lib().gops_rpi_state_bytes(int(env_kind), int(batch)),
                         f"gops_rpi_state_bytes: GOPS_ERR_UNSUPPORTED (env kind {env_kind}, batch {batch}; at most {RPI_MAX_BATCH} lanes)")

    def evaluate(self, weight: torch.Tensor, target_weight: torch.Tensor, max_step: torch.Tensor, pool: torch.Tensor, max_steps: int,
                 lr: float, beta1: float, beta2: float, eps: float, trace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueues the launch; returns the device result [steps taken, last loss, norm_before, norm_after].  `pool` is
        [max_steps + 1, state_dim, B]: the held-out set, then one reset draw per step."""
        self._check(pool, max_steps, trace)
        check(lib().gops_rpi_evaluate(self.kind, self.batch, int(max_steps), self.consts, _ptr(weight), _ptr(target_weight),
                                      _ptr(max_step), _ptr(pool), self.state.data_ptr(), self.state.numel() * 4, float(lr),
                                      float(beta1), float(beta2), float(eps), _ptr(self.result), _ptr(trace), _stream()),
              "gops_rpi_evaluate")
        return self.result


class RpiMlpEvaluator(_RpiState):
    """The same for an MLP value net (`gops_rpi_mlp_evaluate`, csrc/rollout_rpi_mlp.hip): ONE launch per `local_update`; the value
    net's weights and hidden biases are stepped in place through `value`'s pointers.  The state block holds the Adam step count in
    the header, the lanes' states, the two counters per lane, the Adam moments of all parameters in `parameters()` order, and the
    kernel's scratch (include/gops_hip.h)."""

    def __init__(self, env_kind: int, batch: int, state_dim: int, consts, value: GopsMlp, target: GopsMlp,
                 device: Optional[torch.device] = None):
        self.value, self.target = value, target
        super().__init__(env_kind, batch, state_dim, consts, device,
                         lib().gops_rpi_mlp_state_bytes(int(env_kind), int(batch), C.byref(value)),
                         f"gops_rpi_mlp_state_bytes: GOPS_ERR_UNSUPPORTED (env kind {env_kind}, batch {batch}, layer sizes "
                         f"{list(value.sizes[:value.n_layers + 1])}, activation id {value.hidden_act}): one or two hidden layers, "
                         f"widths multiples of 16 up to 64, elu / gelu / tanh / sigmoid, at most {RPI_MAX_BATCH} lanes")
        self.n_params = sum(value.sizes[j + 1] * (value.sizes[j] + 1) for j in range(value.n_layers))

    def moments(self) -> torch.Tensor:
        """[2, P] view: Adam's exp_avg and exp_avg_sq of all parameters, flattened in `parameters()` order."""
        o = RPI_STATE_HEADER + (self.state_dim + 2) * self.batch
        return self.state[o:o + 2 * self.n_params].view(2, self.n_params)

    def evaluate(self, max_step: torch.Tensor, pool: torch.Tensor, max_steps: int, lr: float, beta1: float, beta2: float, eps: float,
                 trace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueues the launch; returns the device result [steps taken, last loss, norm_before, norm_after].  `pool` is
        [max_steps + 1, state_dim, B]: the held-out set, then one reset draw per step."""
        self._check(pool, max_steps, trace)
        check(lib().gops_rpi_mlp_evaluate(self.kind, self.batch, int(max_steps), self.consts, C.byref(self.value), C.byref(self.target),
                                          _ptr(max_step), _ptr(pool), self.state.data_ptr(), self.state.numel() * 4, float(lr),
                                          float(beta1), float(beta2), float(eps), _ptr(self.result), _ptr(trace), _stream()),
              "gops_rpi_mlp_evaluate")
        return self.result


class EpisodeRollout:
    """Whole closed-loop evaluation episodes in ONE launch (`gops_episode_rollout`, csrc/rollout_episode.hip): policy, DATA-env step,
    termination, time limit and return of `episodes` episodes over up to `max_steps` steps.  `env` must carry data_env = 1; the policy
    weights are read in place at every call.  A description the kernel refuses raises (GOPS_ERR_UNSUPPORTED / _BAD_ARG).
    `action_table` [act_num, act_dim] (device tensor): the greedy head over a discrete action set (`gops_episode_rollout_dis`) - the
    policy's outputs are action values or logits, the env steps with the table's row at their arg-max, trace_act [E, T, 1] is the index.
    `mode_head` SAMPLE_GAUSS / SAMPLE_TANH_GAUSS: a stochastic policy's 2A-wide stack (mean, log std) acts with the mode of its action
    distribution (`gops_episode_rollout_mode`); `act_low` / `act_high` [act_dim] then replace the limits `env` carries (in a copy)."""

    def __init__(self, env: GopsEnv, policy: GopsMlp, *, episodes: int, max_steps: int, device: Optional[torch.device] = None,
                 workspace_bytes: Optional[int] = None, action_table: Optional[torch.Tensor] = None, mode_head: Optional[int] = None,
                 act_low=None, act_high=None):
        if mode_head is None:
            assert act_low is None and act_high is None, "act_low / act_high belong to a mode head"
        else:
            assert action_table is None, "a mode head acts without an action table"
            if mode_head not in (SAMPLE_GAUSS, SAMPLE_TANH_GAUSS):
                raise ValueError(f"EpisodeRollout: mode_head {mode_head!r} is neither SAMPLE_GAUSS nor SAMPLE_TANH_GAUSS")
            if act_low is not None or act_high is not None:   # the limits travel as the deterministic head's do: in the description
                env = GopsEnv.from_buffer_copy(env)
                for field, lim in ((env.policy_low, act_low), (env.policy_high, act_high)):
                    if lim is not None:
                        _fill(field, np.broadcast_to(np.asarray(torch.as_tensor(lim).detach().cpu(), dtype=np.float32).reshape(-1), (env.act_dim,)))
        self.env, self.policy, self.episodes, self.max_steps = env, policy, int(episodes), int(max_steps)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.action_table = action_table
        # the one place that knows which of the three forms this is: the query, the entry point, the arguments only `_dis` / `_mode` take
        query, self._name, query_extra, self._extra, self._act_width = "gops_episode_workspace_bytes", "gops_episode_rollout", (), (), env.act_dim
        if action_table is not None:
            assert action_table.dim() == 2 and action_table.shape[1] == env.act_dim, "action_table must be [act_num, act_dim]"
            self.act_num = int(action_table.shape[0])
            query, self._name, self._act_width = "gops_episode_dis_workspace_bytes", "gops_episode_rollout_dis", 1
            query_extra, self._extra = (self.act_num,), (_ptr(action_table), self.act_num)
        elif mode_head is not None:
            query, self._name = "gops_episode_mode_workspace_bytes", "gops_episode_rollout_mode"
            query_extra = self._extra = (int(mode_head),)
        nbytes = getattr(lib(), query)(C.byref(env), C.byref(policy), *query_extra, self.episodes, self.max_steps)
        if workspace_bytes is None:
            if nbytes == 0:   # ask the entry point itself for the reason
                check(self._call(None, None, None, 0, None), self._name)
                raise RuntimeError(query + ": description refused")
            workspace_bytes = nbytes
        self.workspace = torch.empty(max(int(workspace_bytes), 1), dtype=torch.uint8, device=self.device)
        self._workspace_bytes = int(workspace_bytes)

    def _call(self, io, out, ws, ws_bytes, stream):
        ref = lambda x: None if x is None else C.byref(x)   # noqa: E731
        return getattr(lib(), self._name)(C.byref(self.env), C.byref(self.policy), *self._extra, self.episodes, self.max_steps, ref(io),
                                          ref(out), ws, ws_bytes, stream)

    def set_policy(self, policy: GopsMlp):
        self.policy = policy

    def run(self, init: Dict[str, torch.Tensor], *, trace: bool = False, trace_fill: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """`init`: obs [E, obs_dim] (+ state / ref_points / path_num / u_num / ref_time for the vehicle families).  Returns device
        tensors ret [E], length [E] (int32), terminated [E] and - with `trace` - trace_obs [E, T, obs_dim], trace_act [E, T, act_dim],
        trace_rew [E, T] (rows beyond `length` keep `trace_fill`, or are uninitialised when it is None).  Enqueues only."""
        E, T, dev = self.episodes, self.max_steps, self.device
        assert init["obs"].shape[0] == E
        io, out = GopsStepIO(), GopsEpisodeOut()
        io.obs = _ptr(init["obs"])
        for k in ("state", "ref_points", "path_num", "u_num", "ref_time"):
            if init.get(k) is not None:
                setattr(io, k, _ptr(init[k]))
        res = dict(ret=torch.empty(E, dtype=torch.float32, device=dev), length=torch.empty(E, dtype=torch.int32, device=dev),
                   terminated=torch.empty(E, dtype=torch.float32, device=dev))
        if trace:
            mk = (lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)) if trace_fill is None else \
                 (lambda *sh: torch.full(sh, float(trace_fill), dtype=torch.float32, device=dev))
            res.update(trace_obs=mk(E, T, self.env.obs_dim), trace_act=mk(E, T, self._act_width),
                       trace_rew=mk(E, T))
        for k, v in res.items():
            setattr(out, k, v.data_ptr())
        check(self._call(io, out, self.workspace.data_ptr(), self._workspace_bytes, _stream()), self._name)
        return res


class SampleRollout:
    """A whole `sample()` of the device samplers in ONE launch (`gops_sample_rollout`, csrc/rollout_sample.hip): `steps` steps of
    `n_envs` environment instances - policy, exploration head, env step, stored rows, bookkeeping, resets from the pool.  Holds the
    workspace and the time-major output buffers, allocated once for (n_envs, steps): `run` returns VIEWS of them, which the next
    `run` overwrites.  The policy weights are read in place at every call.  A description the kernel refuses raises.
    `action_table` [act_num, act_dim] (device tensor) selects `gops_sample_rollout_dis`: `head` is SAMPLE_EPS_GREEDY or
    SAMPLE_CATEGORICAL, `noise` is [steps, n_envs, 2] uniforms in [0, 1), `act` is the index [steps, n_envs, 1] and `env_act`
    [steps, n_envs, act_dim] the table row applied; `dis.epsilon` is read at every `run` (as `desc.max_episode_steps` is)."""

    def __init__(self, env: GopsEnv, policy: GopsMlp, *, n_envs: int, steps: int, head: int, max_episode_steps: int, pool_rows: int,
                 noise_std: float = 0.0, min_log_std: float = 0.0, max_log_std: float = 0.0, info_like: Optional[Dict[str, torch.Tensor]] = None,
                 device: Optional[torch.device] = None, action_table: Optional[torch.Tensor] = None, epsilon: float = 0.0):
        """`info_like`: the info tensors of the persistent state ([n_envs, ...] each; the vehicle families) - their trailing shapes
        are the output columns'."""
        self.env, self.policy, self.n_envs, self.steps = env, policy, int(n_envs), int(steps)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.desc = GopsSampleDesc(head=int(head), max_episode_steps=int(max_episode_steps), pool_rows=int(pool_rows), reserved=0,
                                   noise_std=float(noise_std), min_log_std=float(min_log_std), max_log_std=float(max_log_std))
        self.action_table, self.dis = action_table, None
        # the one place that knows which of the two forms this is: the query, the entry point, the arguments only `_dis` takes
        query, self._name, query_extra, self._extra = "gops_sample_workspace_bytes", "gops_sample_rollout", (), ()
        self.noise_width = act_width = env.act_dim
        if action_table is not None:
            assert action_table.dim() == 2 and action_table.shape[1] == env.act_dim, "action_table must be [act_num, act_dim]"
            self.dis = GopsSampleDis(action_table=_ptr(action_table), act_num=int(action_table.shape[0]), head=int(head),
                                     epsilon=float(epsilon), env_act=None)
            query, self._name, self.noise_width, act_width = "gops_sample_dis_workspace_bytes", "gops_sample_rollout_dis", 2, 1
            query_extra, self._extra = (self.dis.act_num,), (C.byref(self.dis),)
        nbytes = getattr(lib(), query)(C.byref(env), C.byref(policy), *query_extra, self.n_envs, self.steps)
        if nbytes == 0:
            raise RuntimeError(query + ": description refused")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        T, N = self.steps, self.n_envs
        mk = lambda *sh: torch.empty((T, N) + tuple(sh), dtype=torch.float32, device=self.device)   # noqa: E731
        self.out = dict(obs=mk(env.obs_dim), act=mk(act_width), rew=mk(), done=mk(), obs2=mk(env.obs_dim),
                        logp=mk(), time_limited=mk(), end=mk())
        self.info_keys = tuple(k for k in SAMPLE_INFO_KEYS if info_like and k in info_like)
        for k in self.info_keys:
            self.out[k], self.out["next_" + k] = mk(*info_like[k].shape[1:]), mk(*info_like[k].shape[1:])
        self._out = GopsSampleOut()
        for k, v in self.out.items():
            setattr(self._out, k, v.data_ptr())
        if self.dis is not None:   # (not a field of GopsSampleOut: the dis struct's own output)
            self.out["env_act"] = mk(env.act_dim)
            self.dis.env_act = self.out["env_act"].data_ptr()

    def set_policy(self, policy: GopsMlp):
        self.policy = policy

    def run(self, state: Dict[str, torch.Tensor], pool: Dict[str, torch.Tensor], noise: torch.Tensor) -> Dict[str, torch.Tensor]:
        """`state`: obs [N, obs_dim], the info tensors, t [N] and reset_count [N] (int32) - advanced IN PLACE; `pool`: obs and the
        info tensors as [R, N, ...]; `noise` [T, N, act_dim] standard normals ([T, N, 2] uniforms with an action table).  Returns the output buffers ([T, N, ...] each).  Enqueues only."""
        T, N, R = self.steps, self.n_envs, self.desc.pool_rows
        assert tuple(noise.shape) == (T, N, self.noise_width) and state["obs"].shape[0] == N
        st, pl = GopsSampleState(), GopsSamplePool()
        for k in ("obs",) + self.info_keys:
            assert tuple(pool[k].shape) == (R,) + tuple(state[k].shape), k
            setattr(st, k, _ptr(state[k]))
            setattr(pl, k, _ptr(pool[k]))
        for k in ("t", "reset_count"):
            v = state[k]
            assert v.is_cuda and v.dtype == torch.int32 and v.is_contiguous() and v.numel() == N, k
            setattr(st, k, v.data_ptr())
        check(getattr(lib(), self._name)(C.byref(self.env), C.byref(self.policy), C.byref(self.desc), *self._extra, N, T, C.byref(st),
                                         C.byref(pl), _ptr(noise), C.byref(self._out), self.workspace.data_ptr(), self.workspace.numel(),
                                         _stream()), self._name)
        return self.out


class ValueNet:
    """StateValue batch forward/backward on the HIP path (INFADP PEV, infadp.py:167,185)."""

    def __init__(self, value: GopsMlp, batch: int, device: Optional[torch.device] = None):
        self.mlp, self.batch = value, batch
        nbytes = lib().gops_value_workspace_bytes(C.byref(value), batch)
        if nbytes == 0:
            raise RuntimeError("gops_value_workspace_bytes: unsupported value network for the HIP path")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        v = torch.empty(self.batch, dtype=torch.float32, device=self.device)
        check(lib().gops_value_forward(C.byref(self.mlp), self.batch, _ptr(obs), _ptr(v),
                                       self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_value_forward")
        return v

    def backward(self, obs: torch.Tensor, grad_v: torch.Tensor, grad_w, grad_b, tail: Optional["GopsUpdateTail"] = None):
        """`tail` (ABI v12, `gops_value_backward_update`): Adam step (+ Polyak step of the target) folded into the launch that forms the gradients."""
        g = make_mlp_grad(grad_w, grad_b)
        if tail is not None:
            check(lib().gops_value_backward_update(C.byref(self.mlp), self.batch, _ptr(obs), _ptr(grad_v), C.byref(g), C.byref(tail),
                                                   self.workspace.data_ptr(), self.workspace.numel(), _stream()),
                  "gops_value_backward_update")
            return
        check(lib().gops_value_backward(C.byref(self.mlp), self.batch, _ptr(obs), _ptr(grad_v), C.byref(g),
                                        self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_value_backward")


class MlpNet:
    """Batch evaluation of an MLP with an output layer of any width and its backward into the parameters
    (`gops_mlp_forward / _backward`): FiniteHorizonFullPolicy's single evaluation in FHADP2."""

    def __init__(self, mlp: GopsMlp, batch: int, device: Optional[torch.device] = None):
        self.mlp, self.batch = mlp, batch
        self.out_dim = int(mlp.sizes[mlp.n_layers])
        nbytes = lib().gops_mlp_workspace_bytes(C.byref(mlp), batch)
        if nbytes == 0:
            raise RuntimeError("gops_mlp_workspace_bytes: unsupported network for the HIP path")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`out`: a contiguous tensor of batch * out_dim floats that receives the result (e.g. one row of a [n, batch] buffer)."""
        y = torch.empty(self.batch, self.out_dim, dtype=torch.float32, device=self.device) if out is None else out
        assert y.numel() == self.batch * self.out_dim
        check(lib().gops_mlp_forward(C.byref(self.mlp), self.batch, _ptr(x), _ptr(y), self.workspace.data_ptr(),
                                     self.workspace.numel(), _stream()), "gops_mlp_forward")
        return y

    def backward(self, x: torch.Tensor, grad_y: torch.Tensor, grad_w, grad_b):
        g = make_mlp_grad(grad_w, grad_b)
        check(lib().gops_mlp_backward(C.byref(self.mlp), self.batch, _ptr(x), _ptr(grad_y), C.byref(g),
                                      self.workspace.data_ptr(), self.workspace.numel(), _stream()), "gops_mlp_backward")

    def backward_x(self, x: torch.Tensor, grad_y: torch.Tensor, grad_w=None, grad_b=None) -> torch.Tensor:
        """`gops_mlp_backward_x`: returns d(loss)/d(x); parameter gradients too when grad_w / grad_b are given."""
        g = make_mlp_grad(grad_w, grad_b) if grad_w is not None else None
        gx = torch.empty(self.batch, int(self.mlp.sizes[0]), dtype=torch.float32, device=self.device)
        check(lib().gops_mlp_backward_x(C.byref(self.mlp), self.batch, _ptr(x), _ptr(grad_y), C.byref(g) if g is not None else None,
                                        _ptr(gx), self.workspace.data_ptr(), self.workspace.numel(), _stream()),
              "gops_mlp_backward_x")
        return gx


def env_step(env: GopsEnv, obs, action, done, info: Optional[Dict[str, torch.Tensor]] = None):
    """One wrapped env-model step on the GPU (gops_env_step).  `info["ref_appended"]` [B, 4] (optional): the reference
    point this step appends, from the caller (bit-parity mode, GopsStepIO.ref_appended)."""
    B = obs.shape[0]
    io = GopsStepIO()
    nobs, rew, ndone = torch.empty_like(obs), torch.empty(B, device=obs.device), torch.empty(B, device=obs.device)
    io.obs, io.action, io.done = _ptr(obs), _ptr(action), _ptr(done)
    io.next_obs, io.reward, io.next_done = _ptr(nobs), _ptr(rew), _ptr(ndone)
    ninfo = {}
    if env.kind in (ENV_VEH, ENV_VEH_SURR, ENV_VEH2DOF):
        for k in ("state", "ref_points", "path_num", "u_num", "ref_time"):
            setattr(io, k, _ptr(info[k]))
        ninfo = dict(state=torch.empty_like(info["state"]), ref_points=torch.empty_like(info["ref_points"]),
                     ref_time=torch.empty_like(info["ref_time"]), path_num=info["path_num"], u_num=info["u_num"])
        io.next_state, io.next_ref_points = _ptr(ninfo["state"]), _ptr(ninfo["ref_points"])
        io.next_ref_time = _ptr(ninfo["ref_time"])
        io.ref_appended = _ptr(info.get("ref_appended"))
    if env.kind == ENV_MOBILEROBOT:   # info["noise"] [B, 2]: this step's obstacle draws (drawn here unless handed in)
        noise = (info or {}).get("noise")
        if noise is None:
            noise = mobilerobot_noise((B, 2), obs.device)
        io.noise = _ptr(noise)
    if has_constraints(env) and env.n_surr == 0:
        ninfo["constraint"] = torch.empty(B, env.n_constraint, dtype=torch.float32, device=obs.device)
        io.constraint = _ptr(ninfo["constraint"])
    elif env.kind == ENV_VEH_SURR:
        ninfo["surr_state"] = torch.empty_like(info["surr_state"])
        ninfo["constraint"] = torch.empty(B, env.n_constraint, dtype=torch.float32, device=obs.device)
        io.surr_state, io.next_surr_state = _ptr(info["surr_state"]), _ptr(ninfo["surr_state"])
        io.constraint = _ptr(ninfo["constraint"])
    check(lib().gops_env_step(C.byref(env), B, C.byref(io), _stream()), "gops_env_step")
    return nobs, rew, ndone, ninfo


def env_constraint(env: GopsEnv, obs, info: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """model.get_constraint(obs, info) on the GPU (gops_env_constraint): [B, n_constraint]."""
    B = obs.shape[0]
    io = GopsStepIO()
    out = torch.empty(B, env.n_constraint, dtype=torch.float32, device=obs.device)
    io.obs, io.constraint = _ptr(obs), _ptr(out)
    if info:
        io.state, io.surr_state = _ptr(info.get("state")), _ptr(info.get("surr_state"))
    check(lib().gops_env_constraint(C.byref(env), B, C.byref(io), _stream()), "gops_env_constraint")
    return out


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (default hyper-parameters' semantics) whose `step()` is ONE HIP launch over all
    parameters of a group (`gops_adam_step`).  Same `param_groups` / `state` layout as torch's Adam
    (`step`, `exp_avg`, `exp_avg_sq`), so lr schedulers and optimizer checkpoints are interchangeable.
    The learning rate and step count the kernel uses live in device memory, which makes `step()`
    capturable in a HIP graph: a graph owner calls `sync_hyper()` before and `advance()` after each
    replay.  Parameters must be fp32 CUDA tensors when `step()` is called."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._dev = {}   # group index -> {"state": GopsAdamState device tensors (6 x 8 bytes) per chunk, "lr", "step"}
        # factor applied to every gradient element inside the kernel: 1/N after a SUM all-reduce over N replicas
        # (trainer/grad_sync.py) - the mean costs no separate pass over the gradients
        self.grad_scale = 1.0

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dev = {}   # device mirrors are rebuilt from the loaded host state

    def _prepare(self, gi, group):
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return None, None
        steps = set()
        for p in ps:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            elif st["exp_avg"].device != p.device:   # parameters were moved after the state was made
                st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].to(p.device), st["exp_avg_sq"].to(p.device)
            steps.add(int(st["step"]))
        assert len(steps) == 1, "parameters of one group must share the step count"
        step = steps.pop()
        nchunk = (len(ps) + ADAM_MAX - 1) // ADAM_MAX
        dev = self._dev.get(gi)
        if dev is None or len(dev["state"]) != nchunk or dev["state"][0].device != ps[0].device:
            dev = self._dev[gi] = {"state": [torch.zeros(6, dtype=torch.int64, device=ps[0].device)
                                             for _ in range(nchunk)], "lr": None, "step": None, "gs": None}
        if dev["step"] != step:       # first use, after load_state_dict, or an external edit of state
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HipAdam: device step count out of date while capturing a graph")
            b1, b2 = group["betas"]
            for t in dev["state"]:   # GopsAdamState: lr, step, beta1^step, beta2^step, (ticket, skipped_nonfinite), grad_scale
                t[1] = step
                t.view(torch.float64)[2] = float(b1) ** step
                t.view(torch.float64)[3] = float(b2) ** step
                t.view(torch.int32)[8] = 0   # ticket (the skipped-element counter next to it keeps counting)
            dev["step"] = step
        self._sync_lr(dev, group)
        return ps, dev

    def _sync_lr(self, dev, group):
        lr = float(group["lr"])
        if dev["lr"] != lr:
            for t in dev["state"]:
                t.view(torch.float64)[0] = lr
            dev["lr"] = lr
        gs = float(self.grad_scale)
        if dev.get("gs") != gs:
            for t in dev["state"]:
                t.view(torch.float64)[5] = gs
            dev["gs"] = gs

    def skipped_nonfinite(self) -> int:
        """Gradient elements that were not finite and therefore took no step since the device state was created
        (`GopsAdamState.skipped_nonfinite`, ABI v13: parameter, moments and a fused Polyak target of such an element stay
        untouched).  Reads device memory: one host sync."""
        return sum(int(t.view(torch.int32)[9].item()) & 0xFFFFFFFF for dev in self._dev.values() for t in dev["state"])

    def sync_hyper(self):
        """Push a changed `lr` (schedulers) to the device copies; call before replaying a graph."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev:
                self._sync_lr(self._dev[gi], group)

    def storage_signature(self):
        """Device addresses a captured `step()` has baked in besides parameters and gradients: the Adam moments
        and the device-resident hyper-parameter blocks.  `load_state_dict` (new moment tensors, `_dev` dropped)
        changes it, which makes graph owners re-capture instead of replaying into freed memory."""
        sig = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                st = self.state.get(p, {})
                if len(st):
                    sig.append((st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()))
            if gi in self._dev:
                sig.append(tuple(t.data_ptr() for t in self._dev[gi]["state"]))
        return tuple(sig)

    def resync_device_state(self):
        """Forget the device mirrors of (lr, step, beta powers): the next `step()` re-pushes them from the host
        state.  Used after an aborted graph capture, whose host-side step bookkeeping ran without the kernel."""
        for dev in self._dev.values():
            dev["step"] = dev["lr"] = dev["gs"] = None

    def advance(self, n: int = 1):
        """Account for `n` graph replays of `step()` in the host-side step counters."""
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p in self.state and len(self.state[p]):
                    self.state[p]["step"] = int(self.state[p]["step"]) + n
            if gi in self._dev and self._dev[gi]["step"] is not None:
                self._dev[gi]["step"] += n

    def begin_fused(self):
        """The table / device state / hyper-parameters of THIS step for a caller that folds it into another launch
        (`gops_rollout_backward_update`): `(GopsAdamTensors, state pointer, beta1, beta2, eps, keep-alive)` - or None when the
        optimizer is not one group whose parameters fit one table (the caller then calls `step()` as usual).  Exactly the
        preparation `step()` does; the caller reports the enqueued launch with `end_fused()`."""
        if len(self.param_groups) != 1:
            return None
        group = self.param_groups[0]
        ps, dev = self._prepare(0, group)
        if ps is None or len(ps) > ADAM_MAX or len(ps) != len(group["params"]):
            return None
        t = GopsAdamTensors()
        t.n = len(ps)
        keep = []
        for i, p in enumerate(ps):
            st = self.state[p]
            if not p.grad.is_contiguous():
                return None
            keep.append(p.grad)
            t.numel[i], t.param[i], t.grad[i] = p.numel(), _ptr(p.data), _ptr(p.grad)
            t.exp_avg[i], t.exp_avg_sq[i] = _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"])
        b1, b2 = group["betas"]
        self._fused = (ps, dev)
        return t, dev["state"][0].data_ptr(), float(b1), float(b2), float(group["eps"]), keep

    def end_fused(self):
        """Host-side step bookkeeping of the launch `begin_fused` prepared (what `step()` does after its launch)."""
        ps, dev = self._fused
        self._fused = None
        for p in ps:
            self.state[p]["step"] = int(self.state[p]["step"]) + 1
        dev["step"] += 1

    @torch.no_grad()
    def step(self, closure=None):
        for gi, group in enumerate(self.param_groups):
            ps, dev = self._prepare(gi, group)
            if ps is None:
                continue
            b1, b2 = group["betas"]
            for ci, i0 in enumerate(range(0, len(ps), ADAM_MAX)):
                chunk = ps[i0:i0 + ADAM_MAX]
                t = GopsAdamTensors()
                t.n = len(chunk)
                keep = []
                for i, p in enumerate(chunk):
                    st = self.state[p]
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    keep.append(g)
                    t.numel[i], t.param[i], t.grad[i] = p.numel(), _ptr(p.data), _ptr(g)
                    t.exp_avg[i], t.exp_avg_sq[i] = _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"])
                check(lib().gops_adam_step(C.byref(t), dev["state"][ci].data_ptr(), b1, b2, group["eps"], _stream()),
                      "gops_adam_step")
            for p in ps:
                self.state[p]["step"] = int(self.state[p]["step"]) + 1
            dev["step"] += 1


LOSS_STATS_FLOATS = 260   # include/gops_hip.h: GOPS_LOSS_STATS_FLOATS


class LossStats:
    """Device scalars of a batch in one launch (`gops_value_loss` / `gops_mean_loss`): `stats[0]`, `stats[1]` are the results,
    the rest of the buffer is the kernels' scratch (zero before the first call, left zero by every call)."""

    def __init__(self, device):
        self.buf = torch.zeros(LOSS_STATS_FLOATS, dtype=torch.float32, device=device)

    def value_loss(self, v: torch.Tensor, target: torch.Tensor, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> [mean((v - target)^2), mean(v)]; `grad` <- (2 / n) (v - target) (gops/algorithm/infadp.py:172-173)."""
        n = v.numel()
        check(lib().gops_value_loss(_ptr(v), _ptr(target), n, _ptr(grad), self.buf.data_ptr(), _stream()), "gops_value_loss")
        return self.buf[:2]

    def mean_loss(self, x: torch.Tensor, scale: float = -1.0) -> torch.Tensor:
        """-> [scale * mean(x), mean(x)] (`-v_pi.mean()`: infadp.py:213, fhadp.py:123)."""
        check(lib().gops_mean_loss(_ptr(x), x.numel(), float(scale), self.buf.data_ptr(), _stream()), "gops_mean_loss")
        return self.buf[:2]


AC_LOSS_STATS_FLOATS = 392   # include/gops_hip.h: GOPS_AC_LOSS_STATS_FLOATS


class _BackupBase:
    """What the one-launch backups share: the description's nets (raw pointers, kept alive here), its action limits, the workspace
    with `supported`, and the output tensors of a run."""

    _workspace_fn = None   # name of the entry point that sizes the workspace (0: the kernel does not hold the shape)

    def _init_backup(self, desc, policy: GopsMlp, critics: Sequence[GopsMlp], limits: Dict[str, object], batch: int, device,
                     workspace_bytes: Optional[int]):
        d = self.desc = desc
        self.batch, self.n_q = int(batch), len(critics)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        for name, vals in limits.items():
            _fill(getattr(d, name), np.asarray(vals, dtype=np.float32).reshape(-1)[:MAX_ACT])
        self.set_nets(policy, critics)
        nbytes = getattr(lib(), self._workspace_fn)(C.byref(d), self.batch)
        self.supported = nbytes != 0
        self._workspace_bytes = int(nbytes if workspace_bytes is None else workspace_bytes)
        self.workspace = torch.empty(max(self._workspace_bytes, 1), dtype=torch.uint8, device=self.device)

    def set_nets(self, policy: GopsMlp, critics: Sequence[GopsMlp]):
        assert len(critics) == self.n_q
        C.memmove(C.byref(self.desc.policy), C.byref(policy), C.sizeof(GopsMlp))
        for i, c in enumerate(critics):
            C.memmove(C.byref(self.desc.q[i]), C.byref(c), C.sizeof(GopsMlp))
        self._keep = (policy, list(critics))   # the description holds raw pointers

    def _outputs(self, out: Optional[Dict[str, torch.Tensor]], want, shapes) -> Dict[str, torch.Tensor]:
        """`out`, and a fresh tensor for every output named in `want` that it does not supply."""
        res = dict(out or {})
        for k in want:
            if k not in res:
                res[k] = torch.empty(shapes[k], dtype=torch.float32, device=self.device)
        return res


class AcBackup(_BackupBase):
    """The Bellman backup of a DDPG / TD3 update in ONE launch (`gops_ac_backup`, csrc/actor_critic.hip): target policy with its tanh
    squash, TD3's clipped target noise, one or two target critics on the concatenated input (which never exists in global memory),
    minimum, `rew * reward_scale + gamma * (1 - done) * q`.  `policy` / `critics`: `GopsMlp` views of the TARGET networks (read in
    place at every call).  `supported` is False for a shape the kernel does not hold: the caller then composes the backup from
    `MlpNet.forward` calls; `run` on such a description raises."""

    _workspace_fn = "gops_ac_backup_workspace_bytes"

    def __init__(self, policy: GopsMlp, critics: Sequence[GopsMlp], *, squash_low, squash_high, act_low, act_high, batch: int,
                 smooth: bool, device: Optional[torch.device] = None, workspace_bytes: Optional[int] = None):
        d = GopsAcBackup()
        d.n_q, d.smooth = len(critics), int(bool(smooth))
        self.act_dim = int(policy.sizes[policy.n_layers])
        self._init_backup(d, policy, critics, dict(squash_low=squash_low, squash_high=squash_high, act_low=act_low, act_high=act_high),
                          batch, device, workspace_bytes)

    def run(self, obs2, rew, done, xi=None, *, target_noise=0.0, noise_clip=0.0, reward_scale=1.0, gamma=0.99, want_a2=False,
            want_q=False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """-> {"backup" [B], "a2" [B, A] (want_a2), "q_targ" [n_q, B] (want_q)}; `out` supplies the output tensors instead of fresh
        ones.  Enqueues only."""
        B, d = self.batch, self.desc
        assert obs2.shape[0] == B
        d.target_noise, d.noise_clip, d.reward_scale, d.gamma = float(target_noise), float(noise_clip), float(reward_scale), float(gamma)
        res = self._outputs(out, ("backup",) + (("a2",) if want_a2 else ()) + (("q_targ",) if want_q else ()),
                            dict(backup=(B,), a2=(B, self.act_dim), q_targ=(self.n_q, B)))
        check(lib().gops_ac_backup(C.byref(d), B, _ptr(obs2), _ptr(rew), _ptr(done), _ptr(xi), res["backup"].data_ptr(),
                                   res["a2"].data_ptr() if "a2" in res else None, res["q_targ"].data_ptr() if "q_targ" in res else None,
                                   self.workspace.data_ptr(), self._workspace_bytes, _stream()), "gops_ac_backup")
        return res


class AcCriticLoss:
    """Gradient seeds, losses, mean(q) and |q - backup| of the critic regression in one launch (`gops_ac_critic_loss`).  `buf[:4]` =
    loss_0, loss_1, mean(q_0), loss_0 + loss_1; the rest is the kernel's scratch (zero before the first call, left zero)."""

    def __init__(self, device):
        self.buf = torch.zeros(AC_LOSS_STATS_FLOATS, dtype=torch.float32, device=device)

    def run(self, q: torch.Tensor, backup: torch.Tensor, weight: Optional[torch.Tensor] = None, seed: Optional[torch.Tensor] = None,
            abs_err: Optional[torch.Tensor] = None):
        """q [n_q, B] -> (seed [n_q, B], abs_err [B], stats [4])."""
        n_q, B = q.shape
        seed = torch.empty_like(q) if seed is None else seed
        abs_err = torch.empty(B, dtype=torch.float32, device=q.device) if abs_err is None else abs_err
        check(lib().gops_ac_critic_loss(_ptr(q), _ptr(backup), _ptr(weight), n_q, B, _ptr(seed), _ptr(abs_err), self.buf.data_ptr(),
                                        _stream()), "gops_ac_critic_loss")
        return seed, abs_err, self.buf[:4]


DQN_MAX_ACTIONS = 16           # include/gops_hip.h: GOPS_DQN_MAX_ACTIONS
DQN_LOSS_STATS_FLOATS = 392    # include/gops_hip.h: GOPS_DQN_LOSS_STATS_FLOATS


class DqnBackup:
    """DQN's max-Q backup in ONE launch (`gops_dqn_backup`, csrc/actor_critic.hip): the target ActionValueDis on obs2, the row's
    maximum and arg-max over its `act_num` outputs, `rew * reward_scale + gamma * (1 - done) * max`.  `q`: the `GopsMlp` view of the
    TARGET network (read in place at every call).  `supported` is False for a shape the kernel does not hold: the caller then composes
    the backup from `MlpNet.forward` and `torch.max`; `run` on such a description raises."""

    def __init__(self, q: GopsMlp, *, batch: int, device: Optional[torch.device] = None, workspace_bytes: Optional[int] = None):
        d = self.desc = GopsDqnBackup()
        self.batch = int(batch)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.set_net(q)
        self.act_num = d.act_num = int(q.sizes[q.n_layers])
        nbytes = lib().gops_dqn_backup_workspace_bytes(C.byref(d), self.batch)
        self.supported = nbytes != 0
        self._workspace_bytes = int(nbytes if workspace_bytes is None else workspace_bytes)
        self.workspace = torch.empty(max(self._workspace_bytes, 1), dtype=torch.uint8, device=self.device)

    def set_net(self, q: GopsMlp):
        C.memmove(C.byref(self.desc.q), C.byref(q), C.sizeof(GopsMlp))
        self._keep = q   # the description holds raw pointers

    def run(self, obs2, rew, done, *, reward_scale=1.0, gamma=0.99, want_q=False, want_a=False,
            out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """-> {"backup" [B], "q_targ" [B, act_num] (want_q), "a_star" [B] int32 (want_a)}; `out` supplies the output tensors instead
        of fresh ones.  Enqueues only."""
        B, d = self.batch, self.desc
        assert obs2.shape[0] == B
        d.reward_scale, d.gamma = float(reward_scale), float(gamma)
        res = dict(out or {})
        for k, want, shape, dtype in (("backup", True, (B,), torch.float32), ("q_targ", want_q, (B, self.act_num), torch.float32),
                                      ("a_star", want_a, (B,), torch.int32)):
            if want and k not in res:
                res[k] = torch.empty(shape, dtype=dtype, device=self.device)
        a_star = res.get("a_star")
        assert a_star is None or (a_star.is_cuda and a_star.dtype == torch.int32 and a_star.is_contiguous())
        check(lib().gops_dqn_backup(C.byref(d), B, _ptr(obs2), _ptr(rew), _ptr(done), _ptr(res["backup"]), _ptr(res.get("q_targ")),
                                    None if a_star is None else a_star.data_ptr(), self.workspace.data_ptr(), self._workspace_bytes,
                                    _stream()), "gops_dqn_backup")
        return res


class DqnLoss:
    """The seam between the forward and the backward of DQN's live network in one launch (`gops_dqn_loss`): the dense output-layer
    seed, |q_sel - backup|, and `buf[:3]` = loss, mean(q_sel), rows whose action index is out of range; the rest of `buf` is the
    kernel's scratch (zero before the first call, left zero)."""

    def __init__(self, device):
        self.buf = torch.zeros(DQN_LOSS_STATS_FLOATS, dtype=torch.float32, device=device)

    def run(self, q_all: torch.Tensor, act: torch.Tensor, backup: torch.Tensor, weight: Optional[torch.Tensor] = None,
            seed: Optional[torch.Tensor] = None, abs_err: Optional[torch.Tensor] = None):
        """q_all [B, act_num], act [B] (float indices) -> (seed [B, act_num], abs_err [B], stats [3])."""
        B, N = q_all.shape
        assert act.numel() == B and backup.numel() == B and (weight is None or weight.numel() == B)
        seed = torch.empty_like(q_all) if seed is None else seed
        abs_err = torch.empty(B, dtype=torch.float32, device=q_all.device) if abs_err is None else abs_err
        assert seed.numel() == B * N and abs_err.numel() == B
        check(lib().gops_dqn_loss(_ptr(q_all), _ptr(act), _ptr(backup), _ptr(weight), N, B, _ptr(seed), _ptr(abs_err),
                                  self.buf.data_ptr(), _stream()), "gops_dqn_loss")
        return seed, abs_err, self.buf[:3]


DSACT_STATS_FLOATS = 800        # include/gops_hip.h: GOPS_DSACT_STATS_FLOATS
TANH_GAUSS_STATS_FLOATS = 800   # include/gops_hip.h: GOPS_TANH_GAUSS_STATS_FLOATS


class _SoftBackupBase(_BackupBase):
    def _init_soft(self, desc, policy, critics, act_low, act_high, min_log_std, max_log_std, batch, log_alpha, device, workspace_bytes):
        desc.min_log_std, desc.max_log_std = float(min_log_std), float(max_log_std)
        self.log_alpha = log_alpha
        desc.log_alpha = _ptr(log_alpha)
        self.act_dim = int(policy.sizes[policy.n_layers]) // 2
        self._init_backup(desc, policy, critics, dict(act_low=act_low, act_high=act_high), batch, device, workspace_bytes)


class SoftBackup(_SoftBackupBase):
    """DSAC-T's distributional soft backup in ONE launch (`gops_soft_backup`, csrc/actor_critic.hip): tanh-Gaussian target policy on
    obs2, both target critics' (mean, softplus std) on the concatenated input, minimum, the clipped return sample, entropy term.
    `policy` / `critics`: `GopsMlp` views of the TARGET networks' raw stacks.  `log_alpha`: the device tensor the kernel takes alpha
    from (`exp` inside the kernel), or None for the fixed `alpha` of `run`.  `supported` is False for a shape the kernel does not
    hold; `run` on such a description raises."""

    _workspace_fn = "gops_soft_backup_workspace_bytes"

    def __init__(self, policy: GopsMlp, critics: Sequence[GopsMlp], *, act_low, act_high, min_log_std: float, max_log_std: float,
                 batch: int, log_alpha: Optional[torch.Tensor] = None, device: Optional[torch.device] = None,
                 workspace_bytes: Optional[int] = None):
        assert len(critics) == 2
        self._init_soft(GopsSoftBackup(), policy, critics, act_low, act_high, min_log_std, max_log_std, batch, log_alpha, device,
                        workspace_bytes)

    def run(self, obs2, rew, done, eps_next, z_next, *, gamma=0.99, alpha=0.2, want=(), out: Optional[Dict[str, torch.Tensor]] = None):
        """-> {"target_q" [B], "target_q_sample" [B]} and, named in `want`: "a2" [B, A], "logp" [B], "q_targ" [2, B, 2]; `out` supplies
        output tensors instead of fresh ones.  Enqueues only."""
        B, d = self.batch, self.desc
        assert obs2.shape[0] == B and tuple(z_next.shape) == (2, B)
        d.gamma, d.alpha = float(gamma), float(alpha)
        res = self._outputs(out, ("target_q", "target_q_sample") + tuple(want),
                            dict(target_q=(B,), target_q_sample=(B,), a2=(B, self.act_dim), logp=(B,), q_targ=(2, B, 2)))
        check(lib().gops_soft_backup(C.byref(d), B, _ptr(obs2), _ptr(rew), _ptr(done), _ptr(eps_next), _ptr(z_next), _ptr(res["target_q"]),
                                     _ptr(res["target_q_sample"]), _ptr(res.get("a2")), _ptr(res.get("logp")), _ptr(res.get("q_targ")),
                                     self.workspace.data_ptr(), self._workspace_bytes, _stream()), "gops_soft_backup")
        return res


class DsactCriticLoss:
    """DSAC-T's critic losses, gradient seeds and the running `mean_std` (`gops_dsact_critic_loss`).  `state` = GopsDsactState as four
    32-bit words (mean_std1, mean_std2 as floats, the "initialised" word, a spare one); `buf[:11]` = the statistics, the rest is the
    kernel's scratch (zero before the first call, left zero)."""

    def __init__(self, device):
        self.buf = torch.zeros(DSACT_STATS_FLOATS, dtype=torch.float32, device=device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)

    @property
    def mean_std(self) -> torch.Tensor:
        return self.state.view(torch.float32)[:2]

    def run(self, qraw: torch.Tensor, target_q: torch.Tensor, target_q_sample: torch.Tensor, tau_b: float, seed: Optional[torch.Tensor] = None):
        """qraw [2, B, 2] -> (seed [2, B, 2], stats [11])."""
        B = qraw.shape[1]
        assert tuple(qraw.shape) == (2, B, 2)
        seed = torch.empty_like(qraw) if seed is None else seed
        check(lib().gops_dsact_critic_loss(_ptr(qraw), _ptr(target_q), _ptr(target_q_sample), B, float(tau_b), self.state.data_ptr(),
                                           _ptr(seed), self.buf.data_ptr(), _stream()), "gops_dsact_critic_loss")
        return seed, self.buf[:11]


DSAC_STATS_FLOATS = 264   # include/gops_hip.h: GOPS_DSAC_STATS_FLOATS


class SoftQBackup(_SoftBackupBase):
    """The soft Q backup of a SAC / DSAC update in ONE launch (`gops_soft_q_backup`, csrc/actor_critic.hip): tanh-Gaussian policy on
    obs2 with its log-probability, then one or two scalar critics and their minimum (`distri=False`: SAC), or one critic with a
    (mean, softplus std) head and a clipped return sample (`distri=True`: DSAC), entropy term.  `policy` / `critics`: `GopsMlp` views
    of the networks' raw stacks (read in place at every call).  `log_alpha`: the device tensor the kernel takes alpha from, or None
    for the fixed `alpha` of `run`.  `supported` is False for a shape the kernel does not hold; `run` on such a description raises."""

    _workspace_fn = "gops_soft_q_backup_workspace_bytes"

    def __init__(self, policy: GopsMlp, critics: Sequence[GopsMlp], *, distri: bool, act_low, act_high, min_log_std: float,
                 max_log_std: float, batch: int, log_alpha: Optional[torch.Tensor] = None, device: Optional[torch.device] = None,
                 workspace_bytes: Optional[int] = None):
        d = GopsSoftQBackup()
        self.distri = bool(distri)
        d.n_q, d.distri = len(critics), int(self.distri)
        self._init_soft(d, policy, critics, act_low, act_high, min_log_std, max_log_std, batch, log_alpha, device, workspace_bytes)

    def run(self, obs2, rew, done, eps_next, z_next=None, *, gamma=0.99, alpha=0.2, want=(), out: Optional[Dict[str, torch.Tensor]] = None):
        """-> {"backup" [B]} and, named in `want`: "a2" [B, A], "logp" [B], "q_targ" ([n_q, B], or [B, 2] = (m, s) with `distri`);
        `out` supplies output tensors instead of fresh ones.  Enqueues only."""
        B, d = self.batch, self.desc
        assert obs2.shape[0] == B and (z_next is None or tuple(z_next.shape) == (B,))
        d.gamma, d.alpha = float(gamma), float(alpha)
        res = self._outputs(out, ("backup",) + tuple(want),
                            dict(backup=(B,), a2=(B, self.act_dim), logp=(B,), q_targ=(B, 2) if self.distri else (self.n_q, B)))
        check(lib().gops_soft_q_backup(C.byref(d), B, _ptr(obs2), _ptr(rew), _ptr(done), _ptr(eps_next), _ptr(z_next), _ptr(res["backup"]),
                                       _ptr(res.get("a2")), _ptr(res.get("logp")), _ptr(res.get("q_targ")), self.workspace.data_ptr(),
                                       self._workspace_bytes, _stream()), "gops_soft_q_backup")
        return res


class DsacCriticLoss:
    """DSAC's critic loss and its gradient seeds (`gops_dsac_critic_loss`).  `buf[:4]` = loss, mean(q), mean(std), td_bound; the rest
    is the kernel's scratch (zero before the first call, left zero)."""

    def __init__(self, device):
        self.buf = torch.zeros(DSAC_STATS_FLOATS, dtype=torch.float32, device=device)

    def run(self, qraw: torch.Tensor, target_q: torch.Tensor, bound: bool, seed: Optional[torch.Tensor] = None):
        """qraw [B, 2] -> (seed [B, 2], stats [4])."""
        B = qraw.shape[0]
        assert tuple(qraw.shape) == (B, 2)
        seed = torch.empty_like(qraw) if seed is None else seed
        check(lib().gops_dsac_critic_loss(_ptr(qraw), _ptr(target_q), B, int(bool(bound)), _ptr(seed), self.buf.data_ptr(), _stream()),
              "gops_dsac_critic_loss")
        return seed, self.buf[:4]


class TanhGaussHead:
    """StochaPolicy's sampling head and its reverse (`gops_tanh_gauss_forward / _backward`): raw head [B, 2 A] and draws eps [B, A] ->
    action, log-probability and `buf[:4]` = mean(logp), mean(tanh(mean)), mean(std), -(mean(logp) + target_entropy)."""

    def __init__(self, act_low, act_high, min_log_std: float, max_log_std: float, device):
        d = self.desc = GopsTanhGauss()
        low = np.asarray(act_low, dtype=np.float32).reshape(-1)
        d.act_dim = self.act_dim = len(low)
        _fill(d.act_low, low[:MAX_ACT])
        _fill(d.act_high, np.asarray(act_high, dtype=np.float32).reshape(-1)[:MAX_ACT])
        d.min_log_std, d.max_log_std = float(min_log_std), float(max_log_std)
        self.buf = torch.zeros(TANH_GAUSS_STATS_FLOATS, dtype=torch.float32, device=device)

    def forward(self, head, eps, target_entropy: float = 0.0, act=None, logp=None):
        B = head.shape[0]
        act = torch.empty(B, self.act_dim, dtype=torch.float32, device=head.device) if act is None else act
        logp = torch.empty(B, dtype=torch.float32, device=head.device) if logp is None else logp
        check(lib().gops_tanh_gauss_forward(C.byref(self.desc), B, _ptr(head), _ptr(eps), float(target_entropy), _ptr(act), _ptr(logp),
                                            self.buf.data_ptr(), _stream()), "gops_tanh_gauss_forward")
        return act, logp, self.buf[:4]

    def backward(self, head, eps, g_act, g_logp, g_head=None):
        B = head.shape[0]
        g_head = torch.empty_like(head) if g_head is None else g_head
        check(lib().gops_tanh_gauss_backward(C.byref(self.desc), B, _ptr(head), _ptr(eps), _ptr(g_act), _ptr(g_logp), _ptr(g_head),
                                             _stream()), "gops_tanh_gauss_backward")
        return g_head


PPO_STATS_FLOATS = 656   # include/gops_hip.h: GOPS_PPO_STATS_FLOATS
PPO_HYPER_FLOATS = 8     # include/gops_hip.h: GOPS_PPO_HYPER_FLOATS
ADV_STATS_FLOATS = 264   # include/gops_hip.h: GOPS_ADV_STATS_FLOATS


class PpoLoss:
    """PPO's losses and their gradient seeds for one minibatch in one launch (`gops_ppo_loss`, csrc/ppo.hip).  `buf[:6]` = loss_total,
    loss_surrogate, loss_value, mean entropy, mean kl, clip fraction; the rest is the kernel's scratch (zero before the first call,
    ticket left zero).  `hyper` (device): clip, value_clip, c_kl, c_v, c_ent - the kernel reads them there, so `set_hyper` between
    two replays of a captured graph takes effect."""

    def __init__(self, act_dim: int, min_log_std: float, max_log_std: float, device, loss_value_clip=True, loss_value_norm=False):
        d = self.desc = GopsPpoLoss()
        d.act_dim = self.act_dim = int(act_dim)
        d.loss_value_clip, d.loss_value_norm = int(bool(loss_value_clip)), int(bool(loss_value_norm))
        d.min_log_std, d.max_log_std = float(min_log_std), float(max_log_std)
        self.buf = torch.zeros(PPO_STATS_FLOATS, dtype=torch.float32, device=device)
        self.hyper = torch.zeros(PPO_HYPER_FLOATS, dtype=torch.float32, device=device)
        self._hyper = None

    def set_hyper(self, clip: float, value_clip: float, c_kl: float, c_v: float, c_ent: float):
        vals = (float(clip), float(value_clip), float(c_kl), float(c_v), float(c_ent))
        if vals != self._hyper:   # (a host-to-device copy: never inside a capture - graph owners call this before the replay)
            self.hyper[:5].copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper = vals

    def run(self, head_new, v_new, act, logp_old, adv, ret, val_old, logits_old, seed_head=None, seed_v=None):
        """head_new [M, 2A] raw, v_new [M] -> (seed_head [M, 2A], seed_v [M], stats [6])."""
        M, A = head_new.shape[0], self.act_dim
        assert tuple(head_new.shape) == (M, 2 * A) and tuple(logits_old.shape) == (M, 2 * A) and act.numel() == M * A
        assert all(t.numel() == M for t in (v_new, logp_old, adv, ret, val_old))
        seed_head = torch.empty_like(head_new) if seed_head is None else seed_head
        seed_v = torch.empty(M, dtype=torch.float32, device=head_new.device) if seed_v is None else seed_v
        assert seed_head.numel() == 2 * M * A and seed_v.numel() == M
        check(lib().gops_ppo_loss(C.byref(self.desc), M, _ptr(head_new), _ptr(v_new), _ptr(act), _ptr(logp_old), _ptr(adv), _ptr(ret),
                                  _ptr(val_old), _ptr(logits_old), self.hyper.data_ptr(), _ptr(seed_head), _ptr(seed_v),
                                  self.buf.data_ptr(), _stream()), "gops_ppo_loss")
        return seed_head, seed_v, self.buf[:6]


class AdvNormalize:
    """`(adv - mean) / (std + eps)` with the unbiased std in one launch (`gops_adv_normalize`); `buf[:2]` = mean, std."""

    def __init__(self, device):
        self.buf = torch.zeros(ADV_STATS_FLOATS, dtype=torch.float32, device=device)

    def run(self, adv: torch.Tensor, eps: float = 1e-8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = torch.empty_like(adv) if out is None else out
        assert out.numel() == adv.numel()
        check(lib().gops_adv_normalize(_ptr(adv), adv.numel(), float(eps), _ptr(out), self.buf.data_ptr(), _stream()), "gops_adv_normalize")
        return out


def gae(rew, val, val_next, done, end, gamma: float = 0.99, gae_lambda: float = 0.95, ret=None, adv=None):
    """Value targets and generalised advantages of all environments in one launch (`gops_gae`): time-major [T, N] fp32 tensors ->
    (ret, adv) [T, N]."""
    T, N = rew.shape
    assert all(tuple(t.shape) == (T, N) for t in (val, val_next, done, end))
    ret = torch.empty_like(rew) if ret is None else ret
    adv = torch.empty_like(rew) if adv is None else adv
    assert ret.numel() == T * N and adv.numel() == T * N
    check(lib().gops_gae(_ptr(rew), _ptr(val), _ptr(val_next), _ptr(done), _ptr(end), T, N, float(gamma), float(gae_lambda), _ptr(ret),
                         _ptr(adv), _stream()), "gops_gae")
    return ret, adv


TRPO_STATS_FLOATS = 264   # include/gops_hip.h: GOPS_TRPO_STATS_FLOATS
TRPO_HYPER_FLOATS = 4     # include/gops_hip.h: GOPS_TRPO_HYPER_FLOATS
CG_STATE_FLOATS = 272     # include/gops_hip.h: GOPS_CG_STATE_FLOATS (sizeof(GopsCgState) / 4)
CG_ONE_BLOCK_MAX = 8192   # include/gops_hip.h: GOPS_CG_ONE_BLOCK_MAX


class GopsCgState(C.Structure):   # gops_cg_init / _step / _finish
    _fields_ = [("r_dot", C.c_double), ("p_ap", C.c_double), ("alpha", C.c_double), ("beta", C.c_double), ("g_x", C.c_double),
                ("scale", C.c_double), ("done", C.c_int32), ("calls", C.c_int32), ("iterations", C.c_int32), ("ticket", C.c_int32),
                ("part", C.c_double * 128)]


def flat_views(flat: torch.Tensor, shapes) -> List[torch.Tensor]:
    """Consecutive views of the flat vector `flat` with `shapes`: `parameters_to_vector`'s order when `shapes` are the parameters'."""
    out, at = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(flat[at:at + n].view(*shape))
        at += n
    assert at == flat.numel()
    return out


class FisherSeed:
    """`gops_gauss_fisher_seed` (csrc/trpo.hip): seed [B, 2A] = (1/B) M (J v) of a Gaussian `mlp_shared` policy, v given as per-layer
    tensors (or views of one flat vector) in the weights' layout.  `MlpNet.backward(x, seed, ...)` then yields the Fisher-vector
    product.  The policy's weights are read in place at every call."""

    def __init__(self, mlp: GopsMlp, min_log_std: float, max_log_std: float, device):
        self.mlp, self.device = mlp, device
        self.out_dim = int(mlp.sizes[mlp.n_layers])
        self.min_log_std, self.max_log_std = float(min_log_std), float(max_log_std)

    def run(self, x: torch.Tensor, tangent_w, tangent_b, seed: Optional[torch.Tensor] = None) -> torch.Tensor:
        B = x.shape[0]
        seed = torch.empty(B, self.out_dim, dtype=torch.float32, device=x.device) if seed is None else seed
        assert seed.numel() == B * self.out_dim and x.numel() == B * int(self.mlp.sizes[0])
        assert len(tangent_w) == len(tangent_b) == self.mlp.n_layers
        for j, (w, b) in enumerate(zip(tangent_w, tangent_b)):
            assert w.numel() == int(self.mlp.sizes[j]) * int(self.mlp.sizes[j + 1]) and b.numel() == int(self.mlp.sizes[j + 1])
        self._launch(make_mlp_grad(tangent_w, tangent_b), B, x, seed)
        return seed

    def _launch(self, t: GopsMlpGrad, B: int, x, seed):
        check(lib().gops_gauss_fisher_seed(C.byref(self.mlp), C.byref(t), B, _ptr(x), self.min_log_std, self.max_log_std, _ptr(seed),
                                           _stream()), "gops_gauss_fisher_seed")


class CatFisherSeed(FisherSeed):
    """`gops_cat_fisher_seed`: seed [B, n] = (1/B) (diag(p) - p p^T) (J v) of a categorical policy over n action indices,
    p = softmax(logits) - `FisherSeed`'s call surface."""

    def __init__(self, mlp: GopsMlp, device):
        self.mlp, self.device = mlp, device
        self.out_dim = int(mlp.sizes[mlp.n_layers])

    def _launch(self, t: GopsMlpGrad, B: int, x, seed):
        check(lib().gops_cat_fisher_seed(C.byref(self.mlp), C.byref(t), B, _ptr(x), _ptr(seed), _stream()), "gops_cat_fisher_seed")


class _SurrogateState:
    """What both surrogate kernels keep on the device: `buf` (`buf[:2]` = surrogate, kl; `verdict`, int32 view of `buf[2]` =
    surrogate > 0 and kl < delta) and `hyper` (delta, read by the kernel)."""

    def __init__(self, device):
        self.buf = torch.zeros(TRPO_STATS_FLOATS, dtype=torch.float32, device=device)
        self.hyper = torch.zeros(TRPO_HYPER_FLOATS, dtype=torch.float32, device=device)
        self.verdict = self.buf.view(torch.int32)[2:3]
        self._delta = None

    def set_delta(self, delta: float):
        if float(delta) != self._delta:   # (a host-to-device copy: never inside a capture)
            self.hyper[:1].copy_(torch.tensor([float(delta)], dtype=torch.float32))
            self._delta = float(delta)

    def flags(self):
        """(verdict, rows left out for their action index - always 0 for the Gaussian kernel) of the last call, in ONE read."""
        verdict, bad = self.buf.view(torch.int32)[2:4].tolist()
        return verdict != 0, bad


class TrpoSurrogate(_SurrogateState):
    """TRPO's surrogate advantage, mean KL(new || old), the surrogate's gradient seed and the line search's verdict in one launch
    (`gops_trpo_surrogate`).  `buf[:2]` = surrogate, kl; `verdict` (int32 view of `buf[2]`) = surrogate > 0 and kl < delta; `hyper`
    (device): delta, read by the kernel."""

    def __init__(self, act_dim: int, min_log_std: float, max_log_std: float, device):
        super().__init__(device)
        self.act_dim, self.min_log_std, self.max_log_std = int(act_dim), float(min_log_std), float(max_log_std)

    def run(self, head_new, head_old, act, adv, seed_head=None, want_seed=True):
        """head_new, head_old [M, 2A] raw (may be the same tensor) -> (seed_head [M, 2A] or None, stats [2])."""
        M, A = head_new.shape[0], self.act_dim
        assert tuple(head_new.shape) == (M, 2 * A) and head_old.numel() == 2 * M * A and act.numel() == M * A and adv.numel() == M
        if want_seed and seed_head is None:
            seed_head = torch.empty_like(head_new)
        assert seed_head is None or seed_head.numel() == 2 * M * A
        check(lib().gops_trpo_surrogate(A, M, self.min_log_std, self.max_log_std, _ptr(head_new), _ptr(head_old), _ptr(act), _ptr(adv),
                                        self.hyper.data_ptr(), _ptr(seed_head) if want_seed else None, self.buf.data_ptr(), _stream()),
              "gops_trpo_surrogate")
        return (seed_head if want_seed else None), self.buf[:2]


class CatTrpoSurrogate(_SurrogateState):
    """The same for a categorical policy over `act_num` action indices, from the logits (`gops_cat_trpo_surrogate`) -
    `TrpoSurrogate`'s call surface, and `bad_index` (int32 view of `buf[3]`): the rows of the last call whose index in `act` lies
    outside [0, act_num); they are left out of both means and get a zero seed row."""

    def __init__(self, act_num: int, device):
        super().__init__(device)
        self.act_num = int(act_num)
        self.bad_index = self.buf.view(torch.int32)[3:4]

    def run(self, head_new, head_old, act, adv, seed_head=None, want_seed=True):
        """head_new, head_old [M, n] logits (may be the same tensor), act [M] or [M, 1] indices as floats -> (seed_head [M, n] or
        None, stats [2])."""
        M, N = head_new.shape[0], self.act_num
        assert tuple(head_new.shape) == (M, N) and head_old.numel() == M * N and act.numel() == M and adv.numel() == M
        if want_seed and seed_head is None:
            seed_head = torch.empty_like(head_new)
        assert seed_head is None or seed_head.numel() == M * N
        check(lib().gops_cat_trpo_surrogate(N, M, _ptr(head_new), _ptr(head_old), _ptr(act), _ptr(adv), self.hyper.data_ptr(),
                                            _ptr(seed_head) if want_seed else None, self.buf.data_ptr(), _stream()),
              "gops_cat_trpo_surrogate")
        return (seed_head if want_seed else None), self.buf[:2]


class CgSolver:
    """`_conjugate_gradient` of the reference's TRPO (trpo.py:226-267) on the device (`gops_cg_init / _step / _finish`): owns the
    flat fp32 vectors `g, x, r, p, Ap, step` of `n` elements and the state block (`GopsCgState`); the caller writes the undamped
    product into `Ap` between `init` / `step` calls and reads nothing on the host.  `hyper` (device): delta, for `finish`."""

    def __init__(self, n: int, device, hyper: Optional[torch.Tensor] = None):
        self.n = int(n)
        vec = torch.zeros(6, self.n, dtype=torch.float32, device=device)
        self.g, self.x, self.r, self.p, self.Ap, self.step_vec = vec.unbind(0)
        self._state = torch.zeros(CG_STATE_FLOATS // 2, dtype=torch.float64, device=device)   # (8-byte aligned)
        self.hyper = torch.zeros(TRPO_HYPER_FLOATS, dtype=torch.float32, device=device) if hyper is None else hyper

    def init(self, atol: float):
        check(lib().gops_cg_init(_ptr(self.g), _ptr(self.x), _ptr(self.r), _ptr(self.p), self.n, float(atol), self._state.data_ptr(),
                                 _stream()), "gops_cg_init")

    def step(self, damping: float, atol: float):
        check(lib().gops_cg_step(_ptr(self.p), _ptr(self.Ap), _ptr(self.x), _ptr(self.r), self.n, float(damping), float(atol),
                                 self._state.data_ptr(), _stream()), "gops_cg_step")

    def finish(self):
        check(lib().gops_cg_finish(_ptr(self.g), _ptr(self.x), _ptr(self.step_vec), self.n, self.hyper.data_ptr(), self._state.data_ptr(),
                                   _stream()), "gops_cg_finish")

    def state(self) -> Dict[str, float]:
        """The state block's fields on the host (one synchronisation)."""
        raw = GopsCgState.from_buffer_copy(self._state.cpu().numpy().tobytes())
        return {name: getattr(raw, name) for name, _ in GopsCgState._fields_[:9]}


# gops_mpc_* (include/gops_hip.h: GOPS_MPC_*)
MPC_MAX_DIM, MPC_MAX_HISTORY, MPC_HYPER_FLOATS, MPC_SCALARS, MPC_COUNTERS, MPC_VECTORS = 256, 8, 8, 5, 8, 6
MPC_RUNNING, MPC_CONVERGED_PG, MPC_CONVERGED_F, MPC_LINE_SEARCH, MPC_NONFINITE = range(5)
MPC_FROZEN = 5   # gops_mpc_advance: the row's episode has ended
MPC_STATUS_NAMES = ("running", "converged_pg", "converged_f", "line_search", "nonfinite", "frozen")
# c1, shrink, max_ls, pgtol, ftol (scipy's L-BFGS-B: pgtol 1e-5, ftol = factr epsmch = 1e7 * 2.22e-16), curv_eps (its epsmch)
MPC_HYPER_DEFAULTS = dict(c1=1e-4, shrink=0.5, max_ls=20, pgtol=1e-5, ftol=2.220446049250313e-9, curv_eps=2.220446049250313e-16)
# gops_mpc_al_* (GOPS_MPC_AL_*): the outer status words and the augmented Lagrangian's hyper-parameters
MPC_AL_HYPER_FLOATS, MPC_AL_COUNTERS, MPC_AL_MAX_H, MAX_CONSTRAINT = 8, 4, 65536, 3
MPC_AL_RUNNING, MPC_AL_CONVERGED, MPC_AL_MAX_OUTER = range(3)
MPC_AL_STATUS_NAMES = ("running", "converged", "max_outer")
MPC_AL_HYPER_DEFAULTS = dict(rho0=10.0, growth=10.0, rho_max=1e6, shrink_target=0.25, cstr_tol=1e-4, max_outer=30, lambda_tol=1e-4)


class MpcSolver:
    """`batch` box-constrained L-BFGS problems of `n` variables side by side on the device (`gops_mpc_init / _step / _finish`,
    csrc/mpc_lbfgs.hip): owns the state block, `x_trial [batch, n]` (where the caller evaluates), `f [batch]` and `g [batch, n]`
    (where the caller leaves cost and gradient before `step`) and `hyper` (device: tolerances, `set_hyper`).  Nothing is read on the
    host except by `finish` / `state`.

    `constraints=(H, n_c)`: the solver also owns the augmented-Lagrangian state of H n_c path constraints per row (`gops_mpc_al_eval /
    _update / _advance`): `lam [batch, H, n_c]`, `rho`, `viol`, `viol_prev`, `f_al_in [batch]` (where the caller leaves the ROLLOUT
    cost before `al_eval`, which writes the objective into `f`), `seed [H, batch, n_c]`, `outer [batch, 4]` int32 and `al_hyper`."""

    def __init__(self, batch: int, n: int, lo, hi, device, history: int = 8, constraints: Optional[Tuple[int, int]] = None):
        self.batch, self.n, self.m = int(batch), int(n), int(history)
        nbytes = lib().gops_mpc_state_bytes(self.batch, self.n, self.m)
        if nbytes == 0:
            raise RuntimeError(f"MpcSolver: batch {batch}, n {n}, history {history} is outside 1 <= n <= {MPC_MAX_DIM}, "
                               f"1 <= history <= {MPC_MAX_HISTORY}, batch >= 1")
        self.state_bytes = nbytes
        self._state = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=device)   # (8-byte aligned)
        bound = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1).expand(self.n).contiguous().to(device)
        self.lo, self.hi = bound(lo), bound(hi)
        self.x_trial = torch.zeros(self.batch, self.n, dtype=torch.float32, device=device)
        self.f = torch.zeros(self.batch, dtype=torch.float32, device=device)
        self.g = torch.zeros(self.batch, self.n, dtype=torch.float32, device=device)
        self.x = torch.zeros(self.batch, self.n, dtype=torch.float32, device=device)
        self.f_best = torch.zeros(self.batch, dtype=torch.float32, device=device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.iterations = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.hyper = torch.zeros(MPC_HYPER_FLOATS, dtype=torch.float32, device=device)
        self.set_hyper()
        self.constraints = None
        if constraints is not None:
            H, nc = (int(v) for v in constraints)
            if not (1 <= H <= MPC_AL_MAX_H and 1 <= nc <= MAX_CONSTRAINT):
                raise RuntimeError(f"MpcSolver: constraints {constraints} is outside 1 <= H <= {MPC_AL_MAX_H}, 1 <= n_c <= {MAX_CONSTRAINT}")
            self.constraints = (H, nc)
            f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)
            self.lam, self._lam_next, self.seed = f32(self.batch, H, nc), f32(self.batch, H, nc), f32(H, self.batch, nc)
            self.rho, self.viol, self.viol_prev, self.f_al_in = (f32(self.batch) for _ in range(4))
            self.outer = torch.zeros(self.batch, MPC_AL_COUNTERS, dtype=torch.int32, device=device)
            self.al_hyper = f32(MPC_AL_HYPER_FLOATS)
            self.al_hyper_host = dict(MPC_AL_HYPER_DEFAULTS)
            self.set_al_hyper()
            self.al_reset()

    def set_al_hyper(self, **kw):
        """rho0, growth, rho_max, shrink_target, cstr_tol, max_outer, lambda_tol (MPC_AL_HYPER_DEFAULTS for the ones not given): one
        small host-to-device copy.  `al_reset` / `al_advance` put rho back to rho0."""
        unknown = set(kw) - set(MPC_AL_HYPER_DEFAULTS)
        if unknown:
            raise RuntimeError(f"MpcSolver.set_al_hyper: unknown {sorted(unknown)}")
        h = dict(MPC_AL_HYPER_DEFAULTS, **kw)
        self.al_hyper_host = h
        vals = [h[k] for k in ("rho0", "growth", "rho_max", "shrink_target", "cstr_tol", "max_outer", "lambda_tol")] + [0.0]
        self.al_hyper.copy_(torch.tensor(vals, dtype=torch.float32))

    def al_reset(self):
        """Multipliers 0, rho = rho0, viol_prev = +inf, outer words cleared: the start of a solve (element-wise fills, no host read)."""
        self.lam.zero_(), self.viol.zero_(), self.outer.zero_()
        self.rho.fill_(float(self.al_hyper_host["rho0"])), self.viol_prev.fill_(float("inf"))

    def _al_dims(self):
        assert self.constraints is not None, "MpcSolver was made without constraints=(H, n_c)"
        return self.constraints

    def al_eval(self, c: torch.Tensor):
        """`f`, `seed`, `viol` <- the augmented Lagrangian of the rollout cost in `f_al_in` and the constraint values c [H, batch, n_c]
        at the trial point (gops_mpc_al_eval): call between the rollout forward and its backward, then `step`."""
        H, nc = self._al_dims()
        assert c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (H, self.batch, nc)
        check(lib().gops_mpc_al_eval(self.batch, H, nc, _ptr(c), _ptr(self.lam), _ptr(self.rho), _ptr(self.f_al_in), _ptr(self.f),
                                     _ptr(self.seed), _ptr(self.viol), _stream()), "gops_mpc_al_eval")

    def al_update(self, c: torch.Tensor):
        """The outer step (gops_mpc_al_update) with c [H, batch, n_c] and `viol` those of the rows' ACCEPTED points: rows whose inner
        solve has ended get their multipliers and rho updated and are re-armed, converged or out of outer iterations."""
        H, nc = self._al_dims()
        assert c.dtype == torch.float32 and c.is_contiguous() and tuple(c.shape) == (H, self.batch, nc)
        check(lib().gops_mpc_al_update(*self._args(), H, nc, _ptr(c), _ptr(self.lam), _ptr(self.rho), _ptr(self.viol), _ptr(self.viol_prev),
                                       self.outer.data_ptr(), _ptr(self.al_hyper), _stream()), "gops_mpc_al_update")

    def al_advance(self, frozen: torch.Tensor, action_out: torch.Tensor, record: torch.Tensor, shift: int = 1):
        """`advance` plus the multipliers' hand-over (gops_mpc_al_advance): shifted by `shift` env steps (one control interval) with
        zeros entering at the end, rho back to rho0, outer words cleared; frozen rows keep theirs."""
        H, nc = self._al_dims()
        assert frozen.dtype == torch.float32 and frozen.numel() == self.batch and record.dtype == torch.int32 and record.numel() == 4 * self.batch
        assert action_out.dtype == torch.float32 and action_out.is_contiguous() and action_out.numel() % self.batch == 0
        check(lib().gops_mpc_al_advance(*self._args(), action_out.numel() // self.batch, _ptr(frozen), _ptr(action_out), record.data_ptr(),
                                        _ptr(self.x_trial), H, nc, int(shift), _ptr(self.lam), _ptr(self._lam_next), _ptr(self.rho),
                                        _ptr(self.viol_prev), self.outer.data_ptr(), _ptr(self.al_hyper), _stream()), "gops_mpc_al_advance")
        self.lam, self._lam_next = self._lam_next, self.lam

    def set_hyper(self, **kw):
        """c1, shrink, max_ls, pgtol, ftol, curv_eps (MPC_HYPER_DEFAULTS for the ones not given): one small host-to-device copy."""
        unknown = set(kw) - set(MPC_HYPER_DEFAULTS)
        if unknown:
            raise RuntimeError(f"MpcSolver.set_hyper: unknown {sorted(unknown)}")
        h = dict(MPC_HYPER_DEFAULTS, **kw)
        vals = [h[k] for k in ("c1", "shrink", "max_ls", "pgtol", "ftol", "curv_eps")] + [0.0, 0.0]
        self.hyper.copy_(torch.tensor(vals, dtype=torch.float32))

    def _args(self):
        return self._state.data_ptr(), self.state_bytes, self.batch, self.n, self.m

    def init(self, x0: torch.Tensor):
        check(lib().gops_mpc_init(*self._args(), _ptr(x0), _ptr(self.lo), _ptr(self.hi), _ptr(self.x_trial), _stream()), "gops_mpc_init")

    def step(self):
        check(lib().gops_mpc_step(*self._args(), _ptr(self.f), _ptr(self.g), _ptr(self.x_trial), _ptr(self.hyper), _stream()),
              "gops_mpc_step")

    def finish(self):
        """-> (x [batch, n], f [batch], status [batch] int32, iterations [batch] int32): the accepted points, on the device; with
        `constraints` additionally (viol [batch], outer status [batch] int32 (MPC_AL_*), outer iterations [batch] int32) - the
        violation of the last `al_eval`, views of `outer`."""
        check(lib().gops_mpc_finish(*self._args(), _ptr(self.x), _ptr(self.f_best), self.status.data_ptr(), self.iterations.data_ptr(),
                                    _stream()), "gops_mpc_finish")
        if self.constraints is not None:
            return self.x, self.f_best, self.status, self.iterations, self.viol, self.outer[:, 0], self.outer[:, 1]
        return self.x, self.f_best, self.status, self.iterations

    def advance(self, frozen: torch.Tensor, action_out: torch.Tensor, record: torch.Tensor):
        """The hand-over between two solves of a closed loop, one launch (gops_mpc_advance): `action_out` [batch, act_dim] <- the
        first control point of every row's accepted point (0 where `frozen` [batch] float is non-zero), the block re-initialised
        from the plan shifted by one control point as `init` would (frozen rows: status MPC_FROZEN, never stepped again), `x_trial`
        ready for the next evaluation; `record` [batch, 4] int32: last status, summed iterations, summed evaluations, solves."""
        assert frozen.dtype == torch.float32 and frozen.numel() == self.batch and record.dtype == torch.int32 and record.numel() == 4 * self.batch
        assert action_out.dtype == torch.float32 and action_out.is_contiguous() and action_out.numel() % self.batch == 0
        check(lib().gops_mpc_advance(*self._args(), action_out.numel() // self.batch, _ptr(frozen), _ptr(action_out), record.data_ptr(),
                                     _ptr(self.x_trial), _stream()), "gops_mpc_advance")

    def status_words(self) -> torch.Tensor:
        """The status words of the state block as a strided int32 view [batch] (device; written by element-wise torch operations)."""
        first = 2 * self.batch * (MPC_SCALARS + self.m)
        return self._state.view(torch.int32)[first:first + self.batch * MPC_COUNTERS].view(self.batch, MPC_COUNTERS)[:, 0]

    def state(self) -> Dict[str, np.ndarray]:
        """The state block's sections on the host (one synchronisation), named as in include/gops_hip.h."""
        return mpc_decode_state(self._state.cpu().numpy().tobytes(), self.batch, self.n, self.m)


def mpc_decode_state(raw: bytes, B: int, n: int, m: int) -> Dict[str, np.ndarray]:
    nd, ni, nb = B * (MPC_SCALARS + m), B * MPC_COUNTERS, 2 * ((n + 1) // 2 * 2)
    sc = np.frombuffer(raw, np.float64, nd).reshape(B, MPC_SCALARS + m)
    ct = np.frombuffer(raw, np.int32, ni, 8 * nd).reshape(B, MPC_COUNTERS)
    bounds = np.frombuffer(raw, np.float32, nb, 8 * nd + 4 * ni).reshape(2, nb // 2)[:, :n]
    vec = np.frombuffer(raw, np.float32, B * (MPC_VECTORS + 2 * m) * n, 8 * nd + 4 * ni + 4 * nb).reshape(B, MPC_VECTORS + 2 * m, n)
    out = dict(zip(("f", "f_prev", "alpha", "dphi", "gamma"), sc[:, :MPC_SCALARS].T.copy()), rho=sc[:, MPC_SCALARS:].copy())
    out.update(zip(("status", "iterations", "evaluations", "ls_count", "head", "count"), ct.T.copy()))
    out.update(lo=bounds[0].copy(), hi=bounds[1].copy())
    out.update(zip(("x", "g", "x_prev", "g_prev", "d", "x_trial"), vec[:, :MPC_VECTORS].transpose(1, 0, 2).copy()))
    out.update(s=vec[:, MPC_VECTORS:MPC_VECTORS + m].copy(), y=vec[:, MPC_VECTORS + m:].copy())
    return out


def make_update_tail(fused_adam=None, mean_of: Optional[torch.Tensor] = None, mean_scale: float = -1.0,
                     stats: Optional["LossStats"] = None, polyak: Optional["PolyakUpdater"] = None, tau: float = 0.0) -> "GopsUpdateTail":
    """`GopsUpdateTail` for `Rollout.backward(..., tail=)` / `ValueNet.backward(..., tail=)`: `fused_adam` = what
    `HipAdam.begin_fused()` returned (or None), `mean_of` / `stats`: the values whose mean lands in `stats.buf[:2]` as `gops_mean_loss`
    would leave it, `polyak` / `tau`: the target-network averaging of the stepped network (a one-table `PolyakUpdater`).  The
    returned struct keeps the tensors it points to alive."""
    t = GopsUpdateTail()
    keep = []
    if fused_adam is not None:
        table, state_ptr, b1, b2, eps, kp = fused_adam
        t.adam = C.pointer(table)
        t.adam_state, t.beta1, t.beta2, t.eps = state_ptr, b1, b2, eps
        keep += [table, kp]
    if mean_of is not None:
        t.mean_x, t.mean_n, t.mean_scale, t.mean_stats = _ptr(mean_of), mean_of.numel(), float(mean_scale), stats.buf.data_ptr()
        keep += [mean_of, stats]
    if polyak is not None:
        assert fused_adam is not None and len(polyak.tables) == 1
        t.polyak, t.polyak_tau = C.pointer(polyak.tables[0]), float(tau)
        keep.append(polyak)
    t._keep = keep
    return t


class PolyakUpdater:
    """target <- (1 - tau) target + tau online for all tensors of a network in one launch (`gops_polyak_update`; chunks of
    GOPS_ADAM_MAX_TENSORS), the same two roundings per element as the reference's `mul_` / `add_` passes (infadp.py:124-133)."""

    def __init__(self, target_params, online_params):
        tp, op = list(target_params), list(online_params)
        assert len(tp) == len(op)
        self._keep = (tp, op)
        self._sig = tuple((t.data_ptr(), o.data_ptr(), t.numel()) for t, o in zip(tp, op))
        self.tables = []
        for c0 in range(0, len(tp), ADAM_MAX):
            t = GopsAdamTensors()
            chunk = list(zip(tp[c0:c0 + ADAM_MAX], op[c0:c0 + ADAM_MAX]))
            t.n = len(chunk)
            for i, (a, b) in enumerate(chunk):
                assert a.shape == b.shape
                t.numel[i] = a.numel()
                t.param[i], t.grad[i] = _ptr(a.data), _ptr(b.data)
            self.tables.append(t)

    def matches(self, target_params, online_params) -> bool:
        return self._sig == tuple((t.data_ptr(), o.data_ptr(), t.numel()) for t, o in zip(target_params, online_params))

    def step(self, tau: float):
        for t in self.tables:
            check(lib().gops_polyak_update(C.byref(t), float(tau), _stream()), "gops_polyak_update")


def profile_enable(on: bool):
    lib().gops_profile_enable(int(on))


def profile_reset():
    lib().gops_profile_reset()


def profile_read(kernel_id: int):
    ms, n = C.c_double(0.0), C.c_int64(0)
    check(lib().gops_profile_read(kernel_id, C.byref(ms), C.byref(n)), "gops_profile_read")
    return ms.value, n.value
