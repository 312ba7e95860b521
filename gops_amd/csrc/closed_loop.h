// What the closed-loop kernels (rollout_sample.hip, rollout_episode.hip) share beyond the policy tile (policy_tile.h): the widths of
// the info tensors an env carries, the admission check of an (env, policy) description - the kernels differ in three rules, which
// the caller passes in - and the workspace queries' "the check passed and the LDS plan exists".
#pragma once
#include "common.h"
#include "policy_tile.h"

// Per-instance floats of info["state"] / info["ref_points"] (0: the model has none).
struct InfoWidths { int state_dim, ref_floats; };
inline InfoWidths info_widths(const GopsEnv& e) {
    if (e.kind == GOPS_ENV_VEH3DOFCONTI) return {6, (e.pre_horizon + 1) * 4};
    if (e.kind == GOPS_ENV_VEH2DOF) return {4, (e.pre_horizon + 1) * 2};
    return {0, 0};
}

// Where the two kernels' admission differs.  The kind sets are bit masks (bit k: env kind k).
struct ClosedLoopRules {
    uint32_t data_kinds;    // admitted with data_env = 1
    uint32_t model_kinds;   // admitted with data_env = 0; none: an env model is GOPS_ERR_BAD_ARG, tested before the kind
    bool time_input;        // sizes[0] == O + 1 (FiniteHorizonPolicy) is taken, else GOPS_ERR_UNSUPPORTED
    bool gauss_width;       // an output width 2A (mean, log std) is taken next to A
};

// The data envs both kernels step: not mobilerobot (obstacle noise drawn per step) nor the constrained vehicle models.
constexpr uint32_t CLOSED_LOOP_DATA_KINDS = 1u << GOPS_ENV_LQ | 1u << GOPS_ENV_IDPENDULUM | 1u << GOPS_ENV_CARTPOLE |
                                            1u << GOPS_ENV_VEH3DOFCONTI | 1u << GOPS_ENV_VEH2DOF;

// The description alone (what a workspace query can see): env kind, policy shape, sizes.  `act_num` = 0: the continuous heads
// (output width A, or 2A under rules.gauss_width); else the discrete heads' (output width act_num).  The ORDER of the tests is part
// of the ABI: a description wrong in two ways returns the code of the first.
inline int closed_loop_check(const ClosedLoopRules& rules, const GopsEnv* env, const GopsMlp* pol, int n, int T, int act_num) {
    if (!env || !pol || n < 1 || T < 1) return GOPS_ERR_BAD_ARG;
    if (rules.model_kinds == 0 && !env->data_env) return GOPS_ERR_BAD_ARG;
    const int k = env->kind;
    const uint32_t admitted = env->data_env ? rules.data_kinds : rules.model_kinds;
    if (k < 0 || k > 31 || !(admitted >> k & 1)) return GOPS_ERR_UNSUPPORTED;
    if (env->cstr_err || env->repeat_num > 1) return GOPS_ERR_UNSUPPORTED;
    if (pol->n_layers == 1 || pol->dtype != GOPS_DTYPE_F32) return GOPS_ERR_UNSUPPORTED;   // POLY nets, half-precision contractions
    const int O = env->obs_dim, A = env->act_dim, P = env->pre_horizon;
    if (A < 1 || A > GOPS_MAX_ACT || O < 1) return GOPS_ERR_BAD_ARG;
    if (k == GOPS_ENV_LQ && O > GOPS_MAX_LQ_STATE) return GOPS_ERR_UNSUPPORTED;
    if ((k == GOPS_ENV_IDPENDULUM && (O != 6 || A != 1)) || (k == GOPS_ENV_CARTPOLE && (O != 4 || A != 1))) return GOPS_ERR_BAD_ARG;
    if ((k == GOPS_ENV_PENDULUM && (O != 3 || A != 1)) || (k == GOPS_ENV_MOUNTAINCAR && (O != 2 || A != 1))) return GOPS_ERR_BAD_ARG;
    if (k == GOPS_ENV_VEH3DOFCONTI && (P < 1 || O != 6 + 4 * P || A != 2)) return GOPS_ERR_BAD_ARG;
    if (k == GOPS_ENV_VEH2DOF && (P < 1 || O != 4 + P || A != 1)) return GOPS_ERR_BAD_ARG;
    if (env->scale_obs && (O > 8 || env_has_ref_table(k))) return GOPS_ERR_UNSUPPORTED;
    if (pol->n_layers < 2 || pol->n_layers > GOPS_MAX_LAYERS) return GOPS_ERR_UNSUPPORTED;
    const int n_in = pol->sizes[0], n_out = pol->sizes[pol->n_layers];
    if (n_in == O + 1 && !rules.time_input) return GOPS_ERR_UNSUPPORTED;
    if (n_in != O && n_in != O + 1) return GOPS_ERR_BAD_ARG;
    if (act_num > 0 ? n_out != act_num : (n_out != A && !(rules.gauss_width && n_out == 2 * A))) return GOPS_ERR_BAD_ARG;
    for (int j = 1; j < pol->n_layers; ++j)
        if (pol->sizes[j] < 16 || (pol->sizes[j] & 15)) return GOPS_ERR_UNSUPPORTED;
    if (pol->hidden_act < GOPS_ACT_LINEAR || pol->hidden_act > GOPS_ACT_TANH) return GOPS_ERR_BAD_ARG;
    for (int j = 0; j < pol->n_layers; ++j)
        if (pol->weight[j] == nullptr || pol->bias[j] == nullptr) return GOPS_ERR_BAD_ARG;
    return GOPS_OK;
}

// The workspace queries: the kernel takes the description - the check passed and the LDS plan exists.
inline bool closed_loop_takes(const ClosedLoopRules& rules, const GopsEnv* env, const GopsMlp* pol, int n, int T, int act_num) {
    PolicyTile net;
    return closed_loop_check(rules, env, pol, n, T, act_num) == GOPS_OK && policy_tile_plan(*pol, net) != 0;
}
