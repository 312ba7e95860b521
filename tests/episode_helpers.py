"""Builders shared by tests/test_episode_cpu.py and tests/test_episode_gpu.py."""
import numpy as np

from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

ENVS = {
    "lq": dict(env_id="pyth_lq", lq_config="s4a2"),
    "idp": dict(env_id="pyth_idpendulum"),
    "cartpole": dict(env_id="gym_cartpoleconti"),
    "veh3dof": dict(env_id="pyth_veh3dofconti", pre_horizon=10),
    "veh2dof": dict(env_id="pyth_veh2dofconti", pre_horizon=10),
}
POLICIES = {   # name: (algorithm whose container holds the policy class, hidden sizes, activation)
    "relu64": ("INFADP", (64, 64), "relu"),
    "gelu256": ("INFADP", (256, 256), "gelu"),
    "tanh3": ("INFADP", (48, 32, 16), "tanh"),
    "finite_elu64": ("FHADP", (64, 64), "elu"),   # FiniteHorizonPolicy: virtual_t = 1 at every step
}


def alg_kwargs(env, policy, seed=0, **extra):
    cfg = dict(ENVS[env])
    alg, hidden, act = POLICIES[policy] if isinstance(policy, str) else policy
    A = act_dim_of(cfg)
    kw = dict(algorithm=alg, trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=cfg["env_id"], obsv_dim=obs_dim_of(cfg),
              action_dim=A, action_type="continu", action_high_limit=np.ones(A, dtype=np.float32),
              action_low_limit=-np.ones(A, dtype=np.float32), policy_func_type="MLP",
              policy_func_name="FiniteHorizonPolicy" if alg == "FHADP" else "DetermPolicy", policy_hidden_sizes=list(hidden),
              policy_hidden_activation=act, policy_act_distribution="default", policy_learning_rate=1e-3, use_gpu=True)
    if alg == "INFADP":
        kw.update(value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation=act,
                  value_learning_rate=1e-3)
    if "pre_horizon" in cfg or alg == "FHADP":
        kw["pre_horizon"] = cfg.get("pre_horizon", 10)
    if "lq_config" in cfg:
        kw["lq_config"] = cfg["lq_config"]
    kw.update(extra)
    return cfg, kw
