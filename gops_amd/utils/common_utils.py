"""Helpers shared by the factories and algorithms (interface of the reference's
gops/utils/common_utils.py: get_activation_func :26-55, get_apprfunc_dict :58-135,
seed_everything/set_seed :186-237, ModuleOnDevice :276-289)."""
import random
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from gops_amd.utils import act_distribution
from gops_amd.utils.act_distribution import DiracDistribution, GaussDistribution

_ACTIVATIONS = {"relu": nn.ReLU, "elu": nn.ELU, "gelu": nn.GELU, "selu": nn.SELU,
                "sigmoid": nn.Sigmoid, "tanh": nn.Tanh, "linear": nn.Identity}


def get_activation_func(key: str):
    assert isinstance(key, str)
    if key not in _ACTIVATIONS:
        print("input activation name:" + key)
        raise RuntimeError
    return _ACTIVATIONS[key]


def get_apprfunc_dict(key: str, **kwargs):
    """Collect the per-network constructor arguments `<key>_func_type`, `<key>_hidden_sizes`, ...
    out of the flat args dict (the MLP, POLY, GAUSS and LipsNet families exist on this path)."""
    var = dict()
    var["apprfunc"] = kwargs[key + "_func_type"]
    var["name"] = kwargs[key + "_func_name"]
    var["obs_dim"] = kwargs["obsv_dim"]
    var["pre_horizon"] = kwargs.get("pre_horizon", None)
    var["min_log_std"] = kwargs.get(key + "_min_log_std", float("-20"))   # (StochaPolicy; reference common_utils.py:63-65)
    var["max_log_std"] = kwargs.get(key + "_max_log_std", float("2"))
    var["std_type"] = kwargs.get(key + "_std_type", "mlp_shared")
    apprfunc_type = kwargs[key + "_func_type"]
    if apprfunc_type == "MLP":
        var["hidden_sizes"] = kwargs[key + "_hidden_sizes"]
        var["hidden_activation"] = kwargs[key + "_hidden_activation"]
        var["output_activation"] = kwargs.get(key + "_output_activation", "linear")
    elif apprfunc_type == "POLY":   # gops_amd/apprfunc/poly.py (reference common_utils.py:89-91)
        var["degree"] = kwargs[key + "_degree"]
        var["add_bias"] = kwargs[key + "_add_bias"]
        var["norm_matrix"] = kwargs.get("norm_matrix", None)
    elif apprfunc_type == "GAUSS" and key + "_num_kernel" in kwargs:   # gops_amd/apprfunc/gauss.py (reference common_utils.py:92-93)
        var["num_kernel"] = kwargs[key + "_num_kernel"]
    elif apprfunc_type == "LipsNet":   # gops_amd/apprfunc/lipsnet.py (reference common_utils.py:94-106)
        var["hidden_sizes"] = kwargs[key + "_hidden_sizes"]
        var["hidden_activation"] = kwargs[key + "_hidden_activation"]
        var["output_activation"] = kwargs.get(key + "_output_activation", "linear")
        for name in ("lips_init_value", "lips_auto_adjust", "lips_learning_rate", "lips_hidden_sizes", "eps", "lambda", "local_lips",
                     "squash_action", "learning_rate"):
            var[name] = kwargs[key + "_" + name]
        var["mlp_dtype"] = kwargs.get("mlp_dtype", "fp32")   # (the module refuses fp16 at construction)
    else:
        # (GAUSS lands here without its kernel count: the family has no default for it, in the reference either)
        raise NotImplementedError(f"apprfunc type {apprfunc_type}{' without ' + key + '_num_kernel' if apprfunc_type == 'GAUSS' else ''} "
                                  "is outside the MI355X ADP path (MLP and POLY only, GAUSS for the policy of FHADP and INFADP with "
                                  "<key>_num_kernel, LipsNet for the policy of INFADP)")
    if kwargs["action_type"] == "continu":
        var["act_high_lim"] = np.array(kwargs["action_high_limit"])
        var["act_low_lim"] = np.array(kwargs["action_low_limit"])
        var["act_dim"] = kwargs["action_dim"]
    else:   # discrete actions (reference common_utils.py:115-128): the action count, and a distribution over action indices
        var["act_num"] = kwargs["action_num"]
        dist = kwargs.get("policy_act_distribution", "default")
        if dist == "default":
            dist = "CategoricalDistribution" if kwargs.get("policy_func_name") == "StochaPolicyDis" else "ValueDiracDistribution"
        if dist not in ("CategoricalDistribution", "ValueDiracDistribution"):
            raise NotImplementedError(f"policy_act_distribution {dist!r}: discrete actions take CategoricalDistribution or "
                                      "ValueDiracDistribution")
        var["action_distribution_cls"] = getattr(act_distribution, dist)
        return var
    dist = kwargs.get("policy_act_distribution", "default")   # (reference common_utils.py:118-133)
    if dist == "default":
        var["action_distribution_cls"] = GaussDistribution if kwargs.get("policy_func_name") == "StochaPolicy" else DiracDistribution
    elif dist in ("DiracDistribution", "GaussDistribution", "TanhGaussDistribution"):
        var["action_distribution_cls"] = getattr(act_distribution, dist)
    else:
        raise NotImplementedError(f"policy_act_distribution {dist!r}: DiracDistribution, GaussDistribution and TanhGaussDistribution "
                                  "exist here (discrete actions are outside this path)")
    return var


def make_adam(params, lr: float):
    """Adam with the reference's defaults (gops/algorithm/fhadp.py:45-47): one HIP launch per step
    (`gops_adam_step`) instead of torch's multi-kernel foreach implementation."""
    from gops_amd.hip_backend import HipAdam
    return HipAdam(params, lr=lr)


def seed_everything(seed: Optional[int] = None) -> int:
    if seed is None:
        seed = random.randint(0, 2 ** 32 - 1)
    seed = int(seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def set_seed(trainer_name, seed, offset, env=None):
    """Sub-process seeding rule of the reference: only `*_sync_*` / `*_async_*` trainers reseed
    (with seed + offset); serial trainers leave the global RNG alone."""
    if trainer_name.split("_")[1] in ["async", "sync"]:
        print("Setting seed of a subprocess to {}".format(seed + offset))
        seed_everything(seed + offset)
        if env is not None:
            env.seed(seed + offset)
        return seed + offset, env
    if env is not None:
        env.seed(seed)
    return None, env


class ModuleOnDevice:
    """Context manager moving a module to `device` and back to CPU on exit."""

    def __init__(self, module, device):
        self.module, self.device = module, device
        self.different = next(module.parameters()).device.type != device

    def __enter__(self):
        if self.different:
            self.module.to(self.device)

    def __exit__(self, exc_type, exc_val, exc_tb):
        if self.different:
            self.module.to("cpu")
