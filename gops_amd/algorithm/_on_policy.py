"""What PPO and TRPO share on the HIP kernels: a Gaussian `mlp_shared` StochaPolicy (for TRPO also a categorical StochaPolicyDis) and
a StateValue in one container, the refusal `create_alg` states for anything else, the per-object caches of kernel objects and
buffers, and the captured Adam step.
"""
import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm.base import AlgorithmBase, ApprBase
from gops_amd.apprfunc.mlp import StateValue, StochaPolicy, StochaPolicyDis
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.act_distribution import CategoricalDistribution, GaussDistribution
from gops_amd.utils.common_utils import get_apprfunc_dict

MAX_ACTIONS = 16   # include/gops_hip.h: GOPS_DQN_MAX_ACTIONS, the widest head of gops_cat_fisher_seed / gops_cat_trpo_surrogate


def categorical_refusal(alg: str, kwargs: dict):
    """Why `create_alg` cannot build `alg` on a categorical StochaPolicyDis from these arguments, or None."""
    dist = kwargs.get("policy_act_distribution", "default")
    if kwargs.get("action_type") != "discret":
        return (f"{alg} takes policy_func_name 'StochaPolicyDis' with action_type 'discret' only, not {kwargs.get('action_type')!r}: its "
                "outputs are the logits of action indices (continuous actions take 'StochaPolicy')")
    if dist not in ("default", "CategoricalDistribution"):
        return (f"{alg} takes policy_func_name 'StochaPolicyDis' with a categorical action distribution (policy_act_distribution "
                f"'CategoricalDistribution' or 'default'), not {dist!r}: the softmax Fisher metric and the surrogate kernel are that density's")
    n = kwargs.get("action_num")
    if not isinstance(n, int) or not 2 <= n <= MAX_ACTIONS:
        return f"{alg} takes 2 .. {MAX_ACTIONS} discrete actions (action_num {n!r}): the categorical head kernels hold no other width"
    return None


def refusal(alg: str, density_words: str, kwargs: dict, categorical: bool = False):
    """Why `create_alg` cannot build PPO / TRPO from these arguments, or None (POLY / LipsNet are refused before this is asked).
    `density_words`: what of the algorithm's kernels is the Gaussian density's; `categorical`: the algorithm also has the kernels
    of a categorical StochaPolicyDis (for which the `policy_std_type` / log-std arguments mean nothing and are ignored)."""
    if kwargs.get("policy_func_type") != "MLP" or kwargs.get("value_func_type") != "MLP":
        return f"{alg} runs MLP networks only (policy_func_type {kwargs.get('policy_func_type')!r}, value_func_type {kwargs.get('value_func_type')!r})"
    dist = kwargs.get("policy_act_distribution", "default")
    discrete = categorical and kwargs.get("policy_func_name") == "StochaPolicyDis"
    if discrete:
        reason = categorical_refusal(alg, kwargs)
        if reason is not None:
            return reason
    elif kwargs.get("policy_func_name") != "StochaPolicy" or dist not in ("default", "GaussDistribution"):
        return (f"{alg} takes a stochastic policy with a Gaussian action distribution (policy_func_name 'StochaPolicy', "
                f"policy_act_distribution 'GaussDistribution' or 'default'), not {kwargs.get('policy_func_name')!r} with {dist!r}: "
                f"{density_words}")
    if not discrete and kwargs.get("policy_std_type", "mlp_shared") != "mlp_shared":
        return (f"{alg} runs the policy with policy_std_type 'mlp_shared' only (one stack for mean and log std), not "
                f"{kwargs.get('policy_std_type')!r}: 'parameter' and 'mlp_separated' are not yet supported")
    if kwargs.get("value_func_name") != "StateValue":
        return f"{alg} takes a state-value function (value_func_name 'StateValue'), not {kwargs.get('value_func_name')!r}"
    for key in ("policy", "value"):
        if kwargs.get(f"{key}_output_activation", "linear") != "linear":
            return (f"{alg} takes networks with a linear output layer ({key}_output_activation "
                    f"{kwargs.get(key + '_output_activation')!r}): the HIP kernels apply no output activation")
    if hb.dtype_id(kwargs.get("mlp_dtype")) != 0:
        return f"{alg} is fp32 only (mlp_dtype {kwargs.get('mlp_dtype')!r}): its kernels have no half-precision path"
    trainer = kwargs.get("trainer")
    if trainer is not None and not trainer.startswith("on_serial"):
        return f"{alg} runs under on_serial_trainer only: trainer {trainer!r} has not been run with its on-policy columns"
    return None


class ApproxContainer(ApprBase):
    """policy, then value: construction order (and with it the RNG draws and an optimizer's parameter order) follows the reference's
    ppo.py:39-45 and trpo.py:44-50."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.policy = create_apprfunc(**get_apprfunc_dict("policy", **kwargs))
        self.value = create_apprfunc(**get_apprfunc_dict("value", **kwargs))

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class OnPolicyBase(AlgorithmBase):
    def _init_on_policy(self, kwargs: dict, categorical: bool = False):
        """`self.networks`, checked, and the empty caches.  `categorical`: a StochaPolicyDis with CategoricalDistribution is accepted
        beside the Gaussian StochaPolicy."""
        name = type(self).__name__
        self.networks = nets = ApproxContainer(**kwargs)
        gauss = type(nets.policy) is StochaPolicy and nets.policy.action_distribution_cls is GaussDistribution
        cat = categorical and type(nets.policy) is StochaPolicyDis and nets.policy.action_distribution_cls is CategoricalDistribution
        if cat and not 2 <= nets.policy.act_num <= MAX_ACTIONS:
            raise NotImplementedError(f"{name}: {nets.policy.act_num} discrete actions (2 .. {MAX_ACTIONS} only)")
        if not gauss and not cat:
            raise NotImplementedError(f"{name}: policy {type(nets.policy).__name__} (MLP StochaPolicy with GaussDistribution"
                                      f"{' or MLP StochaPolicyDis with CategoricalDistribution' if categorical else ''} only)")
        if not isinstance(nets.value, StateValue):
            raise NotImplementedError(f"{name}: value network {type(nets.value).__name__} (MLP StateValue only)")
        self.tb_info = dict()
        self._cache, self._bufs = {}, {}

    def _adam_step(self, graph, signature, batch: dict, gradients, opt, counter: str) -> torch.Tensor:
        """`gradients(batch)`, then `opt.step()`: eager, or as a replay of the graph `graph` (a StepGraphCache) holds under
        `signature`, counted in the attribute `counter`.  -> what `gradients` returns (device)."""
        def step(b):
            out = gradients(b)
            opt.step()
            return out

        def replayed():
            opt.advance()
            setattr(self, counter, getattr(self, counter) + 1)

        return graph.run(signature, batch, step, before_replay=opt.sync_hyper, on_replay=replayed, work=batch["obs"].shape[0],
                         on_capture_fail=opt.resync_device_state)

    def _storage(self):
        """The tail of a graph's signature: the workspaces and buffers its launches were captured with."""
        return (tuple(sorted(obj.workspace.data_ptr() for obj in self._cache.values() if hasattr(obj, "workspace"))),
                tuple(sorted(t.data_ptr() for t in self._bufs.values())))

    # ---- kernels' objects ------------------------------------------------------------------------
    def _net(self, role: str, module, B: int, device) -> hb.MlpNet:
        key = (role, B, str(device))
        mlp = module.hip_mlp()
        net = self._cache.get(key)
        if net is None:
            net = self._cache[key] = hb.MlpNet(mlp, B, device=device)
        else:
            net.mlp = mlp
        return net

    def _buf(self, name: str, shape, device) -> torch.Tensor:
        key = (name, tuple(shape), str(device))
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=torch.float32, device=device)
        return t

    def _one(self, key, make):
        obj = self._cache.get(key)
        if obj is None:
            obj = self._cache[key] = make()
        return obj

    def _adv_normalize(self, device) -> hb.AdvNormalize:
        return self._one(("adv_normalize", str(device)), lambda: hb.AdvNormalize(device))
