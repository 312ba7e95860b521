"""What PPO and TRPO share on the HIP kernels: a Gaussian `mlp_shared` StochaPolicy and a StateValue in one container, the refusal
`create_alg` states for anything else, the per-object caches of kernel objects and buffers, and the captured Adam step.
"""
import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm.base import AlgorithmBase, ApprBase
from gops_amd.apprfunc.mlp import StateValue, StochaPolicy
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.act_distribution import GaussDistribution
from gops_amd.utils.common_utils import get_apprfunc_dict


def refusal(alg: str, density_words: str, kwargs: dict):
    """Why `create_alg` cannot build PPO / TRPO from these arguments, or None (POLY / LipsNet are refused before this is asked).
    `density_words`: what of the algorithm's kernels is the Gaussian density's."""
    if kwargs.get("policy_func_type") != "MLP" or kwargs.get("value_func_type") != "MLP":
        return f"{alg} runs MLP networks only (policy_func_type {kwargs.get('policy_func_type')!r}, value_func_type {kwargs.get('value_func_type')!r})"
    dist = kwargs.get("policy_act_distribution", "default")
    if kwargs.get("policy_func_name") != "StochaPolicy" or dist not in ("default", "GaussDistribution"):
        return (f"{alg} takes a stochastic policy with a Gaussian action distribution (policy_func_name 'StochaPolicy', "
                f"policy_act_distribution 'GaussDistribution' or 'default'), not {kwargs.get('policy_func_name')!r} with {dist!r}: "
                f"{density_words}")
    if kwargs.get("policy_std_type", "mlp_shared") != "mlp_shared":
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
    def _init_on_policy(self, kwargs: dict):
        """`self.networks`, checked, and the empty caches."""
        name = type(self).__name__
        self.networks = nets = ApproxContainer(**kwargs)
        if type(nets.policy) is not StochaPolicy or nets.policy.action_distribution_cls is not GaussDistribution:
            raise NotImplementedError(f"{name}: policy {type(nets.policy).__name__} (MLP StochaPolicy with GaussDistribution only)")
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
