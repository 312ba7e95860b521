"""FHADP2 - finite-horizon ADP with an open-loop action sequence - on the HIP rollout.

Same class surface as the reference's gops/algorithm/fhadp2.py (ApproxContainer :26-46, FHADP2
:49-121): `FiniteHorizonFullPolicy` maps obs_0 to all H actions in ONE MLP evaluation, the env model is
rolled out with that sequence, `loss = -mean_b sum_t gamma^t r_t`.  The H-step env-model loop and its
autograd replay run in the fused kernels' open-loop mode (`gops_rollout_forward` with
`open_loop = 1`, `gops_rollout_backward_open_loop`); the single MLP evaluation and its backward run in the
library too (`gops_mlp_forward / _backward`: hidden stack on the rollout tiles, the act_dim * H wide output layer on its
own kernels) - no autograd graph, no rocBLAS.
"""
__all__ = ["FHADP2"]

import time
from typing import Tuple

from gops_amd import hip_backend as hb
from gops_amd.algorithm._model_based import ModelBasedBase
from gops_amd.algorithm.base import grad_buffers, install_grads
from gops_amd.algorithm.fhadp import ApproxContainer  # noqa: F401  (same container; create_alg looks it up here)
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags


class FHADP2(ModelBasedBase):
    """:param int pre_horizon: length of the emitted action sequence = model rollout horizon."""

    def __init__(self, *, pre_horizon: int, index: int = 0, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs, pre_horizon=pre_horizon)
        self.envmodel = create_env_model(**kwargs, pre_horizon=pre_horizon)
        self.forward_step = pre_horizon
        self.gamma = 1.0
        self._rollouts = self._cache

    @property
    def adjustable_parameters(self) -> Tuple[str]:
        return ("forward_step", "gamma")

    def _local_update(self, data, iteration: int):
        self._compute_gradient(data)
        self.networks.policy_optimizer.step()
        return self.tb_info

    def get_remote_update_info(self, data, iteration: int):
        self._compute_gradient(data)
        return self.tb_info, {"grad": [p._grad for p in self.networks.policy.parameters()]}

    def _remote_update(self, update_info):
        install_grads(self.networks.policy, update_info["grad"])
        self.networks.policy_optimizer.step()

    def _rollout_for(self, batch: int, device) -> hb.Rollout:
        policy = self.networks.policy
        if self.forward_step != policy.pre_horizon:
            raise RuntimeError("FHADP2: forward_step must equal the policy's pre_horizon (its output width)")
        return self._cached((batch, self.forward_step, float(self.gamma), str(device)), lambda: hb.Rollout(
            self._hip_env(), None, batch=batch, horizon=self.forward_step, gamma=self.gamma, finite_horizon=False, need_grad=True,
            device=device))

    def _mlp_for(self, batch: int, device) -> hb.MlpNet:
        mlp = self.networks.policy.hip_mlp()
        return self._cached(("mlp", batch, str(device)), lambda: hb.MlpNet(mlp, batch, device=device), lambda net: setattr(net, "mlp", mlp))

    def _compute_gradient(self, data):
        t0 = time.time()
        batch = self._model_batch(data)
        B, device = batch["obs"].shape[0], batch["obs"].device
        policy = self.networks.policy
        # ONE evaluation of the full-horizon policy emits all H actions (fhadp2.py:100-104): hidden stack on the rollout
        # tiles, wide output layer on its own kernels (gops_mlp_forward); no autograd graph, no rocBLAS
        net = self._mlp_for(B, device)
        pre = net.forward(batch["obs"]).view(B, policy.pre_horizon, policy.act_dim)
        ro = self._rollout_for(B, device)
        v_pi = ro.forward(batch, head_pre=pre)["v_pi"]
        loss_policy = -v_pi.mean()
        g_pre = ro.backward_open_loop(self._grad_v(B, device))   # d(loss)/d(head outputs) [B, H, A]
        gw, gb = grad_buffers(policy)
        net.backward(batch["obs"], g_pre.view(B, -1), gw, gb)    # through the MLP into the parameters' .grad
        self.tb_info[tb_tags["loss_actor"]] = scalar(loss_policy)
        self.tb_info[tb_tags["alg_time"]] = (time.time() - t0) * 1000  # ms
