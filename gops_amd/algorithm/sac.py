"""SAC - soft actor-critic - on the HIP kernels.

Same class surface as the reference's gops/algorithm/sac.py (ApproxContainer :32-71, SAC :74-263): a tanh-Gaussian policy, twin
scalar critics with Polyak targets, a learnt temperature; every network steps at every update, and the policy sampled at obs2 is
the ONLINE one (there is no policy_target).

The no-grad target `rew + (1 - done) gamma (min(q1_target, q2_target)(obs2, a2) - alpha logp)` is one launch of `gops_soft_q_backup`
(or composed, see algorithm/_soft_q.py); the critic regression - seeds, both losses, mean(q1) - is `gops_ac_critic_loss`.
`local_update` replays as ONE HIP graph.  Draws: `data["eps_new"]`, `data["eps_next"]` [B, A] (algorithm/_soft_q.py).
"""
__all__ = ["ApproxContainer", "SAC"]

from copy import deepcopy

import torch
import torch.nn as nn

from gops_amd import hip_backend as hb
from gops_amd.algorithm import _soft_q
from gops_amd.algorithm._soft_q import SoftQBase
from gops_amd.algorithm.base import ApprBase, grad_buffers
from gops_amd.apprfunc.mlp import ActionValue
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam
from gops_amd.utils.tensorboard_setup import tb_tags

# what the reference's constructor reads with kwargs[...], in its order (sac.py:63-68, 104)
MANDATORY = ("q_learning_rate", "policy_learning_rate", "alpha_learning_rate")


def refusal(kwargs: dict):
    """Why `create_alg` cannot build SAC from these arguments, or None."""
    return _soft_q.refusal("SAC", "ActionValue", "an action-value function", kwargs)


class ApproxContainer(ApprBase):
    """q1, q2, policy, the critics' targets, log_alpha; construction order (and with it the RNG draws) follows sac.py:38-68."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q1 = create_apprfunc(**q_args)
        self.q2 = create_apprfunc(**q_args)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.policy = create_apprfunc(**policy_args)
        self.q1_target = deepcopy(self.q1)
        self.q2_target = deepcopy(self.q2)
        for net in (self.q1_target, self.q2_target):
            for p in net.parameters():
                p.requires_grad = False
        self.log_alpha = nn.Parameter(torch.tensor(1, dtype=torch.float32))
        self.q1_optimizer = make_adam(self.q1.parameters(), lr=kwargs["q_learning_rate"])
        self.q2_optimizer = make_adam(self.q2.parameters(), lr=kwargs["q_learning_rate"])
        self.policy_optimizer = make_adam(self.policy.parameters(), lr=kwargs["policy_learning_rate"])
        self.alpha_optimizer = make_adam([self.log_alpha], lr=kwargs["alpha_learning_rate"])

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class SAC(SoftQBase):
    """gamma, tau, auto_alpha, alpha, target_entropy: the reference's arguments (sac.py:87-105).  fused_target: the soft backup as one
    `gops_soft_q_backup` launch for networks up to 64 wide ("force": wherever the kernel holds the shape; False: always composed)."""

    _q_names = ("q1", "q2")
    _value_cls = ActionValue
    _polyak_names = ("q1", "q2")
    _OUT = (tb_tags["loss_critic"], tb_tags["loss_actor"], "SAC/critic_avg_q1-RL iter", "SAC/critic_avg_q2-RL iter", "SAC/entropy-RL iter",
            "SAC/alpha-RL iter")

    def __init__(self, index=0, gamma=0.99, tau=0.005, auto_alpha=True, alpha=0.2, target_entropy=None, fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.gamma, self.tau, self.auto_alpha, self.alpha = gamma, tau, auto_alpha, alpha
        self.target_entropy = -kwargs["action_dim"] if target_entropy is None else target_entropy
        self._init_soft(index, fused_target, kwargs)

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "auto_alpha", "alpha", "target_entropy")

    def _steps_policy(self, iteration):
        return True

    def _update(self, iteration):   # sac.py:243-263
        for opt in self._optimizers(True):
            opt.step()
        self._polyak()

    def _gradient_kernels(self, batch) -> torch.Tensor:
        """Enqueue one compute_gradient; returns the update's scalars (`_OUT`) as one device tensor, without synchronising."""
        nets = self.networks
        o, a = batch["obs"], batch["act"]
        B, device = o.shape[0], o.device
        backup = self._backup(batch)

        # ---- critics: loss_q1 + loss_q2 against the one backup (sac.py:224-226) ----
        x = torch.cat([o, a], dim=-1)
        q = self._buf("q", (2, B), device)
        q_nets = [self._net(f"{n}@data", getattr(nets, n), B, device) for n in self._q_names]
        for i, net in enumerate(q_nets):
            net.forward(x, out=q[i])
        key = ("critic_loss", str(device))
        cl = self._cache.get(key)
        if cl is None:
            cl = self._cache[key] = hb.AcCriticLoss(device)
        seed, _, stats = cl.run(q, backup, None, seed=self._buf("seed", (2, B), device), abs_err=self._buf("abs_err", (B,), device))
        for i, (n, net) in enumerate(zip(self._q_names, q_nets)):
            gw, gb = grad_buffers(getattr(nets, n))
            net.backward(x, seed[i].unsqueeze(-1), gw, gb)

        loss_policy, tstats, alpha, _ = self._actor(batch)
        return torch.stack([stats[3], loss_policy, stats[2], q[1].mean(), -tstats[0], alpha])
