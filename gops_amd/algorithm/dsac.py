"""DSAC - distributional soft actor-critic - on the HIP kernels.

Same class surface as the reference's gops/algorithm/dsac.py (ApproxContainer :35-70, DSAC :73-291): a tanh-Gaussian policy, ONE
critic that outputs the mean and the standard deviation of the return, a learnt temperature; the critic steps at every update, the
policy, the temperature and both targets every `delay_update` iterations.

The no-grad target `rew + (1 - done) gamma (m + clamp(z, -3, 3) s - alpha logp)` at the target policy's sample is one launch of
`gops_soft_q_backup` (or composed, see algorithm/_soft_q.py); the critic loss with its td_bound clamp and its seeds is
`gops_dsac_critic_loss`.  `local_update` replays as a HIP graph, one per value of `iteration % delay_update == 0`.
Draws: `data["eps_new"]`, `data["eps_next"]` [B, A] and `data["z_next"]` [B] (algorithm/_soft_q.py); the reference's return samples on
the data and on the new action (dsac.py:223, 256) reach no output and are not drawn.
"""
__all__ = ["ApproxContainer", "DSAC"]

from copy import deepcopy

import torch
import torch.nn as nn

from gops_amd import hip_backend as hb
from gops_amd.algorithm import _soft_q
from gops_amd.algorithm._soft_q import SoftQBase
from gops_amd.algorithm.base import ApprBase, grad_buffers
from gops_amd.apprfunc.mlp import ActionValueDistri
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam
from gops_amd.utils.tensorboard_setup import tb_tags

# what the reference's constructor reads with kwargs[...], in its order (dsac.py:63-67, 92-98)
MANDATORY = ("value_learning_rate", "policy_learning_rate", "alpha_learning_rate", "gamma", "tau", "action_dim", "auto_alpha", "bound",
             "delay_update")


def refusal(kwargs: dict):
    """Why `create_alg` cannot build DSAC from these arguments, or None."""
    return _soft_q.refusal("DSAC", "ActionValueDistri", "a distributional action-value function", kwargs)


class ApproxContainer(ApprBase):
    """q, its target, policy, its target, log_alpha; construction order (and with it the RNG draws) follows dsac.py:41-67."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q = create_apprfunc(**q_args)
        self.q_target = deepcopy(self.q)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.policy = create_apprfunc(**policy_args)
        self.policy_target = deepcopy(self.policy)
        for net in (self.policy_target, self.q_target):
            for p in net.parameters():
                p.requires_grad = False
        self.log_alpha = nn.Parameter(torch.tensor(1, dtype=torch.float32))
        self.q_optimizer = make_adam(self.q.parameters(), lr=kwargs["value_learning_rate"])
        self.policy_optimizer = make_adam(self.policy.parameters(), lr=kwargs["policy_learning_rate"])
        self.alpha_optimizer = make_adam([self.log_alpha], lr=kwargs["alpha_learning_rate"])

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class DSAC(SoftQBase):
    """gamma, tau, auto_alpha, alpha, bound, delay_update: the reference's arguments (dsac.py:92-98).  fused_target: the soft backup as
    one `gops_soft_q_backup` launch for networks up to 64 wide ("force": wherever the kernel holds the shape; False: always composed)."""

    _q_names = ("q",)
    _value_cls = ActionValueDistri
    _distri = True
    _draws = SoftQBase._draws + (("z_next", lambda B, A: (B,)),)
    _policy_at_obs2 = "policy_target"
    _polyak_names = ("q", "policy")
    _OUT = ("DSAC/critic_avg_q-RL iter", "DSAC/critic_avg_std-RL iter", tb_tags["loss_actor"], "DSAC/policy_mean-RL iter",
            "DSAC/policy_std-RL iter", "DSAC/entropy-RL iter", "DSAC/alpha-RL iter")

    def __init__(self, index=0, fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.gamma = kwargs["gamma"]
        self.tau = kwargs["tau"]
        self.target_entropy = -kwargs["action_dim"]
        self.auto_alpha = kwargs["auto_alpha"]
        self.alpha = kwargs.get("alpha", 0.2)
        self.bound = kwargs["bound"]
        self.delay_update = kwargs["delay_update"]
        self._init_soft(index, fused_target, kwargs)

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "auto_alpha", "alpha", "bound", "delay_update")

    @property
    def loss_q(self):
        """The last update's critic loss (a device scalar; the reference does not log it), None before the first update."""
        cl = next((v for k, v in self._cache.items() if k[0] == "critic_loss"), None)
        return None if cl is None else cl.buf[0]

    def _steps_policy(self, iteration):
        return iteration % self.delay_update == 0

    def _update(self, iteration):   # dsac.py:269-290
        step_policy = self._steps_policy(iteration)
        for opt in self._optimizers(step_policy):
            opt.step()
        if step_policy:
            self._polyak()

    def _gradient_kernels(self, batch) -> torch.Tensor:
        """Enqueue one compute_gradient; returns the update's scalars (`_OUT`) as one device tensor, without synchronising."""
        nets = self.networks
        o, a = batch["obs"], batch["act"]
        B, A, device = o.shape[0], a.shape[1], o.device
        target_q = self._backup(batch)

        # ---- critic: Gaussian likelihood of the target, the TD error clamped to 3 mean(std) (dsac.py:235-252) ----
        x = torch.cat([o, a], dim=-1)
        q_net = self._net("q@data", nets.q, B, device)
        qraw = q_net.forward(x, out=self._buf("qraw", (B, 2), device))
        key = ("critic_loss", str(device))
        cl = self._cache.get(key)
        if cl is None:
            cl = self._cache[key] = hb.DsacCriticLoss(device)
        seed, stats = cl.run(qraw, target_q, self.bound, seed=self._buf("seed", (B, 2), device))
        gw, gb = grad_buffers(nets.q)
        q_net.backward(x, seed, gw, gb)

        loss_policy, tstats, alpha, head = self._actor(batch)
        # the reference logs columns 0 and 1 of the policy's (mean, std) output (dsac.py:160-161): with act_dim > 1 the second is a mean
        pol = nets.policy
        col1 = head[:, 1] if A > 1 else torch.clamp(head[:, 1], pol.min_log_std, pol.max_log_std).exp()
        return torch.stack([stats[1], stats[2], loss_policy, torch.tanh(head[:, 0]).mean(), col1.mean(), -tstats[0], alpha])
