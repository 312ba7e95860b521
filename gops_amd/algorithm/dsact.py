"""DSAC-T - distributional soft actor-critic with three refinements - on the HIP kernels.

Same class surface as the reference's gops/algorithm/dsact.py (ApproxContainer :34-74, DSACT :77-358): a tanh-Gaussian policy, twin
critics that output the mean and the standard deviation of the return, a variance-weighted critic loss against a clipped double-Q
soft target, a learnt temperature; the policy, the temperature and ALL three targets step every `delay_update` iterations only.

Where the arithmetic runs:
  * the no-grad target - target policy sample with its log-probability, both target critics, minimum, return sample, entropy term -
    is ONE launch of `gops_soft_backup` (`fused_target=True` for networks up to 64 wide, "force": wherever the kernel holds the
    shape), or composed from `gops_mlp_forward` calls and torch elementwise ops (`fused_target=False`, wider networks, shapes the
    kernel refuses); `backup_path` names what the last update ran;
  * the critic losses, their seeds with respect to the raw heads and the running `mean_std`: `gops_dsact_critic_loss`;
  * the policy's sampling head and its reverse, mean(logp) and the temperature's gradient: `gops_tanh_gauss_forward / _backward`;
  * everything with parameters: `gops_mlp_forward / _backward / _backward_x`, `HipAdam`, `gops_polyak_update`.
The temperature lives on the device (`log_alpha`; the kernels form exp themselves), so `local_update` replays as a HIP graph, one
per value of `iteration % delay_update == 0`.

The draws the result depends on are INPUTS of the update: `data["eps_new"]` [B, A] (the policy sample at obs), `data["eps_next"]`
[B, A] (the target policy sample at obs2) and `data["z_next"]` [2, B] (the target critics' return samples); when the batch has none
they are drawn on the device from a generator this object owns (seed + index), before the graph.  The reference's remaining draws
(dsact.py:241-242, 317-318: return samples nothing reads) are not drawn.
"""
__all__ = ["ApproxContainer", "DSACT"]

from copy import deepcopy

import torch
import torch.nn as nn

from gops_amd import hip_backend as hb
from gops_amd.algorithm import _soft_q
from gops_amd.algorithm._actor_critic import FUSED_MAX_WIDTH
from gops_amd.algorithm._soft_q import SoftQBase
from gops_amd.algorithm.base import ApprBase, grad_buffers
from gops_amd.apprfunc.mlp import ActionValueDistri
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam
from gops_amd.utils.tensorboard_setup import tb_tags


def refusal(kwargs: dict):
    """Why `create_alg` cannot build DSACT from these arguments, or None."""
    return _soft_q.refusal("DSACT", "ActionValueDistri", "a distributional action-value function", kwargs)


class ApproxContainer(ApprBase):
    """q1, q2, their targets, policy, its target, log_alpha; construction order (and with it the RNG draws) follows dsact.py:40-71."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q1 = create_apprfunc(**q_args)
        self.q2 = create_apprfunc(**q_args)
        self.q1_target = deepcopy(self.q1)
        self.q2_target = deepcopy(self.q2)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.policy = create_apprfunc(**policy_args)
        self.policy_target = deepcopy(self.policy)
        for net in (self.policy_target, self.q1_target, self.q2_target):
            for p in net.parameters():
                p.requires_grad = False
        self.log_alpha = nn.Parameter(torch.tensor(1, dtype=torch.float32))
        self.q1_optimizer = make_adam(self.q1.parameters(), lr=kwargs["value_learning_rate"])
        self.q2_optimizer = make_adam(self.q2.parameters(), lr=kwargs["value_learning_rate"])
        self.policy_optimizer = make_adam(self.policy.parameters(), lr=kwargs["policy_learning_rate"])
        self.alpha_optimizer = make_adam([self.log_alpha], lr=kwargs["alpha_learning_rate"])

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class DSACT(SoftQBase):
    """gamma, tau, auto_alpha, alpha, delay_update, tau_b: the reference's arguments (dsact.py:91-102).  fused_target: the soft
    backup as one `gops_soft_backup` launch for networks up to 64 wide ("force": wherever the kernel holds the shape; False: always
    composed from `gops_mlp_forward` calls and torch elementwise ops).  Update API, draws, graph replay, the actor's and the
    temperature's gradients: algorithm/_soft_q.py."""

    _q_names = ("q1", "q2")
    _value_cls = ActionValueDistri
    _policy_at_obs2 = "policy_target"
    _polyak_names = ("q1", "q2", "policy")
    _draws = SoftQBase._draws + (("z_next", lambda B, A: (2, B)),)
    _signature_terms = ("tau_b",)
    # the update's output vector, in this order
    _OUT = ("DSAC2/critic_avg_q1-RL iter", "DSAC2/critic_avg_q2-RL iter", "DSAC2/critic_avg_std1-RL iter",
            "DSAC2/critic_avg_std2-RL iter", "DSAC2/critic_avg_min_std1-RL iter", "DSAC2/critic_avg_min_std2-RL iter",
            tb_tags["loss_actor"], tb_tags["loss_critic"], "DSAC2/policy_mean-RL iter", "DSAC2/policy_std-RL iter",
            "DSAC2/entropy-RL iter", "DSAC2/alpha-RL iter", "DSAC2/mean_std1", "DSAC2/mean_std2")

    def __init__(self, index=0, fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.gamma = kwargs.get("gamma", 0.99)
        self.tau = kwargs.get("tau", 0.005)
        self.target_entropy = -kwargs["action_dim"]
        self.auto_alpha = kwargs.get("auto_alpha", True)
        self.alpha = kwargs.get("alpha", 0.2)
        self.delay_update = kwargs.get("delay_update", 2)
        self.tau_b = kwargs.get("tau_b", self.tau)
        self._init_soft(index, fused_target, kwargs)

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "auto_alpha", "alpha", "delay_update")

    @property
    def mean_std1(self):
        """The running mean of q1's standard deviation (a device scalar), None before the first update - as the reference's."""
        cl = self._critic_loss_obj()
        return None if cl is None or int(cl.state[2].item()) == 0 else cl.mean_std[0]

    @property
    def mean_std2(self):
        cl = self._critic_loss_obj()
        return None if cl is None or int(cl.state[2].item()) == 0 else cl.mean_std[1]

    def _critic_loss_obj(self):
        return next((v for k, v in self._cache.items() if k[0] == "critic_loss"), None)

    def _steps_policy(self, iteration):
        return iteration % self.delay_update == 0

    def _update(self, iteration):   # policy, temperature and all three targets together (dsact.py:335-358)
        step_policy = self._steps_policy(iteration)
        for opt in self._optimizers(step_policy):
            opt.step()
        if step_policy:
            self._polyak()

    # ---- kernels -------------------------------------------------------------------------------
    def _soft_backup(self, B: int, device) -> hb.SoftBackup:
        nets = self.networks
        pol = nets.policy_target.hip_mlp()
        qs = [nets.q1_target.hip_mlp(), nets.q2_target.hip_mlp()]
        key = ("soft_backup", B, str(device), bool(self.auto_alpha))
        sb = self._cache.get(key)
        if sb is None or (self.auto_alpha and sb.log_alpha.data_ptr() != nets.log_alpha.data_ptr()):
            pt = nets.policy_target
            sb = self._cache[key] = hb.SoftBackup(pol, qs, act_low=pt.act_low_lim.cpu().numpy(), act_high=pt.act_high_lim.cpu().numpy(),
                                                  min_log_std=pt.min_log_std, max_log_std=pt.max_log_std, batch=B,
                                                  log_alpha=nets.log_alpha.data if self.auto_alpha else None, device=device)
        else:
            sb.set_nets(pol, qs)
        return sb

    def _targets(self, batch):
        """(target_q [B], target_q_sample [B]) of dsact.py:237-313, no gradient."""
        o2 = batch["obs2"]
        B, device = o2.shape[0], o2.device
        if self.fused_target and (self.fused_target == "force" or self._widest_target_layer() <= FUSED_MAX_WIDTH):
            sb = self._soft_backup(B, device)
            if sb.supported:
                self.backup_path = "fused"
                res = sb.run(o2, batch["rew"], batch["done"], batch["eps_next"], batch["z_next"], gamma=self.gamma, alpha=self.alpha)
                return res["target_q"], res["target_q_sample"]
        self.backup_path = "composed"
        return self._targets_composed(batch)[:2]

    def _targets_composed(self, batch):
        """(target_q, target_q_sample, a2 [B, A], logp [B], q_targ [2, B, 2]) from `gops_mlp_forward` calls and elementwise torch ops."""
        nets = self.networks
        o2, d, r = batch["obs2"], batch["done"], batch["rew"]
        B, device = o2.shape[0], o2.device
        pt = nets.policy_target
        mean, log_std = torch.chunk(self._net("policy_target@o2", pt, B, device).forward(o2), 2, dim=-1)
        dist = pt.get_act_dist(torch.cat((mean, torch.clamp(log_std, pt.min_log_std, pt.max_log_std).exp()), dim=-1))
        a2, logp = dist.rsample(batch["eps_next"])
        x2 = torch.cat([o2, a2], dim=-1)
        heads = [self._net(f"{n}_target@o2", getattr(nets, f"{n}_target"), B, device).forward(x2) for n in self._q_names]
        m = [h[:, 0] for h in heads]
        s = [torch.nn.functional.softplus(h[:, 1]) for h in heads]
        z = torch.clamp(batch["z_next"], -3, 3)
        q_next = torch.min(m[0], m[1])
        q_sample = torch.where(m[0] < m[1], m[0] + z[0] * s[0], m[1] + z[1] * s[1])
        live, ent = (1 - d) * self.gamma, self._alpha_tensor(device) * logp
        q_targ = torch.stack([torch.stack((m[i], s[i]), dim=-1) for i in range(2)])
        return r + live * (q_next - ent), r + live * (q_sample - ent), a2, logp, q_targ

    def _gradient_kernels(self, batch) -> torch.Tensor:
        """Enqueue one compute_gradient; returns the update's scalars (`_OUT`) as one device tensor, without synchronising."""
        nets = self.networks
        o, a = batch["obs"], batch["act"]
        B, device = o.shape[0], o.device
        target_q, target_q_sample = self._targets(batch)

        # ---- critics: variance-weighted regression (dsact.py:284-301) ----------------------------------
        x = torch.cat([o, a], dim=-1)
        qraw = self._buf("qraw", (2, B, 2), device)
        q_nets = [self._net(f"{n}@data", getattr(nets, n), B, device) for n in self._q_names]
        for i, net in enumerate(q_nets):
            net.forward(x, out=qraw[i])
        key = ("critic_loss", str(device))
        cl = self._cache.get(key)
        if cl is None:
            cl = self._cache[key] = hb.DsactCriticLoss(device)
        seed, stats = cl.run(qraw, target_q, target_q_sample, self.tau_b, seed=self._buf("seed", (2, B, 2), device))
        for i, (n, net) in enumerate(zip(self._q_names, q_nets)):
            gw, gb = grad_buffers(getattr(nets, n))
            net.backward(x, seed[i], gw, gb)

        loss_policy, tstats, alpha, _ = self._actor(batch)
        return torch.cat([stats[1:7], torch.stack([loss_policy, stats[0], tstats[1], tstats[2], -tstats[0], alpha]), stats[7:9]])
