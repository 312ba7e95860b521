"""What SAC, DSAC and DSAC-T share on the HIP kernels: one update = soft Q backup (no grad), critic regression, actor gradient through the
live critic(s), temperature gradient, Adam per network, Polyak on the targets.

Where the arithmetic runs:
  * the no-grad target - policy sample at obs2 with its log-probability, the target critic(s), minimum or return sample, entropy
    term - is ONE launch of `gops_soft_q_backup` (`fused_target=True` for networks up to `FUSED_MAX_WIDTH` wide, "force": wherever
    the kernel holds the shape), or composed from `gops_mlp_forward` calls and torch elementwise ops (`fused_target=False`, wider
    networks, shapes the kernel refuses); `backup_path` names what the last update ran;
  * the policy's sampling head and its reverse, mean(logp) and the temperature's gradient: `gops_tanh_gauss_forward / _backward`;
  * everything with parameters: `gops_mlp_forward / _backward / _backward_x`, `HipAdam`, `gops_polyak_update`.
The temperature lives on the device (`log_alpha`; the kernels form exp themselves), so `local_update` replays as a HIP graph.

The draws the result depends on are INPUTS of the update: `data["eps_new"]` [B, A] (the policy sample at obs), `data["eps_next"]`
[B, A] (the policy sample at obs2) and, for DSAC and DSAC-T, `data["z_next"]` (the target critics' return samples: a class's
`_draws`); when the batch has none they are drawn on the device from a generator this object owns (seed + index), before the graph.
"""
import time
from typing import Tuple

import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm._actor_critic import FUSED_MAX_WIDTH, ActorCriticBase
from gops_amd.algorithm.base import batch_to_device, cuda_device_of, grad_buffers, install_grads
from gops_amd.apprfunc.mlp import ActionValueDistri, StochaPolicy
from gops_amd.utils.act_distribution import TanhGaussDistribution
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags


def refusal(alg: str, value_name: str, value_words: str, kwargs: dict):
    """Why `create_alg` cannot build SAC / DSAC / DSAC-T from these arguments, or None (POLY / LipsNet are refused before this is asked)."""
    if kwargs.get("policy_func_type") != "MLP" or kwargs.get("value_func_type") != "MLP":
        return f"{alg} runs MLP networks only (policy_func_type {kwargs.get('policy_func_type')!r}, value_func_type {kwargs.get('value_func_type')!r})"
    if kwargs.get("policy_func_name") != "StochaPolicy" or kwargs.get("policy_act_distribution") != "TanhGaussDistribution":
        return (f"{alg} takes a stochastic policy with a tanh-Gaussian action distribution (policy_func_name 'StochaPolicy', "
                f"policy_act_distribution 'TanhGaussDistribution'), not {kwargs.get('policy_func_name')!r} with "
                f"{kwargs.get('policy_act_distribution')!r}: the kernels sample, squash and differentiate that distribution")
    if kwargs.get("value_func_name") != value_name:
        return f"{alg} takes {value_words} (value_func_name {value_name!r}), not {kwargs.get('value_func_name')!r}"
    for key in ("policy", "value"):
        if kwargs.get(f"{key}_output_activation", "linear") != "linear":
            return (f"{alg} takes networks with a linear output layer ({key}_output_activation "
                    f"{kwargs.get(key + '_output_activation')!r}): the HIP kernels apply no output activation")
    if hb.dtype_id(kwargs.get("mlp_dtype")) != 0:
        return f"{alg} is fp32 only (mlp_dtype {kwargs.get('mlp_dtype')!r}): its kernels have no half-precision path"
    if kwargs.get("buffer_name") == "prioritized_replay_buffer":
        return f"{alg} has no priorities (the reference's {alg} returns none): buffer_name 'prioritized_replay_buffer' is not supported"
    trainer = kwargs.get("trainer")
    if trainer is not None and trainer.startswith(("off_sync", "off_async")):
        return f"{alg} runs under off_serial_trainer only: trainer {trainer!r} (data-parallel replicas) has not been run with its update_info"
    return None


class SoftQBase(ActorCriticBase):
    _q_names: Tuple[str, ...] = ()
    _value_cls = None                  # the critics' module class
    _distri = False                    # the backup samples the return of ONE (mean, softplus std) critic (DSAC: `gops_soft_q_backup`)
    _policy_at_obs2 = "policy"         # the policy the backup samples at obs2
    _polyak_names: Tuple[str, ...] = ()
    _OUT: Tuple[str, ...] = ()         # the update's output vector, in this order
    _draws = (("eps_new", lambda B, A: (B, A)), ("eps_next", lambda B, A: (B, A)))   # (name, shape): the update's random inputs
    _signature_terms: Tuple[str, ...] = ()   # further attributes a captured graph depends on

    def _init_soft(self, index: int, fused_target, kwargs: dict):
        nets, name = self.networks, type(self).__name__
        for n in self._q_names:
            if not isinstance(getattr(nets, n), self._value_cls):
                raise NotImplementedError(f"{name}: value network {type(getattr(nets, n)).__name__} (MLP {self._value_cls.__name__} only)")
        if type(nets.policy) is not StochaPolicy or nets.policy.action_distribution_cls is not TanhGaussDistribution:
            raise NotImplementedError(f"{name}: policy {type(nets.policy).__name__} (MLP StochaPolicy with TanhGaussDistribution only)")
        self.per_flag = False
        self.fused_target = "force" if fused_target == "force" else bool(fused_target)
        self.backup_path = None   # "fused" / "composed": how the last update formed the target
        self._noise_seed = int(kwargs.get("seed") or 0) + int(index)
        self._noise_gen = None
        self.tb_info = dict()
        self._cache, self._graphs, self._bufs = {}, {}, {}

    # ---- update API ----------------------------------------------------------------------------
    def _steps_policy(self, iteration: int) -> bool:
        raise NotImplementedError

    def _optimizers(self, step_policy: bool):
        nets = self.networks
        opts = [getattr(nets, f"{n}_optimizer") for n in self._q_names]
        if step_policy:
            opts += [nets.policy_optimizer] + ([nets.alpha_optimizer] if self.auto_alpha else [])
        return opts

    def local_update(self, data: dict, iteration: int):
        start_time = time.time()
        batch = self._batch(data)
        step_policy = self._steps_policy(iteration)
        opts = self._optimizers(step_policy)

        def update(b):
            out = self._gradient_kernels(b)
            self._update(iteration)
            return out

        cache = self._graphs.setdefault(step_policy, StepGraphCache())
        out = cache.run(self._signature(batch, step_policy), batch, update,
                        before_replay=lambda: [o.sync_hyper() for o in opts], on_replay=lambda: [o.advance() for o in opts],
                        work=batch["obs"].shape[0], on_capture_fail=lambda: [o.resync_device_state() for o in opts])
        self._step_schedulers()
        return self._result(out, data, start_time)

    def get_remote_update_info(self, data: dict, iteration: int) -> Tuple[dict, dict]:
        start_time = time.time()
        tb_info = self._result(self._gradient_kernels(self._batch(data)), data, start_time)
        nets = self.networks
        update_info = {f"{n}_grad": [p.grad for p in getattr(nets, n).parameters()] for n in self._q_names + ("policy",)}
        update_info["iteration"] = iteration
        if self.auto_alpha:
            update_info["log_alpha_grad"] = nets.log_alpha.grad
        return tb_info, update_info

    def remote_update(self, update_info: dict):
        nets = self.networks
        for n in self._q_names + ("policy",):
            install_grads(getattr(nets, n), update_info[f"{n}_grad"])
        if self.auto_alpha:
            nets.log_alpha.grad = update_info["log_alpha_grad"]
        self._update(update_info["iteration"])
        self._step_schedulers()

    def _batch(self, data: dict):
        device = cuda_device_of(self.networks)
        batch = batch_to_device(data, device, ("obs", "act", "rew", "obs2", "done"))
        B, A = batch["act"].shape
        for name, shape in self._draws:   # the caller's draws, or this object's - before the graph
            x = data.get(name)
            if x is None:
                if self._noise_gen is None or self._noise_gen.device != device:
                    self._noise_gen = torch.Generator(device=device).manual_seed(self._noise_seed)
                x = torch.randn(shape(B, A), generator=self._noise_gen, device=device, dtype=torch.float32)
            batch[name] = x.to(device=device, dtype=torch.float32).contiguous()
        return batch

    def _result(self, out: torch.Tensor, data: dict, start_time: float):
        tb_info = {key: scalar(out, i) for i, key in enumerate(self._OUT)}
        tb_info[tb_tags["alg_time"]] = (time.time() - start_time) * 1000
        self.tb_info = tb_info
        return tb_info

    def _signature(self, batch, step_policy):
        nets = self.networks
        return (step_policy, self.fused_target, tuple((k, tuple(v.shape)) for k, v in batch.items()), float(self.gamma), float(self.tau),
                bool(self.auto_alpha), float(self.alpha), float(self.target_entropy), bool(getattr(self, "bound", False)),
                tuple(float(getattr(self, n)) for n in self._signature_terms),
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in nets.parameters()),
                tuple(o.storage_signature() for o in self._optimizers(True)),
                tuple(sorted(obj.workspace.data_ptr() for obj in self._cache.values() if hasattr(obj, "workspace"))),
                tuple(sorted(t.data_ptr() for t in self._bufs.values())))

    def _polyak(self):
        nets = self.networks
        for n in self._polyak_names:
            online, target = list(getattr(nets, n).parameters()), list(getattr(nets, f"{n}_target").parameters())
            up = self._cache.get(("polyak", n))
            if up is None or not up.matches(target, online):
                up = self._cache[("polyak", n)] = hb.PolyakUpdater(target, online)
            up.step(self.tau)

    # ---- kernels -------------------------------------------------------------------------------
    def _alpha_tensor(self, device) -> torch.Tensor:
        if self.auto_alpha:
            return self.networks.log_alpha.detach().exp()
        return self._buf(f"alpha={float(self.alpha)!r}", (), device, fill=self.alpha)

    def _backup_modules(self):
        nets = self.networks
        return getattr(nets, self._policy_at_obs2), [getattr(nets, f"{n}_target") for n in self._q_names]

    def _widest_target_layer(self) -> int:
        pol, qs = self._backup_modules()
        return max(l.out_features for m in [pol] + qs for l in m.linear_layers()[:-1])

    def _soft_q_backup(self, B: int, device) -> hb.SoftQBackup:
        nets = self.networks
        pt, q_mods = self._backup_modules()
        pol, qs = pt.hip_mlp(), [m.hip_mlp() for m in q_mods]
        key = ("soft_q_backup", B, str(device), bool(self.auto_alpha))
        sb = self._cache.get(key)
        if sb is None or (self.auto_alpha and sb.log_alpha.data_ptr() != nets.log_alpha.data_ptr()):
            sb = self._cache[key] = hb.SoftQBackup(pol, qs, distri=self._distri, act_low=pt.act_low_lim.cpu().numpy(),
                                                   act_high=pt.act_high_lim.cpu().numpy(), min_log_std=pt.min_log_std,
                                                   max_log_std=pt.max_log_std, batch=B,
                                                   log_alpha=nets.log_alpha.data if self.auto_alpha else None, device=device)
        else:
            sb.set_nets(pol, qs)
        return sb

    def _backup(self, batch) -> torch.Tensor:
        """The soft target [B] of sac.py:214-223 / dsac.py:219-252, no gradient."""
        o2 = batch["obs2"]
        B, device = o2.shape[0], o2.device
        if self.fused_target and (self.fused_target == "force" or self._widest_target_layer() <= FUSED_MAX_WIDTH):
            sb = self._soft_q_backup(B, device)
            if sb.supported:
                self.backup_path = "fused"
                return sb.run(o2, batch["rew"], batch["done"], batch["eps_next"], batch.get("z_next"), gamma=self.gamma,
                              alpha=self.alpha)["backup"]
        self.backup_path = "composed"
        return self._backup_composed(batch)[0]

    def _backup_composed(self, batch):
        """(backup [B], a2 [B, A], logp [B], q_targ - [n_q, B], or [B, 2] = (m, s) for a distributional critic) from `gops_mlp_forward`
        calls and elementwise torch ops."""
        o2, d, r = batch["obs2"], batch["done"], batch["rew"]
        B, device = o2.shape[0], o2.device
        pt, q_mods = self._backup_modules()
        mean, log_std = torch.chunk(self._net(f"{self._policy_at_obs2}@o2", pt, B, device).forward(o2), 2, dim=-1)
        dist = pt.get_act_dist(torch.cat((mean, torch.clamp(log_std, pt.min_log_std, pt.max_log_std).exp()), dim=-1))
        a2, logp = dist.rsample(batch["eps_next"])
        x2 = torch.cat([o2, a2], dim=-1)
        heads = [self._net(f"{n}_target@o2", m, B, device).forward(x2) for n, m in zip(self._q_names, q_mods)]
        if self._distri:
            m, s = heads[0][:, 0], torch.nn.functional.softplus(heads[0][:, 1])
            q_next, q_targ = m + torch.clamp(batch["z_next"], -3, 3) * s, torch.stack((m, s), dim=-1)
        else:
            q_targ = torch.stack([h[:, 0] for h in heads])
            q_next = q_targ[0] if len(heads) == 1 else torch.min(q_targ[0], q_targ[1])
        return r + (1 - d) * self.gamma * (q_next - self._alpha_tensor(device) * logp), a2, logp, q_targ

    def _actor(self, batch):
        """The actor's and the temperature's gradients: mean(alpha logp - min_i q_i(obs, new_act)) through the live critics, their
        parameters frozen; loss_alpha = -log_alpha mean(logp + target_entropy).  -> (loss_policy, the sampling head's statistics
        [mean(logp), mean(tanh(mean)), mean(std), d loss_alpha / d log_alpha], alpha, the policy's raw head [B, 2 A])."""
        nets = self.networks
        o = batch["obs"]
        B, O, device = o.shape[0], o.shape[1], o.device
        pol = nets.policy
        key = ("tanh_gauss", str(device))
        tg = self._cache.get(key)
        if tg is None:
            tg = self._cache[key] = hb.TanhGaussHead(pol.act_low_lim.cpu().numpy(), pol.act_high_lim.cpu().numpy(), pol.min_log_std,
                                                     pol.max_log_std, device)
        pol_o = self._net("policy@o", pol, B, device)
        head = pol_o.forward(o)
        new_act, _, tstats = tg.forward(head, batch["eps_new"], self.target_entropy, act=self._buf("new_act", batch["act"].shape, device),
                                        logp=self._buf("new_logp", (B,), device))
        xq = torch.cat([o, new_act], dim=-1)
        pi_nets = [self._net(f"{n}@pi", getattr(nets, n), B, device) for n in self._q_names]
        qs = [net.forward(xq)[:, 0] for net in pi_nets]
        if len(qs) == 2:   # the row's seed goes to whichever critic is the minimum
            first = (qs[0] <= qs[1]).to(torch.float32)
            share, q_min = [first, 1 - first], torch.min(qs[0], qs[1])
        else:
            share, q_min = [torch.ones_like(qs[0])], qs[0]
        # (mean, softplus std) critic heads: the std output carries no gradient
        zero = [torch.zeros_like(qs[0])] if issubclass(self._value_cls, ActionValueDistri) else []
        g_xq = None
        for net, w in zip(pi_nets, share):
            cols = [w * (-1.0 / B)] + zero
            g = net.backward_x(xq, torch.stack(cols, dim=-1))
            g_xq = g if g_xq is None else g_xq + g
        alpha = self._alpha_tensor(device)
        g_head = tg.backward(head, batch["eps_new"], g_xq[:, O:].contiguous(), (alpha / B).expand(B).contiguous())
        gw, gb = grad_buffers(pol)
        pol_o.backward(o, g_head, gw, gb)
        if self.auto_alpha:
            if nets.log_alpha.grad is None:
                nets.log_alpha.grad = torch.zeros_like(nets.log_alpha)
            nets.log_alpha.grad.copy_(tstats[3])
        return alpha * tstats[0] - q_min.mean(), tstats, alpha, head
