"""What DDPG and TD3 share on the HIP kernels: one update = Bellman backup (no grad), critic regression, actor gradient through
the live critic, Adam per network, Polyak on every target.

Where the arithmetic runs:
  * the backup - target policy, TD3's clipped target noise, target critic(s), minimum, `r + gamma (1 - d) q` - is ONE launch of
    `gops_ac_backup` (`fused_target=True`, the default, for networks up to 64 wide - where it was measured faster; "force": for
    every shape the kernel holds), or composed from `gops_mlp_forward` calls and elementwise torch ops (`fused_target=False`, wider
    networks, and whenever the kernel refuses the shape); `backup_path` names what the last update ran;
  * seeds `2 w (q_i - backup) / B`, the losses, mean(q) and PER's `|q - backup|` are one launch of `gops_ac_critic_loss`;
  * everything with gradients is `gops_mlp_forward / _backward / _backward_x` over the concatenated (obs, act) input, `HipAdam`
    and `gops_polyak_update`.
`local_update` replays as a HIP graph (one per value of `iteration % delay_update == 0`); the batch - with TD3's unit-normal
draws `target_noise` - is the graph's input.
"""
import time
from typing import Tuple

import numpy as np
import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm.base import AlgorithmBase, batch_to_device, cuda_device_of, grad_buffers, install_grads
from gops_amd.apprfunc.mlp import ActionValue, DetermPolicy
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags

# `fused_target=True` takes the one-launch backup where it was measured to win (TD3 update, ms fused / composed, graph
# replay: 64-64 nets 0.250 / 0.303 at B = 256 and 0.869 / 0.981 at B = 65536; 256-256 nets 0.602 / 0.496 and 3.50 / 2.14 - the
# fp32 fmaf kernel loses to the matrix-core kernels behind `gops_mlp_forward` once the layers are wide); "force" takes it wherever
# the kernel holds the shape.
FUSED_MAX_WIDTH = 64
N_SCALARS = 4   # loss_q, critic value to log, loss_policy, (spare): the head of the update's output vector, PER's abs_err behind it


def refusal(alg: str, kwargs: dict):
    """Why `create_alg` cannot build DDPG / TD3 from these arguments, or None (POLY / LipsNet are refused before this is asked)."""
    if kwargs.get("policy_func_type") != "MLP" or kwargs.get("value_func_type") != "MLP":
        return f"{alg} runs MLP networks only (policy_func_type {kwargs.get('policy_func_type')!r}, value_func_type {kwargs.get('value_func_type')!r})"
    if kwargs.get("policy_func_name") != "DetermPolicy":
        return (f"{alg} takes a deterministic policy (policy_func_name 'DetermPolicy'), not {kwargs.get('policy_func_name')!r}: "
                "stochastic policies are outside the HIP path")
    if kwargs.get("value_func_name") != "ActionValue":
        return f"{alg} takes an action-value function (value_func_name 'ActionValue'), not {kwargs.get('value_func_name')!r}"
    for key in ("policy", "value"):   # (`hip_mlp()` and `gops_ac_backup` describe a linear output layer)
        if kwargs.get(f"{key}_output_activation", "linear") != "linear":
            return (f"{alg} takes networks with a linear output layer ({key}_output_activation "
                    f"{kwargs.get(key + '_output_activation')!r}): the HIP kernels apply no output activation")
    trainer = kwargs.get("trainer")
    if trainer is not None and trainer.startswith(("off_sync", "off_async")):
        return (f"{alg} runs under off_serial_trainer only: trainer {trainer!r} (data-parallel replicas) has not been run with its "
                "update_info, least of all with a prioritized buffer's (tb_info, idx, abs_err)")
    if hb.dtype_id(kwargs.get("mlp_dtype")) != 0:
        return f"{alg} is fp32 only (mlp_dtype {kwargs.get('mlp_dtype')!r}): its kernels have no half-precision path"
    return None


class NetCache:
    """The kernel objects and scratch tensors an update keeps between calls (`self._cache`, `self._bufs`); DQN (algorithm/dqn.py) keeps
    its own the same way."""

    def _net(self, role: str, module, B: int, device) -> hb.MlpNet:
        """One MlpNet (own activation stash) per use of a network inside an update: a backward follows ITS forward."""
        key = (role, B, str(device))
        mlp = module.hip_mlp()
        net = self._cache.get(key)
        if net is None:
            net = self._cache[key] = hb.MlpNet(mlp, B, device=device)
        else:
            net.mlp = mlp
        return net

    def _buf(self, name: str, shape, device, fill=None) -> torch.Tensor:
        key = (name, tuple(shape), str(device))
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = (torch.empty(shape, dtype=torch.float32, device=device) if fill is None else
                                   torch.full(shape, float(fill), dtype=torch.float32, device=device))
        return t


class ActorCriticBase(NetCache, AlgorithmBase):
    _q_names: Tuple[str, ...] = ("q",)   # the critics; the first one carries the actor gradient and PER's priorities
    _smooth = False                      # TD3's target-policy smoothing

    def _init_common(self, index: int, buffer_name: str, fused_target: bool, kwargs: dict):
        nets = self.networks
        for n in self._q_names:
            if not isinstance(getattr(nets, n), ActionValue):
                raise NotImplementedError(f"{type(self).__name__}: value network {type(getattr(nets, n)).__name__} (MLP ActionValue only)")
        if type(nets.policy) is not DetermPolicy:
            raise NotImplementedError(f"{type(self).__name__}: policy {type(nets.policy).__name__} (MLP DetermPolicy only)")
        self.per_flag = buffer_name == "prioritized_replay_buffer"
        self.fused_target = "force" if fused_target == "force" else bool(fused_target)
        self.backup_path = None   # "fused" / "composed": how the last update formed the backup
        self.act_low_limit = kwargs["action_low_limit"]
        self.act_high_limit = kwargs["action_high_limit"]
        self._noise_seed = int(kwargs.get("seed") or 0) + int(index)
        self._noise_gen = None
        self.tb_info = dict()
        self._cache, self._graphs, self._bufs = {}, {}, {}

    # ---- update API ----------------------------------------------------------------------------
    def local_update(self, data: dict, iteration: int):
        start_time = time.time()
        batch = self._batch(data)
        step_policy = iteration % self.delay_update == 0
        opts = [getattr(self.networks, f"{n}_optimizer") for n in self._q_names + (("policy",) if step_policy else ())]

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
        extra_info = self._result(self._gradient_kernels(self._batch(data)), data, start_time)
        update_info = {f"{n}_grad": [p.grad for p in getattr(self.networks, n).parameters()] for n in self._q_names + ("policy",)}
        update_info["iteration"] = iteration
        return extra_info, update_info

    def remote_update(self, update_info: dict):
        for n in self._q_names + ("policy",):
            install_grads(getattr(self.networks, n), update_info[f"{n}_grad"])
        self._update(update_info["iteration"])
        self._step_schedulers()

    def _batch(self, data: dict):
        device = cuda_device_of(self.networks)
        batch = batch_to_device(data, device, ("obs", "act", "rew", "obs2", "done") + (("weight",) if self.per_flag else ()))
        if self._smooth:   # the unit-normal draws are an input of the update: the caller's, or drawn here - before the graph
            xi = data.get("target_noise")
            if xi is None:
                if self._noise_gen is None or self._noise_gen.device != device:
                    self._noise_gen = torch.Generator(device=device).manual_seed(self._noise_seed)
                xi = torch.randn(batch["act"].shape, generator=self._noise_gen, device=device, dtype=torch.float32)
            batch["target_noise"] = xi.to(device=device, dtype=torch.float32).contiguous()
        return batch

    def _result(self, out: torch.Tensor, data: dict, start_time: float):
        tb_info = dict()
        tb_info[tb_tags["loss_critic"]] = scalar(out, 0)
        tb_info[tb_tags["critic_avg_value"]] = scalar(out, 1)
        tb_info[tb_tags["alg_time"]] = (time.time() - start_time) * 1000
        tb_info[tb_tags["loss_actor"]] = scalar(out, 2)
        self.tb_info = tb_info
        if self.per_flag:
            return tb_info, data["idx"], out[N_SCALARS:]
        return tb_info

    def _signature(self, batch, step_policy):
        nets = self.networks
        opts = [getattr(nets, f"{n}_optimizer") for n in self._q_names + ("policy",)]
        return (step_policy, self.fused_target, tuple((k, tuple(v.shape)) for k, v in batch.items()), float(self.gamma), float(self.tau),
                float(getattr(self, "reward_scale", 1.0)), float(getattr(self, "target_noise", 0.0)), float(getattr(self, "noise_clip", 0.0)),
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for m in nets.children() for p in m.parameters()),
                tuple(o.storage_signature() for o in opts),
                tuple(sorted(obj.workspace.data_ptr() for obj in self._cache.values() if hasattr(obj, "workspace"))),
                tuple(sorted(t.data_ptr() for t in self._bufs.values())))

    def _update(self, iteration):
        nets = self.networks
        for n in self._q_names:
            getattr(nets, f"{n}_optimizer").step()
        if iteration % self.delay_update == 0:
            nets.policy_optimizer.step()
        self._polyak()

    def _polyak(self):
        nets, polyak = self.networks, 1 - self.tau
        for n in self._q_names + ("policy",):   # p_targ <- polyak p_targ + (1 - polyak) p   (ddpg.py:182-193, td3.py:234-251)
            online, target = list(getattr(nets, n).parameters()), list(getattr(nets, f"{n}_target").parameters())
            up = self._cache.get(("polyak", n))
            if up is None or not up.matches(target, online):
                up = self._cache[("polyak", n)] = hb.PolyakUpdater(target, online)
            up.step(1 - polyak)

    # ---- kernels -------------------------------------------------------------------------------
    @staticmethod
    def _squash(pol, pre):
        """(action, d action / d pre) of DetermPolicy's tanh squash (apprfunc/mlp.py: `_squash`)."""
        half = (pol.act_high_lim - pol.act_low_lim) / 2
        th = torch.tanh(pre)
        return half * th + (pol.act_high_lim + pol.act_low_lim) / 2, half * (1 - th * th)

    def _limits(self, device):
        key = ("limits", str(device))
        lim = self._bufs.get(key)
        if lim is None:
            lim = self._bufs[key] = torch.tensor(np.stack([np.asarray(self.act_low_limit, dtype=np.float32).reshape(-1),
                                                           np.asarray(self.act_high_limit, dtype=np.float32).reshape(-1)]), device=device)
        return lim[0], lim[1]

    def _ac_backup(self, B: int, device) -> hb.AcBackup:
        nets = self.networks
        pol = nets.policy_target.hip_mlp()
        qs = [getattr(nets, f"{n}_target").hip_mlp() for n in self._q_names]
        key = ("ac_backup", B, str(device))
        ab = self._cache.get(key)
        if ab is None:
            pt = nets.policy_target
            ab = self._cache[key] = hb.AcBackup(pol, qs, squash_low=pt.act_low_lim.cpu().numpy(), squash_high=pt.act_high_lim.cpu().numpy(),
                                                act_low=self.act_low_limit, act_high=self.act_high_limit, batch=B, smooth=self._smooth,
                                                device=device)
        else:
            ab.set_nets(pol, qs)
        return ab

    def _backup(self, batch) -> torch.Tensor:
        """`r + gamma (1 - d) min_i q_i_target(o2, a2)` [B], no gradient (ddpg.py:149-151, td3.py:166-183)."""
        nets = self.networks
        o2, d, r = batch["obs2"], batch["done"], batch["rew"]
        B, device = o2.shape[0], o2.device
        rs = float(getattr(self, "reward_scale", 1.0))
        if self.fused_target and (self.fused_target == "force" or self._widest_target_layer() <= FUSED_MAX_WIDTH):
            ab = self._ac_backup(B, device)
            if ab.supported:
                self.backup_path = "fused"
                return ab.run(o2, r, d, batch.get("target_noise"), target_noise=getattr(self, "target_noise", 0.0),
                              noise_clip=getattr(self, "noise_clip", 0.0), reward_scale=rs, gamma=self.gamma)["backup"]
        self.backup_path = "composed"
        return self._backup_composed(batch)[0]

    def _widest_target_layer(self) -> int:
        nets = self.networks
        mods = [nets.policy_target] + [getattr(nets, f"{n}_target") for n in self._q_names]
        return max(l.out_features for m in mods for l in m.linear_layers()[:-1])

    def _backup_composed(self, batch):
        """(backup [B], a2 [B, A], q_targ [n_q, B]) from `gops_mlp_forward` calls and elementwise torch ops."""
        nets = self.networks
        o2, d, r = batch["obs2"], batch["done"], batch["rew"]
        B, device = o2.shape[0], o2.device
        a2, _ = self._squash(nets.policy_target, self._net("policy_target@o2", nets.policy_target, B, device).forward(o2))
        if self._smooth:
            low, high = self._limits(device)
            eps = torch.clamp(batch["target_noise"] * self.target_noise, -self.noise_clip, self.noise_clip)
            a2 = torch.clamp(a2 + eps, low, high)
        x2 = torch.cat([o2, a2], dim=-1)
        q_t = [self._net(f"{n}_target@o2", getattr(nets, f"{n}_target"), B, device).forward(x2).squeeze(-1) for n in self._q_names]
        q_min = q_t[0] if len(q_t) == 1 else torch.min(q_t[0], q_t[1])
        if hasattr(self, "reward_scale"):
            r = r * self.reward_scale
        return r + self.gamma * (1 - d) * q_min, a2, torch.stack(q_t)

    def _gradient_kernels(self, batch) -> torch.Tensor:
        """Enqueue one compute_gradient; returns [loss_q, logged critic value, loss_policy, 0] (+ abs_err [B] with PER) as one
        device tensor, without synchronising."""
        nets = self.networks
        o, a = batch["obs"], batch["act"]
        B, O, device = o.shape[0], o.shape[1], o.device
        nq = len(self._q_names)
        backup = self._backup(batch)

        # ---- critic regression ---------------------------------------------------------------------
        x = torch.cat([o, a], dim=-1)
        q = self._buf("q", (nq, B), device)
        q_nets = [self._net(f"{n}@data", getattr(nets, n), B, device) for n in self._q_names]
        for i, net in enumerate(q_nets):
            net.forward(x, out=q[i])
        key = ("critic_loss", str(device))
        cl = self._cache.get(key)
        if cl is None:
            cl = self._cache[key] = hb.AcCriticLoss(device)
        seed, abs_err, stats = cl.run(q, backup, batch.get("weight") if self.per_flag else None,
                                      seed=self._buf("seed", (nq, B), device), abs_err=self._buf("abs_err", (B,), device))
        for i, (n, net) in enumerate(zip(self._q_names, q_nets)):
            gw, gb = grad_buffers(getattr(nets, n))
            net.backward(x, seed[i].unsqueeze(-1), gw, gb)

        # ---- actor: -mean q(o, pi(o)) through the live first critic, its parameters frozen -----------
        pol_o = self._net("policy@o", nets.policy, B, device)
        a0, da0 = self._squash(nets.policy, pol_o.forward(o))
        xq = torch.cat([o, a0], dim=-1)
        q_pi_net = self._net(f"{self._q_names[0]}@pi", getattr(nets, self._q_names[0]), B, device)
        q_pi = q_pi_net.forward(xq)
        g_xq = q_pi_net.backward_x(xq, self._buf("actor_seed", (B, 1), device, fill=-1.0 / B))
        gw, gb = grad_buffers(nets.policy)
        pol_o.backward(o, (g_xq[:, O:] * da0).contiguous(), gw, gb)

        head = torch.stack([self._loss_q(stats), self._logged_value(stats), -q_pi.mean(), stats[3] * 0])
        return torch.cat([head, abs_err]) if self.per_flag else head

    def _loss_q(self, stats):
        return stats[3] if len(self._q_names) == 2 else stats[0]

    def _logged_value(self, stats):
        raise NotImplementedError

