"""INFADP - infinite-horizon approximate dynamic programming - on the fused HIP rollout.

Same class surface as the reference's gops/algorithm/infadp.py (ApproxContainer :31-64, INFADP
:67-213): alternating policy evaluation (PEV: regress V(o) onto the n-step model return plus the
bootstrapped target value, rollout without gradient) and policy improvement (PIM: ascend the
same quantity through policy, model and the target value's input), Adam + Polyak target update.
"""
__all__ = ["INFADP"]

import os
import time
from copy import deepcopy
from typing import Tuple

import torch
from gops_amd.utils.common_utils import make_adam

from gops_amd import hip_backend as hb
from gops_amd.algorithm._model_based import ModelBasedBase, lane_alg_check, lane_env_check, polyak_foreach_
from gops_amd.algorithm.base import ApprBase, PrecisionGuard, install_grads, is_poly, is_rbf, net_grad_buffers, rbf_grad_buffers
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.utils.common_utils import get_apprfunc_dict
from gops_amd.utils.tensorboard_setup import tb_tags


class ApproxContainer(ApprBase):
    """Value + policy networks, frozen target copies, one Adam per online network.  The value
    network is constructed BEFORE the policy (RNG draw order of the reference, infadp.py:41-42)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        v_args = get_apprfunc_dict("value", **kwargs)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.v = create_apprfunc(**v_args)
        self.policy = create_apprfunc(**policy_args)
        self.v_target = deepcopy(self.v)
        self.policy_target = deepcopy(self.policy)
        for p in list(self.v_target.parameters()) + list(self.policy_target.parameters()):
            p.requires_grad = False
        # a LipsNet policy trains its two parameter groups at their own learning rates (reference lipsnet.py:211-221): one HipAdam
        # with two groups - a launch and a device state block per group
        self.policy_optimizer = make_adam(self.policy.param_groups() if getattr(self.policy, "is_lipsnet", False)
                                          else self.policy.parameters(), lr=kwargs["policy_learning_rate"])
        self.v_optimizer = make_adam(self.v.parameters(), lr=kwargs["value_learning_rate"])
        self.net_dict = {"v": self.v, "policy": self.policy}
        self.target_net_dict = {"v": self.v_target, "policy": self.policy_target}
        self.optimizer_dict = {"v": self.v_optimizer, "policy": self.policy_optimizer}

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class INFADP(ModelBasedBase):
    """forward_step: model rollout length; gamma; tau: Polyak factor; pev_step / pim_step:
    alternation period of evaluation and improvement."""

    def __init__(self, index=0, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.envmodel = create_env_model(**kwargs)
        self.gamma = 0.99
        self.tau = 0.005
        self.pev_step = 1
        self.pim_step = 1
        self.forward_step = 10
        # arithmetic of the MLP contractions: "fp32" (exact, the 1e-4 parity path) or "fp16" (half-precision
        # MFMA, BASELINE.json configs[4])
        self.mlp_dtype = kwargs.get("mlp_dtype", "fp32")
        self._graphs = {}
        self._polyak = {}   # net name -> hb.PolyakUpdater
        # measured rule for leaving the plane-split forward (algorithm/base.py PrecisionGuard), one per trained network
        self.precision_guard = {m: PrecisionGuard(kwargs.get("precision_check_interval"), kwargs.get("precision_threshold")) for m in ("v", "policy")}
        self._bufs = {}     # persistent device scratch: loss gradient, loss scalars (read them before the next update of the same mode)
        # POLY policy AND value (apprfunc/poly.py): the one-lane-per-trajectory rollout (hb.PolyRollout) and hb.PolyValueNet
        self._poly = is_poly(self.networks.policy)
        self._plain = self._is_plain(INFADP)   # (a subclass with gradient kernels or an update of its own stays off the paths below)
        if self._poly != is_poly(self.networks.v):
            raise NotImplementedError("INFADP: a POLY policy needs a POLY value and the reverse (the rollout's tail value is "
                                      "evaluated by the policy's kernel)")
        if self._poly:
            if not self._plain:
                raise NotImplementedError(f"{type(self).__name__} with an apprfunc of type POLY: only plain INFADP runs the POLY rollout")
            lane_env_check(self.envmodel, type(self).__name__, "POLY")
            lane_alg_check(self, time_input=False, family="POLY")
        # GAUSS policy (apprfunc/gauss.py) with an MLP value: the RBF rollout has no tail, the host composes it (`_rbf_return`)
        self._rbf = is_rbf(self.networks.policy)
        if is_rbf(self.networks.v):
            raise NotImplementedError("INFADP with a GAUSS value function: the reference itself cannot run it (its [B, 1] value does "
                                      "not broadcast into the in-place backup)")
        if self._rbf:
            name = type(self).__name__
            if not self._plain:
                raise NotImplementedError(f"{name} with an apprfunc of type GAUSS: only plain INFADP runs the RBF rollout")
            if self._poly or getattr(self.networks.v, "is_lipsnet", False) or not hasattr(self.networks.v, "hip_mlp"):
                raise NotImplementedError(f"{name} with a GAUSS policy needs an MLP StateValue")
            lane_env_check(self.envmodel, name, "GAUSS")
            lane_alg_check(self, time_input=False, family="GAUSS")
        # LipsNet policy (apprfunc/lipsnet.py): the policy sits OUTSIDE an open-loop one-step rollout (`_lips_return`)
        self._lips = bool(getattr(self.networks.policy, "is_lipsnet", False))
        if self._lips:
            name = type(self).__name__
            if not self._plain:
                raise NotImplementedError(f"{name} with a LipsNet policy: only plain INFADP composes the LipsNet kernels with the model rollout")
            if self._poly or getattr(self.networks.v, "is_lipsnet", False) or not hasattr(self.networks.v, "hip_mlp"):
                raise NotImplementedError(f"{name} with a LipsNet policy needs an MLP StateValue")
            if hb.dtype_id(self.mlp_dtype) != 0:
                raise NotImplementedError(f"{name} with a LipsNet policy: mlp_dtype {self.mlp_dtype!r} - the LipsNet path is fp32 only")
            if getattr(self.envmodel.unwrapped, "hip_kind", None) not in hb.STATE_OBS_ENV_KINDS:   # (gops_rollout_backward_open_loop_adj's env kinds)
                raise NotImplementedError(f"{name} with a LipsNet policy: env model {type(self.envmodel.unwrapped).__name__} is outside the "
                                          "path (models whose observation is the state: pyth_lq, pyth_idpendulum, gym cartpoleconti / pendulum)")

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "pev_step", "pim_step", "forward_step", "reward_scale")

    LIPS_FORWARD_STEP_ERROR = ("INFADP with a LipsNet policy is defined for forward_step = 1 only: with lips_auto_adjust the reference itself "
                               "fails on longer rollouts (the second firing of its backward hook calls .backward() on the integer 0), and "
                               "without it they need the policy's input gradient through the Jacobian norm, which the kernels do not form")

    def set_parameters(self, param_dict):
        super().set_parameters(param_dict)
        if getattr(self, "_lips", False) and "forward_step" in param_dict and self.forward_step != 1:
            raise NotImplementedError(self.LIPS_FORWARD_STEP_ERROR)

    def local_update(self, data: dict, iteration: int) -> dict:
        # gradient + Adam + Polyak of the iteration's mode as one HIP graph when the update is launch-bound
        # (replay batches of the shipped examples are 64-256 samples); eager kernels otherwise
        start_time = time.time()
        batch = self._model_batch(data)
        mode = self._mode(iteration)
        opt = self.networks.optimizer_dict[mode]
        self._precision_check(mode, batch)

        # The plain algorithm: Adam step, Polyak step of the target (and, for PIM, the loss mean) ride on the backward's last launch
        # (ABI v12, gops_rollout_backward_update / gops_value_backward_update)
        fuse = self._plain and os.environ.get("GOPS_FUSED_UPDATE", "1") != "0"   # (host-side A/B knob)
        fuse = fuse and not self._poly   # (POLY: Adam and Polyak steps as launches of their own)
        fuse = fuse and not self._lips   # (LipsNet: two optimizer groups, more tensors than one fused table)
        fuse = fuse and not self._rbf    # (GAUSS: the return is composed on the host; Adam and Polyak steps as launches of their own)

        def update(b):
            if fuse:
                scalars, stepped = self._gradient_kernels(mode, b, fused_opt=opt)
                self._update([mode], optimizer_stepped=stepped)   # (stepped: Adam AND Polyak were part of the backward call)
                return scalars
            scalars = self._gradient_kernels(mode, b)
            self._update([mode])
            return scalars

        opt.grad_scale = 1.0   # (a data-parallel remote_update may have left 1/N behind)
        if self._lips:
            # No HIP-graph replay on this path: the composition allocates its intermediate tensors (actions, final observation,
            # adjoints) per call and `LipsPolicy` re-reads the module's training flag on the host at every forward - a replay would
            # freeze both.
            self._log(mode, update(batch), start_time)
            return self.tb_info
        cache = self._graphs.setdefault(mode, StepGraphCache())
        scalars = cache.run(self._signature(mode, batch), batch, update, before_replay=opt.sync_hyper,
                            on_replay=opt.advance, work=batch["obs"].shape[0] * self.forward_step,
                            on_capture_fail=opt.resync_device_state)
        self._log(mode, scalars, start_time)
        return self.tb_info

    accepts_grad_scale = True   # remote_update honours update_info["_grad_scale"] (trainer/grad_sync.py)

    def get_remote_update_info(self, data: dict, iteration: int) -> Tuple[dict, dict]:
        # Data-parallel path: no host sync between the backward sweep and the gradient all-reduce - the loss
        # scalars stay on the device in tb_info and are read at log time.
        start_time = time.time()
        batch = self._model_batch(data)
        mode = self._mode(iteration)
        self._precision_check(mode, batch)
        scalars = self._gradient_kernels(mode, batch)
        if mode == "v":
            self.tb_info[tb_tags["loss_critic"]], self.tb_info[tb_tags["critic_avg_value"]] = scalars[0], scalars[1]
        else:
            self.tb_info[tb_tags["loss_actor"]] = scalars[0]
        self.tb_info[tb_tags["alg_time"]] = (time.time() - start_time) * 1000  # ms of host enqueue time
        update_info = {mode: [p.grad for p in self.networks.net_dict[mode].parameters()]}
        return self.tb_info, update_info

    def remote_update(self, update_info: dict):
        names = [k for k in update_info if not k.startswith("_")]
        for net_name in names:
            install_grads(self.networks.net_dict[net_name], update_info[net_name])
            self.networks.optimizer_dict[net_name].grad_scale = float(update_info.get("_grad_scale", 1.0))
        self._update(names)
        for net_name in names:   # a later local_update on this object must not inherit the 1/N
            self.networks.optimizer_dict[net_name].grad_scale = 1.0

    def _update(self, update_list, optimizer_stepped=False):
        tau = self.tau
        if optimizer_stepped:   # Adam and Polyak step were part of the backward call (_gradient_kernels(fused_opt=))
            return
        for net_name in update_list:
            self.networks.optimizer_dict[net_name].step()
        with torch.no_grad():
            for net_name in update_list:   # Polyak averaging (reference :124-133), all tensors of the network in one launch
                online = list(self.networks.net_dict[net_name].parameters())
                target = list(self.networks.target_net_dict[net_name].parameters())
                if not online[0].is_cuda:
                    polyak_foreach_(target, online, tau)
                    continue
                pk = self._polyak.get(net_name)
                if pk is None or not pk.matches(target, online):
                    pk = self._polyak[net_name] = hb.PolyakUpdater(target, online)
                pk.step(tau)

    # ------------------------------------------------------------------------------------------
    def _rollout_for(self, batch: int, device, need_grad: bool) -> hb.Rollout:
        nets = self.networks
        flags = self._variant_flags("policy" if need_grad else "v")   # (PEV's gradient-free backup belongs to the value update)
        key = (batch, self.forward_step, float(self.gamma), str(device), need_grad, hb.dtype_id(self.mlp_dtype), flags)
        pol, vt = nets.policy.hip_mlp(), nets.v_target.hip_mlp()
        return self._cached(key, lambda: (hb.PolyRollout if self._poly else hb.Rollout)(
            self._hip_env(), pol, batch=batch, horizon=self.forward_step, gamma=self.gamma, finite_horizon=False, need_grad=need_grad,
            value=vt, device=device, dtype=self.mlp_dtype, variant_flags=flags), lambda ro: ro.set_policy(pol, vt))

    def _value_for(self, batch: int, device) -> hb.ValueNet:
        flags = self._variant_flags("v")
        key = ("v", batch, str(device), hb.dtype_id(self.mlp_dtype), flags)
        mlp = self.networks.v.hip_mlp(self.mlp_dtype, variant_flags=flags)
        if self._poly:
            return self._cached(key, lambda: hb.PolyValueNet(mlp, batch, self.envmodel.hip_env().obs_dim, device=device),
                                lambda vn: vn.set_net(mlp))
        return self._cached(key, lambda: hb.ValueNet(mlp, batch, device=device), lambda vn: setattr(vn, "mlp", mlp))

    def _precision_check(self, mode: str, batch):
        """The guard of the network this iteration trains, on ITS gradients."""
        nets = self.networks
        if self._rbf and mode == "policy":   # (the RBF rollout has no kernel variants: nothing to compare; the value update keeps its guard)
            return
        self._guard_check(self.precision_guard[mode], (nets.policy, nets.v), lambda: self._gradient_kernels(mode, batch), nets.net_dict[mode])

    def _mode(self, iteration) -> str:
        return "v" if iteration % (self.pev_step + self.pim_step) < self.pev_step else "policy"

    def _gradient_kernels(self, mode: str, batch, fused_opt=None) -> torch.Tensor:
        """Enqueue one policy-evaluation ("v") or policy-improvement ("policy") gradient; returns the
        device scalars the log needs ([loss_v, mean V] / [loss_policy]) without synchronising."""
        B, device = batch["obs"].shape[0], batch["obs"].device
        if self._lips and mode == "policy":
            return self._lips_improvement(batch)
        if self._rbf and mode == "policy":
            return self._rbf_improvement(batch)
        if mode == "v":
            # PEV: loss_v = mean((V(o) - [sum_t gamma^t r_t + (~d) gamma^n V_target(o_n)])^2)
            backup = (self._lips_return(batch, need_grad=False)[0] if self._lips
                      else self._rbf_return(batch, need_grad=False)[0] if self._rbf
                      else self._rollout_for(B, device, need_grad=False).forward(batch)["v_pi"])
            vn = self._value_for(B, device)
            v = vn.forward(batch["obs"])
            # loss_v, mean V and d(loss_v)/dV = (2 / B)(V - backup) in one launch (they were six torch passes)
            gdiff = self._scratch("gdiff", B, device)
            scalars = self._loss_stats("v", device).value_loss(v, backup, gdiff)
            gw, gb = net_grad_buffers(self.networks.v)
            if fused_opt is not None:   # -> (scalars, whether Adam + Polyak were part of the backward call)
                fa, pk = self._fused_parts("v", fused_opt)
                if fa is None:
                    vn.backward(batch["obs"], gdiff, gw, gb)
                    return scalars, False
                vn.backward(batch["obs"], gdiff, gw, gb, tail=hb.make_update_tail(fa, polyak=pk, tau=self.tau))
                fused_opt.end_fused()
                return scalars, True
            vn.backward(batch["obs"], gdiff, gw, gb)
            return scalars
        # PIM: loss = -mean(sum_t gamma^t r_t + (~d) gamma^n V_target(o_n)), grads into the policy
        ro = self._rollout_for(B, device, need_grad=True)
        v_pi = ro.forward(batch)["v_pi"]
        gw, gb = net_grad_buffers(self.networks.policy)
        if fused_opt is not None:   # -> (scalars, whether Adam + Polyak were part of the backward call)
            fa, pk = self._fused_parts("policy", fused_opt)
            stats = self._loss_stats("policy", device)
            if fa is None:
                ro.backward(self._grad_v(B, device), gw, gb)
                return stats.mean_loss(v_pi, -1.0)[:1], False
            ro.backward(self._grad_v(B, device), gw, gb, tail=hb.make_update_tail(fa, v_pi, -1.0, stats, polyak=pk, tau=self.tau))
            fused_opt.end_fused()
            return stats.buf[:1], True
        stats = self._loss_stats("policy", device)   # (the loss mean rides on the backward's reduce launch: it needs no gradient)
        if self._poly:   # (POLY: the loss mean in a launch of its own)
            ro.backward(self._grad_v(B, device), gw, gb)
            return stats.mean_loss(v_pi, -1.0)[:1]
        ro.backward(self._grad_v(B, device), gw, gb, tail=hb.make_update_tail(None, v_pi, -1.0, stats))
        return stats.buf[:1]

    # ---- LipsNet policy: policy -> wrapper chain on the action -> open-loop one-step rollout -> target value -----------------------
    def _lips_parts(self, B, device, need_grad):
        def make():
            env = self._hip_env()
            ro = hb.Rollout(env, None, batch=B, horizon=1, gamma=self.gamma, finite_horizon=False, need_grad=need_grad,
                            device=device, raw_actions=True)
            A = env.act_dim
            t = lambda v: torch.tensor([float(v[i]) for i in range(A)], dtype=torch.float32, device=device)   # noqa: E731
            return dict(ro=ro, lp=hb.LipsPolicy(self.networks.policy, B, device=device), wrap=tuple(
                t(v) for v in (env.min_action, env.max_action, env.act_low, env.act_high)))
        return self._cached(("lips", B, str(device), need_grad, float(self.gamma)), make)

    def _lips_return(self, batch, need_grad):
        """r + gamma (1 - done') V_target(obs') of one wrapped model step under the LipsNet policy -> (value [B], what the backward
        needs).  `open_loop = 2` of the rollout takes the MODEL action: ScaleAction / ClipAction (create_env_model.py:120-126) act on the
        policy's output here, between the two launches, exactly as `wrap_action` of csrc/common.h does inside a closed-loop rollout;
        MaskAtDone, ShapingReward and the observation wrappers are the rollout's."""
        if self.forward_step != 1:
            raise NotImplementedError(self.LIPS_FORWARD_STEP_ERROR)
        B, device = batch["obs"].shape[0], batch["obs"].device
        parts = self._lips_parts(B, device, need_grad)
        pol = self.networks.policy
        act, K, _ = parts["lp"].forward(batch["obs"], training=need_grad and pol.training)
        mn, mx, lo, hi = parts["wrap"]
        a2 = lo + (hi - lo) * ((act.clamp(mn, mx) - mn) / (mx - mn))
        u = a2.clamp(lo, hi)
        res = parts["ro"].forward(batch, head_pre=u.unsqueeze(1).contiguous(), want_final=True)
        vt = self._lips_vt(B, device, need_grad)
        v_next = vt.forward(res["final_obs"]).reshape(B)
        tail = float(self.gamma) * (1.0 - res["final_done"])
        value = res["v_pi"] + tail * v_next
        pass_through = ((act >= mn) & (act <= mx) & (a2 >= lo) & (a2 <= hi)).float() * ((hi - lo) / (mx - mn))
        return value, dict(parts=parts, vt=vt, res=res, tail=tail, pass_through=pass_through, K=K)

    def _lips_vt(self, B, device, need_grad):
        mlp = self.networks.v_target.hip_mlp()
        return self._cached(("lips_vt", B, str(device), need_grad), lambda: hb.MlpNet(mlp, B, device=device), lambda net: setattr(net, "mlp", mlp))

    def _lips_improvement(self, batch):
        """PIM: loss = -mean(value); the adjoint walks back through the target value's input, the model step and the action
        wrappers into `LipsPolicy.backward`, which adds the regular loss's gradient in training mode (not part of the logged loss,
        as in the reference)."""
        B, device = batch["obs"].shape[0], batch["obs"].device
        value, ctx = self._lips_return(batch, need_grad=True)
        gv = self._grad_v(B, device)
        g_obs2 = ctx["vt"].backward_x(ctx["res"]["final_obs"], (gv * ctx["tail"]).unsqueeze(1).contiguous())
        g_u, _ = ctx["parts"]["ro"].backward_open_loop_adj(gv, g_obs2.contiguous())
        ctx["parts"]["lp"].backward((g_u.reshape(B, -1) * ctx["pass_through"]).contiguous())
        self.tb_info["Train/LipsNet K mean"] = scalar(ctx["K"].mean().reshape(1), 0)
        return self._loss_stats("policy", device).mean_loss(value.contiguous(), -1.0)[:1]

    # ---- GAUSS policy: RBF rollout without a tail -> target value on final_obs -> v_pi + (1 - done_H) gamma^H V --------------------------
    def _rbf_rollout(self, B, device, need_grad):
        pol = self.networks.policy.hip_mlp()
        return self._cached(("rbf", B, self.forward_step, float(self.gamma), str(device), need_grad), lambda: hb.RbfRollout(
            self._hip_env(), pol, batch=B, horizon=self.forward_step, gamma=self.gamma, finite_horizon=False, need_grad=need_grad,
            device=device), lambda ro: ro.set_policy(pol))

    def _rbf_return(self, batch, need_grad):
        """sum_t gamma^t r_t + (1 - done_H) gamma^H V_target(obs_H) under the GAUSS policy -> (value [B], what the backward needs):
        the rollout's v_pi and final observation, the existing `hb.MlpNet` of the target value on it, one fused multiply-add."""
        B, device = batch["obs"].shape[0], batch["obs"].device
        ro = self._rbf_rollout(B, device, need_grad)
        res = ro.forward(batch, want_final=True)
        vt = self._lips_vt(B, device, need_grad)
        v_next = vt.forward(res["final_obs"]).reshape(B)
        tail = float(self.gamma) ** self.forward_step * (1.0 - res["final_done"])
        value = torch.addcmul(res["v_pi"], tail, v_next)
        return value, dict(ro=ro, vt=vt, res=res, tail=tail)

    def _rbf_improvement(self, batch):
        """PIM: loss = -mean(value); grad_final_obs = grad_v (1 - done_H) gamma^H dV/dx through `gops_mlp_backward_x`, then the RBF
        rollout's backward into the policy's four gradient tensors."""
        B, device = batch["obs"].shape[0], batch["obs"].device
        value, ctx = self._rbf_return(batch, need_grad=True)
        gv = self._grad_v(B, device)
        g_final = ctx["vt"].backward_x(ctx["res"]["final_obs"], (gv * ctx["tail"]).unsqueeze(1).contiguous())
        ctx["ro"].backward(gv, rbf_grad_buffers(self.networks.policy), grad_final_obs=g_final.contiguous())
        return self._loss_stats("policy", device).mean_loss(value, -1.0)[:1]

    def _fused_parts(self, net_name, opt):
        """(what `HipAdam.begin_fused` returns, the network's one-table PolyakUpdater) for a backward call that carries the update's
        tail - or (None, None) when optimizer or target averaging do not fit one table each (the separate launches then)."""
        online = list(self.networks.net_dict[net_name].parameters())
        target = list(self.networks.target_net_dict[net_name].parameters())
        pk = self._polyak.get(net_name)
        if pk is None or not pk.matches(target, online):
            pk = self._polyak[net_name] = hb.PolyakUpdater(target, online)
        if len(pk.tables) != 1:
            return None, None
        fa = opt.begin_fused()
        return (fa, pk) if fa is not None else (None, None)

    def _scratch(self, name, n, device):
        t = self._bufs.get(name)
        if t is None or t.numel() != n or t.device != device:
            t = self._bufs[name] = torch.empty(n, dtype=torch.float32, device=device)
        return t

    def _loss_stats(self, mode, device) -> hb.LossStats:
        st = self._bufs.get(("stats", mode))
        if st is None or st.buf.device != device:
            st = self._bufs[("stats", mode)] = hb.LossStats(device)
        return st

    def _log(self, mode: str, scalars: torch.Tensor, start_time: float):
        # (LazyScalar: read back on first use; GOPS_EAGER_LOG=1: host sync here, as in the reference)
        if mode == "v":
            self.tb_info[tb_tags["loss_critic"]] = scalar(scalars, 0, on_value=self.precision_guard["v"].observe_loss)
            self.tb_info[tb_tags["critic_avg_value"]] = scalar(scalars, 1)
        else:
            self.tb_info[tb_tags["loss_actor"]] = scalar(scalars, 0, on_value=self.precision_guard["policy"].observe_loss)
        self.tb_info[tb_tags["alg_time"]] = (time.time() - start_time) * 1000  # ms

    def _compute_gradient(self, data, iteration):
        start_time = time.time()
        batch = self._model_batch(data)
        mode = self._mode(iteration)
        self._log(mode, self._gradient_kernels(mode, batch), start_time)
        return [mode]

    def _signature(self, mode, batch):
        nets = self.networks
        mods = (nets.v, nets.v_target, nets.policy) if mode == "v" else (nets.policy, nets.policy_target, nets.v_target)
        return (mode, tuple((k, tuple(v.shape)) for k, v in batch.items()), self.forward_step, float(self.gamma),
                float(self.tau), self._variant_flags(mode), self._variant_flags("v"),   # (a tripped guard forces a re-capture)
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for m in mods for p in m.parameters()),
                nets.optimizer_dict[mode].storage_signature(),   # Adam moments / device state, workspaces: raw pointers
                tuple(sorted(obj.workspace.data_ptr() for obj in self._cache.values())))
