"""TRPO - trust region policy optimisation - on the HIP kernels.

Same class surface as the reference's gops/algorithm/trpo.py (ApproxContainer :38-53, TRPO :56-267): a Gaussian StochaPolicy - or,
on discrete actions, a categorical StochaPolicyDis - stepped along the natural gradient within a KL ball, and a StateValue under its
own Adam, on the on-policy columns `obs, act, adv, ret`.

The Fisher-vector product.  The reference forms `H v`, H the Hessian of `mean KL(pi || pi_old)` at theta_old, by a double backward
through autograd, `max_cg + 1` times per update (trpo.py:150-169).  At theta_old `pi` and `pi_old` are the same numbers, the KL's
gradient with respect to the head is exactly zero, and only the Gauss-Newton term of the Hessian survives:
`H v = (1/B) sum_i J_i^T M_i J_i v` with J_i the Jacobian of the raw head (mean, raw log std) and M_i = diag(1 / sigma^2, 2 inside the
log-std clamp | 0 outside).  One product is `gops_gauss_fisher_seed` (the parameter-tangent forward fused with M / B) followed by the
`gops_mlp_backward` that exists already.  The reference's first product, with x0 = 0, is zero and is not formed.

Where the arithmetic runs.  Once per `local_update`: `gops_adv_normalize` (when `norm_adv`), one `gops_mlp_forward` of the policy (its
head is `head_old`; its stash serves every later backward - nothing between two backwards overwrites it, and the weights stay put
until the line search), `gops_trpo_surrogate` at theta_old for the gradient seed, `gops_mlp_backward` into the flat `g`,
`gops_cg_init`.  The CG loop is `max_cg` times (seed, backward into the flat `Ap`, `gops_cg_step`) without a host read - the
iteration's scalars and the `done` flag live in a device state block, and a step after `done` changes nothing - captured and
replayed as ONE graph by `StepGraphCache`.  `gops_cg_finish` scales the step.  The line search writes `theta_old + alpha**i step`
into the parameters, runs the forward and `gops_trpo_surrogate` against `head_old`, and reads the kernel's verdict word: one
synchronisation per candidate, as in the reference.  The value function then takes `train_v_iters` steps of (`gops_mlp_forward`,
`gops_value_loss`, `gops_mlp_backward`, `HipAdam.step`), each a replay of one captured step.

Kept as the reference has them: `loss_actor` is minus the surrogate at theta_old; `loss_critic` and `critic_avg_value` are the LAST
value iteration's, computed before that iteration's step; "fail to improve policy!" is printed when no candidate is accepted, and
the policy stays at theta_old.

The policy is the reference's `std_type="mlp_shared"` StochaPolicy with a GaussDistribution; `"parameter"` (the default of the
reference's continuous TRPO examples) and `"mlp_separated"` are not yet supported - `create_alg` refuses them with that reason.

Discrete actions (`action_type="discret"`, `policy_func_name="StochaPolicyDis"`, 2 .. 16 actions; the reference's
trpo_mlp_cartpole_onserial.py).  The head is the `act_num` logits, `act` holds the action indices as floats [B, 1], and the metric
of the Gauss-Newton form is the softmax Fisher metric M_i = diag(p_i) - p_i p_i^T, p_i = softmax(logits_i).  Two kernel objects
differ - `_fisher` returns `gops_cat_fisher_seed`'s, `_surrogate` `gops_cat_trpo_surrogate`'s, with the Gaussian ones' call
surfaces - and nothing else does: the launch sequence, the graphs and the line search are the same code.  The categorical surrogate
also counts the rows whose index lies outside [0, act_num) (the reference raises inside `gather`); the count is read together
with the first candidate's verdict, and `local_update` raises ValueError - the policy back at theta_old - when it is not zero.
`policy_std_type` and the log-std bounds mean nothing for this policy and are ignored.
"""
__all__ = ["ApproxContainer", "TRPO"]

import time
from typing import Callable, Tuple

import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm import _on_policy
from gops_amd.algorithm._on_policy import ApproxContainer, OnPolicyBase
from gops_amd.algorithm.base import batch_to_device, cuda_device_of, grad_buffers
from gops_amd.apprfunc.mlp import StochaPolicyDis
from gops_amd.utils.common_utils import make_adam
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags

EPSILON = 1e-8
# the reference's keyword-only arguments without defaults (trpo.py:72-84)
MANDATORY = ("delta", "rtol", "atol", "damping_factor", "max_cg", "alpha", "max_search", "train_v_iters", "value_learning_rate")


def refusal(kwargs: dict):
    """Why `create_alg` cannot build TRPO from these arguments, or None."""
    return _on_policy.refusal("TRPO", "the Fisher metric and the surrogate kernel are that density's", kwargs, categorical=True)


class TRPO(OnPolicyBase):
    """delta: KL constraint; rtol, atol: CG's tolerances (rtol multiplies |0|: it has no effect, as in the reference); damping_factor:
    lambda of H + lambda I; max_cg; alpha, max_search: the backtracking line search; train_v_iters, value_learning_rate: the value
    function's training; norm_adv (trpo.py:60-69)."""

    def __init__(self, *, delta: float, rtol: float, atol: float, damping_factor: float, max_cg: int, alpha: float, max_search: int,
                 train_v_iters: int, value_learning_rate: float, norm_adv: bool = True, index=0, **kwargs):
        super().__init__(index, **kwargs)
        self.delta = delta
        self.norm_adv = norm_adv
        self.rtol = rtol
        self.atol = atol
        self.damping_factor = damping_factor
        self.max_cg = max_cg
        self.alpha = alpha
        self.max_search = max_search
        self.train_v_iters = train_v_iters
        self.value_learning_rate = value_learning_rate
        self._init_on_policy(kwargs, categorical=True)
        self.value_optimizer = make_adam(self.networks.value.parameters(), lr=value_learning_rate)
        self._cg_graph, self._v_graph = StepGraphCache(), StepGraphCache()
        self.cg_graph_replays = 0      # CG loops that ran as a graph replay
        self.value_graph_replays = 0   # value steps that ran as a graph replay
        self.last_cg_iterations = None   # iterations of the last update's CG solve that changed x (where the reference's loop returns)
        self.last_search_index = None    # the accepted candidate of the last update's line search; None: none was accepted

    @property
    def adjustable_parameters(self):
        return ("delta", "norm_adv", "train_v_iters", "value_learning_rate", "rtol", "atol", "damping_factor", "max_cg", "alpha", "max_search")

    # ---- update API ----------------------------------------------------------------------------
    def local_update(self, data: dict, iteration: int) -> dict:
        start_time = time.perf_counter()
        device = cuda_device_of(self.networks)
        nets = self.networks
        cols = batch_to_device(data, device, ("obs", "act", "adv", "ret"))
        obs = cols["obs"]
        B = obs.shape[0]
        act, adv, ret = cols["act"].reshape(B, -1), cols["adv"].reshape(B), cols["ret"].reshape(B)
        if self.norm_adv:
            adv = self._adv_normalize(device).run(adv, EPSILON, out=self._buf("adv", (B,), device))

        pol, cg, sur = self._net("policy", nets.policy, B, device), self._cg(device), self._surrogate(device)
        # (everything the two captured steps allocate on first use exists before their signatures are taken)
        self._fisher(device), self._buf("fisher_seed", (B, pol.out_dim), device), self._net("value", nets.value, B, device)
        self._buf("v", (B, 1), device), self._buf("seed_v", (B, 1), device), self._loss_stats(device), grad_buffers(nets.value)
        head_old, head_new = self._buf("head_old", (B, pol.out_dim), device), self._buf("head_new", (B, pol.out_dim), device)
        seed = self._buf("seed", (B, pol.out_dim), device)
        sur.set_delta(self.delta)
        params = list(nets.policy.parameters())
        pol.forward(obs, out=head_old)
        _, stats = sur.run(head_old, head_old, act, adv, seed_head=seed)
        at_old = stats.clone()
        pol.backward(obs, seed, *self._layers(cg.g))
        cg.init(self.atol)

        self._cg_graph.run(self._cg_signature(B, obs), {"obs": obs}, self.cg_loop, on_replay=self._cg_replayed, work=B)
        cg.finish()

        theta_old = torch.nn.utils.parameters_to_vector(params)
        datas = [p.data for p in params]
        self.last_search_index = None
        for i in range(self.max_search):
            torch._foreach_copy_(datas, self._views(theta_old.add(cg.step_vec, alpha=self.alpha ** i), params))
            pol.forward(obs, out=head_new)
            sur.run(head_new, head_old, act, adv, want_seed=False)
            accepted, bad_rows = sur.flags()   # surrogate > 0 and kl < delta: one synchronisation per candidate, as in the reference
            if bad_rows:   # (a categorical policy's rows with an index outside the head: the reference raises inside `gather`)
                torch._foreach_copy_(datas, self._views(theta_old, params))
                raise ValueError(f"TRPO: {bad_rows} rows of `act` hold an action index outside [0, {pol.out_dim})")
            if accepted:
                self.last_search_index = i
                break
        else:
            torch._foreach_copy_(datas, self._views(theta_old, params))
            print("fail to improve policy!")

        out = None
        for _ in range(self.train_v_iters):
            out = self._value_step({"obs": obs, "ret": ret})
        self.last_cg_iterations = cg.state()["iterations"]

        tb_info = {}
        if out is not None:
            tb_info[tb_tags["loss_critic"]] = scalar(out, 0)
            tb_info[tb_tags["critic_avg_value"]] = scalar(out, 1)
        tb_info[tb_tags["alg_time"]] = (time.perf_counter() - start_time) * 1000
        tb_info[tb_tags["loss_actor"]] = scalar(at_old, 0, negate=True)
        self.tb_info = tb_info
        return tb_info

    def cg_loop(self, batch: dict) -> torch.Tensor:
        """`max_cg` times: the Fisher-vector product of `p` into `Ap` (`gops_gauss_fisher_seed`, `gops_mlp_backward` on the stash of
        the update's policy forward), then `gops_cg_step`.  A fixed launch sequence without a host read; -> the state block (device)."""
        obs = batch["obs"]
        B, device = obs.shape[0], obs.device
        nets = self.networks
        pol, cg, fisher = self._net("policy", nets.policy, B, device), self._cg(device), self._fisher(device)
        seed = self._buf("fisher_seed", (B, pol.out_dim), device)
        p_w, p_b = self._layers(cg.p)
        ap = self._layers(cg.Ap)
        for _ in range(self.max_cg):
            fisher.run(obs, p_w, p_b, seed=seed)
            pol.backward(obs, seed, *ap)
            cg.step(self.damping_factor, self.atol)
        return cg._state

    def _cg_replayed(self):
        self.cg_graph_replays += 1

    def _value_step(self, batch: dict) -> torch.Tensor:
        """One step of trpo.py:201-206, eager or as a graph replay; -> [mse_loss, mean(v)] before the step (device)."""
        return self._adam_step(self._v_graph, self._value_signature(batch), batch, self.value_gradients, self.value_optimizer,
                               "value_graph_replays")

    def value_gradients(self, batch: dict) -> torch.Tensor:
        nets = self.networks
        o, ret = batch["obs"], batch["ret"]
        B, device = o.shape[0], o.device
        val = self._net("value", nets.value, B, device)
        v = val.forward(o, out=self._buf("v", (B, 1), device))
        seed_v = self._buf("seed_v", (B, 1), device)
        stats = self._loss_stats(device).value_loss(v.view(B), ret, grad=seed_v.view(B))
        gw, gb = grad_buffers(nets.value)
        val.backward(o, seed_v, gw, gb)
        return stats.clone()

    def _cg_signature(self, B, obs):
        cg = self._cache.get("cg")
        return (B, tuple(obs.shape), int(self.max_cg), float(self.damping_factor), float(self.atol),
                tuple(p.data_ptr() for p in self.networks.policy.parameters()), cg.g.data_ptr(), cg._state.data_ptr(), self._storage())

    def _value_signature(self, batch):
        return (tuple((k, tuple(v.shape)) for k, v in batch.items()),
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in self.networks.value.parameters()),
                self.value_optimizer.storage_signature(), self._storage())

    # ---- flat vectors ----------------------------------------------------------------------------
    @staticmethod
    def _views(flat, params):
        return hb.flat_views(flat, [tuple(p.shape) for p in params])

    def _layers(self, flat):
        """(weights, biases) per layer as views of a flat vector in `parameters_to_vector`'s order (W0, b0, W1, b1, ...)."""
        v = self._views(flat, list(self.networks.policy.parameters()))
        return v[0::2], v[1::2]

    # ---- kernels' objects ------------------------------------------------------------------------
    def _surrogate(self, device):
        """hb.TrpoSurrogate, or hb.CatTrpoSurrogate for a StochaPolicyDis: the same call surface."""
        pol = self.networks.policy
        if isinstance(pol, StochaPolicyDis):
            return self._one("surrogate", lambda: hb.CatTrpoSurrogate(pol.act_num, device))
        return self._one("surrogate", lambda: hb.TrpoSurrogate(pol.act_dim, pol.min_log_std, pol.max_log_std, device))

    def _fisher(self, device) -> hb.FisherSeed:
        """hb.FisherSeed, or hb.CatFisherSeed for a StochaPolicyDis."""
        pol = self.networks.policy
        if isinstance(pol, StochaPolicyDis):
            fisher = self._one("fisher", lambda: hb.CatFisherSeed(pol.hip_mlp(), device))
        else:
            fisher = self._one("fisher", lambda: hb.FisherSeed(pol.hip_mlp(), pol.min_log_std, pol.max_log_std, device))
        fisher.mlp = pol.hip_mlp()
        return fisher

    def _cg(self, device) -> hb.CgSolver:
        n = sum(p.numel() for p in self.networks.policy.parameters())
        return self._one("cg", lambda: hb.CgSolver(n, device, hyper=self._surrogate(device).hyper))

    def _loss_stats(self, device) -> hb.LossStats:
        return self._one("loss_stats", lambda: hb.LossStats(device))

    # ---- the reference's host solver, for users who call it ---------------------------------------
    @staticmethod
    def _conjugate_gradient(Ax: Callable[[torch.Tensor], torch.Tensor], b: torch.Tensor, x: torch.Tensor, rtol: float, atol: float,
                            max_cg: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Conjugate gradients for A x = b, A positive definite, on the host with the reference's semantics (trpo.py:226-267): `x`
        is the start and is updated in place; the solve ends after `max_cg` iterations or as soon as the residue is within
        `allclose(r, 0, rtol, atol)`; 1e-8 guards both quotients.  -> (solution, residue).  `local_update` does not call this: its
        solve is `gops_cg_init / _step / _finish` on the device."""
        def converged(res):
            return torch.allclose(res, torch.zeros((), dtype=res.dtype, device=res.device), rtol=rtol, atol=atol)

        r = b - Ax(x)
        if converged(r):
            return x, r
        p, rr = r.clone(), torch.dot(r, r)
        for _ in range(max_cg):
            Ap = Ax(p)
            step = rr / (torch.dot(p, Ap) + EPSILON)
            x.add_(p, alpha=step)
            r.add_(Ap, alpha=-step)
            if converged(r):
                break
            rr_new = torch.dot(r, r)
            p = r.add(p, alpha=rr_new / (rr + EPSILON))
            rr = rr_new
        return x, r
