"""Shared by test_trpo_dis_cpu.py and test_trpo_dis_gpu.py (TRPO on discrete actions): create_alg's arguments for a categorical
StochaPolicyDis, loading a fixture of tests/golden/make_golden_trpo_dis.py, and the categorical restatements at any dtype - the
softmax-metric seed through torch.func.jvp, the reference's double backward of the KL, the surrogate kernel's outputs and a whole
TRPO update (gops/algorithm/trpo.py:118-217).  What does not depend on the density comes from trpo_helpers."""
import copy
import json
import os

import numpy as np
import torch

import trpo_helpers as th
from conftest import GOLDEN, golden_meta, load_golden
from trpo_helpers import EPS, QUANTITIES, flat, unflat   # noqa: F401  (the tests reach them as td.*)

from gops_amd.create_pkg.create_alg import create_alg

FIXTURES = ["trpo_dis_cart_relu", "trpo_dis_o3n5_gelu", "trpo_dis_backtrack", "trpo_dis_all_rejected"]


def dis_kwargs(obs, act_num, hidden, activation, seed=0, use_gpu=False, algorithm="TRPO", **over):
    """create_alg's arguments for TRPO on a StochaPolicyDis of this shape (the keys of example_train/trpo/trpo_mlp_cartpole_onserial.py,
    `policy_std_type="parameter"` included: it means nothing for this policy)."""
    kw = dict(algorithm=algorithm, seed=seed, cnn_shared=False, env_id="gym_cartpole", obsv_dim=obs,
              action_type="discret", action_num=act_num, policy_func_type="MLP", policy_func_name="StochaPolicyDis",
              policy_act_distribution="default", policy_hidden_sizes=list(hidden), policy_hidden_activation=activation,
              policy_std_type="parameter", value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=list(hidden),
              value_hidden_activation=activation, value_output_activation="linear", use_gpu=use_gpu, **th.CTOR)
    kw.update(over)
    return kw


def case_kwargs(meta, use_gpu=False, **over):
    c = meta["cfg"]
    return dis_kwargs(c["obs"], c["act_num"], c["hidden"], c["act"], meta["seed"], use_gpu, **dict(meta["ctor"], **over))


def fresh(name, use_gpu=False, **over):
    """(alg, fixture, meta): built through create_alg with the fixture's seed, nothing loaded."""
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    return create_alg(**case_kwargs(meta, use_gpu, **over)), g, meta


def load_trpo_dis(name, use_gpu=False, **over):
    alg, g, meta = fresh(name, use_gpu, **over)
    alg.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")})
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def reference_error():
    with open(os.path.join(GOLDEN, "trpo_dis_reference_error.json")) as f:
        return json.load(f)


# ---- the categorical density on logits -------------------------------------------------------------------------------------------
def log_prob(logits, act):
    """log softmax(logits) at the index column `act` ([M] or [M, 1] floats, truncated as `.long()` does)."""
    return torch.log_softmax(logits, dim=-1).gather(1, act.reshape(-1, 1).long()).squeeze(1)


def kl_rows(new, old):
    """KL(softmax(new) || softmax(old)) per row."""
    ln, lo = torch.log_softmax(new, dim=-1), torch.log_softmax(old, dim=-1)
    return (ln.exp() * (ln - lo)).sum(dim=-1)


def kl_new_old(new, old):
    return kl_rows(new, old).mean()


def metric_seed(seq, obs, tangent):
    """(1/B) (diag(p) - p p^T) (J v) [B, n] at the dtype of `seq`: torch.func.jvp of the logits along `tangent` (per-parameter
    tensors), then p * (u - p.u) / B with p = softmax(logits) (shifted by the row's maximum, as softmax is).  -> (seed, logits)."""
    params = [p.detach() for p in seq.parameters()]
    f = th.head_fn(seq)
    logits, u = torch.func.jvp(lambda *ps: f(ps, obs), tuple(params), tuple(tangent))
    p = torch.softmax(logits, dim=-1)
    return p * (u - (p * u).sum(dim=-1, keepdim=True)) / obs.shape[0], logits


def diagonal_seed(seq, obs, tangent):
    """What a metric without the - p p^T term would give: p * u / B (the properties only the softmax metric has fail on this)."""
    params = [p.detach() for p in seq.parameters()]
    f = th.head_fn(seq)
    logits, u = torch.func.jvp(lambda *ps: f(ps, obs), tuple(params), tuple(tangent))
    return torch.softmax(logits, dim=-1) * u / obs.shape[0]


def gauss_newton_product(seq, obs, tangent):
    """J^T (diag p - p p^T) J v / B as per-parameter tensors: metric_seed, then one backward of the logits."""
    seed, _ = metric_seed(seq, obs, tangent)
    return torch.autograd.grad(seq(obs), list(seq.parameters()), grad_outputs=seed)


def hessian_product(seq, obs, tangent):
    """The reference's `hvp` (trpo.py:150-162): double backward of the categorical KL against the detached logits at the same
    parameters."""
    params = list(seq.parameters())
    logits = seq(obs)
    grads = torch.autograd.grad(kl_new_old(logits, logits.detach()), params, create_graph=True)
    return torch.autograd.grad(torch.dot(flat(grads), flat(tangent)), params)


# ---- the surrogate kernel --------------------------------------------------------------------------------------------------------
def synthetic_logits(M, n, seed=0):
    """logits_new, logits_old (gaps within a row at most 30: torch's fp32 probabilities stay positive), act (uniform indices as floats,
    [M]) and adv in fp32 on the host."""
    g = torch.Generator().manual_seed(1000 * n + seed + M)
    f64 = torch.float64
    old = torch.randn(M, n, generator=g, dtype=f64) * torch.rand(M, 1, generator=g, dtype=f64) * 6
    old = old.clamp(-15, 15)
    new = (old + torch.randn(M, n, generator=g, dtype=f64)).clamp(-15, 15)
    act = torch.randint(n, (M,), generator=g).float()
    adv = torch.randn(M, generator=g, dtype=f64).float()
    return dict(head_new=new.float(), head_old=old.float(), act=act, adv=adv)


def restate_surrogate(t, dtype=torch.float64, device="cpu", rows=None):
    """-> (surrogate, kl, seed_head) of the inputs `t` at `dtype` on `device`; `rows` (bool [M]): the rows that count - the others
    add nothing, the means still divide by M, and their seed rows are zero."""
    c = {k: v.detach().to(device=device, dtype=dtype) for k, v in t.items()}
    M = c["head_new"].shape[0]
    keep = torch.ones(M, dtype=torch.bool, device=device) if rows is None else rows.to(device)
    head = c["head_new"][keep].clone().requires_grad_(True)
    act = c["act"][keep]
    sur = torch.sum(torch.exp(log_prob(head, act) - log_prob(c["head_old"][keep], act)) * c["adv"][keep]) / M
    kl = kl_rows(head, c["head_old"][keep]).sum() / M
    sur.backward()
    seed = torch.zeros_like(c["head_new"])
    seed[keep] = head.grad
    return sur.detach(), kl.detach(), seed


# ---- the whole update --------------------------------------------------------------------------------------------------------------
def restate_trpo_update(alg, data, dtype=torch.float64):
    """One `local_update` of the reference (trpo.py:118-217) with a categorical policy on copies of `alg.networks` at `dtype` on the
    host, the Hessian-vector product by double backward as the reference forms it, torch's Adam for the value function.  -> what
    trpo_helpers.restate_trpo_update returns (without `zones`)."""
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items()}
    obs, adv, ret = d["obs"], d["adv"].reshape(-1), d["ret"].reshape(-1)
    act = d["act"].reshape(-1)
    seq = nets.policy.q
    params = list(seq.parameters())
    if alg.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + EPS)
    head_old = seq(obs).detach()
    logp_old = log_prob(head_old, act)

    def surrogate(head):
        return torch.mean(torch.exp(log_prob(head, act) - logp_old) * adv)

    at_old = surrogate(seq(obs))
    g = flat(torch.autograd.grad(at_old, params)).detach()

    def Ax(v):
        return flat(hessian_product(seq, obs, unflat(v, params))).detach() + alg.damping_factor * v

    x, r, n_cg = th.solve_cg(Ax, g, alg.atol, alg.max_cg)
    step = torch.sqrt(2 * alg.delta / (torch.dot(g, x) + EPS)) * x
    theta_old = flat(params).detach().clone()
    cand, index = [], None
    with torch.no_grad():
        for i in range(alg.max_search):
            for p, v in zip(params, unflat(theta_old + alg.alpha ** i * step, params)):
                p.copy_(v)
            head = seq(obs)
            cand.append((float(surrogate(head)), float(kl_new_old(head, head_old))))
            if cand[-1][0] > 0 and cand[-1][1] < alg.delta:
                index = i
                break
        else:
            for p, v in zip(params, unflat(theta_old, params)):
                p.copy_(v)
    opt = torch.optim.Adam(nets.value.parameters(), lr=alg.value_learning_rate)
    v_loss = val = None
    for _ in range(alg.train_v_iters):
        val = nets.value(obs)
        opt.zero_grad()
        v_loss = torch.nn.functional.mse_loss(val, ret)
        v_loss.backward()
        opt.step()
    return dict(g=g, x=x, r=r, step=step, index=index, cand=cand, policy=[p.detach().clone() for p in seq.parameters()],
                value=[p.detach().clone() for p in nets.value.parameters()], cg_iterations=n_cg,
                tb={"Loss/Critic loss-RL iter": float(v_loss.detach()), "Train/Critic avg value-RL iter": float(val.detach().mean()),
                    "Loss/Actor loss-RL iter": -float(at_old.detach())})
