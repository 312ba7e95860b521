"""Shared by test_trpo_cpu.py and test_trpo_gpu.py: loading a fixture of tests/golden/make_golden_trpo.py into the algorithm create_alg
builds (on ac_helpers.load_alg), the Fisher-vector product both ways (the reference's double backward of the KL, and the Gauss-Newton
form J^T M J v / B through torch.func.jvp) at any dtype, the restatement of a whole TRPO update (gops/algorithm/trpo.py:118-217) in
float64, synthetic heads for the surrogate kernel and the conjugate-gradient recurrence."""
import copy
import json
import os

import numpy as np
import torch

import ac_helpers as ah
from conftest import GOLDEN
from gauss_helpers import MAX_LS, MIN_LS, gauss, kl_new_old, log_prob, raw_log_std   # noqa: F401  (the tests reach them as th.*)

# create_alg's arguments for TRPO beyond ac_helpers' common dictionary (registered next to the other families', for alg_kwargs);
# the nine mandatory ones travel in a fixture's `ctor`
ah.FAMILY.setdefault("TRPO", dict(policy_func_name="StochaPolicy", policy_act_distribution="default", value_func_name="StateValue"))

CTOR = dict(delta=0.01, rtol=1e-5, atol=1e-8, damping_factor=0.1, max_cg=10, alpha=0.8, max_search=10, train_v_iters=5,
            value_learning_rate=1e-3, trainer="on_serial_trainer")
FIXTURES = ["trpo_pend_relu", "trpo_lqs4a2_gelu", "trpo_pend_backtrack", "trpo_pend_all_rejected", "trpo_pend_no_norm"]
EPS = 1e-8
QUANTITIES = ("g", "x", "step", "policy")


def load_trpo(name, use_gpu=False, **over):
    return ah.load_alg(name, use_gpu=use_gpu, **over)


def data_of(g):
    return {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("in/")}


def reference_error():
    with open(os.path.join(GOLDEN, "trpo_reference_error.json")) as f:
        return json.load(f)


def flat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors])


def unflat(vec, like):
    out, at = [], 0
    for p in like:
        out.append(vec[at:at + p.numel()].view_as(p))
        at += p.numel()
    return out


def rel_max(a, b):
    """max |a - b| relative to the largest |b|."""
    a, b = torch.as_tensor(np.asarray(a)).double().reshape(-1), torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- the policy's raw head as a function of its parameters -------------------------------------------------------------------------
def mlp_stack(sizes, act, seed, dtype=torch.float64):
    """A plain Sequential in>hidden..>out with activation `act` (torch's name) between the layers, default init under `seed`."""
    torch.manual_seed(seed)
    layers = []
    for j in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[j], sizes[j + 1]))
        if j < len(sizes) - 2:
            layers.append(dict(relu=torch.nn.ReLU, elu=torch.nn.ELU, gelu=torch.nn.GELU, selu=torch.nn.SELU, sigmoid=torch.nn.Sigmoid,
                               tanh=torch.nn.Tanh, linear=torch.nn.Identity)[act]())
    return torch.nn.Sequential(*layers).to(dtype)


def head_fn(seq):
    names = [n for n, _ in seq.named_parameters()]

    def f(params, obs):
        return torch.func.functional_call(seq, dict(zip(names, params)), (obs,))
    return f


def metric_seed(seq, obs, tangent, min_ls=MIN_LS, max_ls=MAX_LS):
    """(1/B) M (J v) [B, 2A] at the dtype of `seq`: torch.func.jvp of the raw head along `tangent` (per-parameter tensors), scaled by
    M = diag(1 / sigma^2, 2 inside the closed clamp interval | 0 outside).  -> (seed, raw head)."""
    params = [p.detach() for p in seq.parameters()]
    f = head_fn(seq)
    head, jv = torch.func.jvp(lambda *ps: f(ps, obs), tuple(params), tuple(tangent))
    A = head.shape[1] // 2
    raw = head[:, A:]
    std = torch.clamp(raw, min_ls, max_ls).exp()
    inside = ((raw >= min_ls) & (raw <= max_ls)).to(head.dtype)
    return torch.cat((jv[:, :A] / std ** 2, 2 * inside * jv[:, A:]), dim=-1) / obs.shape[0], head


def gauss_newton_product(seq, obs, tangent, min_ls=MIN_LS, max_ls=MAX_LS):
    """J^T M J v / B as per-parameter tensors: metric_seed, then one backward of the raw head."""
    seed, _ = metric_seed(seq, obs, tangent, min_ls, max_ls)
    params = list(seq.parameters())
    return torch.autograd.grad(seq(obs), params, grad_outputs=seed)


def hessian_product(seq, obs, tangent, min_ls=MIN_LS, max_ls=MAX_LS):
    """The reference's `hvp` (trpo.py:150-162): double backward of the KL against the detached head at the same parameters."""
    params = list(seq.parameters())
    head = seq(obs)
    kl = kl_new_old(head, head.detach(), min_ls, max_ls)
    grads = torch.autograd.grad(kl, params, create_graph=True)
    return torch.autograd.grad(torch.dot(flat(grads), flat(tangent)), params)


def clamp_zones(raw, min_ls=MIN_LS, max_ls=MAX_LS):
    return int((raw < min_ls).sum()), int(((raw >= min_ls) & (raw <= max_ls)).sum()), int((raw > max_ls).sum())


def spread_log_std(seq, obs, A, min_ls=MIN_LS, max_ls=MAX_LS):
    """Rescale and shift the log-std half of the head of `seq` so that, per action dimension, the 0.3 and 0.7 quantiles of the raw log
    stds over `obs` sit on the clamp's bounds: about 30 % of the elements below, 40 % inside, 30 % above."""
    with torch.no_grad():
        head = [m for m in seq if isinstance(m, torch.nn.Linear)][-1]
        raw = seq(obs)[:, A:]
        q = torch.quantile(raw, torch.tensor([0.3, 0.7], dtype=raw.dtype), dim=0)
        scale = (max_ls - min_ls) / (q[1] - q[0]).clamp_min(1e-9)
        head.weight[A:].mul_(scale[:, None])
        head.bias[A:].mul_(scale)
        head.bias[A:].sub_(torch.quantile(seq(obs)[:, A:], 0.3, dim=0) - min_ls)


# ---- conjugate gradients ---------------------------------------------------------------------------------------------------------
def cg_recurrence_step(x, r, p, Ap, r_dot, damping, atol):
    """One iteration of trpo.py:257-266 in float64 on copies of the inputs (Ap: the UNDAMPED product)."""
    x, r, p, Ap = (t.double().clone() for t in (x, r, p, Ap))
    Ap = Ap + damping * p
    alpha = r_dot / (torch.dot(p, Ap) + EPS)
    x, r = x + alpha * p, r - alpha * Ap
    done = bool((r.abs() <= atol).all())
    r_dot_new = torch.dot(r, r)
    if not done:
        p = r + r_dot_new / (r_dot + EPS) * p
    return dict(x=x, r=r, p=p, Ap=Ap, r_dot=float(r_dot_new), done=done, alpha=float(alpha))


def solve_cg(Ax, b, atol, max_cg):
    """trpo.py:226-267 from x = 0 in the dtype of `b`: -> (x, r, iterations that updated x)."""
    x, r = torch.zeros_like(b), b.clone()
    if bool((r.abs() <= atol).all()):
        return x, r, 0
    p, r_dot, n = r.clone(), torch.dot(r, r), 0
    for _ in range(max_cg):
        Ap = Ax(p)
        alpha = r_dot / (torch.dot(p, Ap) + EPS)
        x, r, n = x + alpha * p, r - alpha * Ap, n + 1
        if bool((r.abs() <= atol).all()):
            break
        r_new = torch.dot(r, r)
        p, r_dot = r + r_new / (r_dot + EPS) * p, r_new
    return x, r, n


# ---- the whole update --------------------------------------------------------------------------------------------------------------
def restate_trpo_update(alg, data, dtype=torch.float64):
    """One `local_update` of the reference (trpo.py:118-217) on copies of `alg.networks` at `dtype` on the host, the Hessian-vector
    product by double backward as the reference forms it, torch's Adam for the value function.  -> dict(g, x, r, step [flat], index
    (None: no candidate accepted), cand [(surrogate, kl) per tried candidate], policy / value [parameters afterwards], tb, zones,
    cg_iterations)."""
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items()}
    obs, adv, ret = d["obs"], d["adv"].reshape(-1), d["ret"].reshape(-1)
    act = d["act"].reshape(obs.shape[0], -1)
    pol = nets.policy
    seq, lo, hi = pol.policy, pol.min_log_std, pol.max_log_std
    params = list(seq.parameters())
    if alg.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + EPS)
    head_old = seq(obs).detach()
    logp_old = log_prob(head_old, act, lo, hi)

    def surrogate(head):
        return torch.mean(torch.exp(log_prob(head, act, lo, hi) - logp_old) * adv)

    at_old = surrogate(seq(obs))
    g = flat(torch.autograd.grad(at_old, params)).detach()

    def Ax(v):
        return flat(hessian_product(seq, obs, unflat(v, params), lo, hi)).detach() + alg.damping_factor * v

    x, r, n_cg = solve_cg(Ax, g, alg.atol, alg.max_cg)
    step = torch.sqrt(2 * alg.delta / (torch.dot(g, x) + EPS)) * x
    theta_old = flat(params).detach().clone()
    cand, index = [], None
    with torch.no_grad():
        for i in range(alg.max_search):
            for p, v in zip(params, unflat(theta_old + alg.alpha ** i * step, params)):
                p.copy_(v)
            head = seq(obs)
            cand.append((float(surrogate(head)), float(kl_new_old(head, head_old, lo, hi))))
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
    raw = head_old[:, act.shape[1]:]
    return dict(g=g, x=x, r=r, step=step, index=index, cand=cand, policy=[p.detach().clone() for p in pol.parameters()],
                value=[p.detach().clone() for p in nets.value.parameters()], cg_iterations=n_cg, zones=clamp_zones(raw, lo, hi),
                tb={"Loss/Critic loss-RL iter": float(v_loss.detach()), "Train/Critic avg value-RL iter": float(val.detach().mean()),
                    "Loss/Actor loss-RL iter": -float(at_old.detach())})


# ---- synthetic heads of the surrogate kernel's tests -----------------------------------------------------------------------------------
def synthetic_heads(M, A, seed=0):
    """head_new, head_old (raw, log stds on both sides of the clamp and at least 0.01 away from it), act, adv in fp32 on the host."""
    g = torch.Generator().manual_seed(1000 * A + seed + M)
    f64 = torch.float64
    mean = 0.5 * torch.randn(M, A, generator=g, dtype=f64)
    head_new = torch.cat((mean, raw_log_std(M, A, g)), dim=-1).float()
    head_old = torch.cat((mean + 0.05 * torch.randn(M, A, generator=g, dtype=f64), raw_log_std(M, A, g)), dim=-1).float()
    std = gauss(head_old.double())[1]
    act = (head_old[:, :A].double() + std * torch.randn(M, A, generator=g, dtype=f64)).float()
    adv = torch.randn(M, generator=g, dtype=f64).float()
    return dict(head_new=head_new, head_old=head_old, act=act, adv=adv)


def restate_surrogate(t, dtype=torch.float64, device="cpu"):
    """-> (surrogate, kl, seed_head) of the inputs `t` at `dtype` on `device`."""
    c = {k: v.detach().to(device=device, dtype=dtype) for k, v in t.items()}
    head = c["head_new"].requires_grad_(True)
    sur = torch.mean(torch.exp(log_prob(head, c["act"]) - log_prob(c["head_old"], c["act"])) * c["adv"])
    kl = kl_new_old(head, c["head_old"])
    sur.backward()
    return sur.detach(), kl.detach(), head.grad
