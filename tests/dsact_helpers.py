"""Shared by tests/test_dsact_cpu.py and tests/test_dsact_gpu.py: building DSACT from the fixtures of tests/golden/make_golden_dsact.py
and the restatement of one update (gops/algorithm/dsact.py:162-329) in torch, at any dtype, with the draws as inputs."""
import copy

import numpy as np
import torch

from conftest import golden_meta, load_golden
from helpers import data_from_golden

from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

ONE_UPDATE = ["dsact_pend_relu", "dsact_lqs4a2_gelu", "dsact_pend_fixed_alpha"]
TOL = 1e-4   # the project's parity bound against the reference (rel-L2), as in td3_helpers.py
GRAD_KEYS = ("q1", "q2", "policy")


def alg_kwargs(meta, use_gpu, **over):
    cfg, lim = meta["cfg"], meta["lim"]
    c = dict(cfg, alg="INFADP", horizon=1)
    kw = dict(algorithm="DSACT", trainer="off_serial_trainer", seed=meta["seed"], cnn_shared=False, env_id=cfg["env_id"],
              obsv_dim=obs_dim_of(c), action_dim=act_dim_of(c), action_type="continu",
              action_low_limit=np.array(lim[0], dtype=np.float32), action_high_limit=np.array(lim[1], dtype=np.float32),
              policy_func_type="MLP", policy_func_name="StochaPolicy", policy_hidden_sizes=list(cfg["hidden"]),
              policy_hidden_activation=cfg["act"], policy_act_distribution="TanhGaussDistribution", policy_learning_rate=1e-3,
              policy_min_log_std=meta["min_log_std"], policy_max_log_std=meta["max_log_std"],
              value_func_type="MLP", value_func_name="ActionValueDistri", value_hidden_sizes=list(cfg["hidden"]),
              value_hidden_activation=cfg["act"], value_output_activation="linear", value_learning_rate=1e-3,
              alpha_learning_rate=3e-4, use_gpu=use_gpu, buffer_name="replay_buffer")
    kw.update(meta["ctor"])
    kw.update(over)
    return kw


def load_alg(name, use_gpu=False, prefix="sd/", **over):
    """(alg, fixture, meta): built through create_alg with the fixture's seed, then the fixture's state dict loaded."""
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    alg = create_alg(**alg_kwargs(meta, use_gpu, **over))
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})
    if "lr" in meta:
        for n in ("q1", "q2", "policy", "alpha"):
            for group in getattr(alg.networks, f"{n}_optimizer").param_groups:
                group["lr"] = meta["lr"]
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def batch_of(g, prefix="in/"):
    return data_from_golden(g, prefix)


def restate_update(alg, data, dtype=torch.float64, mean_std=None):
    """One compute_gradient of DSACT restated with autograd on copies of `alg.networks` at `dtype` (on the host).  `data` holds the
    draws eps_new, eps_next, z_next; `mean_std`: the running values before this update ([2], or None for the first one; they are
    fp32 state, and the updated pair is rounded to fp32 as the device state holds it).  Returns the targets, the target policy's
    sample, losses, statistics and grads {net: [tensors]} + log_alpha_grad."""
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items()}
    for n in GRAD_KEYS:
        for p in getattr(nets, n).parameters():
            p.requires_grad_(True)
            p.grad = None
    alpha = float(nets.log_alpha.detach().exp()) if alg.auto_alpha else float(alg.alpha)
    with torch.no_grad():
        a2, logp2 = nets.create_action_distributions(nets.policy_target(d["obs2"])).rsample(d["eps_next"])
        qt = torch.stack([nets.q1_target(d["obs2"], a2), nets.q2_target(d["obs2"], a2)])
        z = torch.clamp(d["z_next"], -3, 3)
        q_next = torch.min(qt[0, :, 0], qt[1, :, 0])
        q_sample = torch.where(qt[0, :, 0] < qt[1, :, 0], qt[0, :, 0] + z[0] * qt[0, :, 1], qt[1, :, 0] + z[1] * qt[1, :, 1])
        live = (1 - d["done"]) * alg.gamma
        tq, tqs = d["rew"] + live * (q_next - alpha * logp2), d["rew"] + live * (q_sample - alpha * logp2)
    heads = [nets.q1(d["obs"], d["act"]), nets.q2(d["obs"], d["act"])]
    losses, new_ms, binds = [], [], []
    for i, h in enumerate(heads):
        q, s = h[:, 0], h[:, 1]
        sd, qd = s.detach(), q.detach()
        ms = sd.mean() if mean_std is None else (1 - alg.tau_b) * float(mean_std[i]) + alg.tau_b * sd.mean()
        ms = ms.to(torch.float32).to(dtype)
        diff = tqs - qd
        bound = qd + torch.clamp(diff, -3 * ms, 3 * ms)
        losses.append((ms ** 2 + 0.1) * torch.mean(-(tq - qd) / (sd ** 2 + 0.1) * q - ((qd - bound) ** 2 - sd ** 2) / (sd ** 3 + 0.1) * s))
        new_ms.append(ms)
        binds.append(diff.abs() > 3 * ms)
    sum(losses).backward()
    grads = {n: [p.grad.detach().clone() for p in getattr(nets, n).parameters()] for n in ("q1", "q2")}
    for n in ("q1", "q2"):
        for p in getattr(nets, n).parameters():
            p.requires_grad_(False)
    logits = nets.policy(d["obs"])
    new_act, new_logp = nets.create_action_distributions(logits).rsample(d["eps_new"])
    qn = torch.stack([nets.q1(d["obs"], new_act)[:, 0], nets.q2(d["obs"], new_act)[:, 0]])
    loss_pi = (alpha * new_logp - torch.min(qn[0], qn[1])).mean()
    loss_pi.backward()
    grads["policy"] = [p.grad.detach().clone() for p in nets.policy.parameters()]
    mean_l, std_l = torch.chunk(logits.detach(), 2, dim=-1)
    A = d["act"].shape[1]
    tb = {"DSAC2/critic_avg_q1-RL iter": heads[0][:, 0].mean(), "DSAC2/critic_avg_q2-RL iter": heads[1][:, 0].mean(),
          "DSAC2/critic_avg_std1-RL iter": heads[0][:, 1].mean(), "DSAC2/critic_avg_std2-RL iter": heads[1][:, 1].mean(),
          "DSAC2/critic_avg_min_std1-RL iter": heads[0][:, 1].min(), "DSAC2/critic_avg_min_std2-RL iter": heads[1][:, 1].min(),
          "Loss/Actor loss-RL iter": loss_pi, "Loss/Critic loss-RL iter": sum(losses), "DSAC2/policy_mean-RL iter": torch.tanh(mean_l).mean(),
          "DSAC2/policy_std-RL iter": std_l.mean(), "DSAC2/entropy-RL iter": -new_logp.mean(), "DSAC2/alpha-RL iter": alpha,
          "DSAC2/mean_std1": new_ms[0], "DSAC2/mean_std2": new_ms[1]}
    return dict(target_q=tq, target_q_sample=tqs, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act.detach(), new_logp=new_logp.detach(),
                mean_std=torch.stack(new_ms).detach(), tb={k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in tb.items()}, grads=grads, qn=qn.detach(),
                log_alpha_grad=float(-(new_logp.detach().mean() + (-A))), binds=torch.stack(binds), heads=torch.stack(heads).detach())
