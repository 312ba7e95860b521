"""Shared by tests/test_sac_cpu.py and tests/test_sac_gpu.py: building SAC / DSAC from the fixtures of tests/golden/make_golden_sac.py
and the restatement of one update (gops/algorithm/sac.py:159-241, dsac.py:155-267) in torch, at any dtype, with the draws as inputs."""
import copy

import numpy as np
import torch

from conftest import golden_meta, load_golden
from helpers import data_from_golden

from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

ONE_UPDATE = ["sac_pend_relu", "sac_lqs4a2_gelu", "sac_pend_fixed_alpha", "dsac_pend_relu_bound", "dsac_lqs4a2_gelu_nobound",
              "dsac_pend_fixed_alpha"]
FIVE_UPDATES = ["sac_pend_5updates", "dsac_pend_5updates"]
TOL = 1e-4   # the project's parity bound against the reference (rel-L2), as in td3_helpers.py / dsact_helpers.py
Q_NAMES = {"SAC": ("q1", "q2"), "DSAC": ("q",)}
POLICY_AT_OBS2 = {"SAC": "policy", "DSAC": "policy_target"}


def alg_kwargs(meta, use_gpu, **over):
    cfg, lim = meta["cfg"], meta["lim"]
    c = dict(cfg, alg="INFADP", horizon=1)
    kw = dict(algorithm=cfg["alg"], trainer="off_serial_trainer", seed=meta["seed"], cnn_shared=False, env_id=cfg["env_id"],
              obsv_dim=obs_dim_of(c), action_dim=act_dim_of(c), action_type="continu",
              action_low_limit=np.array(lim[0], dtype=np.float32), action_high_limit=np.array(lim[1], dtype=np.float32),
              policy_func_type="MLP", policy_func_name="StochaPolicy", policy_hidden_sizes=list(cfg["hidden"]),
              policy_hidden_activation=cfg["act"], policy_act_distribution="TanhGaussDistribution", policy_learning_rate=1e-3,
              policy_min_log_std=meta["min_log_std"], policy_max_log_std=meta["max_log_std"],
              value_func_type="MLP", value_func_name="ActionValue" if cfg["alg"] == "SAC" else "ActionValueDistri",
              value_hidden_sizes=list(cfg["hidden"]), value_hidden_activation=cfg["act"], value_output_activation="linear",
              value_learning_rate=1e-3, q_learning_rate=1e-3, alpha_learning_rate=3e-4, use_gpu=use_gpu, buffer_name="replay_buffer")
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
        for n in Q_NAMES[meta["cfg"]["alg"]] + ("policy", "alpha"):
            for group in getattr(alg.networks, f"{n}_optimizer").param_groups:
                group["lr"] = meta["lr"]
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def batch_of(g, prefix="in/"):
    return data_from_golden(g, prefix)


def restate_update(alg, data, dtype=torch.float64):
    """One compute_gradient of SAC / DSAC restated with autograd on copies of `alg.networks` at `dtype` (on the host).  `data` holds
    the draws eps_new, eps_next (and z_next).  Returns the backup, the sample at obs2, q_targ, losses, tb values and grads
    {net: [tensors]} + log_alpha_grad."""
    name = type(alg).__name__
    names = Q_NAMES[name]
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items()}
    for n in names + ("policy",):
        for p in getattr(nets, n).parameters():
            p.requires_grad_(True)
            p.grad = None
    alpha = float(nets.log_alpha.detach().exp()) if alg.auto_alpha else float(alg.alpha)
    with torch.no_grad():
        a2, logp2 = nets.create_action_distributions(getattr(nets, POLICY_AT_OBS2[name])(d["obs2"])).rsample(d["eps_next"])
        if name == "SAC":
            qt = torch.stack([nets.q1_target(d["obs2"], a2), nets.q2_target(d["obs2"], a2)])   # [2, B]
            q_next = torch.min(qt[0], qt[1])
        else:
            qt = nets.q_target(d["obs2"], a2)                                                   # [B, 2] = (m, s)
            q_next = qt[:, 0] + torch.clamp(d["z_next"], -3, 3) * qt[:, 1]
        backup = d["rew"] + (1 - d["done"]) * alg.gamma * (q_next - alpha * logp2)
    out, tb = {}, {}
    if name == "SAC":
        q1, q2 = nets.q1(d["obs"], d["act"]), nets.q2(d["obs"], d["act"])
        loss_q = ((q1 - backup) ** 2).mean() + ((q2 - backup) ** 2).mean()
        tb.update({"Loss/Critic loss-RL iter": loss_q, "SAC/critic_avg_q1-RL iter": q1.mean(), "SAC/critic_avg_q2-RL iter": q2.mean()})
    else:
        h = nets.q(d["obs"], d["act"])
        q, sd = h[:, 0], h[:, 1]
        td = (3 * sd.detach().mean()).to(torch.float32).to(dtype)   # (the kernel hands td_bound on as fp32)
        diff = backup - q.detach()
        bound = q.detach() + torch.clamp(diff, -td, td)
        if alg.bound:
            loss_q = torch.mean((q - backup) ** 2 / (2 * sd.detach() ** 2) + (q.detach() - bound) ** 2 / (2 * sd ** 2) + torch.log(sd))
        else:
            loss_q = -torch.distributions.Normal(q, sd).log_prob(backup).mean()
        tb.update({"DSAC/critic_avg_q-RL iter": q.mean(), "DSAC/critic_avg_std-RL iter": sd.mean()})
        out.update(td_bound=td, binds=diff.abs() > td)
    loss_q.backward()
    grads = {n: [p.grad.detach().clone() for p in getattr(nets, n).parameters()] for n in names}
    for n in names:
        for p in getattr(nets, n).parameters():
            p.requires_grad_(False)
    logits = nets.policy(d["obs"])
    new_act, new_logp = nets.create_action_distributions(logits).rsample(d["eps_new"])
    if name == "SAC":
        qn = torch.stack([nets.q1(d["obs"], new_act), nets.q2(d["obs"], new_act)])
        loss_pi = (alpha * new_logp - torch.min(qn[0], qn[1])).mean()
    else:
        qn = nets.q(d["obs"], new_act)[:, 0]
        loss_pi = (alpha * new_logp - qn).mean()
        tb.update({"DSAC/policy_mean-RL iter": torch.tanh(logits[..., 0]).mean(), "DSAC/policy_std-RL iter": logits[..., 1].mean()})
    loss_pi.backward()
    grads["policy"] = [p.grad.detach().clone() for p in nets.policy.parameters()]
    tb.update({"Loss/Actor loss-RL iter": loss_pi, f"{name}/entropy-RL iter": -new_logp.mean(), f"{name}/alpha-RL iter": alpha})
    out.update(backup=backup, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act.detach(), new_logp=new_logp.detach(), qn=qn.detach(),
               loss_q=float(loss_q.detach()), loss_pi=float(loss_pi.detach()), grads=grads,
               tb={k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in tb.items()},
               log_alpha_grad=float(-(new_logp.detach().mean() + alg.target_entropy)))
    return out
