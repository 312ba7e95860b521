"""Shared by the CPU and GPU tests of the actor-critic families - DDPG / TD3 (test_td3_*.py), SAC / DSAC (test_sac_*.py) and DSAC-T
(test_dsact_*.py): building an algorithm from a fixture of tests/golden/make_golden_{td3,sac,dsact}.py or from synthetic networks,
the restatement of one update of each family in torch at any dtype, and the bodies the three families' tests have in common.  The
bodies are plain functions: they take the algorithm (or how to make it), the batch and what the family expects, and assert."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import data_from_golden

from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

TD3_ONE_UPDATE = ["td3_pend_relu", "td3_lqs4a2_gelu", "td3_per_pend_relu", "ddpg_pend_relu", "ddpg_lqs4a2_gelu", "ddpg_per_lqs4a2_gelu"]
SAC_ONE_UPDATE = ["sac_pend_relu", "sac_lqs4a2_gelu", "sac_pend_fixed_alpha", "dsac_pend_relu_bound", "dsac_lqs4a2_gelu_nobound",
                  "dsac_pend_fixed_alpha"]
SAC_FIVE_UPDATES = ["sac_pend_5updates", "dsac_pend_5updates"]
DSACT_ONE_UPDATE = ["dsact_pend_relu", "dsact_lqs4a2_gelu", "dsact_pend_fixed_alpha"]
TOL = 1e-4            # the project's parity bound against the reference (rel-L2 of tensors, `close` for scalars)
EPS32 = 2.0 ** -23
S = -777.0            # sentinel behind the rows a kernel may write

# What create_alg is given per algorithm beyond the common dictionary of `_common_kwargs`.
_DETERM = dict(policy_func_name="DetermPolicy", policy_act_distribution="default", value_func_name="ActionValue")
_STOCHA = dict(policy_func_name="StochaPolicy", policy_act_distribution="TanhGaussDistribution", alpha_learning_rate=3e-4)
FAMILY = {"DDPG": _DETERM, "TD3": _DETERM,
          "SAC": dict(_STOCHA, value_func_name="ActionValue", q_learning_rate=1e-3),
          "DSAC": dict(_STOCHA, value_func_name="ActionValueDistri", q_learning_rate=1e-3),
          "DSACT": dict(_STOCHA, value_func_name="ActionValueDistri")}
CTOR_ATTRS = ("target_noise", "noise_clip")   # of a TD3 fixture's `attrs`: constructor arguments; the rest is set on the object


def close(a, b):
    return abs(float(a) - float(b)) <= TOL * max(1.0, abs(float(b)))


def q_names(alg):
    return alg._q_names


def _common_kwargs(name, env_id, obs_dim, act_dim, lim, hidden, activation, seed, use_gpu):
    return dict(algorithm=name, trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=env_id, obsv_dim=obs_dim,
                action_dim=act_dim, action_type="continu", action_low_limit=np.array(lim[0], dtype=np.float32),
                action_high_limit=np.array(lim[1], dtype=np.float32), policy_func_type="MLP", policy_hidden_sizes=list(hidden),
                policy_hidden_activation=activation, policy_learning_rate=1e-3, value_func_type="MLP", value_hidden_sizes=list(hidden),
                value_hidden_activation=activation, value_output_activation="linear", value_learning_rate=1e-3, use_gpu=use_gpu,
                buffer_name="replay_buffer", **FAMILY[name])


def alg_kwargs(meta, use_gpu, **over):
    """create_alg's arguments for a fixture's `meta` (or one a test wrote in its form).  The deterministic family's meta carries
    `per` and `attrs`, the soft families' the log-std clamp and `ctor`: each is used where it is present."""
    cfg = meta["cfg"]
    c = dict(cfg, alg="INFADP", horizon=1)
    kw = _common_kwargs(cfg["alg"], cfg["env_id"], obs_dim_of(c), act_dim_of(c), meta["lim"], cfg["hidden"], cfg["act"], meta["seed"], use_gpu)
    if meta.get("per"):
        kw["buffer_name"] = "prioritized_replay_buffer"
    if "min_log_std" in meta:
        kw.update(policy_min_log_std=meta["min_log_std"], policy_max_log_std=meta["max_log_std"])
    kw.update({k: v for k, v in meta.get("attrs", {}).items() if k in CTOR_ATTRS})
    kw.update(meta.get("ctor", {}))
    kw.update(over)
    return kw


def load_alg(name, use_gpu=False, prefix="sd/", **over):
    """(alg, fixture, meta): built through create_alg with the fixture's seed (its own RNG draws), attributes and learning rates set
    as the maker set them, then the fixture's state dict loaded."""
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    alg = create_alg(**alg_kwargs(meta, use_gpu, **over))
    for k, v in meta.get("attrs", {}).items():
        if k not in CTOR_ATTRS:
            setattr(alg, k, v)
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})
    if "lr" in meta:
        for opt in [v for k, v in vars(alg.networks).items() if k.endswith("_optimizer")]:
            for group in opt.param_groups:
                group["lr"] = meta["lr"]
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def batch_of(g, prefix="in/"):
    return data_from_golden(g, prefix)


# ------------------------------------------------------------------------------------------
# One update restated on the host, one body per family
# ------------------------------------------------------------------------------------------
def _float_copies(alg, data, dtype, grad_names):
    """Copies of `alg.networks` and of the batch at `dtype` on the host; the networks named take gradients."""
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items() if k != "idx"}
    for n in grad_names:
        for p in getattr(nets, n).parameters():
            p.requires_grad_(True)
            p.grad = None
    return nets, d


def _collect(nets, names):
    return {n: [p.grad.detach().clone() for p in getattr(nets, n).parameters()] for n in names}


def _freeze(nets, names):
    for n in names:
        for p in getattr(nets, n).parameters():
            p.requires_grad_(False)


def _tb_floats(tb):
    return {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in tb.items()}


def restate_td3(alg, data, dtype=torch.float64):
    """One compute_gradient of DDPG / TD3 (gops/algorithm/ddpg.py:95-172, td3.py:106-225) restated with autograd:
    dict(backup, a2, q_targ, loss_q [per critic], loss, q_mean, loss_pi, abs_err, grads {net: [tensors]})."""
    names = q_names(alg)
    nets, d = _float_copies(alg, data, dtype, names + ("policy",))
    with torch.no_grad():
        a2 = nets.policy_target(d["obs2"])
        if "target_noise" in d and len(names) == 2:
            eps = torch.clamp(d["target_noise"] * alg.target_noise, -alg.noise_clip, alg.noise_clip)
            a2 = torch.clamp(a2 + eps, torch.as_tensor(alg.act_low_limit, dtype=dtype), torch.as_tensor(alg.act_high_limit, dtype=dtype))
        q_t = torch.stack([getattr(nets, f"{n}_target")(d["obs2"], a2) for n in names])
        backup = d["rew"] * getattr(alg, "reward_scale", 1) + alg.gamma * (1 - d["done"]) * q_t.min(dim=0).values
    w = d.get("weight") if alg.per_flag else None
    qs = [getattr(nets, n)(d["obs"], d["act"]) for n in names]
    loss_q = [((q - backup) ** 2).mean() if w is None else (w * (q - backup) ** 2).mean() for q in qs]
    sum(loss_q).backward()
    grads = _collect(nets, names)
    _freeze(nets, names[:1])
    loss_pi = -getattr(nets, names[0])(d["obs"], nets.policy(d["obs"])).mean()
    loss_pi.backward()
    grads.update(_collect(nets, ("policy",)))
    return dict(backup=backup, a2=a2, q_targ=q_t, loss_q=[l.detach() for l in loss_q], loss=sum(loss_q).detach(), q_mean=qs[0].mean().detach(),
                loss_pi=loss_pi.detach(), abs_err=(qs[0] - backup).abs().detach(), grads=grads)


def restate_soft_q(alg, data, dtype=torch.float64):
    """One compute_gradient of SAC / DSAC (gops/algorithm/sac.py:159-241, dsac.py:155-267) restated with autograd.  `data` holds the
    draws eps_new, eps_next (and z_next).  Returns the backup, the sample at obs2, q_targ, losses, tb values and grads
    {net: [tensors]} + log_alpha_grad."""
    name = type(alg).__name__
    names = q_names(alg)
    nets, d = _float_copies(alg, data, dtype, names + ("policy",))
    alpha = float(nets.log_alpha.detach().exp()) if alg.auto_alpha else float(alg.alpha)
    with torch.no_grad():
        at_obs2 = nets.policy if name == "SAC" else nets.policy_target   # (sac.py has no target policy)
        a2, logp2 = nets.create_action_distributions(at_obs2(d["obs2"])).rsample(d["eps_next"])
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
    grads = _collect(nets, names)
    _freeze(nets, names)
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
    grads.update(_collect(nets, ("policy",)))
    tb.update({"Loss/Actor loss-RL iter": loss_pi, f"{name}/entropy-RL iter": -new_logp.mean(), f"{name}/alpha-RL iter": alpha})
    out.update(backup=backup, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act.detach(), new_logp=new_logp.detach(), qn=qn.detach(),
               loss_q=float(loss_q.detach()), loss_pi=float(loss_pi.detach()), grads=grads, tb=_tb_floats(tb),
               log_alpha_grad=float(-(new_logp.detach().mean() + alg.target_entropy)))
    return out


def restate_dsact(alg, data, dtype=torch.float64, mean_std=None):
    """One compute_gradient of DSAC-T (gops/algorithm/dsact.py:162-329) restated with autograd.  `data` holds the draws eps_new,
    eps_next, z_next; `mean_std`: the running values before this update ([2], or None for the first one; they are fp32 state, and
    the updated pair is rounded to fp32 as the device state holds it).  Returns the targets, the target policy's sample, losses,
    statistics and grads {net: [tensors]} + log_alpha_grad."""
    nets, d = _float_copies(alg, data, dtype, ("q1", "q2", "policy"))
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
    grads = _collect(nets, ("q1", "q2"))
    _freeze(nets, ("q1", "q2"))
    logits = nets.policy(d["obs"])
    new_act, new_logp = nets.create_action_distributions(logits).rsample(d["eps_new"])
    qn = torch.stack([nets.q1(d["obs"], new_act)[:, 0], nets.q2(d["obs"], new_act)[:, 0]])
    loss_pi = (alpha * new_logp - torch.min(qn[0], qn[1])).mean()
    loss_pi.backward()
    grads.update(_collect(nets, ("policy",)))
    mean_l, std_l = torch.chunk(logits.detach(), 2, dim=-1)
    A = d["act"].shape[1]
    tb = {"DSAC2/critic_avg_q1-RL iter": heads[0][:, 0].mean(), "DSAC2/critic_avg_q2-RL iter": heads[1][:, 0].mean(),
          "DSAC2/critic_avg_std1-RL iter": heads[0][:, 1].mean(), "DSAC2/critic_avg_std2-RL iter": heads[1][:, 1].mean(),
          "DSAC2/critic_avg_min_std1-RL iter": heads[0][:, 1].min(), "DSAC2/critic_avg_min_std2-RL iter": heads[1][:, 1].min(),
          "Loss/Actor loss-RL iter": loss_pi, "Loss/Critic loss-RL iter": sum(losses), "DSAC2/policy_mean-RL iter": torch.tanh(mean_l).mean(),
          "DSAC2/policy_std-RL iter": std_l.mean(), "DSAC2/entropy-RL iter": -new_logp.mean(), "DSAC2/alpha-RL iter": alpha,
          "DSAC2/mean_std1": new_ms[0], "DSAC2/mean_std2": new_ms[1]}
    return dict(target_q=tq, target_q_sample=tqs, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act.detach(), new_logp=new_logp.detach(),
                mean_std=torch.stack(new_ms).detach(), tb=_tb_floats(tb), grads=grads, qn=qn.detach(),
                log_alpha_grad=float(-(new_logp.detach().mean() + (-A))), binds=torch.stack(binds), heads=torch.stack(heads).detach())


_RESTATE = {"DDPG": restate_td3, "TD3": restate_td3, "SAC": restate_soft_q, "DSAC": restate_soft_q, "DSACT": restate_dsact}


def restate_update(alg, data, dtype=torch.float64, **kw):
    """The family's restatement of one update on copies of `alg.networks` at `dtype` (on the host)."""
    return _RESTATE[type(alg).__name__](alg, data, dtype, **kw)


# ------------------------------------------------------------------------------------------
# Bodies of the CPU tests
# ------------------------------------------------------------------------------------------
def check_host_restatement(name, keys, what, capsys):
    """The fixture's state dict loaded into the networks create_alg built, one update restated on the host in fp32: the outputs
    named in `keys` and every gradient against the reference's, rel-L2 <= TOL.  -> (alg, fixture, meta, restatement) for what the
    family compares beyond that."""
    alg, g, meta = load_alg(name)
    got = restate_update(alg, batch_of(g), dtype=torch.float32)
    worst = 0.0
    for key in keys:
        worst = max(worst, rel_l2(got[key], g[key]))
    for n in q_names(alg) + ("policy",):
        for i, gr in enumerate(got["grads"][n]):
            worst = max(worst, rel_l2(gr, g[f"{n}_grad/{i}"]))
    with capsys.disabled():
        print(f"\n{name}: worst rel-L2 of {what} / gradients against the reference {worst:.2e}")
    assert worst <= TOL
    return alg, g, meta, got


def check_soft_tb_and_alpha(alg, g, got):
    """The soft families' restated tb values (the reference's keys, each one) and log_alpha's gradient against the fixture."""
    tb_keys = [k for k in g if k.startswith("tb/")]
    assert {k[3:] for k in tb_keys} == set(got["tb"])
    for k in tb_keys:
        assert close(got["tb"][k[3:]], g[k]), k
    if alg.auto_alpha:
        assert close(got["log_alpha_grad"], g["log_alpha_grad"])
    else:
        assert "log_alpha_grad" not in g


# What every family refuses, and what the two soft families refuse on top; a module adds what is its own.
REFUSALS = [(dict(policy_func_type="POLY", policy_degree=1, policy_add_bias=False), "POLY"),
            (dict(value_func_type="POLY", value_degree=2, value_add_bias=False), "POLY"),
            (dict(policy_func_type="LipsNet"), "LipsNet"),
            (dict(mlp_dtype="fp16"), "fp32 only"),
            (dict(value_output_activation="tanh"), "linear output"),
            (dict(policy_output_activation="relu"), "linear output"),
            (dict(trainer="off_sync_trainer"), "off_serial"),
            (dict(trainer="off_async_trainer"), "off_serial")]
SOFT_REFUSALS = [(dict(policy_func_name="DetermPolicy"), "stochastic policy"),
                 (dict(policy_act_distribution="GaussDistribution"), "tanh-Gaussian"),
                 (dict(policy_act_distribution="default"), "tanh-Gaussian"),
                 (dict(buffer_name="prioritized_replay_buffer"), "no priorities")]


def check_refusals(kw_of, cases):
    """create_alg(**kw_of(**over)) raises NotImplementedError naming `reason`, for every (over, reason) of `cases`."""
    for over, reason in cases:
        with pytest.raises(NotImplementedError, match=reason):
            create_alg(**kw_of(**over))


# ------------------------------------------------------------------------------------------
# Synthetic algorithms and batches of the GPU tests
# ------------------------------------------------------------------------------------------
ENV_OF_OBS = {3: "gym_pendulum", 4: "pyth_lq", 6: "pyth_idpendulum"}
LIM_OF_ACT = {1: ([-2.0], [2.0]), 2: ([-1.0, -0.5], [2.0, 0.5]), 4: ([-1.0, -0.5, -2.0, -1.0], [2.0, 0.5, 2.0, 1.0])}


def synthetic_meta(name, obs, act, hidden, activation, seed, **family):
    """A fixture's `meta` for networks of this shape; `family`: per / attrs, or the log-std clamp and ctor."""
    meta = dict(cfg=dict(alg=name, env_id=ENV_OF_OBS[obs], hidden=hidden, act=activation), lim=LIM_OF_ACT[act], seed=seed, **family)
    if obs == 4:
        meta["cfg"]["lq_config"] = "s4a2"
    return meta


def synthetic_alg(meta, obs, act, shape_heads, **over):
    """The algorithm of `meta` on the GPU with every target network randomised apart from its online twin, then
    `shape_heads(alg, probe, act)` on 256 probe observations (so that the batches of `synthetic_batch` meet every branch)."""
    seed = meta["seed"]
    torch.manual_seed(seed)
    a = create_alg(**alg_kwargs(meta, True, **dict(dict(action_dim=act), **over)))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in a.networks.named_parameters():
            if "_target." in n:
                p.add_(0.3 * (torch.rand(p.shape, generator=g) - 0.5))
        shape_heads(a, torch.randn(256, obs, generator=g), act)
    a.networks.cuda()
    return a


def spread_target_head(a, probe, act):
    """DDPG / TD3: the target head spread to +-3 around zero on inputs like `synthetic_batch`'s (tanh saturates on some rows, not on
    others) and the twin targets centred on each other: rows on both sides of every clamp and of the minimum."""
    nets = a.networks
    head = nets.policy_target.linear_layers()[-1]
    spread = 3.0 / nets.policy_target.pi(probe).std(dim=0)
    head.weight.mul_(spread[:, None])
    head.bias.mul_(spread)
    head.bias.sub_(nets.policy_target.pi(probe).median(dim=0).values)
    if len(q_names(a)) == 2:
        a2 = nets.policy_target(probe)
        nets.q2_target.linear_layers()[-1].bias.add_((nets.q1_target(probe, a2) - nets.q2_target(probe, a2)).median())


def shape_soft_heads(a, probe, act):
    """SAC / DSAC / DSAC-T: every policy's head with means within +-0.9 and log stds on both sides of the clamp [-3, -0.5] (so
    |u| <= 0.9 + 3.3 * exp(-0.5) stays where fp32 resolves 1 + 1e-6 - tanh(u)^2), twin target critics' means centred on each other
    at the mode of the policy the backup samples."""
    nets = a.networks
    for pol in [nets.policy] + ([nets.policy_target] if hasattr(nets, "policy_target") else []):
        head, y = pol.linear_layers()[-1], pol.policy(probe)
        scale = torch.cat([0.9 / y[:, :act].abs().max(dim=0).values.clamp_min(0.9), 1.6 / y[:, act:].std(dim=0)])
        head.weight.mul_(scale[:, None])
        head.bias.mul_(scale)
        head.bias[act:].sub_(pol.policy(probe)[:, act:].median(dim=0).values + 1.75)
    if len(q_names(a)) == 2:
        pol = getattr(nets, a._policy_at_obs2)
        a2 = pol.get_act_dist(pol(probe)).mode()
        gap = nets.q1_target(probe, a2) - nets.q2_target(probe, a2)   # [256], or [256, 2] = (mean, std) of distributional critics
        nets.q2_target.linear_layers()[-1].bias[0].add_((gap if gap.dim() == 1 else gap[:, 0]).median())


TRANSITION = ("obs", "act", "rew", "obs2", "done")


def synthetic_batch(B, obs, act, seed=0, z_next=None):
    """A transition batch with done rows at both ends, and the update's draws behind it: `z_next` None - target_noise (TD3);
    a shape - eps_new, eps_next (within +-3.3) and return samples z_next of that shape (the soft families)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, obs, generator=g)
    d = (torch.rand(B, generator=g) < 0.2).float()
    if B > 1:
        d[0], d[-1] = 1.0, 0.0
    data = dict(obs=o, act=torch.rand(B, act, generator=g) * 2 - 1, rew=torch.randn(B, generator=g), obs2=o + 0.1 * torch.randn(B, obs, generator=g),
                done=d)
    if z_next is None:
        data.update(target_noise=torch.randn(B, act, generator=g))
    else:
        data.update(eps_new=torch.randn(B, act, generator=g), eps_next=torch.randn(B, act, generator=g).clamp(-3.3, 3.3),
                    z_next=2 * torch.randn(z_next, generator=g))
    return data


# ------------------------------------------------------------------------------------------
# Bodies of the GPU tests
# ------------------------------------------------------------------------------------------
def check_backup(got, again, comp, ref, keys, label):
    """The rule of the fused backups: the composed path's max error against the float64 restatement `ref` is measured on the same
    inputs first; the fused kernel (`got`) may use twice that, but not less than 4 fp32 ulp of the largest |value| of the tensor
    compared.  Prints both errors.  A second launch (`again`) gives the same bits."""
    for k in keys:
        want = ref[k].reshape(got[k].shape)
        err_c = (comp[k].double().cpu() - want).abs().max().item()
        err_f = (got[k].double().cpu() - want).abs().max().item()
        bound = max(2 * err_c, 4 * EPS32 * want.abs().max().item())
        print(f"{label} {k}: fused {err_f:.3e} composed {err_c:.3e} bound {bound:.3e}")
        assert err_f <= bound, (label, k, err_f, err_c, bound)
        assert torch.equal(got[k], again[k]), (label, k)


def check_rows_beyond_the_batch(run, sizes, pad=64):
    """`run(out=...)` with every output of `sizes` (name: floats) allocated with `pad` floats of sentinel behind it: the kernel
    writes all of the batch's floats and none beyond.  -> what `run` returned."""
    bufs = {k: torch.full((n + pad,), S, device="cuda") for k, n in sizes.items()}
    got = run(out={k: v[:sizes[k]] for k, v in bufs.items()})
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert (t[sizes[k]:] == S).all() and (t[:sizes[k]] != S).all(), k
    return got


def check_one_update(alg, g, meta, fused):
    """One get_remote_update_info on the fixture's batch: the path taken, every recorded tb value, the keys of the update info, every
    gradient (and log_alpha's where it is learnt) against the reference's.  -> (data, extra, tb, info)."""
    data = batch_of(g)
    extra, info = alg.get_remote_update_info(data, 0)
    assert alg.backup_path == ("fused" if fused else "composed")
    tb = extra[0] if meta.get("per") else extra
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), (k, float(tb[k[3:]]), float(g[k]))
    names = q_names(alg) + ("policy",)
    auto = getattr(alg, "auto_alpha", False)
    assert set(info) == {f"{n}_grad" for n in names} | {"iteration"} | ({"log_alpha_grad"} if auto else set()) and info["iteration"] == 0
    for n in names:
        for i, gr in enumerate(info[f"{n}_grad"]):
            assert rel_l2(gr.cpu(), g[f"{n}_grad/{i}"]) < TOL, (n, i, rel_l2(gr.cpu(), g[f"{n}_grad/{i}"]))
    if auto:
        assert close(info["log_alpha_grad"], g["log_alpha_grad"])
    return data, extra, tb, info


def check_the_step_moves_everything(alg, info):
    """remote_update: every parameter stays finite and moves (the action limits and a fixed log_alpha stay)."""
    before = {k: v.detach().clone() for k, v in alg.networks.state_dict().items()}
    alg.remote_update(info)
    after = alg.networks.state_dict()
    assert all(torch.isfinite(p).all() for p in after.values())
    assert all((after[k] - before[k]).abs().max() > 0 for k in before if "lim" not in k and (getattr(alg, "auto_alpha", True) or k != "log_alpha"))


def check_fused_and_composed_agree(name, check_backup_of):
    """The two backups differ by fp32 rounding only (`check_backup`'s bound, measured on the fixture's own inputs by the module's
    `check_backup_of(alg, data, label)`); the gradients are linear in the backup: 1e-5 relative, a tenth of the parity bound,
    leaves two decades for their conditioning."""
    out = {}
    for fused in (True, False):
        alg, g, meta = load_alg(name, use_gpu=True, fused_target=fused)
        _, info = alg.get_remote_update_info(batch_of(g), 0)
        out[fused] = {n: [t.clone() for t in v] for n, v in info.items() if n.endswith("_grad") and n != "log_alpha_grad"}
    check_backup_of(alg, batch_of(g), name)
    for n in out[True]:
        for a, b in zip(out[True][n], out[False][n]):
            assert rel_l2(a.cpu(), b.cpu()) <= 1e-5, n


def five_updates(name, critic_loss=True):
    """Five `local_update` calls on the fixture `name` with the reference's own draws handed in.  After each: the actor loss (and
    the critic loss, where the reference reports one) and every entry of the state dict against the reference's, rel-L2 < TOL;
    then yields (alg, fixture, k, state dict before the call) for the family's own assertions."""
    alg, g, meta = load_alg(name, use_gpu=True, prefix="sd0/")
    for k in range(5):
        before = {key: v.detach().clone() for key, v in alg.networks.state_dict().items()}
        tb = alg.local_update(batch_of(g, f"in{k}/"), k)
        assert close(tb["Loss/Actor loss-RL iter"], g[f"loss_pi{k}"]), k
        if critic_loss:
            assert close(tb["Loss/Critic loss-RL iter"], g[f"loss_q{k}"]), k
        for key, p in alg.networks.state_dict().items():
            assert rel_l2(p.cpu().double(), g[f"sd{k + 1}/{key}"]) < TOL, (k, key)
        yield alg, g, k, before


def delayed(key):
    """State-dict keys that step only when `iteration % delay_update == 0` in DSAC and DSAC-T."""
    return key == "log_alpha" or key.startswith("policy.") or "_target." in key


def check_graph_replay(make_alg, n_graphs, monkeypatch):
    """local_update captured into HIP graphs (one per value of `iteration % delay_update == 0`; the draws are made by the
    algorithm's own generator - same seed, same draws in both runs - and travel with the batch as graph inputs) walks exactly the
    parameter trajectory of the eager launches: 14 updates, of which at least 6 are replays.  -> (eager, graph)."""
    def run(mode):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        alg = make_alg()
        logs = []
        for it in range(14):
            data = synthetic_batch(70, 3, 1, seed=100 + it)
            logs.append(dict(alg.local_update({k: data[k] for k in TRANSITION}, it)))
        return alg, logs

    eager, log_e = run("0")
    graph, log_g = run("1")
    assert all(c.graph is not None for c in graph._graphs.values()) and len(graph._graphs) == n_graphs
    assert all(c.graph is None for c in eager._graphs.values())
    for (ne, pe), (ng, pg) in zip(eager.networks.named_parameters(), graph.networks.named_parameters()):
        assert ne == ng and torch.equal(pe, pg), ne
    for a, b in zip(log_e, log_g):
        for k in a:
            if not k.startswith("Time/"):
                assert float(a[k]) == float(b[k]), k
    return eager, graph


def trainer_kwargs(name, env_id, obs, lim, tmp_path, **over):
    """Arguments of a short OffSerialTrainer run of `name` with 64-wide networks and one action within +-lim."""
    kw = _common_kwargs(name, env_id, obs, 1, ([-lim], [lim]), [64, 64], "relu", 0, True)
    kw.update(buffer_max_size=4096, buffer_warm_size=512, replay_batch_size=64, sample_interval=1, additional_info={}, max_iteration=8,
              log_save_interval=1000, apprfunc_save_interval=1000, eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    kw.update(over)
    return kw


def build_trainer(kw, make_sampler, evaluator):
    """Algorithm on the GPU, env model, `make_sampler(model, alg)`, buffer, (evaluator,) OffSerialTrainer, constructed in this order
    after torch.manual_seed(0).  -> (alg, buffer, evaluator or None, trainer)."""
    from gops_amd.create_pkg.create_buffer import create_buffer
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    from gops_amd.create_pkg.create_trainer import create_trainer
    torch.manual_seed(0)
    alg = create_alg(**kw)
    alg.networks.to("cuda")
    model = create_env_model(**kw)
    smp = make_sampler(model, alg)
    buf = create_buffer(**kw)
    ev = create_evaluator(**dict(kw, env_model=model, networks=alg.networks, num_eval_episode=4, eval_save=False, is_render=False,
                                 max_episode_steps=40)) if evaluator else None
    return alg, buf, ev, create_trainer(alg, smp, buf, ev, **kw)


def run_trainer(trainer, alg, each_step=None):
    """Six trainer steps (`each_step()` after each); the updates took the one-launch backup."""
    for _ in range(6):
        trainer.step()
        trainer.iteration += 1
        if each_step is not None:
            each_step()
    assert alg.backup_path == "fused"
