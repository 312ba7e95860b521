"""Generate the SAC and DSAC fixtures (`sac_*.npz`, `dsac_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_sac.py
Every array written here is an input, or an output of the reference's own classes (`gops.algorithm.sac.SAC`, `gops.algorithm.dsac.DSAC`)
built with the helpers of make_golden.py and _make_ac_common.py.  The reference draws inside the update (see DrawTap there): SAC two
policy samples; DSAC two policy samples and three return samples, of which only the target critic's reaches an output.  The fixture
stores the draws that reach an output - `eps_new`, `eps_next`, DSAC's `z_next` [B] - and the targets, log-probabilities and losses are
recomputed here from those with the reference's own networks and checked against what the reference reported (DSAC reports no critic
loss: there the recomputed loss's gradient is checked against the reference's `q_grad`): the draws are attributed correctly.
"""
import copy
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)
from _make_ac_common import (LIM_A, LIM_B, MAX_LOG_STD, MIN_LOG_STD, SHAPE_A, SHAPE_B, STOCHA, DrawTap, arrays, batch_of, build_reference,  # noqa: E402
                             close, five_batches, last_linear, meta_entry, state, tanh_gauss_rsample, update_entries)

from gops.algorithm.dsac import DSAC  # noqa: E402
from gops.algorithm.sac import SAC  # noqa: E402
from gops.utils.act_distribution_type import TanhGaussDistribution  # noqa: E402

# name: (algorithm, cfg, action limits, constructor arguments)
CASES = {
    "sac_pend_relu": ("SAC", SHAPE_A, LIM_A, dict(gamma=0.97, tau=0.005, auto_alpha=True)),
    "sac_lqs4a2_gelu": ("SAC", SHAPE_B, LIM_B, dict(gamma=0.99, tau=0.005, auto_alpha=True, target_entropy=-1.5)),
    "sac_pend_fixed_alpha": ("SAC", SHAPE_A, LIM_A, dict(gamma=0.99, tau=0.005, auto_alpha=False, alpha=0.2, target_entropy=-0.5)),
    "dsac_pend_relu_bound": ("DSAC", SHAPE_A, LIM_A, dict(gamma=0.97, tau=0.005, auto_alpha=True, bound=True, delay_update=2)),
    "dsac_lqs4a2_gelu_nobound": ("DSAC", SHAPE_B, LIM_B, dict(gamma=0.99, tau=0.005, auto_alpha=True, bound=False, delay_update=2)),
    "dsac_pend_fixed_alpha": ("DSAC", SHAPE_A, LIM_A, dict(gamma=0.99, tau=0.005, auto_alpha=False, alpha=0.2, bound=True, delay_update=2)),
}
Q_NAMES = {"SAC": ("q1", "q2"), "DSAC": ("q",)}
POLICY_AT_OBS2 = {"SAC": "policy", "DSAC": "policy_target"}
MIN_STD = 0.05   # of the online critic on the data (DSAC): 1 / sd^3 must not amplify fp32 rounding


def draws_of(name, tap):
    """SAC (sac.py:165, 217): rsample at obs, rsample at obs2.  DSAC (dsac.py:164, 221, 223-226, 256): the same two, then return
    samples for q on the data (unused), q_target at obs2 (z_next), q on the new action (unused)."""
    assert len(tap.rsamples) == 2 and len(tap.samples) == (0 if name == "SAC" else 3), (len(tap.rsamples), len(tap.samples))
    dr = dict(eps_new=tap.rsamples[0], eps_next=tap.rsamples[1])
    if name == "DSAC":
        dr["z_next"] = tap.samples[1]
    return dr


def build(name, cfg, lim, ctor, seed):
    return build_reference(SAC if name == "SAC" else DSAC, cfg, lim, seed, q_learning_rate=1e-3,
                           value_func_name="ActionValue" if name == "SAC" else "ActionValueDistri", **STOCHA, **ctor)


def balance(name, alg, data):
    """make_golden_dsact.balance for these networks: both uses of the policy get means within +-0.9 and log stds on both sides of the
    clamp (SAC samples its ONE policy at obs and at obs2: it is shaped on both), SAC's twin critics are centred on each other."""
    nets, A = alg.networks, data["act"].shape[1]
    with torch.no_grad():
        uses = ((nets.policy, torch.cat([data["obs"], data["obs2"]])),) if name == "SAC" else ((nets.policy, data["obs"]), (nets.policy_target, data["obs2"]))
        for pol, o in uses:
            head, y = last_linear(pol.policy), pol.policy(o)
            scale = torch.cat([0.9 / y[:, :A].abs().max(dim=0).values, 1.6 / y[:, A:].std(dim=0)])
            head.weight.mul_(scale[:, None])
            head.bias.mul_(scale)
            head.bias[A:].sub_(pol.policy(o)[:, A:].median(dim=0).values - 0.5 * (MIN_LOG_STD + MAX_LOG_STD))
        if name == "SAC":
            a2 = TanhGaussDistribution(nets.policy(data["obs2"])).mode()
            last_linear(nets.q2_target.q).bias[0].add_((nets.q1_target(data["obs2"], a2) - nets.q2_target(data["obs2"], a2)).median())
            a1 = TanhGaussDistribution(nets.policy(data["obs"])).mode()
            last_linear(nets.q2.q).bias[0].add_((nets.q1(data["obs"], a1) - nets.q2(data["obs"], a1)).median())


def recompute(name, alg, data, dr):
    """The update's intermediate values from the recorded draws with the reference's own networks (fp32, as the reference computes);
    the critic loss keeps its graph."""
    nets = alg.networks
    alpha = float(nets.log_alpha.exp()) if alg.auto_alpha else alg.alpha
    rsample = lambda logits, eps: tanh_gauss_rsample(nets.policy, logits, eps)   # noqa: E731
    out = {}
    with torch.no_grad():
        a2, logp2, u2 = rsample(getattr(nets, POLICY_AT_OBS2[name])(data["obs2"]), dr["eps_next"])
        live = (1 - data["done"]) * alg.gamma
        if name == "SAC":
            qt = torch.stack([nets.q1_target(data["obs2"], a2), nets.q2_target(data["obs2"], a2)])   # [2, B]
            q_next = torch.min(qt[0], qt[1])
        else:
            qt = nets.q_target(data["obs2"], a2)                                                       # [B, 2]
            q_next = qt[:, 0] + torch.clamp(dr["z_next"], -3, 3) * qt[:, 1]
        backup = data["rew"] + live * (q_next - alpha * logp2)
        new_act, new_logp, u1 = rsample(nets.policy(data["obs"]), dr["eps_new"])
    if name == "SAC":
        q1, q2 = nets.q1(data["obs"], data["act"]), nets.q2(data["obs"], data["act"])
        loss_q = ((q1 - backup) ** 2).mean() + ((q2 - backup) ** 2).mean()
        with torch.no_grad():
            qn = torch.stack([nets.q1(data["obs"], new_act), nets.q2(data["obs"], new_act)])
            loss_pi = (alpha * new_logp - torch.min(qn[0], qn[1])).mean()
        out.update(qn=qn, avg=(q1.detach().mean(), q2.detach().mean()))
    else:
        h = nets.q(data["obs"], data["act"])
        q, sd = h[:, 0], h[:, 1]
        td = 3 * sd.detach().mean()
        diff = backup - q.detach()
        tb_ = q.detach() + torch.clamp(diff, -td, td)
        if alg.bound:
            loss_q = torch.mean((q - backup) ** 2 / (2 * sd.detach() ** 2) + (q.detach() - tb_) ** 2 / (2 * sd ** 2) + torch.log(sd))
        else:
            loss_q = -torch.distributions.Normal(q, sd).log_prob(backup).mean()
        with torch.no_grad():
            loss_pi = (alpha * new_logp - nets.q(data["obs"], new_act)[:, 0]).mean()
        out.update(binds=diff.abs() > td, td_bound=td, min_std=sd.detach().min(), avg=(q.detach().mean(), sd.detach().mean()))
    out.update(backup=backup, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act, new_logp=new_logp, loss_q=loss_q, loss_pi=loss_pi,
               u=torch.cat([u1.reshape(-1), u2.reshape(-1)]))
    return out


def assert_cases(tag, name, alg, data, rc):
    """Every branch of the update has rows on both sides in the batch (otherwise the fixtures leave it untested)."""
    nets, A = alg.networks, data["act"].shape[1]
    checks = {"done rows": bool((data["done"] == 1).any()) and bool((data["done"] == 0).any()), "max |u| <= 3": float(rc["u"].abs().max()) <= 3.0}
    if name == "SAC":
        checks.update({"q1_target < q2_target": bool((rc["q_targ"][0] < rc["q_targ"][1]).any()),
                       "q2_target < q1_target": bool((rc["q_targ"][1] < rc["q_targ"][0]).any()),
                       "q1 < q2 at the new action": bool((rc["qn"][0] < rc["qn"][1]).any()),
                       "q2 < q1 at the new action": bool((rc["qn"][1] < rc["qn"][0]).any())})
    else:
        checks.update({"td_bound clamp binds": bool(rc["binds"].any()), "td_bound clamp idle": bool((~rc["binds"]).any()),
                       f"min(sd) >= {MIN_STD}": float(rc["min_std"]) >= MIN_STD})
    uses = (("policy at obs", nets.policy, data["obs"]), ("policy at obs2", getattr(nets, POLICY_AT_OBS2[name]), data["obs2"]))
    for use, pol, o in uses:
        ls = pol.policy(o)[:, A:].detach()
        checks[f"{use}: log std below the clamp"] = bool((ls < MIN_LOG_STD).any())
        checks[f"{use}: log std inside the clamp"] = bool(((ls > MIN_LOG_STD) & (ls < MAX_LOG_STD)).any())
        checks[f"{use}: log std above the clamp"] = bool((ls > MAX_LOG_STD).any())
    for n, p in nets.named_parameters():
        if "_target." in n:
            checks[f"{n} moved"] = not torch.equal(p, dict(nets.named_parameters())[n.replace("_target", "")])
    missing = [k for k, ok in checks.items() if not ok]
    assert not missing, (tag, missing)


def check_reported(tag, name, alg, rc, tb, info):
    """The recomputed values against what the reference reported for the same update."""
    assert close(rc["loss_pi"], tb["Loss/Actor loss-RL iter"]), tag
    if name == "SAC":
        assert close(rc["loss_q"], tb["Loss/Critic loss-RL iter"]), tag
        assert close(rc["avg"][0], tb["SAC/critic_avg_q1-RL iter"]) and close(rc["avg"][1], tb["SAC/critic_avg_q2-RL iter"]), tag
    else:
        assert close(rc["avg"][0], tb["DSAC/critic_avg_q-RL iter"]) and close(rc["avg"][1], tb["DSAC/critic_avg_std-RL iter"]), tag
        grads = torch.autograd.grad(rc["loss_q"], list(alg.networks.q.parameters()))
        for mine, ref in zip(grads, info["q_grad"]):
            assert float((mine - ref).norm()) <= 1e-5 * float(ref.norm()), tag


def one_update(tag):
    """The seed is the first one from the tag's checksum on at which the INPUTS populate every branch (assert_cases)."""
    base = zlib.crc32(tag.encode()) % 1000
    for seed in range(base, base + 8):
        try:
            return one_update_at(tag, seed)
        except AssertionError as e:
            if not (len(e.args) == 1 and isinstance(e.args[0], tuple) and e.args[0][0] == tag and isinstance(e.args[0][1], list)):
                raise
            print(f"{tag}: seed {seed} leaves {e.args[0][1]} without rows")
    raise AssertionError(tag)


def one_update_at(tag, seed):
    name, cfg, lim, ctor = CASES[tag]
    alg, g = build(name, cfg, lim, ctor, seed)
    data = batch_of(cfg, seed, g)
    balance(name, alg, data)
    out = {**arrays(data, "in/"), **meta_entry(cfg=dict(cfg, alg=name), lim=lim, ctor=ctor, seed=seed, min_log_std=MIN_LOG_STD,
                                               max_log_std=MAX_LOG_STD), **state(alg)}
    before = copy.deepcopy(alg.networks)
    with DrawTap() as tap:
        tb, info = alg.get_remote_update_info(dict(data), 0)
    dr = draws_of(name, tap)
    out.update(arrays(dr, "in/"))
    after, alg.networks = alg.networks, before
    rc = recompute(name, alg, data, dr)
    check_reported(tag, name, alg, rc, tb, info)
    assert_cases(tag, name, alg, data, rc)
    alg.networks = after
    for k in ("backup", "a2", "logp_next", "q_targ", "new_act", "new_logp", "loss_q", "loss_pi") + (("td_bound",) if name == "DSAC" else ()):
        out[k] = rc[k].detach().numpy().copy()
    out.update(update_entries(info, tb, log_alpha=alg.auto_alpha))
    mg.save(tag, **out)


def five_updates(name):
    """Every parameter and log_alpha after each of five consecutive `local_update` calls (DSAC: delay_update = 2 - policy, temperature
    and targets step at iterations 0, 2, 4 only); learning rates raised so that every step is well above fp32 rounding."""
    tag = f"{name.lower()}_pend_5updates"
    cfg, lim = SHAPE_A, LIM_A
    ctor = dict(gamma=0.97, tau=0.05, auto_alpha=True, **(dict(bound=True, delay_update=2) if name == "DSAC" else {}))
    seed = zlib.crc32(tag.encode()) % 1000
    alg, g = build(name, cfg, lim, ctor, seed)
    nets = alg.networks
    out = meta_entry(cfg=dict(cfg, alg=name), lim=lim, ctor=ctor, seed=seed, lr=1e-2, min_log_std=MIN_LOG_STD, max_log_std=MAX_LOG_STD)
    batches, sd0 = five_batches(alg, cfg, seed, g, lambda data: balance(name, alg, data))
    out.update(sd0)
    for k, data in enumerate(batches):
        out.update(arrays(data, f"in{k}/"))
        if name == "DSAC":
            assert float(nets.q(data["obs"], data["act"])[:, 1].min()) >= MIN_STD, (tag, k)
        with DrawTap() as tap:
            tb = alg.local_update(dict(data), k)
        out.update(arrays(draws_of(name, tap), f"in{k}/"))
        out[f"loss_pi{k}"] = np.float64(tb["Loss/Actor loss-RL iter"])
        if name == "SAC":
            out[f"loss_q{k}"] = np.float64(tb["Loss/Critic loss-RL iter"])
        out.update(state(alg, f"sd{k + 1}/"))
    mg.save(tag, **out)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for tag in CASES:
        if not only or tag in only:
            one_update(tag)
    for name in ("SAC", "DSAC"):
        if not only or "five_updates" in only:
            five_updates(name)
