"""Generate the DSAC-T fixtures (`dsact_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_dsact.py
Every array written here is an input, or an output of the reference's own class (`gops.algorithm.dsact.DSACT`) built with the helpers
of make_golden.py.  The reference draws inside the update: `Independent(Normal).rsample()` for the two policy samples (through
`torch.distributions.normal._standard_normal`) and `Normal.sample()` for the return samples (through `torch.normal`).  Both calls are
wrapped in this process; of the eight draws of one update the fixture stores the four that reach an output - `eps_new`, `eps_next`,
`z_next` [2, B] - and the targets, log-probabilities and losses are recomputed here from those with the reference's own networks and
checked against the losses the reference reported: the draws are attributed correctly.
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

from gops.algorithm.dsact import DSACT  # noqa: E402
from gops.utils.act_distribution_type import GaussDistribution, TanhGaussDistribution  # noqa: E402

# name: (cfg, action limits, constructor arguments)
CASES = {
    "dsact_pend_relu": (SHAPE_A, LIM_A, dict(gamma=0.97, tau=0.005, auto_alpha=True, delay_update=2)),
    "dsact_lqs4a2_gelu": (SHAPE_B, LIM_B, dict(gamma=0.99, tau=0.005, auto_alpha=True, delay_update=2, tau_b=0.01)),
    "dsact_pend_fixed_alpha": (SHAPE_A, LIM_A, dict(gamma=0.99, tau=0.005, auto_alpha=False, alpha=0.2, delay_update=2)),
}


def draws_of(tap):
    """The update's order (dsact.py:172, 239, 241-242, 254-260, 317-318): rsample at obs, rsample at obs2; samples for q1, q2 on the
    data (unused), q1_target, q2_target (z_next), q1, q2 on the new action (unused)."""
    assert len(tap.rsamples) == 2 and len(tap.samples) == 6
    return dict(eps_new=tap.rsamples[0], eps_next=tap.rsamples[1], z_next=torch.stack([tap.samples[2], tap.samples[3]]))


def build(cfg, lim, ctor, seed):
    return build_reference(DSACT, cfg, lim, seed, value_func_name="ActionValueDistri", **STOCHA, **ctor)


def balance(alg, data):
    """Shape both policies' heads on this batch - means within +-0.9 (so that |u| stays below 3, where fp32 still resolves
    1 + 1e-6 - tanh(u)^2), log stds spread over both sides of the clamp - and centre the twin target critics' means on each other."""
    nets, A = alg.networks, data["act"].shape[1]
    with torch.no_grad():
        for pol, o in ((nets.policy, data["obs"]), (nets.policy_target, data["obs2"])):
            head, y = last_linear(pol.policy), pol.policy(o)
            scale = torch.cat([0.9 / y[:, :A].abs().max(dim=0).values, 1.6 / y[:, A:].std(dim=0)])
            head.weight.mul_(scale[:, None])
            head.bias.mul_(scale)
            shift = pol.policy(o)[:, A:].median(dim=0).values - 0.5 * (MIN_LOG_STD + MAX_LOG_STD)
            head.bias[A:].sub_(shift)
        a2 = TanhGaussDistribution(nets.policy_target(data["obs2"])).mode()
        last_linear(nets.q2_target.q).bias[0].add_((nets.q1_target(data["obs2"], a2)[:, 0] - nets.q2_target(data["obs2"], a2)[:, 0]).median())
        a1 = TanhGaussDistribution(nets.policy(data["obs"])).mode()   # and the online pair at the policy's action: both carry the actor gradient
        last_linear(nets.q2.q).bias[0].add_((nets.q1(data["obs"], a1)[:, 0] - nets.q2(data["obs"], a1)[:, 0]).median())


def recompute(alg, data, dr, mean_std_before):
    """The update's intermediate values from the recorded draws with the reference's own networks (fp32, as the reference computes)."""
    nets = alg.networks
    alpha = float(nets.log_alpha.exp()) if alg.auto_alpha else alg.alpha
    rsample = lambda logits, eps: tanh_gauss_rsample(nets.policy, logits, eps)   # noqa: E731
    with torch.no_grad():
        a2, logp2, u2 = rsample(nets.policy_target(data["obs2"]), dr["eps_next"])
        qt = torch.stack([nets.q1_target(data["obs2"], a2), nets.q2_target(data["obs2"], a2)])   # [2, B, 2]
        z = torch.clamp(dr["z_next"], -3, 3)
        q_next = torch.min(qt[0, :, 0], qt[1, :, 0])
        q_sample = torch.where(qt[0, :, 0] < qt[1, :, 0], qt[0, :, 0] + z[0] * qt[0, :, 1], qt[1, :, 0] + z[1] * qt[1, :, 1])
        live = (1 - data["done"]) * alg.gamma
        tq = data["rew"] + live * (q_next - alpha * logp2)
        tqs = data["rew"] + live * (q_sample - alpha * logp2)
        qs = [nets.q1(data["obs"], data["act"]), nets.q2(data["obs"], data["act"])]
        losses, mean_std, binds = [], [], []
        for i, q in enumerate(qs):
            m, s = q[:, 0], q[:, 1]
            ms = s.mean() if mean_std_before is None else (1 - alg.tau_b) * mean_std_before[i] + alg.tau_b * s.mean()
            diff = tqs - m
            bound = m + torch.clamp(diff, -3 * ms, 3 * ms)
            losses.append((ms ** 2 + 0.1) * torch.mean(-(tq - m) / (s ** 2 + 0.1) * m - ((m - bound) ** 2 - s ** 2) / (s ** 3 + 0.1) * s))
            mean_std.append(ms)
            binds.append(diff.abs() > 3 * ms)
        new_act, new_logp, u1 = rsample(nets.policy(data["obs"]), dr["eps_new"])
        qn = [nets.q1(data["obs"], new_act)[:, 0], nets.q2(data["obs"], new_act)[:, 0]]
        loss_pi = (alpha * new_logp - torch.min(qn[0], qn[1])).mean()
    return dict(target_q=tq, target_q_sample=tqs, a2=a2, logp_next=logp2, q_targ=qt, new_act=new_act, new_logp=new_logp, losses=losses,
                mean_std=torch.stack(mean_std), loss_pi=loss_pi, binds=torch.stack(binds), u=torch.cat([u1.reshape(-1), u2.reshape(-1)]),
                qn=torch.stack(qn))


def assert_cases(name, alg, data, rc):
    """Every branch of the update has rows on both sides in the batch (otherwise the fixtures leave it untested)."""
    nets, A = alg.networks, data["act"].shape[1]
    checks = {"done rows": bool((data["done"] == 1).any()) and bool((data["done"] == 0).any()),
              "q1_target < q2_target": bool((rc["q_targ"][0, :, 0] < rc["q_targ"][1, :, 0]).any()),
              "q2_target < q1_target": bool((rc["q_targ"][1, :, 0] < rc["q_targ"][0, :, 0]).any()),
              "q1 < q2 at the new action": bool((rc["qn"][0] < rc["qn"][1]).any()), "q2 < q1 at the new action": bool((rc["qn"][1] < rc["qn"][0]).any()),
              "3 mean_std clamp binds": bool(rc["binds"][0].any()) and bool(rc["binds"][1].any()),
              "3 mean_std clamp idle": bool((~rc["binds"][0]).any()) and bool((~rc["binds"][1]).any()),
              "max |u| <= 3": float(rc["u"].abs().max()) <= 3.0}
    for tag, pol, o in (("policy", nets.policy, data["obs"]), ("policy_target", nets.policy_target, data["obs2"])):
        ls = pol.policy(o)[:, A:].detach()
        checks[f"{tag}: log std below the clamp"] = bool((ls < MIN_LOG_STD).any())
        checks[f"{tag}: log std inside the clamp"] = bool(((ls > MIN_LOG_STD) & (ls < MAX_LOG_STD)).any())
        checks[f"{tag}: log std above the clamp"] = bool((ls > MAX_LOG_STD).any())
    for n in ("q1", "q2", "policy"):
        checks[f"{n}_target moved"] = any(not torch.equal(p, t) for p, t in zip(getattr(nets, n).parameters(), getattr(nets, f"{n}_target").parameters()))
    missing = [k for k, ok in checks.items() if not ok]
    assert not missing, (name, missing)


def distribution_values(seed):
    """Inputs and outputs of the reference's two continuous distributions, for tests of their restatement."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for tag, cls in (("gauss", GaussDistribution), ("tanh_gauss", TanhGaussDistribution)):
        logits = torch.cat([torch.randn(9, 2, generator=g), 0.1 + torch.rand(9, 2, generator=g)], dim=-1)
        dist = cls(logits)
        dist.act_high_lim, dist.act_low_lim = torch.tensor(LIM_B[1]), torch.tensor(LIM_B[0])
        with DrawTap() as tap:
            act, logp = dist.rsample()
        inner = torch.rand(9, 2, generator=g) * 0.8 + 0.1
        at = dist.act_low_lim + inner * (dist.act_high_lim - dist.act_low_lim)
        out.update({f"dist/{tag}/logits": logits.numpy(), f"dist/{tag}/eps": tap.rsamples[0].numpy(), f"dist/{tag}/act": act.numpy(),
                    f"dist/{tag}/logp": logp.numpy(), f"dist/{tag}/at": at.numpy(), f"dist/{tag}/log_prob": dist.log_prob(at).numpy(),
                    f"dist/{tag}/mode": dist.mode().numpy(), f"dist/{tag}/entropy": dist.entropy().numpy()})
    return out


def one_update(name):
    cfg, lim, ctor = CASES[name]
    seed = zlib.crc32(name.encode()) % 1000
    alg, g = build(cfg, lim, ctor, seed)
    data = batch_of(cfg, seed, g)
    balance(alg, data)
    out = {**arrays(data, "in/"), **meta_entry(cfg=dict(cfg, alg="DSACT"), lim=lim, ctor=ctor, seed=seed, min_log_std=MIN_LOG_STD,
                                               max_log_std=MAX_LOG_STD), **state(alg)}
    before = copy.deepcopy(alg.networks)
    with DrawTap() as tap:
        tb, info = alg.get_remote_update_info(dict(data), 0)
    dr = draws_of(tap)
    out.update(arrays(dr, "in/"))
    after, alg.networks = alg.networks, before
    rc = recompute(alg, data, dr, None)
    alg.networks = after
    assert close(sum(rc["losses"]), tb["Loss/Critic loss-RL iter"]) and close(rc["loss_pi"], tb["Loss/Actor loss-RL iter"]), name
    assert close(rc["mean_std"][0], alg.mean_std1) and close(rc["mean_std"][1], alg.mean_std2), name
    assert_cases(name, alg, data, rc)
    for k in ("target_q", "target_q_sample", "a2", "logp_next", "q_targ", "new_act", "new_logp", "mean_std"):
        out[k] = rc[k].numpy().copy()
    out.update(update_entries(info, tb, log_alpha=alg.auto_alpha))
    if name == "dsact_lqs4a2_gelu":
        out.update(distribution_values(seed))
    mg.save(name, **out)


def five_updates():
    """Every parameter, log_alpha and mean_std after each of five consecutive `local_update` calls with delay_update = 2 (policy,
    temperature and targets step at iterations 0, 2, 4 only); learning rates raised so that every step is well above fp32 rounding."""
    name = "dsact_pend_5updates"
    cfg, lim = SHAPE_A, LIM_A
    ctor = dict(gamma=0.97, tau=0.05, auto_alpha=True, delay_update=2)
    seed = zlib.crc32(name.encode()) % 1000
    alg, g = build(cfg, lim, ctor, seed)
    out = meta_entry(cfg=dict(cfg, alg="DSACT"), lim=lim, ctor=ctor, seed=seed, lr=1e-2, min_log_std=MIN_LOG_STD, max_log_std=MAX_LOG_STD)
    batches, sd0 = five_batches(alg, cfg, seed, g, lambda data: balance(alg, data))
    out.update(sd0)
    for k, data in enumerate(batches):
        out.update(arrays(data, f"in{k}/"))
        with DrawTap() as tap:
            tb = alg.local_update(dict(data), k)
        out.update(arrays(draws_of(tap), f"in{k}/"))
        out[f"loss_q{k}"] = np.float64(tb["Loss/Critic loss-RL iter"])
        out[f"loss_pi{k}"] = np.float64(tb["Loss/Actor loss-RL iter"])
        out[f"mean_std{k + 1}"] = np.array([float(alg.mean_std1), float(alg.mean_std2)], dtype=np.float32)
        out.update(state(alg, f"sd{k + 1}/"))
        assert float(max(abs(tb["DSAC2/policy_mean-RL iter"]), 0)) <= 1.0
    mg.save(name, **out)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name in CASES:
        if not only or name in only:
            one_update(name)
    if not only or "five_updates" in only:
        five_updates()
