"""Generate the DDPG / TD3 fixtures (`ddpg_*.npz`, `td3_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_td3.py
Every array written here is an input, or an output of the reference's own classes (`gops.algorithm.ddpg.DDPG`,
`gops.algorithm.td3.TD3`) built with the helpers of make_golden.py.  TD3 draws its target-policy noise with `torch.randn_like`
inside the update (td3.py:170): the call is wrapped in this process, and the fixture stores the unit-normal draws `xi` it returned.
`backup`, `a2`, `q_targ` and the per-critic losses are not returned by the reference's update: they are evaluated here with the
reference's own target networks on the recorded draws, and the recorded critic loss is checked against them.
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
import _make_ac_common as common  # noqa: E402
from _make_ac_common import LIM_A, LIM_B, SHAPE_A, SHAPE_B, DrawTap, arrays, last_linear, meta_entry, state  # noqa: E402

from gops.algorithm.ddpg import DDPG  # noqa: E402
from gops.algorithm.td3 import TD3  # noqa: E402

# name: (cfg, action limits (low, high), attributes set after construction, PER)
CASES = {
    "td3_pend_relu": (dict(SHAPE_A, alg="TD3"), LIM_A, dict(target_noise=0.4, noise_clip=0.5, reward_scale=0.5), False),
    "td3_lqs4a2_gelu": (dict(SHAPE_B, alg="TD3"), LIM_B, dict(target_noise=0.3, noise_clip=0.4, gamma=0.97), False),
    "td3_per_pend_relu": (dict(SHAPE_A, alg="TD3"), LIM_A, dict(target_noise=0.4, noise_clip=0.5), True),
    "ddpg_pend_relu": (dict(SHAPE_A, alg="DDPG"), LIM_A, dict(gamma=0.95), False),
    "ddpg_lqs4a2_gelu": (dict(SHAPE_B, alg="DDPG"), LIM_B, dict(), False),
    "ddpg_per_lqs4a2_gelu": (dict(SHAPE_B, alg="DDPG"), LIM_B, dict(), True),
}


def build(cfg, lim, attrs, per, seed):
    ctor = {k: attrs[k] for k in ("target_noise", "noise_clip") if k in attrs}
    alg, g = common.build_reference(TD3 if cfg["alg"] == "TD3" else DDPG, cfg, lim, seed, value_func_name="ActionValue",
                                    buffer_name="prioritized_replay_buffer" if per else "replay_buffer", **ctor)
    for k, v in attrs.items():
        if k not in ctor:
            setattr(alg, k, v)
    with torch.no_grad():   # a steep target head saturates the squash on some rows
        last_linear(alg.networks.policy_target.pi).weight.mul_(12.0)
    return alg, ["q1", "q2"] if cfg["alg"] == "TD3" else ["q"], g


def batch_of(cfg, seed, g, per):
    B = cfg["batch"]
    data = common.batch_of(cfg, seed, g)
    if per:
        data["idx"] = torch.randperm(4 * B, generator=g)[:B].to(torch.int32) + (4 * B - 1)
        data["weight"] = 0.2 + 0.8 * torch.rand(B, generator=g)
    return data


def balance(alg, q_names, data, spread=None):
    """Centre the target policy's head and the twin target critics on this batch: rows on both sides of the squash, and of the minimum.
    `spread`: the standard deviation the head's outputs are scaled to first (several batches have to saturate on both sides)."""
    nets, o2 = alg.networks, data["obs2"]
    last = last_linear
    with torch.no_grad():
        if spread is not None:
            scale = spread / nets.policy_target.pi(o2).std(dim=0)
            last(nets.policy_target.pi).weight.mul_(scale[:, None])
            last(nets.policy_target.pi).bias.mul_(scale)
        last(nets.policy_target.pi).bias.sub_(nets.policy_target.pi(o2).median(dim=0).values)
        if len(q_names) == 2:
            a2 = nets.policy_target(o2)
            last(nets.q2_target.q).bias.add_((nets.q1_target(o2, a2) - nets.q2_target(o2, a2)).median())


def backup_of(alg, q_names, data, xi):
    """backup / a2 / q_targ of td3.py:166-183 (ddpg.py:149-151) from the reference's target networks and the recorded draws."""
    nets = alg.networks
    with torch.no_grad():
        a2 = nets.policy_target(data["obs2"])
        if xi is not None:
            eps = torch.clamp(xi * alg.target_noise, -alg.noise_clip, alg.noise_clip)
            a2 = torch.clamp(a2 + eps, torch.tensor(alg.act_low_limit), torch.tensor(alg.act_high_limit))
        q_t = torch.stack([getattr(nets, f"{q}_target")(data["obs2"], a2) for q in q_names])
        r = data["rew"] * getattr(alg, "reward_scale", 1)
        backup = r + alg.gamma * (1 - data["done"]) * q_t.min(dim=0).values
        losses = []
        for q in q_names:
            d2 = (getattr(nets, q)(data["obs"], data["act"]) - backup) ** 2
            losses.append((data["weight"] * d2).mean() if "weight" in data else d2.mean())
    return backup, a2, q_t, losses


def assert_td3_cases(name, alg, data, xi, a2, q_t):
    """Every clamp of the TD3 backup has rows on both sides in the batch (otherwise the fixtures leave it untested)."""
    lo, hi = torch.tensor(alg.act_low_limit), torch.tensor(alg.act_high_limit)
    raw = xi * alg.target_noise
    pre = alg.networks.policy_target(data["obs2"]).detach() + torch.clamp(raw, -alg.noise_clip, alg.noise_clip)
    checks = {"done rows": bool((data["done"] == 1).any()) and bool((data["done"] == 0).any()),
              "noise clipped at +c": bool((raw > alg.noise_clip).any()), "noise clipped at -c": bool((raw < -alg.noise_clip).any()),
              "noise not clipped": bool((raw.abs() < alg.noise_clip).any()),
              "action clipped at the upper limit": bool((pre > hi).any()), "action clipped at the lower limit": bool((pre < lo).any()),
              "action not clipped": bool(((pre > lo) & (pre < hi)).any()),
              "q1_target < q2_target": bool((q_t[0] < q_t[1]).any()), "q2_target < q1_target": bool((q_t[1] < q_t[0]).any())}
    missing = [k for k, ok in checks.items() if not ok]
    assert not missing, (name, missing)


def one_update(name):
    cfg, lim, attrs, per = CASES[name]
    seed = zlib.crc32(name.encode()) % 1000
    alg, q_names, g = build(cfg, lim, attrs, per, seed)
    data = batch_of(cfg, seed, g, per)
    balance(alg, q_names, data)
    out = {**arrays(data, "in/"), **meta_entry(cfg=cfg, lim=lim, attrs=attrs, per=per, seed=seed), **state(alg)}
    with DrawTap() as tap:
        extra, info = alg.get_remote_update_info(data, 0)
    tb = extra[0] if per else extra
    xi = None
    if cfg["alg"] == "TD3":
        assert len(tap.noise) == 1
        xi = tap.noise[0]
        out["in/target_noise"] = xi.numpy().copy()
    else:
        assert not tap.noise
    backup, a2, q_t, losses = backup_of(alg, q_names, data, xi)
    assert abs(float(sum(losses)) - tb["Loss/Critic loss-RL iter"]) <= 1e-6 * max(1.0, abs(tb["Loss/Critic loss-RL iter"])), name
    if cfg["alg"] == "TD3":
        assert_td3_cases(name, alg, data, xi, a2, q_t)
    out.update(backup=backup.numpy(), a2=a2.numpy(), q_targ=q_t.numpy())
    for q, l in zip(q_names, losses):
        out[f"loss_{q}"] = np.float64(l)
    out.update(common.update_entries(info, tb, log_alpha=False))
    if per:
        assert torch.equal(extra[1], data["idx"])
        out["abs_err"] = extra[2].detach().numpy().copy()
    mg.save(name, **out)


def five_updates():
    """All online and target parameters after each of five consecutive TD3 `local_update` calls with delay_update = 2 (the policy
    steps at iterations 0, 2, 4 only); learning rates raised so that every step is well above fp32 rounding."""
    name = "td3_pend_5updates"
    cfg, lim = dict(SHAPE_A, alg="TD3"), LIM_A
    attrs = dict(target_noise=0.4, noise_clip=0.5, delay_update=2, tau=0.05)
    seed = zlib.crc32(name.encode()) % 1000
    alg, q_names, g = build(cfg, lim, attrs, False, seed)
    out = meta_entry(cfg=cfg, lim=lim, attrs=attrs, per=False, seed=seed, lr=1e-2)
    batches, sd0 = common.five_batches(alg, cfg, seed, g, lambda data: balance(alg, q_names, data, spread=3.0))
    out.update(sd0)
    for k, data in enumerate(batches):
        out.update(arrays(data, f"in{k}/"))
        before = copy.deepcopy(alg.networks)   # the targets this update's backup is formed with
        with DrawTap() as tap:
            tb = alg.local_update(data, k)
        assert len(tap.noise) == 1
        out[f"in{k}/target_noise"] = tap.noise[0].numpy().copy()
        after, alg.networks = alg.networks, before
        _, a2, q_t, _ = backup_of(alg, q_names, data, tap.noise[0])
        assert_td3_cases(f"{name}[{k}]", alg, data, tap.noise[0], a2, q_t)
        alg.networks = after
        out[f"loss_q{k}"] = np.float64(tb["Loss/Critic loss-RL iter"])
        out[f"loss_pi{k}"] = np.float64(tb["Loss/Actor loss-RL iter"])
        out.update(state(alg, f"sd{k + 1}/"))
    mg.save(name, **out)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name in CASES:
        if not only or name in only:
            one_update(name)
    if not only or "five_updates" in only:
        five_updates()
