"""Generate the PPO fixtures (`ppo_*.npz`) and the GAE fixture (`gae_segments.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_ppo.py
Every array written here is an input, or an output of the reference's own classes: `gops.algorithm.ppo.PPO` (its `__compute_loss`
for the one-minibatch fixtures, its `local_update` for `ppo_pend_local_update`) and `gops.trainer.sampler.on_sampler.OnSampler`
(`_finish_trajs`, on an instance made with `object.__new__` whose arrays are set by hand: no environment is needed).

The inputs are shaped so that every branch of the loss has rows: `logp_old` puts the ratios below, inside and above the clip range
with advantages of both signs; `val_old` puts |v_new - val_old| on both sides of `value_clip`, which is of the order of the value
spread; the log-std clamp is [-3, -0.5] with raw log stds on both sides.
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)
from _make_ac_common import LIM_A, LIM_B, MAX_LOG_STD, MIN_LOG_STD, SHAPE_A, SHAPE_B, arrays, build_reference, last_linear, meta_entry, state  # noqa: E402

from gops.algorithm.ppo import PPO  # noqa: E402
from gops.utils.tensorboard_setup import tb_tags  # noqa: E402

from gops_amd.utils.synthetic import act_dim_of, make_batch  # noqa: E402

# name: (cfg, action limits, attributes set on the object)
CASES = {
    "ppo_pend_relu": (SHAPE_A, LIM_A, dict()),
    "ppo_lqs4a2_gelu": (SHAPE_B, LIM_B, dict()),
    "ppo_pend_value_norm": (SHAPE_A, LIM_A, dict(loss_value_clip=False, loss_value_norm=True)),
    "ppo_pend_entropy": (SHAPE_A, LIM_A, dict(loss_coefficient_entropy=0.01)),
}
TERMS = ("loss_total", "loss_surrogate", "loss_value", "loss_entropy", "approximate_kl", "clip_fraction")
MIN_ROWS, MARGIN = 4, 1e-3


def build(cfg, lim, seed, **ctor):
    ctor = dict(dict(max_iteration=10, num_repeat=1, num_mini_batch=1, mini_batch_size=cfg["batch"], sample_batch_size=cfg["batch"],
                     trainer="on_serial_trainer"), **ctor)
    alg, g = build_reference(PPO, cfg, lim, seed, policy_func_name="StochaPolicy", policy_act_distribution="default",
                             policy_min_log_std=MIN_LOG_STD, policy_max_log_std=MAX_LOG_STD, learning_rate=1e-3, **ctor)
    return alg, g, ctor


def shaped_batch(alg, cfg, seed, g):
    """obs, act, logp, adv, ret (the sampler's columns) and val, logits (what local_update adds) for the networks of `alg`, whose
    policy head and value_clip are shaped here too."""
    nets, B, A = alg.networks, cfg["batch"], act_dim_of(cfg)
    obs = make_batch(dict(cfg, alg="INFADP", horizon=1), seed)["obs"]
    with torch.no_grad():
        head, y = last_linear(nets.policy.policy), nets.policy.policy(obs)
        scale = torch.cat([0.9 / y[:, :A].abs().max(dim=0).values, 1.6 / y[:, A:].std(dim=0)])
        head.weight.mul_(scale[:, None])
        head.bias.mul_(scale)
        head.bias[A:].sub_(nets.policy.policy(obs)[:, A:].median(dim=0).values - 0.5 * (MIN_LOG_STD + MAX_LOG_STD))
        logits = nets.policy(obs)
        mean, std = torch.chunk(logits, 2, dim=-1)
        act = mean + std * torch.randn(B, A, generator=g)
        logp_new = nets.create_action_distributions(logits).log_prob(act)
        cell = torch.arange(B) % 6   # ratio below / inside / above the clip range x advantage sign
        lo, hi = torch.tensor([0.55, 0.85, 1.25])[cell % 3], torch.tensor([0.75, 1.15, 1.5])[cell % 3]
        logp = logp_new - torch.log(lo + (hi - lo) * torch.rand(B, generator=g))
        adv = torch.where(cell < 3, 1.0, -1.0) * (0.1 + torch.randn(B, generator=g).abs())
        v = nets.value(obs)
        alg.value_clip = max(round(float(v.std()), 3), 0.02)
        far = (torch.arange(B) // 6) % 2 == 1
        size = torch.where(far, 1.3 + 0.7 * torch.rand(B, generator=g), 0.2 + 0.6 * torch.rand(B, generator=g)) * alg.value_clip
        val = v + size * torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
        ret = v + 2 * alg.value_clip * torch.randn(B, generator=g)
        old = torch.cat((mean + 0.1 * std * torch.randn(B, A, generator=g), std * torch.exp(0.2 * torch.randn(B, A, generator=g))), dim=-1)
    return dict(obs=obs, act=act, logp=logp, adv=adv, ret=ret, val=val, logits=old)


def branches(alg, mb, value=True):
    """name -> rows (elements for the log std) of each branch at the current parameters, and the smallest distance of any row to a
    branch boundary."""
    nets, A = alg.networks, mb["act"].shape[1]
    with torch.no_grad():
        raw = nets.policy.policy(mb["obs"])[:, A:]
        ratio = torch.exp(nets.create_action_distributions(nets.policy(mb["obs"])).log_prob(mb["act"]) - mb["logp"])
        c, adv = alg.clip_now, mb["adv"]
        out = {}
        for zone, m in (("below", ratio < 1 - c), ("inside", (ratio > 1 - c) & (ratio < 1 + c)), ("above", ratio > 1 + c)):
            out[f"ratio {zone}, adv > 0"], out[f"ratio {zone}, adv < 0"] = int((m & (adv > 0)).sum()), int((m & (adv < 0)).sum())
        out.update({"log std below": int((raw < MIN_LOG_STD).sum()), "log std inside": int(((raw > MIN_LOG_STD) & (raw < MAX_LOG_STD)).sum()),
                    "log std above": int((raw > MAX_LOG_STD).sum())})
        gap = torch.cat([(ratio - (1 - c)).abs(), (ratio - (1 + c)).abs(), adv.abs(), (raw - MIN_LOG_STD).abs().reshape(-1),
                         (raw - MAX_LOG_STD).abs().reshape(-1)])
        if value and alg.loss_value_clip:
            v, r, vo = nets.value(mb["obs"]), mb["ret"], mb["val"]
            vc = vo + (v - vo).clamp(-alg.value_clip, alg.value_clip)
            l1, l2 = (v - r) ** 2, (vc - r) ** 2
            clipped = (v - vo).abs() > alg.value_clip
            out.update({"value clipped": int(clipped.sum()), "value not clipped": int((~clipped).sum()),
                        "l2 > l1": int((l2 > l1).sum()), "l2 <= l1": int((l2 <= l1).sum())})
            gap = torch.cat([gap, ((v - vo).abs() - alg.value_clip).abs(), (l2 - l1).abs()[clipped]])
    return out, float(gap.min())


def assert_branches(tag, alg, mb, value=True):
    got, gap = branches(alg, mb, value)
    missing = [k for k, n in got.items() if n < MIN_ROWS] + ([f"a row within {gap:.1e} of a boundary"] if gap < MARGIN else [])
    assert not missing, (tag, missing)


def grads(alg):
    out = {}
    for n in ("policy", "value"):
        for i, p in enumerate(getattr(alg.networks, n).parameters()):
            out[f"{n}_grad/{i}"] = p.grad.detach().numpy().copy()
    return out


def seeds_from(tag, fn):
    """The seed is the first one from the tag's checksum on at which the INPUTS populate every branch (assert_branches)."""
    base = zlib.crc32(tag.encode()) % 1000
    for seed in range(base, base + 16):
        try:
            return fn(tag, seed)
        except AssertionError as e:
            if not (len(e.args) == 1 and isinstance(e.args[0], tuple) and e.args[0][0] == tag and isinstance(e.args[0][1], list)):
                raise
            print(f"{tag}: seed {seed} leaves {e.args[0][1]}")
    raise AssertionError(tag)


def one_step_at(tag, seed):
    cfg, lim, attrs = CASES[tag]
    alg, g, ctor = build(cfg, lim, seed)
    for k, v in attrs.items():
        setattr(alg, k, v)
    mb = shaped_batch(alg, cfg, seed, g)
    assert_branches(tag, alg, mb)
    attrs = dict(attrs, value_clip=alg.value_clip)
    out = {**arrays(mb, "in/"), **state(alg), **meta_entry(cfg=dict(cfg, alg="PPO"), lim=lim, ctor=ctor, attrs=attrs, seed=seed,
                                                           min_log_std=MIN_LOG_STD, max_log_std=MAX_LOG_STD)}
    terms = alg._PPO__compute_loss(dict(mb), 0)
    alg.approximate_optimizer.zero_grad()
    terms[0].backward()
    out.update(grads(alg))
    alg.approximate_optimizer.step()
    out.update(state(alg, "sd_after/"))
    for k, v in zip(TERMS, terms):
        out["loss/" + k] = np.float64(v.detach())
    out.update({"tb/" + tb_tags["loss_actor"]: np.float64(terms[1].detach()), "tb/" + tb_tags["loss_critic"]: np.float64(terms[2].detach()),
                "tb/PPO/KL_divergence-RL iter": np.float64(terms[4].detach())})
    # the distributions' own values (utils/act_distribution.py is checked against them)
    with torch.no_grad():
        new = alg.networks.create_action_distributions(torch.from_numpy(out["in/logits"]))
        oldd = alg.networks.create_action_distributions(torch.flip(torch.from_numpy(out["in/logits"]), dims=[0]))
        out["dist/entropy"], out["dist/kl"] = new.entropy().numpy().copy(), oldd.kl_divergence(new).numpy().copy()
    mg.save(tag, **out)


def local_update_at(tag, seed):
    """One full local_update: 2 repeats x 2 minibatches of 35 rows, both linear schedules, iteration 3 of 10."""
    cfg, lim = SHAPE_A, LIM_A
    alg, g, ctor = build(cfg, lim, seed, num_repeat=2, num_mini_batch=2, mini_batch_size=35, sample_batch_size=70)
    mb = shaped_batch(alg, cfg, seed, g)
    with torch.no_grad():
        normed = dict(mb, adv=(mb["adv"] - mb["adv"].mean()) / (mb["adv"].std() + alg.EPS))   # (as the update normalises them)
    attrs = dict(schedule_adam="linear", schedule_clip="linear", learning_rate=1e-2, value_clip=alg.value_clip)
    for k, v in attrs.items():
        setattr(alg, k, v)
    for group in alg.approximate_optimizer.param_groups:
        group["lr"] = 1e-2
    assert_branches(tag, alg, normed, value=False)   # (val_old is the value net's own output at the start: no value branch to populate)
    data = {k: mb[k].clone() for k in ("obs", "act", "logp", "adv", "ret")}
    out = {**arrays(data, "in/"), **state(alg), **meta_entry(cfg=dict(cfg, alg="PPO"), lim=lim, ctor=ctor, attrs=attrs, seed=seed, lr=1e-2,
                                                             iteration=3, min_log_std=MIN_LOG_STD, max_log_std=MAX_LOG_STD)}
    perms, shuffle = [], np.random.shuffle

    def tapped(x):
        shuffle(x)
        perms.append(np.array(x, dtype=np.int64))

    np.random.seed(seed)
    np.random.shuffle = tapped
    try:
        tb = alg.local_update(data, 3)
    finally:
        np.random.shuffle = shuffle
    assert len(perms) == 2
    out["in/perm"] = np.stack(perms)
    out.update(grads(alg))
    out.update(state(alg, "sd_after/"))
    for k, v in tb.items():
        if not k.startswith("Time/"):
            out["tb/" + k] = np.float64(v)
    out["lr_after"], out["clip_now_after"] = np.float64(alg.approximate_optimizer.param_groups[0]["lr"]), np.float64(alg.clip_now)
    mg.save(tag, **out)


def gae_segments():
    """`_finish_trajs` of the reference's OnSampler on hand-set arrays, N = 5, T = 12: segments that end by done, by the time limit and
    by the horizon; environment 1 has three ends before the horizon, environment 4 none.

    Segments are handed over disjoint: each starts one step after the previous one's last.  (The reference's `_process_experiences`
    sets `last_ptr = ptr`, on_sampler.py:166, so that ITS next segment starts ON the previous segment's last step and overwrites that
    step's ret / adv with values that bootstrap across the episode boundary; `gops_gae` implements `_finish_trajs`' recurrence per
    segment and does not reproduce that overlap.)"""
    from gops.trainer.sampler.on_sampler import OnSampler
    N, T = 5, 12
    rng = np.random.RandomState(12)
    smp = object.__new__(OnSampler)
    smp.gamma, smp.gae_lambda = 0.97, 0.9
    smp.mb_rew = rng.randn(N, T).astype(np.float32)
    smp.mb_val = (2 * rng.randn(N, T)).astype(np.float32)
    smp.mb_ret, smp.mb_adv = np.zeros((N, T), dtype=np.float32), np.zeros((N, T), dtype=np.float32)
    val_next = (2 * rng.randn(N, T)).astype(np.float32)
    done, tlim = np.zeros((N, T), dtype=np.float32), np.zeros((N, T), dtype=np.float32)
    done[0, 4] = done[1, 2] = done[1, 9] = done[3, 11] = 1
    tlim[1, 6] = tlim[2, 7] = tlim[3, 0] = 1
    end = np.maximum(done, tlim)
    end[:, T - 1] = 1
    smp.ptr, smp.last_ptr = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for t in range(T):   # one call per segment, its last value estimate a Python float as on_sampler.py:161-165 forms it
        for i in range(N):
            if end[i, t]:
                smp.ptr[i] = t
                smp._finish_trajs(i, float(val_next[i, t]) * (1 - int(done[i, t])))
                smp.last_ptr[i] = t + 1   # disjoint segments (see the docstring)
    # time-major [T, N], as the device sampler lays its columns out
    mg.save("gae_segments", rew=smp.mb_rew.T.copy(), val=smp.mb_val.T.copy(), val_next=val_next.T.copy(), done=done.T.copy(), end=end.T.copy(),
            ret=smp.mb_ret.T.copy(), adv=smp.mb_adv.T.copy(), gamma=np.float64(smp.gamma), gae_lambda=np.float64(smp.gae_lambda))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for tag in CASES:
        if not only or tag in only:
            seeds_from(tag, one_step_at)
    if not only or "ppo_pend_local_update" in only:
        seeds_from("ppo_pend_local_update", local_update_at)
    if not only or "gae_segments" in only:
        gae_segments()
