"""Time one PPO `local_update` on the GPU three ways: HIP graph replay, eager HIP launches, and the same update as plain torch
autograd + torch.optim.Adam (the tests' `restate_ppo_loss` at fp32 on the device).

    python tools/microbench/ppo_update.py            # prints one JSON line per shape

Shapes: the pendulum example's (64-64 ReLU nets, sample_batch_size 512, num_repeat 10, num_mini_batch 8: 80 steps of 64 rows) and
minibatches of 4096 rows (sample_batch_size 32768, 10 x 8 steps).  Each variant: 3 warm-up updates (they include the graph capture),
then 15 timed updates, each bracketed by a device synchronise; median and min .. max in ms.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402

WARMUP, TIMED = 3, 15


def make_alg(S, M, repeat=10):
    torch.manual_seed(0)
    alg = create_alg(algorithm="PPO", trainer="on_serial_trainer", seed=0, cnn_shared=False, env_id="gym_pendulum", obsv_dim=3, action_dim=1,
                     action_type="continu", action_low_limit=np.array([-2.0], dtype=np.float32), action_high_limit=np.array([2.0], dtype=np.float32),
                     policy_func_type="MLP", policy_func_name="StochaPolicy", policy_act_distribution="default", policy_hidden_sizes=[64, 64],
                     policy_hidden_activation="relu", policy_min_log_std=-20, policy_max_log_std=1, value_func_type="MLP",
                     value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation="relu", learning_rate=3e-4,
                     max_iteration=1000, num_repeat=repeat, num_mini_batch=S // M, mini_batch_size=M, sample_batch_size=S)
    alg.networks.cuda()
    return alg


def make_data(alg, S):
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(S, 3, generator=g).cuda()
    with torch.no_grad():
        dist = alg.networks.create_action_distributions(alg.networks.policy(obs))
        act, logp = dist.sample()
    return dict(obs=obs, act=act, logp=logp, adv=torch.randn(S, generator=g).cuda(), ret=torch.randn(S, generator=g).cuda())


def torch_update(alg, opt, data, hyper):
    """ppo.py:121-155 with torch ops, autograd and torch's Adam on the device."""
    from ppo_helpers import restate_ppo_loss
    nets = alg.networks
    d = dict(data)
    d["adv"] = (d["adv"] - d["adv"].mean()) / (d["adv"].std() + alg.EPS)
    with torch.no_grad():
        d["val"], d["logits"] = nets.value(d["obs"]), nets.policy(d["obs"])
    M = alg.mini_batch_size
    for _ in range(alg.num_repeat):
        idx = torch.randperm(alg.sample_batch_size, device="cuda")
        for n in range(alg.num_mini_batch):
            mb = {k: v[idx[M * n:M * (n + 1)]] for k, v in d.items()}
            got = restate_ppo_loss(nets.policy.policy(mb["obs"]), nets.value(mb["obs"]), mb["act"], mb["logp"], mb["adv"], mb["ret"], mb["val"],
                                   mb["logits"], **hyper)
            opt.zero_grad()
            got["terms"][0].backward()
            opt.step()


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1000)
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    from ppo_helpers import hyper_of
    for S, M in ((512, 64), (32768, 4096)):
        row = dict(sample_batch_size=S, mini_batch_size=M, steps_per_update=10 * (S // M), hidden=[64, 64])
        for mode in ("1", "0"):
            os.environ["GOPS_HIP_GRAPH"] = mode
            alg = make_alg(S, M)
            data = make_data(alg, S)
            row["graph" if mode == "1" else "eager"] = timed(lambda: alg.local_update(dict(data), 0))
            if mode == "1":
                row["graph_replays"] = alg.graph_replays
        alg = make_alg(S, M)
        data = make_data(alg, S)
        opt = torch.optim.Adam(alg.networks.parameters(), lr=3e-4)
        hyper = hyper_of(alg)
        row["torch_autograd"] = timed(lambda: torch_update(alg, opt, data, hyper))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
