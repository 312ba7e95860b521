"""Time one TRPO `local_update` on the GPU three ways: HIP graph replay (the CG loop and the value step), eager HIP launches, and the
same update as plain torch autograd with the reference's double-backward Hessian-vector product and torch.optim.Adam (the tests'
`restate_trpo_update` arithmetic at fp32 on the device).

    python tools/microbench/trpo_update.py            # prints one JSON line per shape
    python tools/microbench/trpo_update.py --discrete # the discrete example's shape, and the continuous case beside it

Shapes: the pendulum example's 400 rows and 4096 rows, 64-64 ReLU nets, max_cg = 10, train_v_iters = 40.  Each variant: 5 warm-up
updates (they include the graph captures), then 15 timed updates, each bracketed by a device synchronise; median and min .. max in ms.
The data is the same in every update; the policy moves, so the line search's length may differ between updates (reported).

`--discrete`: the shape of example_train/trpo/trpo_mlp_cartpole_onserial.py - obs 4, 2 actions (a categorical StochaPolicyDis), 64-64
ReLU nets, 512 rows (its sample_batch_size) - graph replay and eager launches, and in the same run the continuous case of the same
hidden shape and row count (the launch sequences are the same; only the seed and surrogate kernels differ).
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

WARMUP, TIMED = 5, 15


def make_alg():
    torch.manual_seed(0)
    alg = create_alg(algorithm="TRPO", trainer="on_serial_trainer", seed=0, cnn_shared=False, env_id="gym_pendulum", obsv_dim=3, action_dim=1,
                     action_type="continu", action_low_limit=np.array([-2.0], dtype=np.float32), action_high_limit=np.array([2.0], dtype=np.float32),
                     policy_func_type="MLP", policy_func_name="StochaPolicy", policy_act_distribution="default", policy_hidden_sizes=[64, 64],
                     policy_hidden_activation="relu", policy_min_log_std=-20, policy_max_log_std=1, value_func_type="MLP",
                     value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation="relu", delta=0.01, rtol=1e-5,
                     atol=1e-8, damping_factor=0.1, max_cg=10, alpha=0.8, max_search=10, train_v_iters=40, value_learning_rate=1e-3)
    alg.networks.cuda()
    return alg


def make_discrete_alg():
    torch.manual_seed(0)
    alg = create_alg(algorithm="TRPO", trainer="on_serial_trainer", seed=0, cnn_shared=False, env_id="gym_cartpole", obsv_dim=4,
                     action_type="discret", action_num=2, policy_func_type="MLP", policy_func_name="StochaPolicyDis",
                     policy_act_distribution="default", policy_hidden_sizes=[64, 64], policy_hidden_activation="relu",
                     policy_std_type="parameter", value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=[64, 64],
                     value_hidden_activation="relu", delta=0.01, rtol=1e-5, atol=1e-8, damping_factor=0.1, max_cg=10, alpha=0.8,
                     max_search=10, train_v_iters=40, value_learning_rate=1e-3)
    alg.networks.cuda()
    return alg


def make_data(alg, B):
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(B, alg.networks.policy.linear_layers()[0].in_features, generator=g).cuda()
    with torch.no_grad():
        act, _ = alg.networks.create_action_distributions(alg.networks.policy(obs)).sample()
    act = act.float().reshape(B, -1)   # (a categorical sample is an int64 index column)
    return dict(obs=obs, act=act, adv=torch.randn(B, generator=g).cuda(), ret=torch.randn(B, generator=g).cuda())


def torch_update(alg, opt, data):
    """trpo.py:118-217 with torch ops and autograd on the device (the policy is updated in place)."""
    import trpo_helpers as th
    nets = alg.networks
    seq, lo, hi = nets.policy.policy, nets.policy.min_log_std, nets.policy.max_log_std
    params = list(seq.parameters())
    obs, act, adv, ret = data["obs"], data["act"], data["adv"], data["ret"]
    adv = (adv - adv.mean()) / (adv.std() + th.EPS)
    head_old = seq(obs).detach()
    logp_old = th.log_prob(head_old, act, lo, hi)

    def surrogate(head):
        return torch.mean(torch.exp(th.log_prob(head, act, lo, hi) - logp_old) * adv)

    g = th.flat(torch.autograd.grad(surrogate(seq(obs)), params)).detach()
    x, _, _ = th.solve_cg(lambda v: th.flat(th.hessian_product(seq, obs, th.unflat(v, params), lo, hi)).detach() + alg.damping_factor * v,
                          g, alg.atol, alg.max_cg)
    step = torch.sqrt(2 * alg.delta / (torch.dot(g, x) + th.EPS)) * x
    theta_old = th.flat(params).detach().clone()
    with torch.no_grad():
        for i in range(alg.max_search):
            for p, v in zip(params, th.unflat(theta_old + alg.alpha ** i * step, params)):
                p.copy_(v)
            head = seq(obs)
            if surrogate(head) > 0 and th.kl_new_old(head, head_old, lo, hi) < alg.delta:
                break
        else:
            for p, v in zip(params, th.unflat(theta_old, params)):
                p.copy_(v)
    for _ in range(alg.train_v_iters):
        opt.zero_grad()
        torch.nn.functional.mse_loss(nets.value(obs), ret).backward()
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


def hip_rows(make, B, row):
    """`row` with the graph-replay and eager timings of `local_update` on the algorithm `make()` builds, B rows."""
    for mode in ("1", "0"):
        os.environ["GOPS_HIP_GRAPH"] = mode
        alg = make()
        data = make_data(alg, B)
        searches = []

        def update():
            alg.local_update(dict(data), 0)
            searches.append(alg.last_search_index)

        row["graph" if mode == "1" else "eager"] = timed(update)
        row["search_indices_" + ("graph" if mode == "1" else "eager")] = sorted(set(-1 if s is None else s for s in searches[WARMUP:]))
        if mode == "1":
            row["cg_graph_replays"], row["value_graph_replays"] = alg.cg_graph_replays, alg.value_graph_replays
    return row


def main():
    if "--discrete" in sys.argv[1:]:
        for policy, make in (("StochaPolicyDis obs 4, 2 actions", make_discrete_alg), ("StochaPolicy obs 3, 1 action", make_alg)):
            print(json.dumps(hip_rows(make, 512, dict(policy=policy, rows=512, hidden=[64, 64], max_cg=10, train_v_iters=40))), flush=True)
        return
    for B in (400, 4096):
        row = hip_rows(make_alg, B, dict(rows=B, hidden=[64, 64], max_cg=10, train_v_iters=40))
        alg = make_alg()
        data = make_data(alg, B)
        opt = torch.optim.Adam(alg.networks.value.parameters(), lr=1e-3)
        row["torch_autograd"] = timed(lambda: torch_update(alg, opt, data))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
