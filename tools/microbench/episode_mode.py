"""Time one evaluation of a stochastic policy on the GPU two ways: `Evaluator(stochastic_mode=True)` (one `gops_episode_rollout_mode`
launch for all episodes and steps) and the per-step loop (`step_loop`: torch policy, `mode()`, one `gops_env_step` per step) on the
same commit, in the same process, on the same initial conditions.

    python tools/microbench/episode_mode.py       # prints one JSON line per env

Shapes: E = 10 episodes (`num_eval_episode` of the SAC example scripts) at the data env's step limit (gym_cartpoleconti registers
none: the evaluator's 200; pyth_idpendulum 500), a 64-64 ReLU SAC policy (StochaPolicy, TanhGaussDistribution).  The last layer is
zeroed and the episodes start at the upright equilibrium, so that every episode runs to the limit and each path does the work the
shape names (`mean_length` says so).  Beside them the deterministic head (`gops_episode_rollout`, a 64-64 DetermPolicy with a zeroed
last layer) at the same shape: the stack is A wide instead of 2A, nothing else differs.
Each figure ends in `ret.mean().item()`, the one read an evaluation pays.  3 warm-up calls per path, then 7 blocks per path,
alternating path by path, every block bracketed by a device synchronise; median of the blocks' ms per evaluation and min .. max over
the blocks.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

from gops_amd.apprfunc.mlp import DetermPolicy, StochaPolicy  # noqa: E402
from gops_amd.create_pkg.create_env_model import create_env_model  # noqa: E402
from gops_amd.trainer.evaluator import Evaluator  # noqa: E402
from gops_amd.utils.act_distribution import DiracDistribution, TanhGaussDistribution  # noqa: E402
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of  # noqa: E402

EPISODES, WARMUP, BLOCKS = 10, 3, 7
CALLS = {"fused": 20, "loop": 3, "determ_fused": 20}   # calls per block: the loop costs hundreds of launches per call
ENVS = [dict(env_id="gym_cartpoleconti"), dict(env_id="pyth_idpendulum")]


class Nets(torch.nn.Module):
    def __init__(self, cfg, stochastic):
        super().__init__()
        torch.manual_seed(0)
        O, A = obs_dim_of(cfg), act_dim_of(cfg)
        kw = dict(obs_dim=O, act_dim=A, hidden_sizes=[64, 64], hidden_activation="relu", act_high_lim=np.ones(A, np.float32),
                  act_low_lim=-np.ones(A, np.float32))
        if stochastic:
            self.policy = StochaPolicy(min_log_std=-20, max_log_std=0.5, action_distribution_cls=TanhGaussDistribution, **kw)
        else:
            self.policy = DetermPolicy(action_distribution_cls=DiracDistribution, **kw)
        last = self.policy.linear_layers()[-1]
        with torch.no_grad():
            last.weight.zero_(), last.bias.zero_()


def evaluator(cfg, stochastic, **extra):
    return Evaluator(env_model=create_env_model(**cfg), networks=Nets(cfg, stochastic).cuda(), cfg=cfg, num_eval_episode=EPISODES,
                     eval_save=False, **extra)


def block(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000 / calls


def main():
    for cfg in ENVS:
        ev = evaluator(cfg, True, stochastic_mode=True)
        det = evaluator(cfg, False)
        init = {"obs": torch.zeros(EPISODES, obs_dim_of(cfg), device="cuda")}   # the upright equilibrium, action 0: no termination
        paths = {"fused": lambda: ev.run_episodes(init)["ret"].mean().item(), "loop": lambda: ev.step_loop(init)["ret"].mean().item(),
                 "determ_fused": lambda: det.run_episodes(init)["ret"].mean().item()}
        row = dict(env_id=cfg["env_id"], episodes=EPISODES, max_steps=ev.max_episode_steps, hidden=[64, 64])
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
        row["path_fused"], row["path_determ"] = ev.path, det.path
        assert ev.path == "fused" and det.path == "fused", (ev.path, det.path)   # a refused kernel is not what this file times
        row["mean_length"] = {"fused": float(ev.run_episodes(init)["length"].float().mean()),
                              "loop": float(ev.step_loop(init)["length"].float().mean())}
        ms = {k: [] for k in paths}
        for _ in range(BLOCKS):
            for k, fn in paths.items():
                ms[k].append(block(fn, CALLS[k]))
        for k, v in ms.items():
            row[k] = dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
        row["loop_over_fused"] = round(row["loop"]["median_ms"] / row["fused"]["median_ms"], 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
