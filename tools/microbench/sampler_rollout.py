"""Time one `OnPolicyDeviceSampler.sample()` on the GPU two ways: `fused=True` (one `gops_sample_rollout` launch for all steps, then
the two value forwards and `gops_gae`) and the per-step loop (`fused=False`) on the same commit, in the same run.

    python tools/microbench/sampler_rollout.py       # prints one JSON line per shape

Shapes: the pendulum PPO example (64-64 ReLU policy and value, `env_step="model"`, sample_batch_size 512 as 8 environments x 64
steps, max_episode_steps 200) and N = 4096, T = 16 on pyth_lq (s4a2, data env).  Each variant: 3 warm-up calls, then 15 timed
calls, each bracketed by a device synchronise; median and min .. max in ms.
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

from gops_amd.apprfunc.mlp import StateValue, StochaPolicy  # noqa: E402
from gops_amd.create_pkg.create_env_model import create_env_model  # noqa: E402
from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler  # noqa: E402
from gops_amd.utils.act_distribution import GaussDistribution  # noqa: E402
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of  # noqa: E402

WARMUP, TIMED = 3, 15
SHAPES = [(dict(env_id="gym_pendulum"), "model", 8, 64, 2.0), (dict(env_id="pyth_lq", lq_config="s4a2"), "data", 4096, 16, 1.0)]


class Nets(torch.nn.Module):
    def __init__(self, O, A, lim):
        super().__init__()
        torch.manual_seed(0)
        self.policy = StochaPolicy(obs_dim=O, act_dim=A, hidden_sizes=[64, 64], hidden_activation="relu", min_log_std=-20, max_log_std=1,
                                   act_high_lim=np.full(A, lim, np.float32), act_low_lim=np.full(A, -lim, np.float32),
                                   action_distribution_cls=GaussDistribution)
        self.value = StateValue(obs_dim=O, hidden_sizes=[64, 64], hidden_activation="relu", output_activation="linear",
                                action_distribution_cls=None)


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
    for cfg, step, N, T, lim in SHAPES:
        row = dict(env_id=cfg["env_id"], env_step=step, n_envs=N, steps=T, hidden=[64, 64])
        for fused in (True, False):
            smp = OnPolicyDeviceSampler(cfg, create_env_model(**cfg), n_envs=N, steps_per_sample=T, max_episode_steps=200, seed=0,
                                        env_step=step, fused=fused)
            smp.networks = Nets(obs_dim_of(cfg), act_dim_of(cfg), lim).cuda()
            row["fused" if fused else "loop"] = timed(smp.sample)
            row["path_fused" if fused else "path_loop"] = smp.path
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
