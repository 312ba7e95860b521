"""Time one `sample()` of the device samplers with an ACTION TABLE on the GPU two ways: `fused=True` (one `gops_sample_rollout_dis`
launch for all steps) and the per-step loop (`fused=False`: policy, argmax / multinomial, rand, randint, where, the table gather
and `gops_env_step` per step, plus one host read per step) on the same commit, in the same run.

    python tools/microbench/sampler_rollout_dis.py       # prints one JSON line per shape

Shapes:
  dqn       DeviceEnvSampler, gym_cartpoleconti (data env) with the table [[-1], [1]], N = 256, T = 16, a 64-64 ReLU ActionValueDis,
            epsilon 0.1 (EPS_GREEDY);
  trpo_dis  OnPolicyDeviceSampler as tests/test_trpo_dis_gpu.py's trainer test builds it: gym_cartpoleconti, env_step="model",
            the same table, N = 8, T = 16, max_episode_steps 50, a 64-64 ReLU StochaPolicyDis and StateValue (CATEGORICAL; the
            sample() includes the two value forwards and `gops_gae`).  The sample kernel steps cartpole as a DATA env only, so this
            shape reports the loop on both sides ("path_fused" says why);
  trpo_dis_data  the same sampler with env_step="data", which the kernel takes.
The two variants alternate block by block: 3 warm-up calls each, then BLOCKS = 7 blocks of CALLS = 20 calls per variant, every
block bracketed by a device synchronise; per variant the median of the blocks' ms per call and min .. max over the blocks.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

from gops_amd.apprfunc.mlp import ActionValueDis, StateValue, StochaPolicyDis  # noqa: E402
from gops_amd.create_pkg.create_env_model import create_env_model  # noqa: E402
from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler  # noqa: E402
from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler  # noqa: E402
from gops_amd.utils.act_distribution import CategoricalDistribution, ValueDiracDistribution  # noqa: E402

WARMUP, BLOCKS, CALLS = 3, 7, 20
CFG = dict(env_id="gym_cartpoleconti")
TABLE = [[-1.0], [1.0]]
SHAPES = [   # name, sampler class, policy class, env_step, N, T, max_episode_steps, epsilon
    ("dqn", DeviceEnvSampler, ActionValueDis, "data", 256, 16, 200, 0.1),
    ("trpo_dis", OnPolicyDeviceSampler, StochaPolicyDis, "model", 8, 16, 50, 0.0),
    ("trpo_dis_data", OnPolicyDeviceSampler, StochaPolicyDis, "data", 8, 16, 50, 0.0),
]


class Nets(torch.nn.Module):
    def __init__(self, policy_cls):
        super().__init__()
        torch.manual_seed(0)
        dist = ValueDiracDistribution if policy_cls is ActionValueDis else CategoricalDistribution
        self.policy = policy_cls(obs_dim=4, act_num=2, hidden_sizes=[64, 64], hidden_activation="relu", action_distribution_cls=dist)
        self.value = StateValue(obs_dim=4, hidden_sizes=[64, 64], hidden_activation="relu", output_activation="linear",
                                action_distribution_cls=None)


def block_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000 / CALLS


def main():
    for name, cls, policy_cls, step, N, T, limit, eps in SHAPES:
        row = dict(shape=name, env_id=CFG["env_id"], env_step=step, n_envs=N, steps=T, hidden=[64, 64], epsilon=eps, blocks=BLOCKS,
                   calls_per_block=CALLS)
        pair = {}
        for fused in (True, False):
            smp = cls(CFG, create_env_model(**CFG), n_envs=N, steps_per_sample=T, max_episode_steps=limit, seed=0, env_step=step,
                      fused=fused, action_table=TABLE, epsilon=eps)
            smp.networks = Nets(policy_cls).cuda()
            for _ in range(WARMUP):
                smp.sample()
            pair["fused" if fused else "loop"] = smp
        ms = dict(fused=[], loop=[])
        for _ in range(BLOCKS):
            for key, smp in pair.items():
                ms[key].append(block_ms(smp.sample))
        for key, smp in pair.items():
            row[key] = dict(median_ms=round(statistics.median(ms[key]), 3), min_ms=round(min(ms[key]), 3), max_ms=round(max(ms[key]), 3))
            row["path_" + key] = smp.path
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
