"""Time one sample() of T = 200 steps on gym_cartpolecontiwithstack (L = 5, O = 4, H = 64, head hidden (64,)) on the GPU two ways, in
the same process, the variants alternating window by window:

  stack:  one `gops_stack_sample_rollout` launch for all steps (hip_backend.StackSampleRollout);
  loop:   what the library offered before it - per step one `RnnNet.forward` on the windows, the exploration head in torch, one
          `gops_env_step` on the newest rows (the flat cart-pole's step: the same arithmetic at another force) and a torch roll of the
          window; no resets, no books - a lower bound of a per-step sampler.

    python tools/microbench/stack_sampler.py       # prints one JSON line per n_envs

Each variant: 3 warm-up windows, then 15 timed ones, each ending in a device synchronise; median and min .. max in ms.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gops_amd import hip_backend as hb  # noqa: E402
from gops_amd.create_pkg.create_apprfunc import create_apprfunc  # noqa: E402
from gops_amd.create_pkg.create_env_model import create_env_model  # noqa: E402
from rnn_helpers import apprfunc_kwargs  # noqa: E402

WARMUP, TIMED, T, L, H, R = 3, 15, 200, 5, 64, 8


def main():
    torch.manual_seed(0)
    net = create_apprfunc(**apprfunc_kwargs("StochaPolicy", (H, 64), "tanh", O=4, out=1)).cuda()
    lim = (net.act_low_lim.cpu().numpy(), net.act_high_lim.cpu().numpy())
    env = create_env_model("gym_cartpolecontiwithstack").hip_env(*lim, data_env=True)
    flat = create_env_model("gym_cartpoleconti").hip_env(*lim, data_env=True)
    for N in (64, 4096):
        half = torch.tensor([2.0, 0.05, 0.2, 0.05], device="cuda")
        x0, pool = (torch.rand(N, 4, device="cuda") * 2 - 1) * half, (torch.rand(R, N, 4, device="cuda") * 2 - 1) * half
        noise = torch.randn(T, N, 1, device="cuda")
        ro = hb.StackSampleRollout(env, net.hip_rnn(L), n_envs=N, steps=T, max_episode_steps=200, pool_rows=R, min_log_std=net.min_log_std,
                                   max_log_std=net.max_log_std)
        rnn_net, zeros = hb.RnnNet(net.hip_rnn(L), N), torch.zeros(N, device="cuda")

        def stack():
            state = dict(obs=x0.unsqueeze(1).repeat(1, L, 1).contiguous(), t=torch.zeros(N, dtype=torch.int32, device="cuda"),
                         reset_count=torch.zeros(N, dtype=torch.int32, device="cuda"))
            ro.run(state, dict(obs=pool), noise)

        def loop():
            window = x0.unsqueeze(1).repeat(1, L, 1).contiguous()
            for t in range(T):
                y = rnn_net.forward(window)
                act = y[:, :1] + torch.clamp(y[:, 1:], net.min_log_std, net.max_log_std).exp() * noise[t]
                nxt = hb.env_step(flat, window[:, -1].contiguous(), act.contiguous(), zeros, {})[0]
                window = torch.roll(window, -1, 1)
                window[:, -1] = nxt

        ms = dict(stack=[], loop=[])
        for i in range(WARMUP + TIMED):
            for name, fn in (("stack", stack), ("loop", loop)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= WARMUP:
                    ms[name].append((time.perf_counter() - t0) * 1000)
        row = dict(n_envs=N, steps=T, stack_length=L, hidden=H, launches=dict(stack=1, loop=f"{T} x (gops_rnn_forward + gops_env_step + torch's element-wise and copy kernels)"))
        for name, v in ms.items():
            row[name] = dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
