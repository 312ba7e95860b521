"""Time one `local_update` of DQN on recurrent networks two ways: `fused_target="force"` (one gops_rnn_dqn_step, then gops_rnn_backward,
Adam, Polyak) and `fused_target=False` (target gops_rnn_forward, torch.max, online gops_rnn_forward, gops_dqn_loss, then the same).

    python tools/microbench/rnn_dqn.py            # prints one JSON line per shape

Shapes (B, L, O, H, head hidden, N): the reference's stacked cart-pole env (L = 5, O = 4) at a small and a large replay batch, and the
widest net the kernels hold.  Both variants alternate in the same process, each on its own algorithm object built from the same seed and
fed the same batch: 20 warm-up rounds (the update's graph is captured inside them where capture is on), then 15 timed windows per
variant, each of as many rounds as fill about a quarter of a second (counted from one calibration window of 50 rounds, at least 50)
and bracketed by a device synchronise; median and min .. max of the per-round time in us, the rounds per window, the ratio of the
medians, and whether the timed rounds were graph replays.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402

WARMUP, WINDOWS, CALIBRATION_ROUNDS, WINDOW_SECONDS = 20, 15, 50, 0.25
SHAPES = ((64, 5, 4, 64, (64,), 2), (4096, 5, 4, 64, (64,), 2), (4096, 32, 64, 128, (128,), 16))


def window(fn, rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / rounds


def make(fused, L, O, H, head, N):
    torch.manual_seed(0)
    alg = create_alg(algorithm="DQN", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="gym_cartpolecontiwithstack",
                     obsv_dim=(L, O), action_type="discret", action_num=N, value_func_type="RNN", value_func_name="ActionValueDis",
                     value_hidden_sizes=[H] + list(head), value_hidden_activation="tanh", value_output_activation="linear",
                     value_learning_rate=1e-4, policy_func_name="DetermPolicyDis", policy_act_distribution="default",
                     buffer_name="replay_buffer", use_gpu=True, fused_target=fused)
    alg.networks.cuda()
    return alg


def main():
    for B, L, O, H, head, N in SHAPES:
        g = torch.Generator().manual_seed(1)
        data = dict(obs=torch.randn(B, L, O, generator=g), obs2=torch.randn(B, L, O, generator=g),
                    act=torch.randint(N, (B, 1), generator=g).float(), rew=torch.randn(B, generator=g),
                    done=(torch.rand(B, generator=g) < 0.1).float())
        data = {k: v.cuda() for k, v in data.items()}
        algs = {"fused": make("force", L, O, H, head, N), "composed": make(False, L, O, H, head, N)}
        fns = {k: (lambda a=a: a.local_update(data, 0)) for k, a in algs.items()}
        for _ in range(WARMUP):
            for fn in fns.values():
                fn()
        assert [a.backup_path for a in algs.values()] == ["fused", "composed"]
        rounds = {k: max(CALIBRATION_ROUNDS, int(WINDOW_SECONDS * 1e6 / window(fn, CALIBRATION_ROUNDS))) for k, fn in fns.items()}
        us = {k: [] for k in fns}
        for _ in range(WINDOWS):   # alternating: both see the same neighbours on the machine
            for k, fn in fns.items():
                us[k].append(window(fn, rounds[k]))
        row = dict(B=B, L=L, O=O, H=H, head_hidden=list(head), N=N)
        for k, v in us.items():
            row[k] = dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1), rounds=rounds[k],
                          graph_replay=algs[k]._graphs["update"].graph is not None)
        row["composed_over_fused"] = round(row["composed"]["median_us"] / row["fused"]["median_us"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
