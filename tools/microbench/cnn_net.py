"""Time one forward + backward of a type_2 convolutional StochaPolicy on (4, 96, 96) images on the GPU two ways: `CnnNet`
(gops_conv_forward / _backward plus gops_mlp_forward / _backward_x for the two heads) and the same module under torch autograd on the
device (its convolution library's kernels, two Linear stacks, autograd's backward).

    python tools/microbench/cnn_net.py            # prints one JSON line per batch size

Batch sizes: a PPO minibatch of 64 and the reference script's 256.  Both variants alternate in the same process: 20 warm-up rounds, then 15 timed windows per variant,
each of as many rounds as fill about a quarter of a second (counted from one calibration window of 50 rounds, at least 50) and bracketed
by a device synchronise; median and min .. max of the per-round time in us, the rounds per window, and the ratio of the medians.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from gops_amd import hip_backend as hb  # noqa: E402
from gops_amd.create_pkg.create_apprfunc import create_apprfunc  # noqa: E402
from gops_amd.utils.act_distribution import GaussDistribution  # noqa: E402

WARMUP, WINDOWS, CALIBRATION_ROUNDS, WINDOW_SECONDS = 20, 15, 50, 0.25
BATCHES, IMAGE = (64, 256), (4, 96, 96)


def window(fn, rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / rounds


def main():
    lim = np.array([1.0, 1.0], np.float32)
    for B in BATCHES:
        torch.manual_seed(0)
        net = create_apprfunc(apprfunc="CNN", name="StochaPolicy", obs_dim=IMAGE, act_dim=2, conv_type="type_2",
                              hidden_activation="tanh", output_activation="linear", min_log_std=-20.0, max_log_std=2.0,
                              action_distribution_cls=GaussDistribution, act_low_lim=-lim, act_high_lim=lim).cuda()
        x, gy = torch.randn((B,) + IMAGE, device="cuda"), torch.randn(B, 4, device="cuda")
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        cnn_net, y = hb.CnnNet(*net.hip_cnn(), B, x.device), torch.empty(B, 4, device="cuda")
        grads = net.hip_cnn_grad()

        def hip():
            cnn_net.forward(x, out=y)
            cnn_net.backward(x, gy, grads)

        def autograd():
            net.policy(x).backward(gy)

        for _ in range(WARMUP):
            hip()
            autograd()
        fns = {"hip": hip, "torch_autograd": autograd}
        rounds = {k: max(CALIBRATION_ROUNDS, int(WINDOW_SECONDS * 1e6 / window(fn, CALIBRATION_ROUNDS))) for k, fn in fns.items()}
        us = {k: [] for k in fns}
        for _ in range(WINDOWS):   # alternating: both see the same neighbours on the machine
            for k, fn in fns.items():
                us[k].append(window(fn, rounds[k]))
        row = dict(B=B, image=list(IMAGE), conv_type="type_2")
        for k, v in us.items():
            row[k] = dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1), rounds=rounds[k])
        row["torch_over_hip"] = round(row["torch_autograd"]["median_us"] / row["hip"]["median_us"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
