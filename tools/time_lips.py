"""Time the LipsNet path on the GPU: the example configuration (lqs2a1, policy [64, 64] relu, local K [32], value [64, 64] relu) at
B = 64 and B = 65 536.

  kernel   `hip_backend.LipsPolicy` forward + backward (gops_lips_forward / gops_lips_backward)
  eager    the same forward + backward of the eager module (gops_amd/apprfunc/lipsnet.py) by torch autograd on the same GPU
  pim      one INFADP policy-improvement `local_update` (policy, wrappers, open-loop model step, target value, adjoints, LipsNet
           backward, Adam of both groups, Polyak); GOPS_HIP_GRAPH has no effect on this path (algorithm/infadp.py), so one column

One warm-up round, then REPEATS timed rounds of INNER calls each between two device synchronisations; prints the median and
min .. max of ms per call as one JSON line per batch size.   python tools/time_lips.py [--repeats 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gops_amd import hip_backend as hb  # noqa: E402
from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402


def timed(fn, repeats, inner):
    out = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        if r:
            out.append((time.perf_counter() - t0) * 1e3 / inner)
    return dict(median_ms=round(statistics.median(out), 4), min_ms=round(min(out), 4), max_ms=round(max(out), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert args.repeats >= 7
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=1, env_id="pyth_lq", lq_config="s2a1", obsv_dim=2, action_dim=1,
              action_type="continu", action_high_limit=np.ones(1, dtype=np.float32), action_low_limit=-np.ones(1, dtype=np.float32),
              policy_func_type="LipsNet", policy_func_name="DetermPolicy", policy_hidden_sizes=[64, 64], policy_hidden_activation="relu",
              policy_act_distribution="default", policy_lips_init_value=1.0, policy_lips_auto_adjust=True, policy_lips_learning_rate=1e-5,
              policy_lips_hidden_sizes=[32], policy_eps=1e-4, policy_lambda=1e-3, policy_local_lips=True, policy_squash_action=False,
              policy_learning_rate=3e-5, value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=[64, 64],
              value_hidden_activation="relu", value_learning_rate=8e-5, use_gpu=True)
    for B in (64, 65536):
        alg = create_alg(**kw)
        alg.networks.cuda()
        alg.set_parameters({"gamma": 0.99, "tau": 0.2, "forward_step": 1})
        alg.train()
        pol = alg.networks.policy
        g = torch.Generator().manual_seed(B)
        obs = torch.randn(B, 2, generator=g).cuda()
        ga = torch.randn(B, 1, generator=g).cuda()
        data = dict(obs=obs, done=torch.zeros(B).cuda())
        lp = hb.LipsPolicy(pol, B)

        def kernel():
            lp.forward(obs, training=True)
            lp.backward(ga)

        def eager():
            pol.zero_grad()
            (pol(obs) * ga).sum().backward()

        inner = 20 if B == 64 else 5
        res = dict(batch=B, repeats=args.repeats, kernel=timed(kernel, args.repeats, inner), eager=timed(eager, args.repeats, inner),
                   pim=timed(lambda: alg.local_update(data, 1), args.repeats, inner))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
