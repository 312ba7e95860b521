"""Wall time of BatchOptController.solve against B sequential OptController calls (not part of bench.py).

Workload: pyth_lq s4a2, num_pred_step 10, ctrl_interval 1, B in {1, 64, 1024} initial states from gops_amd.utils.synthetic, every
solve a cold start.  Batched: warm-up solves, then 15 timed solves, each between two device synchronisations; median, min, max,
the iteration counts and the share of rows by final status.  Sequential: the existing OptController (scipy's L-BFGS-B, one state
per call, reset before each) over the same states, timed per pass over all B states - 15 passes up to B = 64, 3 passes at
B = 1024 (a pass takes tens of seconds there).  Prints one JSON line per B.

    python tools/microbench/mpc_batch.py [--batches 1 64 1024] [--solves 15] [--warmup 3]

`--episodes`: closed-loop episodes instead - `BatchOptController.run_episodes` (the plan handed over on the device, one
gops_mpc_advance launch per control step) against the loop a user writes around `solve()` (finish, three clones and a cat on the
host side of every hand-over, then the env step), same states, 20 control steps, every episode a cold start; `--solves` timed runs
after `--warmup` warm-ups, each between two synchronisations; median (min .. max) of both and their ratio, one JSON line per B.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gops_amd import hip_backend as hb  # noqa: E402
from gops_amd.create_pkg.create_env_model import create_env_model  # noqa: E402
from gops_amd.sys_simulator import BatchOptController, OptController  # noqa: E402
from gops_amd.utils.synthetic import make_batch  # noqa: E402

CFG = dict(env_id="pyth_lq", lq_config="s4a2")
T = 10


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), n=len(ms))


def hand_loop(ctrl, x0, steps):
    """The closed loop around solve(): per control step a solve of all rows, then the env model stepped with the first action."""
    ctrl.reset()
    obs = torch.from_numpy(x0).to(ctrl.device)
    zeros = torch.zeros(x0.shape[0], device=ctrl.device)
    ret, evals = zeros.clone(), 0
    for _ in range(steps):
        res = ctrl.solve(obs)
        evals += res["evaluations"]
        for _ in range(ctrl.ctrl_interval):
            obs, rew, _, _ = hb.env_step(ctrl._env, obs, res["action"], zeros, {})
            ret = ret + rew
    return ret, evals


def episodes(args, model):
    steps = 20
    for B in args.batches:
        x0 = make_batch(dict(CFG, batch=B), 900 + B)["obs"].numpy().astype(np.float32)
        ctrl = BatchOptController(model, num_pred_step=T, gamma=1.0)
        runs = {"run_episodes": lambda: (lambda r: (r["return"], r["evaluations"]))(ctrl.run_episodes(x0, steps)),
                "hand_loop": lambda: hand_loop(ctrl, x0, steps)}
        ms, last = {k: [] for k in runs}, {}
        for k in range(args.warmup + args.solves):
            for name, run in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = run()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        same = bool(torch.equal(last["run_episodes"][0], last["hand_loop"][0]))   # (pyth_lq never reports done: no row freezes)
        print(json.dumps(dict(B=B, control_steps=steps, run_episodes=stats(ms["run_episodes"]), hand_loop=stats(ms["hand_loop"]),
                              ratio_median=round(statistics.median(ms["hand_loop"]) / statistics.median(ms["run_episodes"]), 3),
                              evaluations=dict(run_episodes=last["run_episodes"][1], hand_loop=last["hand_loop"][1]), same_returns=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--solves", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", action="store_true", help="time run_episodes against the hand-written loop over solve()")
    args = ap.parse_args()
    model = create_env_model(**CFG, use_gpu=True)
    if args.episodes:
        return episodes(args, model)
    for B in args.batches:
        x0 = make_batch(dict(CFG, batch=B), 900 + B)["obs"].numpy().astype(np.float32)
        batched = BatchOptController(model, num_pred_step=T, gamma=1.0)
        ms = []
        for k in range(args.warmup + args.solves):
            batched.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = batched.solve(x0)
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        it = res["iterations"].cpu().numpy()
        share = np.bincount(res["status"].cpu().numpy(), minlength=5) / B
        single = OptController(model, num_pred_step=T, gamma=1.0, mode="shooting")
        passes, seq, nit, nfev = (args.solves if B <= 64 else 3), [], [], []
        for k in range(1 + passes):   # one warm-up pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(B):
                single.reset()
                single(x0[b])
                if k == passes:
                    nit.append(single.last_result.nit), nfev.append(single.last_result.nfev)
            torch.cuda.synchronize()
            if k >= 1:
                seq.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(B=B, batched=stats(ms), sequential=stats(seq), speedup_median=round(statistics.median(seq) / statistics.median(ms), 2),
                              batched_evaluations=res["evaluations"], batched_iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max())),
                              batched_status_share=dict(zip(hb.MPC_STATUS_NAMES, np.round(share, 4).tolist())),
                              sequential_iterations_median=float(np.median(nit)), sequential_evaluations_median=float(np.median(nfev)))), flush=True)


if __name__ == "__main__":
    main()
