"""Wall time of BatchOptController.solve with path_constraints="augmented_lagrangian" against B sequential OptController calls
(SLSQP on kernel constraint values and Jacobians); not part of bench.py.

Workload: pyth_veh3dofconti_surrcstr, pre_horizon 5, num_pred_step 5, one surrounding vehicle; B in {4, 64, 256} states with the ego
vehicle on its reference path and a slower vehicle 5.9 .. 6.5 m ahead, up to 0.6 m to either side - the constraint is active at the
optimum of most rows.  Batched: warm-up solves, then `--solves` timed cold solves, each between two device synchronisations.
Sequential: one OptController per pass over all B states (reset before each state), `--passes` timed passes after one warm-up pass.
Prints one JSON line per B: medians, their ratio, the outer / inner status shares, the violations of both.

    python tools/microbench/mpc_constrained.py [--batches 4 64 256] [--solves 10] [--warmup 3] [--passes 2]
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
from gops_amd.utils.synthetic import make_batch, veh_obs_f32  # noqa: E402

CFG = dict(env_id="pyth_veh3dofconti_surrcstr", pre_horizon=5, surr_veh_num=1)
T = 5


def states(B, seed):
    d = {k: v.numpy() for k, v in make_batch(dict(CFG, batch=B), seed).items()}
    rng = np.random.RandomState(seed)
    ref = d["ref_points"]
    state = np.concatenate((ref[:, 0, :4], np.zeros((B, 2), np.float32)), 1).astype(np.float32)
    phi = state[:, 2].astype(np.float64)
    lon, lat, du = rng.uniform(5.9, 6.5, B), rng.uniform(-0.6, 0.6, B), rng.uniform(0.8, 1.6, B)
    surr = np.stack((state[:, 0] + lon * np.cos(phi) - lat * np.sin(phi), state[:, 1] + lon * np.sin(phi) + lat * np.cos(phi), phi,
                     state[:, 3] - du, np.zeros(B)), 1).astype(np.float32)[:, None, :]
    obs = np.concatenate((veh_obs_f32(state, ref), (surr[..., :4] - state[:, None, :4]).reshape(B, -1)), 1).astype(np.float32)
    return obs, dict(state=state, ref_points=ref, path_num=d["path_num"], u_num=d["u_num"], ref_time=d["ref_time"], surr_state=surr)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), n=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 64, 256])
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    model = create_env_model(**CFG, use_gpu=True)
    for B in args.batches:
        obs, info = states(B, 700 + B)
        batched = BatchOptController(model, num_pred_step=T, gamma=1.0, path_constraints="augmented_lagrangian")
        ms = []
        for k in range(args.warmup + args.solves):
            batched.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = batched.solve(obs, info)
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        outer = np.bincount(res["outer_status"].cpu().numpy(), minlength=3) / B
        viol = res["constraint_violation"].cpu().numpy()
        active = float((res["multipliers"].flatten(1).max(1).values > 0).float().mean().item())
        single = OptController(model, num_pred_step=T, gamma=1.0, mode="shooting")
        seq, ok = [], []
        for k in range(1 + args.passes):   # one warm-up pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(B):
                single.reset()
                single(obs[b], {key: v[b] for key, v in info.items()})
                if k == args.passes:
                    ok.append(bool(single.last_result.success))
            torch.cuda.synchronize()
            if k >= 1:
                seq.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(B=B, batched=stats(ms), sequential=stats(seq), speedup_median=round(statistics.median(seq) / statistics.median(ms), 2),
                              batched_evaluations=res["evaluations"], outer_status_share=dict(zip(hb.MPC_AL_STATUS_NAMES, np.round(outer, 4).tolist())),
                              outer_iterations_max=int(res["outer_iterations"].max().item()), rows_with_active_constraint=round(active, 4),
                              batched_violation_max=float(viol.max()), slsqp_success_share=round(float(np.mean(ok)), 4))), flush=True)


if __name__ == "__main__":
    main()
