"""Time `Evaluator.run_evaluation`-sized work three ways on the MI355X: the fused episode kernel (`gops_episode_rollout`), the
per-step device loop, and that loop with the per-step host sync `DeviceEnvSampler`'s bookkeeping has today.

    python tools/microbench/eval_episode.py [--steps 200] [--reps 20]

Cases: pyth_idpendulum 64-64 and pyth_veh3dofconti 256-256, 5 / 16 / 1024 episodes x `steps`.  The policies are random-init with
the output layer zeroed (action 0): episodes then run to the time limit instead of ending in a few steps, so every case does the
work it names.  Each figure is the median wall time of `reps` calls after 3 warm-up calls, timed around a device synchronisation
(the call returns a Python float, so the sync is part of what a trainer pays).  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def alg_kwargs(cfg, hidden, act="relu"):
    """INFADP kwargs of a workload dict (env_id, pre_horizon) with an MLP policy of `hidden` widths."""
    import numpy as np
    from gops_amd.utils.synthetic import act_dim_of, obs_dim_of
    A = act_dim_of(cfg)
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id=cfg["env_id"], obsv_dim=obs_dim_of(cfg),
              action_dim=A, action_type="continu", action_high_limit=np.ones(A, dtype=np.float32),
              action_low_limit=-np.ones(A, dtype=np.float32), policy_func_type="MLP", policy_func_name="DetermPolicy",
              policy_hidden_sizes=list(hidden), policy_hidden_activation=act, policy_act_distribution="default",
              policy_learning_rate=1e-3, use_gpu=True, value_func_type="MLP", value_func_name="StateValue",
              value_hidden_sizes=[64, 64], value_hidden_activation=act, value_learning_rate=1e-3)
    if "pre_horizon" in cfg:
        kw["pre_horizon"] = cfg["pre_horizon"]
    return kw


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.trainer.evaluator import Evaluator
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    for cfg, hidden in ((dict(env_id="pyth_idpendulum"), (64, 64)), (dict(env_id="pyth_veh3dofconti", pre_horizon=10), (256, 256))):
        kw = alg_kwargs(cfg, hidden)
        alg = create_alg(**kw)
        alg.networks.to("cuda")
        with torch.no_grad():
            last = [m for m in alg.networks.policy.pi if isinstance(m, torch.nn.Linear)][-1]
            last.weight.zero_(), last.bias.zero_()
        for E in (5, 16, 1024):
            ev = Evaluator(env_model=alg.envmodel, networks=alg.networks, cfg=cfg, num_eval_episode=E, eval_save=False,
                           max_episode_steps=args.steps)
            init = ev.draw_initial_conditions(E)
            if cfg["env_id"] == "pyth_idpendulum":
                init["obs"] = init["obs"] * 0.01   # near upright: no termination inside the limit under action 0
            row = dict(env=cfg["env_id"], hidden=list(hidden), episodes=E, steps=args.steps)
            for name, fn in (("fused_ms", lambda: ev.run_episodes(init, fused=True)["ret"].mean().item()),
                             ("loop_ms", lambda: ev.step_loop(init)["ret"].mean().item()),
                             ("loop_sync_per_step_ms", lambda: ev.step_loop(init, sync_every_step=True)["ret"].mean().item())):
                med, lo, hi = timed(fn, args.reps if name == "fused_ms" else max(3, args.reps // 4))
                row[name] = round(med, 3)
                row[name + "_range"] = [round(lo, 3), round(hi, 3)]
            row["mean_length_fused"] = float(ev.run_episodes(init, fused=True)["length"].float().mean().item())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
