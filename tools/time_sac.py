"""ms per SAC / DSAC update with the soft Q backup as one `gops_soft_q_backup` launch (fused_target="force") against the composed path
(`gops_mlp_forward` + torch elementwise ops, fused_target=False), eager and under HIP-graph replay.

    python tools/time_sac.py [--iters 200] [--repeats 5] [--wide]

Shapes: B = 256 and B = 4096, 64-64 networks (obs 6 / act 1); `--wide` adds 256-256.  Each figure is the median over `repeats` timed
blocks of `iters` updates between two device events, after a warm-up that also captures the graphs; the batch is resident on the
device, log scalars stay lazy (no host sync inside a block).  Prints one JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(name, hidden, fused):
    from gops_amd.create_pkg.create_alg import create_alg
    torch.manual_seed(0)
    alg = create_alg(algorithm=name, trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_idpendulum", obsv_dim=6,
                     action_dim=1, action_type="continu", action_low_limit=-np.ones(1, dtype=np.float32),
                     action_high_limit=np.ones(1, dtype=np.float32), policy_func_type="MLP", policy_func_name="StochaPolicy",
                     policy_hidden_sizes=list(hidden), policy_hidden_activation="relu", policy_act_distribution="TanhGaussDistribution",
                     policy_learning_rate=1e-4, value_func_type="MLP", value_func_name="ActionValue" if name == "SAC" else "ActionValueDistri",
                     value_hidden_sizes=list(hidden), value_hidden_activation="relu", value_learning_rate=1e-4, q_learning_rate=1e-4,
                     alpha_learning_rate=3e-4, gamma=0.99, tau=0.005, auto_alpha=True, bound=True, delay_update=2, use_gpu=True,
                     fused_target="force" if fused else False)
    alg.networks.cuda()
    return alg


def time_config(name, hidden, B, fused, graph, iters, repeats):
    os.environ["GOPS_HIP_GRAPH"] = "1" if graph else "0"
    alg = build(name, hidden, fused)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")   # noqa: E731
    data = dict(obs=rnd(B, 6), act=rnd(B, 1).clamp(-1, 1), rew=rnd(B), obs2=rnd(B, 6), done=(rnd(B) > 1).float(), eps_new=rnd(B, 1),
                eps_next=rnd(B, 1), z_next=rnd(B))
    it = 0
    for _ in range(12):   # warm-up: every kernel, every graph captured
        alg.local_update(data, it)
        it += 1
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            alg.local_update(data, it)
            it += 1
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / iters)
    return dict(algorithm=name, hidden=list(hidden), batch=B, fused_target=fused, graph=graph, backup_path=alg.backup_path,
                ms_per_update=round(statistics.median(times), 4), spread=[round(min(times), 4), round(max(times), 4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    for name in ("SAC", "DSAC"):
        for hidden in ((64, 64),) + (((256, 256),) if args.wide else ()):
            for B in (256, 4096):
                for graph in (False, True):
                    for fused in (True, False):
                        print(json.dumps(time_config(name, hidden, B, fused, graph, args.iters, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
