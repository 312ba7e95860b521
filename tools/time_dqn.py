"""ms per DQN update with the max-Q backup as one `gops_dqn_backup` launch (fused_target="force") against the composed path
(`gops_mlp_forward` + `torch.max`, fused_target=False), eager and under HIP-graph replay.

    python tools/time_dqn.py [--iters 200] [--repeats 5] [--graph-only]

Shapes: B = 256 and B = 65536, 64-64 and 256-256 networks (obs 6, 4 actions).  Each figure is the median over `repeats` timed
blocks of `iters` updates between two device events, after a warm-up that also captures the graph; the batch is resident on the
device, log scalars stay lazy (no host sync inside a block).  Prints one JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OBS, ACT_NUM = 6, 4


def build(hidden, fused):
    from gops_amd.create_pkg.create_alg import create_alg
    torch.manual_seed(0)
    alg = create_alg(algorithm="DQN", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="gym_cartpole", obsv_dim=OBS,
                     action_type="discret", action_num=ACT_NUM, value_func_type="MLP", value_func_name="ActionValueDis",
                     value_hidden_sizes=list(hidden), value_hidden_activation="relu", value_output_activation="linear",
                     value_learning_rate=1e-4, policy_func_name="DetermPolicyDis", policy_act_distribution="default",
                     buffer_name="replay_buffer", use_gpu=True, fused_target="force" if fused else False)
    alg.networks.cuda()
    return alg


def time_config(hidden, B, fused, graph, iters, repeats):
    os.environ["GOPS_HIP_GRAPH"] = "1" if graph else "0"
    alg = build(hidden, fused)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")   # noqa: E731
    data = dict(obs=rnd(B, OBS), act=torch.randint(ACT_NUM, (B, 1), generator=g, device="cuda").float(), rew=rnd(B), obs2=rnd(B, OBS),
                done=(rnd(B) > 1).float())
    it = 0
    for _ in range(12):   # warm-up: every kernel, the graph captured
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
    return dict(hidden=list(hidden), batch=B, fused_target=fused, graph=graph, backup_path=alg.backup_path,
                ms_per_update=round(statistics.median(times), 4), spread=[round(min(times), 4), round(max(times), 4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-only", action="store_true", help="skip the eager configurations")
    args = ap.parse_args()
    for hidden in ((64, 64), (256, 256)):
        for B in (256, 65536):
            for graph in ((True,) if args.graph_only else (False, True)):
                for fused in (True, False):
                    iters = args.iters if B <= 4096 else max(20, args.iters // 10)
                    print(json.dumps(time_config(hidden, B, fused, graph, iters, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
