"""Generate the DQN fixtures (`dqn_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_dqn.py
Every array written here is an input, or an output of the reference's own class (`gops.algorithm.dqn.DQN`, non-PER: its PER path
raises, dqn.py:149).  `backup` and `q_targ` are not returned by the reference's update: they are evaluated here with the reference's
own target network, and the recorded critic loss is checked against them.

Before saving, each case centres every column of the target head on the batch (the per-column median is subtracted from the head's
bias) and asserts that every action is the arg-max of the target on at least one row, that every action occurs in `act`, and that
`done` has both values.  The seed is the first one from the case's name on for which this holds; it is stored in `meta/cfg`.
"""
import copy
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)
from _make_ac_common import arrays, last_linear, meta_entry, state  # noqa: E402

from gops.algorithm.dqn import DQN  # noqa: E402

# name: network and batch shape, attributes set after construction
CASES = {
    "dqn_o3n2_relu": dict(obs=3, act_num=2, hidden=(32, 16), act="relu", batch=70, attrs={}),
    "dqn_o4n5_gelu": dict(obs=4, act_num=5, hidden=(64, 48), act="gelu", batch=70, attrs=dict(gamma=0.97, reward_scale=0.5)),
}
FIVE = dict(obs=3, act_num=2, hidden=(32, 16), act="relu", batch=70, attrs=dict(tau=0.05))


class Unbalanced(Exception):
    pass


def alg_kwargs(case, seed):
    return dict(algorithm="DQN", trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id="gym_cartpole", obsv_dim=case["obs"],
                action_type="discret", action_num=case["act_num"], value_func_type="MLP", value_func_name="ActionValueDis",
                value_hidden_sizes=list(case["hidden"]), value_hidden_activation=case["act"], value_output_activation="linear",
                value_learning_rate=1e-3, policy_func_name="DetermPolicyDis", policy_act_distribution="default",
                buffer_name="replay_buffer", use_gpu=False)


def build(case, seed):
    """(alg, generator): the reference's DQN, its target - which starts as a copy - moved apart."""
    torch.manual_seed(seed)
    alg = DQN(**alg_kwargs(case, seed))
    for k, v in case["attrs"].items():
        setattr(alg, k, v)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in alg.networks.q_target.parameters():
            p.add_(0.6 * (torch.rand(p.shape, generator=g) - 0.5))
    return alg, g


def batch_of(case, g):
    B, O, N = case["batch"], case["obs"], case["act_num"]
    obs = torch.randn(B, O, generator=g)
    return dict(obs=obs, act=torch.randint(N, (B, 1), generator=g).float(), rew=torch.randn(B, generator=g),
                obs2=obs + 0.05 * torch.randn(B, O, generator=g), done=(torch.rand(B, generator=g) < 0.15).float())


def balance(alg, data):
    with torch.no_grad():
        last_linear(alg.networks.q_target.q).bias.sub_(alg.networks.q_target(data["obs2"]).median(dim=0).values)


def assert_cases(name, alg, data, N):
    with torch.no_grad():
        best = alg.networks.q_target(data["obs2"]).argmax(dim=1)
    checks = {"every action is the arg-max somewhere": set(best.tolist()) == set(range(N)),
              "every action occurs in act": set(data["act"].long().flatten().tolist()) == set(range(N)),
              "done rows": bool((data["done"] == 1).any()) and bool((data["done"] == 0).any())}
    missing = [k for k, ok in checks.items() if not ok]
    if missing:
        raise Unbalanced(name, missing)


def backup_of(alg, data):
    """backup / q_targ / loss of dqn.py:104,136-141 from the reference's networks."""
    nets = alg.networks
    with torch.no_grad():
        q_t = nets.q_target(data["obs2"])
        backup = data["rew"] * alg.reward_scale + alg.gamma * (1 - data["done"]) * q_t.max(dim=1).values
        q = nets.q(data["obs"]).gather(1, data["act"].to(torch.long)).squeeze(1)
        return backup, q_t, ((q - backup) ** 2).mean()


def first_seed(name, attempt):
    """`attempt(seed)` for the first seed from the name's on whose batch holds every case."""
    base = zlib.crc32(name.encode()) % 1000
    for seed in range(base, base + 50):
        try:
            return attempt(seed)
        except Unbalanced as e:
            print("  seed", seed, "skipped:", e.args[1])
    raise RuntimeError(f"{name}: no seed in {base} .. {base + 49} holds every case")


def one_update(name):
    case = CASES[name]

    def attempt(seed):
        alg, g = build(case, seed)
        data = batch_of(case, g)
        balance(alg, data)
        assert_cases(name, alg, data, case["act_num"])
        out = {**arrays(data, "in/"), **meta_entry(case=case, seed=seed), **state(alg)}
        tb, info = alg.get_remote_update_info(data, 0)
        backup, q_t, loss = backup_of(alg, data)
        assert abs(float(loss) - tb["Loss/Critic loss-RL iter"]) <= 1e-6 * max(1.0, abs(tb["Loss/Critic loss-RL iter"])), name
        assert set(tb) == {"Loss/Critic loss-RL iter", "Time/Algorithm time [ms]-RL iter"}, set(tb)
        out.update(backup=backup.numpy(), q_targ=q_t.numpy(), loss_q=np.float64(tb["Loss/Critic loss-RL iter"]))
        for i, gr in enumerate(info["q_grad"]):
            out[f"q_grad/{i}"] = gr.detach().numpy().copy()
        mg.save(name, **out)

    first_seed(name, attempt)


def five_updates():
    """All online and target parameters after each of five consecutive `local_update` calls with tau = 0.05; the learning rate raised
    so that every step is well above fp32 rounding."""
    name, case, lr = "dqn_o3n2_5updates", FIVE, 1e-2

    def attempt(seed):
        alg, g = build(case, seed)
        for group in alg.networks.q_optimizer.param_groups:
            group["lr"] = lr
        batches = [batch_of(case, g) for _ in range(5)]
        balance(alg, {key: torch.cat([b[key] for b in batches]) for key in batches[0]})
        out = {**meta_entry(case=case, seed=seed, lr=lr), **state(alg, "sd0/")}
        for k, data in enumerate(batches):
            assert_cases(f"{name}[{k}]", alg, data, case["act_num"])   # (against the target this update's backup is formed with)
            out.update(arrays(data, f"in{k}/"))
            tb = alg.local_update(copy.deepcopy(data), k)
            out[f"loss_q{k}"] = np.float64(tb["Loss/Critic loss-RL iter"])
            out.update(state(alg, f"sd{k + 1}/"))
        mg.save(name, **out)

    first_seed(name, attempt)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name in CASES:
        if not only or name in only:
            one_update(name)
    if not only or "five_updates" in only:
        five_updates()
