"""Shared by test_dqn_cpu.py and test_dqn_gpu.py: building DQN from a fixture of tests/golden/make_golden_dqn.py or from synthetic
networks, batches with integer actions, and one update restated in torch at any dtype (the oracle of the GPU tests at float64)."""
import copy

import numpy as np
import torch

from ac_helpers import synthetic_batch
from conftest import golden_meta, load_golden

from gops_amd.create_pkg.create_alg import create_alg

DQN_ONE_UPDATE = ["dqn_o3n2_relu", "dqn_o4n5_gelu"]
DQN_FIVE_UPDATES = "dqn_o3n2_5updates"


def dqn_kwargs(obs, act_num, hidden, activation, seed=0, use_gpu=False, **over):
    """create_alg's arguments for DQN on a network of this shape (the keys of example_train/dqn/dqn_mlp_cartpole_offserial.py)."""
    kw = dict(algorithm="DQN", trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id="gym_cartpole", obsv_dim=obs,
              action_type="discret", action_num=act_num, value_func_type="MLP", value_func_name="ActionValueDis",
              value_hidden_sizes=list(hidden), value_hidden_activation=activation, value_output_activation="linear",
              value_learning_rate=1e-3, policy_func_name="DetermPolicyDis", policy_act_distribution="default",
              buffer_name="replay_buffer", use_gpu=use_gpu)
    kw.update(over)
    return kw


def case_kwargs(meta, use_gpu=False, **over):
    c = meta["case"]
    return dqn_kwargs(c["obs"], c["act_num"], c["hidden"], c["act"], meta["seed"], use_gpu, **over)


def fresh(name, **over):
    """(alg, fixture, meta): built through create_alg with the fixture's seed, nothing loaded."""
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    return create_alg(**case_kwargs(meta, **over)), g, meta


def load_dqn(name, use_gpu=False, prefix="sd/", **over):
    """(alg, fixture, meta): `fresh`, then the attributes and the learning rate set as the maker set them and the fixture's state
    dict loaded."""
    alg, g, meta = fresh(name, use_gpu=use_gpu, **over)
    for k, v in meta["case"]["attrs"].items():
        setattr(alg, k, v)
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})
    if "lr" in meta:
        for group in alg.networks.q_optimizer.param_groups:
            group["lr"] = meta["lr"]
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def restate_dqn(alg, data, dtype=torch.float64):
    """One compute_gradient of DQN (gops/algorithm/dqn.py:94-154; with PER the evident intent of :145-154 - `q_target`, the weighted
    loss) restated with autograd on copies of the networks at `dtype` on the host:
    dict(backup, q_targ, a_star, loss, q_mean, abs_err, grads {"q": [tensors]})."""
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items() if k != "idx"}
    for p in nets.q.parameters():
        p.requires_grad_(True)
        p.grad = None
    with torch.no_grad():
        q_t = nets.q_target(d["obs2"])
        q_max, a_star = torch.max(q_t, dim=1)
        backup = d["rew"] * alg.reward_scale + alg.gamma * (1 - d["done"]) * q_max
    q = nets.q(d["obs"]).gather(1, d["act"].reshape(-1, 1).to(torch.long)).squeeze(1)
    w = d.get("weight") if alg.per_flag else None
    loss = ((q - backup) ** 2).mean() if w is None else (w * (q - backup) ** 2).mean()
    loss.backward()
    return dict(backup=backup, q_targ=q_t, a_star=a_star, loss=loss.detach(), q_mean=q.detach().mean(), abs_err=(q - backup).abs().detach(),
                grads={"q": [p.grad.detach().clone() for p in nets.q.parameters()]})


def synthetic_dqn(obs, act_num, hidden, activation, seed=5, **over):
    """DQN on the GPU with the target randomised apart from its online twin and every column of the target head scaled to unit
    spread and centred on 256 probe observations (so that every action is the arg-max on some rows of `dqn_batch`); gamma and
    reward_scale off their defaults."""
    torch.manual_seed(seed)
    a = create_alg(**dqn_kwargs(obs, act_num, hidden, activation, seed, True, **over))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in a.networks.q_target.parameters():
            p.add_(0.3 * (torch.rand(p.shape, generator=g) - 0.5))
        probe = torch.randn(256, obs, generator=g)
        head = a.networks.q_target.linear_layers()[-1]
        scale = 1.0 / a.networks.q_target(probe).std(dim=0)   # (columns of equal spread: none of them wins everywhere or nowhere)
        head.weight.mul_(scale[:, None])
        head.bias.mul_(scale)
        head.bias.sub_(a.networks.q_target(probe).median(dim=0).values)
    a.networks.cuda()
    a.gamma, a.reward_scale = 0.97, 0.5
    return a


def dqn_batch(B, obs, act_num, seed=0, weight=False):
    """`ac_helpers.synthetic_batch`'s transitions (done rows at both ends) with uniform action indices as floats, [B, 1]."""
    data = synthetic_batch(B, obs, 1, seed)
    data.pop("target_noise")
    g = torch.Generator().manual_seed(seed + 77)
    data["act"] = torch.randint(act_num, (B, 1), generator=g).float()
    if weight:
        data["weight"] = 0.2 + 0.8 * torch.rand(B, generator=g)
        data["idx"] = torch.randperm(4 * B, generator=g)[:B].to(torch.int32)
    return data
