"""Shared by tests/test_td3_cpu.py and tests/test_td3_gpu.py: building DDPG / TD3 from the fixtures of tests/golden/make_golden_td3.py
and the restatement of one update (gops/algorithm/ddpg.py:95-172, td3.py:106-225) in torch, at any dtype."""
import numpy as np
import torch

from conftest import golden_meta, load_golden
from helpers import data_from_golden

from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

ONE_UPDATE = ["td3_pend_relu", "td3_lqs4a2_gelu", "td3_per_pend_relu", "ddpg_pend_relu", "ddpg_lqs4a2_gelu", "ddpg_per_lqs4a2_gelu"]
TOL = 1e-4   # the project's parity bound for gradients against the reference (rel-L2)


def q_names_of(alg_name):
    return ("q1", "q2") if alg_name == "TD3" else ("q",)


def alg_kwargs(meta, use_gpu, **over):
    cfg, lim = meta["cfg"], meta["lim"]
    c = dict(cfg, alg="INFADP", horizon=1)
    kw = dict(algorithm=cfg["alg"], trainer="off_serial_trainer", seed=meta["seed"], cnn_shared=False, env_id=cfg["env_id"],
              obsv_dim=obs_dim_of(c), action_dim=act_dim_of(c), action_type="continu",
              action_low_limit=np.array(lim[0], dtype=np.float32), action_high_limit=np.array(lim[1], dtype=np.float32),
              policy_func_type="MLP", policy_func_name="DetermPolicy", policy_hidden_sizes=list(cfg["hidden"]),
              policy_hidden_activation=cfg["act"], policy_act_distribution="default", policy_learning_rate=1e-3,
              value_func_type="MLP", value_func_name="ActionValue", value_hidden_sizes=list(cfg["hidden"]),
              value_hidden_activation=cfg["act"], value_output_activation="linear", value_learning_rate=1e-3, use_gpu=use_gpu,
              buffer_name="prioritized_replay_buffer" if meta["per"] else "replay_buffer")
    kw.update({k: meta["attrs"][k] for k in ("target_noise", "noise_clip") if k in meta["attrs"]})
    kw.update(over)
    return kw


def load_alg(name, use_gpu=False, prefix="sd/", **over):
    """(alg, fixture, meta): built through create_alg with the fixture's seed (its own RNG draws), attributes set as the maker set
    them, then the fixture's state dict loaded."""
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    alg = create_alg(**alg_kwargs(meta, use_gpu, **over))
    for k, v in meta["attrs"].items():
        if k not in ("target_noise", "noise_clip"):
            setattr(alg, k, v)
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})
    if use_gpu:
        alg.networks.cuda()
    return alg, g, meta


def batch_of(g, prefix="in/"):
    return data_from_golden(g, prefix)


def restate_update(alg, data, dtype=torch.float64):
    """One compute_gradient of DDPG / TD3 restated with autograd on copies of `alg.networks` at `dtype` (on the host):
    dict(backup, a2, q_targ, loss_q [per critic], loss, q_mean, loss_pi, abs_err, grads {net: [tensors]})."""
    import copy
    nets = copy.deepcopy(alg.networks).cpu().to(dtype)
    names = q_names_of(type(alg).__name__)
    d = {k: v.detach().cpu().to(dtype) for k, v in data.items() if k != "idx"}
    for n in names + ("policy",):
        for p in getattr(nets, n).parameters():
            p.requires_grad_(True)
            p.grad = None
    with torch.no_grad():
        a2 = nets.policy_target(d["obs2"])
        if "target_noise" in d and len(names) == 2:
            eps = torch.clamp(d["target_noise"] * alg.target_noise, -alg.noise_clip, alg.noise_clip)
            a2 = torch.clamp(a2 + eps, torch.as_tensor(alg.act_low_limit, dtype=dtype), torch.as_tensor(alg.act_high_limit, dtype=dtype))
        q_t = torch.stack([getattr(nets, f"{n}_target")(d["obs2"], a2) for n in names])
        backup = d["rew"] * getattr(alg, "reward_scale", 1) + alg.gamma * (1 - d["done"]) * q_t.min(dim=0).values
    w = d.get("weight") if alg.per_flag else None
    qs = [getattr(nets, n)(d["obs"], d["act"]) for n in names]
    loss_q = [((q - backup) ** 2).mean() if w is None else (w * (q - backup) ** 2).mean() for q in qs]
    sum(loss_q).backward()
    grads = {n: [p.grad.detach().clone() for p in getattr(nets, n).parameters()] for n in names}
    first = getattr(nets, names[0])
    for p in first.parameters():
        p.requires_grad_(False)
    loss_pi = -first(d["obs"], nets.policy(d["obs"])).mean()
    loss_pi.backward()
    grads["policy"] = [p.grad.detach().clone() for p in nets.policy.parameters()]
    return dict(backup=backup, a2=a2, q_targ=q_t, loss_q=[l.detach() for l in loss_q], loss=sum(loss_q).detach(), q_mean=qs[0].mean().detach(),
                loss_pi=loss_pi.detach(), abs_err=(qs[0] - backup).abs().detach(), grads=grads)
