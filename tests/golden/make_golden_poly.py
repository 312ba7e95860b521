"""Generate the POLY fixtures (`poly_*.npz`, `fhadp_poly_*.npz`, `infadp_*poly*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_poly.py
Every array written here is an output of the reference's own classes (`gops.apprfunc.poly`, `gops.algorithm.fhadp.FHADP`,
`gops.algorithm.infadp.INFADP`) on inputs from `gops_amd.utils.synthetic`, built with the helpers of make_golden.py.
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)

from gops.apprfunc import poly as ref_poly  # noqa: E402
from gops.utils.act_distribution_type import DiracDistribution  # noqa: E402

from gops_amd.utils.synthetic import make_batch  # noqa: E402


def poly_kwargs(policy_degree, policy_bias, value_degree=None, value_bias=False, norm_matrix=None):
    kw = dict(policy_func_type="POLY", policy_degree=policy_degree, policy_add_bias=policy_bias)
    if value_degree is not None:
        kw.update(value_func_type="POLY", value_func_name="StateValue", value_degree=value_degree, value_add_bias=value_bias,
                  value_learning_rate=3e-4)
    if norm_matrix is not None:
        kw["norm_matrix"] = norm_matrix
    return kw


# name: (cfg, extra kwargs of the algorithm)
FHADP_CASES = {
    # example_train/fhadp/fhadp_poly_lqs2a1_serial.py: FiniteHorizonPolicy degree 1, no bias, H = 80, B = 64
    "fhadp_poly_lqs2a1_h80": (dict(alg="FHADP", env_id="pyth_lq", lq_config="s2a1", batch=64, horizon=80, hidden=(), act="linear",
                                   gamma=1.0), poly_kwargs(1, False)),
    "fhadp_poly_lqs6a3_d2_bias_h30": (dict(alg="FHADP", env_id="pyth_lq", lq_config="s6a3", batch=80, horizon=30, hidden=(),
                                           act="linear", gamma=0.99), poly_kwargs(2, True)),
    "fhadp_poly_idp_d1_bias_h20": (dict(alg="FHADP", env_id="pyth_idpendulum", batch=64, horizon=20, hidden=(), act="linear",
                                        gamma=1.0), poly_kwargs(1, True)),
    "fhadp_poly_lqs3a1_obsscale_repeat2": (dict(alg="FHADP", env_id="pyth_lq", lq_config="s3a1", batch=48, horizon=20, hidden=(),
                                                act="linear", gamma=1.0),
                                           dict(poly_kwargs(1, False), obs_scale=[1, 2, 0.5], repeat_num=2, reward_scale=0.5,
                                                reward_shift=1.0)),
}
INFADP_CASES = {   # example_train/infadp/infadp_poly_lqs4a2_offserial.py: policy degree 1, value degree 2, reward_scale 0.1
    "infadp_poly_lqs4a2": (dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=64, horizon=1, hidden=(), act="linear",
                                gamma=0.99), dict(poly_kwargs(1, False, 2, False), reward_scale=0.1)),
    "infadp_poly_lqs4a2_fs5": (dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=64, horizon=5, hidden=(), act="linear",
                                    gamma=0.99), dict(poly_kwargs(1, False, 2, False), reward_scale=0.1)),
}


def policy_grads(alg, data, out):
    alg._compute_gradient(data)
    for i, gr in enumerate(mg.grads_of(alg.networks.policy)):
        out[f"grad/{i}"] = gr.numpy()
    out["loss"] = alg.tb_info["Loss/Actor loss-RL iter"]


def infadp_grads(alg, data, out):
    _, info = alg.get_remote_update_info(data, 0)  # PEV
    for i, gr in enumerate(info["v"]):
        out[f"pev_grad/{i}"] = gr.detach().numpy().copy()
    out["pev_loss"] = alg.tb_info["Loss/Critic loss-RL iter"]
    out["pev_vmean"] = alg.tb_info["Train/Critic avg value-RL iter"]
    _, info = alg.get_remote_update_info(data, 1)  # PIM
    for i, gr in enumerate(info["policy"]):
        out[f"pim_grad/{i}"] = gr.detach().numpy().copy()
    out["pim_loss"] = alg.tb_info["Loss/Actor loss-RL iter"]


def golden_features():
    """The reference modules' outputs on random inputs (policies at several degrees, the value with a non-unit norm_matrix)."""
    g = torch.Generator().manual_seed(7)
    out = {}
    base = dict(act_high_lim=np.ones(2, dtype=np.float32), act_low_lim=-np.ones(2, dtype=np.float32), action_distribution_cls=DiracDistribution)
    cases = [("determ_d1", ref_poly.DetermPolicy, 4, dict(degree=1, add_bias=False)),
             ("determ_d2", ref_poly.DetermPolicy, 4, dict(degree=2, add_bias=True)),
             ("determ_d3", ref_poly.DetermPolicy, 3, dict(degree=3, add_bias=False)),
             ("fh_d1_bias", ref_poly.FiniteHorizonPolicy, 3, dict(degree=1, add_bias=True))]
    for name, cls, n, kw in cases:
        torch.manual_seed(zlib.crc32(name.encode()) % 1000)
        net = cls(obs_dim=n, act_dim=2, **base, **kw)
        x = torch.randn(32, n, generator=g)
        out[f"{name}/obs"] = x.numpy()
        out.update({f"{name}/sd/{k}": v.detach().numpy() for k, v in net.state_dict().items()})
        if cls is ref_poly.FiniteHorizonPolicy:
            for t in (1, 37):
                out[f"{name}/out_t{t}"] = net(x, t).detach().numpy()
        else:
            out[f"{name}/out"] = net(x).detach().numpy()
    for name, bias, norm in (("value_nobias", False, [1.0, 0.5, 2.0, 0.25]), ("value_bias", True, None)):
        torch.manual_seed(zlib.crc32(name.encode()) % 1000)
        net = ref_poly.StateValue(obs_dim=4, degree=2, add_bias=bias, norm_matrix=norm, action_distribution_cls=DiracDistribution)
        x = torch.randn(32, 4, generator=g)
        out[f"{name}/obs"] = x.numpy()
        out[f"{name}/norm"] = np.asarray([1.0] * 4 if norm is None else norm, dtype=np.float32)
        out.update({f"{name}/sd/{k}": v.detach().numpy() for k, v in net.state_dict().items()})
        out[f"{name}/out"] = net(x).detach().numpy()
    mg.save("poly_features", **out)


def golden_algs():
    for name, (cfg, extra) in {**FHADP_CASES, **INFADP_CASES}.items():
        seed = zlib.crc32(name.encode()) % 1000
        alg = mg.build_alg(cfg, seed, **extra)
        data = make_batch(cfg, seed)
        if "idp" in name:
            data["obs"][:5, 1] = 0.9  # some trajectories fall over within the horizon
            data["obs2"] = data["obs"].clone()
        data["done"][-3:] = 1.0
        out = {"in/" + k: v.numpy().copy() for k, v in data.items()}
        out["meta/cfg"] = json.dumps(dict(cfg=cfg, extra=extra, seed=seed))
        out.update(mg.model_consts(alg.envmodel))
        if cfg["alg"] == "FHADP":
            out.update(mg.sd_to_np(alg.networks.state_dict()))
            policy_grads(alg, data, out)
        else:
            mg.perturb_targets(alg, seed)
            out.update(mg.sd_to_np(alg.networks.state_dict()))
            infadp_grads(alg, data, out)
        mg.save(name, **out)


def golden_trained_poly():
    """results/INFADP/lqs4a2_poly/apprfunc/apprfunc_115000_opt.pkl loaded as make_golden.golden_trained() loads the MLP ones."""
    run, ckpt = "INFADP/lqs4a2_poly", "apprfunc_115000_opt.pkl"
    rc = json.load(open(os.path.join(mg.REF_ROOT, "results", run, "config.json")))
    cfg = dict(alg="INFADP", env_id=rc["env_id"], lq_config=rc["lq_config"], hidden=(), act="linear", batch=64,
               horizon=int(rc.get("forward_step", 1) or 1), gamma=0.99)
    extra = dict(poly_kwargs(rc["policy_degree"], rc["policy_add_bias"], rc["value_degree"], rc["value_add_bias"]),
                 reward_scale=rc["reward_scale"])
    lim = dict(action_high_limit=np.array(rc["action_high_limit"], dtype=np.float32),
               action_low_limit=np.array(rc["action_low_limit"], dtype=np.float32))
    name = "infadp_trained_poly_lqs4a2"
    seed = zlib.crc32(name.encode()) % 1000
    alg = mg.build_alg(cfg, seed, **extra, **lim)
    sd = torch.load(os.path.join(mg.REF_ROOT, "results", run, "apprfunc", ckpt), map_location="cpu")
    alg.networks.load_state_dict(sd)
    data = make_batch(cfg, seed)
    data["done"][-2:] = 1.0
    out = {"in/" + k: v.numpy().copy() for k, v in data.items()}
    out["meta/cfg"] = json.dumps(dict(cfg=cfg, extra=extra, seed=seed, lim=[rc["action_low_limit"], rc["action_high_limit"]],
                                      checkpoint=f"results/{run}/apprfunc/{ckpt}"))
    out["meta/sd_keys"] = json.dumps(sorted(sd.keys()))
    out.update(mg.sd_to_np(alg.networks.state_dict()))
    out.update(mg.model_consts(alg.envmodel))
    infadp_grads(alg, data, out)
    mg.save(name, **out)


def golden_updates():
    """Weights after five reference `_local_update` calls (Adam included) of the s2a1 example on fixed batches."""
    name = "fhadp_poly_lqs2a1_5updates"
    cfg, extra = FHADP_CASES["fhadp_poly_lqs2a1_h80"]
    seed = zlib.crc32(name.encode()) % 1000
    alg = mg.build_alg(cfg, seed, **extra)
    out = {"meta/cfg": json.dumps(dict(cfg=cfg, extra=extra, seed=seed))}
    out.update({k: v.copy() for k, v in mg.sd_to_np(alg.networks.state_dict(), "sd0/").items()})   # (views of the parameters otherwise)
    out.update(mg.model_consts(alg.envmodel))
    for k in range(5):
        data = make_batch(cfg, seed + k)
        out.update({f"in{k}/" + key: v.numpy().copy() for key, v in data.items()})
        alg._local_update(data, k)
        out[f"loss{k}"] = alg.tb_info["Loss/Actor loss-RL iter"]
    out.update(mg.sd_to_np(alg.networks.state_dict(), "sd5/"))
    mg.save(name, **out)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for fn in (golden_features, golden_algs, golden_trained_poly, golden_updates):
        if not only or fn.__name__ in only:
            fn()
