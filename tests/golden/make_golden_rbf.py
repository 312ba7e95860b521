"""Generate the GAUSS (RBF) fixtures (`rbf_features.npz`, `fhadp_rbf_*.npz`, `infadp_rbf_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_rbf.py
Every array written here is an output of the reference's own classes (`gops.apprfunc.gauss`, `gops.algorithm.fhadp.FHADP`,
`gops.algorithm.infadp.INFADP`) on inputs from `gops_amd.utils.synthetic`, built with the helpers of make_golden.py.

Before the reference is called, some PARAMETERS are changed (data, recorded in the fixture's state dict), so that the cases test
something: with the reference's N(0, 1) centres the time coordinate of a FiniteHorizonPolicy is so far from virtual_t = 2, 3, ...
that every kernel underflows to exactly 0 after the first few steps - the time coordinate of every centre is re-drawn uniformly
over [1, H]; and every fourth sigma_square is negated (all stay at |s| >= 0.1), which exercises |s| and sign(s).
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

from gops.apprfunc import gauss as ref_gauss  # noqa: E402
from gops.utils.act_distribution_type import DiracDistribution  # noqa: E402

from gops_amd.utils.synthetic import make_batch  # noqa: E402

from make_golden_poly import infadp_grads, policy_grads  # noqa: E402


def rbf_kwargs(num_kernel, value_hidden=None):
    kw = dict(policy_func_type="GAUSS", policy_num_kernel=num_kernel)
    if value_hidden is not None:
        kw.update(value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=list(value_hidden),
                  value_hidden_activation="elu", value_learning_rate=1e-3)
    return kw


def lq(config, batch, horizon, alg="FHADP", gamma=1.0):
    return dict(alg=alg, env_id="pyth_lq", lq_config=config, batch=batch, horizon=horizon, hidden=(), act="linear", gamma=gamma)


# name: (cfg, extra kwargs of the algorithm)
FHADP_CASES = {
    "fhadp_rbf_lqs2a1_k35_h20": (lq("s2a1", 64, 20), rbf_kwargs(35)),
    "fhadp_rbf_lqs6a3_k64_h10": (lq("s6a3", 80, 10, gamma=0.99), rbf_kwargs(64)),   # the bound case: input width 7, A = 3
    "fhadp_rbf_idp_k8_h20": (dict(alg="FHADP", env_id="pyth_idpendulum", batch=64, horizon=20, hidden=(), act="linear", gamma=1.0),
                             rbf_kwargs(8)),
    # (H = 6: over the POLY case's 20 steps this rollout leaves the neighbourhood of its three centres and only b keeps a gradient)
    "fhadp_rbf_lqs3a1_k3_obsscale_repeat2": (lq("s3a1", 48, 6),
                                             dict(rbf_kwargs(3), obs_scale=[1, 2, 0.5], repeat_num=2, reward_scale=0.5, reward_shift=1.0)),
}
INFADP_CASES = {
    "infadp_rbf_lqs4a2_k35": (lq("s4a2", 64, 1, "INFADP", 0.99), dict(rbf_kwargs(35, (64, 64)), reward_scale=0.1)),
    "infadp_rbf_lqs4a2_k35_fs5": (lq("s4a2", 64, 5, "INFADP", 0.99), dict(rbf_kwargs(35, (64, 64)), reward_scale=0.1)),
}


def retouch(alg, cfg, seed):
    """The parameter changes of the module docstring, on the online policy (and INFADP's target copy alike)."""
    g = torch.Generator().manual_seed(seed + 2000)
    nets = [alg.networks.policy] + ([alg.networks.policy_target] if hasattr(alg.networks, "policy_target") else [])
    K = nets[0].pi.C.shape[1]
    t_col = 1.0 + (cfg["horizon"] - 1.0) * torch.rand(K, generator=g)
    with torch.no_grad():
        for net in nets:
            if cfg["alg"] == "FHADP":
                net.pi.C[0, :, -1] = t_col
            net.pi.sigma_square[0, ::4] *= -1.0
    assert float(nets[0].pi.sigma_square.abs().min()) >= 0.1


def golden_features():
    """The reference modules' outputs on random inputs: DetermPolicy (K = 1, K = 35) with asymmetric limits, FiniteHorizonPolicy at two
    virtual times; with the state dict, i.e. what the seed draws."""
    g = torch.Generator().manual_seed(7)
    out = {}
    lim = dict(act_high_lim=np.array([1.0, 3.0], dtype=np.float32), act_low_lim=np.array([-2.0, 0.5], dtype=np.float32),
               action_distribution_cls=DiracDistribution)
    cases = [("determ_k1", ref_gauss.DetermPolicy, 4, 1), ("determ_k35", ref_gauss.DetermPolicy, 4, 35),
             ("fh_k3", ref_gauss.FiniteHorizonPolicy, 3, 3)]
    for name, cls, n, K in cases:
        seed = zlib.crc32(name.encode()) % 1000
        torch.manual_seed(seed)
        net = cls(obs_dim=n, act_dim=2, num_kernel=K, **lim)
        x = torch.randn(32, n, generator=g)
        out[f"{name}/obs"] = x.numpy()
        out[f"{name}/seed"] = np.int64(seed)
        out.update({f"{name}/sd/{k}": v.detach().numpy() for k, v in net.state_dict().items()})
        if cls is ref_gauss.FiniteHorizonPolicy:
            for t in (1, 7):
                out[f"{name}/out_t{t}"] = net(x, t).detach().numpy()
        else:
            out[f"{name}/out"] = net(x).detach().numpy()
    mg.save("rbf_features", **out)


def golden_algs(only=()):
    for name, (cfg, extra) in {**FHADP_CASES, **INFADP_CASES}.items():
        if only and name not in only:
            continue
        seed = zlib.crc32(name.encode()) % 1000
        alg = mg.build_alg(cfg, seed, **extra)
        retouch(alg, cfg, seed)
        data = make_batch(cfg, seed)
        if "idp" in name:
            data["obs"][:5, 1] = 0.9  # some trajectories fall over within the horizon
            data["obs2"] = data["obs"].clone()
        data["done"][-3:] = 1.0
        out = {"in/" + k: v.numpy().copy() for k, v in data.items()}
        out["meta/cfg"] = json.dumps(dict(cfg=cfg, extra=extra, seed=seed))
        out.update(mg.model_consts(alg.envmodel))
        if cfg["alg"] == "FHADP":
            out.update({k: v.copy() for k, v in mg.sd_to_np(alg.networks.state_dict()).items()})
            policy_grads(alg, data, out)
        else:
            mg.perturb_targets(alg, seed)
            out.update({k: v.copy() for k, v in mg.sd_to_np(alg.networks.state_dict()).items()})
            infadp_grads(alg, data, out)
        mg.save(name, **out)


def golden_updates():
    """Weights after five reference `_local_update` calls (Adam included) of the s2a1 case on fixed batches."""
    name = "fhadp_rbf_lqs2a1_5updates"
    cfg, extra = FHADP_CASES["fhadp_rbf_lqs2a1_k35_h20"]
    seed = zlib.crc32(name.encode()) % 1000
    alg = mg.build_alg(cfg, seed, **extra)
    retouch(alg, cfg, seed)
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
    if not only or "golden_features" in only:
        golden_features()
    if not only or "golden_algs" in only or only & set({**FHADP_CASES, **INFADP_CASES}):
        golden_algs(only & set({**FHADP_CASES, **INFADP_CASES}))
    if not only or "golden_updates" in only:
        golden_updates()
