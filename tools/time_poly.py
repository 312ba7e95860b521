"""Time one POLY update (FHADP s2a1 example: FiniteHorizonPolicy degree 1, H = 80; INFADP s4a2 example: DetermPolicy degree 1 +
StateValue degree 2, forward_step 1) at the example batch (64) and at B = 65 536, with and without HIP-graph replay, next to a
torch-eager autograd rollout of the same POLY net on the same GPU:   python tools/time_poly.py"""
import os
import sys
import time

import torch

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np  # noqa: E402
from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402
from gops_amd.utils.synthetic import act_dim_of, make_batch, obs_dim_of  # noqa: E402


def _kwargs(cfg, extra, seed):
    A = act_dim_of(cfg)
    kw = dict(algorithm=cfg["alg"], trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=cfg["env_id"],
              lq_config=cfg["lq_config"], obsv_dim=obs_dim_of(cfg), action_dim=A, action_type="continu",
              action_high_limit=np.ones(A, dtype=np.float32), action_low_limit=-np.ones(A, dtype=np.float32),
              policy_func_name="FiniteHorizonPolicy" if cfg["alg"] == "FHADP" else "DetermPolicy",
              policy_act_distribution="default", policy_learning_rate=1e-3, use_gpu=True)
    if cfg["alg"] == "FHADP":
        kw["pre_horizon"] = cfg["horizon"]
    kw.update(extra)
    return kw


FH = (dict(alg="FHADP", env_id="pyth_lq", lq_config="s2a1", horizon=80, gamma=1.0),
      dict(policy_func_type="POLY", policy_degree=1, policy_add_bias=False))
INF = (dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", horizon=1, gamma=0.99),
       dict(policy_func_type="POLY", policy_degree=1, policy_add_bias=False, value_func_type="POLY", value_func_name="StateValue",
            value_degree=2, value_add_bias=False, value_learning_rate=3e-4, reward_scale=0.1))


def eager_fhadp_update(alg, data):
    """The reference's FHADP loop restated in torch on the device (pyth_lq with ScaleAction / ClipAction / MaskAtDone), autograd + Adam."""
    env = alg.envmodel.hip_env()
    n, m = env.obs_dim, env.act_dim
    dev = data["obs"].device
    if not hasattr(alg, "_eager"):
        inv = torch.tensor(list(env.lq_inv_IA)[:n * n], device=dev).reshape(n, n)
        Bm = torch.tensor(list(env.lq_B)[:n * m], device=dev).reshape(n, m)
        alg._eager = (inv, Bm, torch.tensor(list(env.lq_Q)[:n], device=dev), torch.tensor(list(env.lq_R)[:m], device=dev),
                      torch.optim.Adam(alg.networks.policy.parameters(), lr=1e-3))
    inv, Bm, Q, R, opt = alg._eager
    lo, hi = torch.tensor(list(env.act_low)[:m], device=dev), torch.tensor(list(env.act_high)[:m], device=dev)
    o, d = data["obs"], data["done"] != 0
    v = torch.zeros(o.shape[0], device=dev)
    for t in range(alg.pre_horizon):
        a = alg.networks.policy(o, t + 1)
        u = (lo + (hi - lo) * (a.clamp(-1, 1) + 1) / 2).clamp(lo, hi)
        r = env.lq_reward_scale * (env.lq_reward_shift - ((Q * o * o).sum(1) + (R * u * u).sum(1)))
        on = (o + env.lq_dt * u @ Bm.T) @ inv.T
        v = v + torch.where(d, torch.zeros_like(r), r) * alg.gamma ** t
        o = torch.where(d[:, None], o, on)
    loss = -v.mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def run(name, cfg, extra, B, steps):
    cfg = dict(cfg, batch=B)
    data = {k: v.cuda() for k, v in make_batch(cfg, 3).items()}
    for mode in ("0", "1"):
        os.environ["GOPS_HIP_GRAPH"] = mode
        torch.manual_seed(0)
        alg = create_alg(**_kwargs(cfg, extra, 0))
        alg.networks.to("cuda")
        if cfg["alg"] == "INFADP":
            alg.forward_step = cfg["horizon"]
        for it in range(20):
            alg.local_update(data, it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(steps):
            alg.local_update(data, 20 + it)
        torch.cuda.synchronize()
        print(f"{name} B={B} GOPS_HIP_GRAPH={mode}: {(time.perf_counter() - t0) / steps * 1e3:.3f} ms per update "
              f"(incl. the log's host sync)")
    if cfg["alg"] == "FHADP":
        torch.manual_seed(0)
        alg = create_alg(**_kwargs(cfg, extra, 0))
        alg.networks.to("cuda")
        for _ in range(5):
            eager_fhadp_update(alg, data).item()
        torch.cuda.synchronize()
        n = max(3, steps // 10)
        t0 = time.perf_counter()
        for _ in range(n):
            eager_fhadp_update(alg, data).item()
        torch.cuda.synchronize()
        print(f"{name} B={B} torch eager autograd: {(time.perf_counter() - t0) / n * 1e3:.3f} ms per update")


if __name__ == "__main__":
    run("FHADP poly s2a1 H=80", *FH, 64, 200)
    run("FHADP poly s2a1 H=80", *FH, 65536, 50)
    run("INFADP poly s4a2 fs=1", *INF, 64, 200)
    run("INFADP poly s4a2 fs=1", *INF, 65536, 50)
