"""Generate the gym_mountaincarconti fixtures (`step_mountaincar*.npz`, `fhadp_mountaincar_*.npz`, `infadp_mountaincar_*.npz`) by
running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_mountaincar.py
Every array written here is an output of the reference's own classes (`gops.create_pkg.create_env_model.create_env_model`,
`gops.algorithm.fhadp.FHADP`, `gops.algorithm.infadp.INFADP`, the MLP / POLY / GAUSS approximators), built with the helpers of
make_golden.py.

The INPUTS are crafted (tests/mcar_common.py: crafted_batch), not only drawn: gym's own reset (pos ~ U[-0.6, -0.4], vel = 0) never
reaches a clamp within 12 steps.  Every batch holds rows that hit the speed clamp from above and from below, the left wall with a
negative speed, the right bound, that become done inside the horizon, that are done on entry, and rows that do none of these; the
maker replays the reference's rollout, asserts that every population has rows and otherwise moves on to the next seed (as
make_golden_sac.one_update does)."""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (installs the reference import hook)

from gops.create_pkg.create_env_model import create_env_model  # noqa: E402

import mcar_common as mc  # noqa: E402
from make_golden_poly import infadp_grads, policy_grads, poly_kwargs  # noqa: E402
from make_golden_rbf import rbf_kwargs, retouch  # noqa: E402


def case(alg, batch, horizon, hidden, act, gamma):
    return dict(alg=alg, env_id=mc.ENV_ID, batch=batch, horizon=horizon, hidden=hidden, act=act, gamma=gamma)


STEP_CASES = {"step_mountaincar": {}, "step_mountaincar_repeat2_nomask": dict(repeat_num=2, mask_at_done=False)}
ALG_CASES = {   # name: (cfg, extra kwargs of the algorithm)
    "fhadp_mountaincar_gelu": (case("FHADP", 70, 12, (64, 64), "gelu", 1.0), {}),
    "infadp_mountaincar_elu": (case("INFADP", 33, 8, (32, 32), "elu", 0.99), {}),
    "fhadp_mountaincar_poly_d2": (case("FHADP", 48, 10, (), "linear", 0.99), poly_kwargs(2, True)),
    "fhadp_mountaincar_rbf_k16": (case("FHADP", 40, 8, (), "linear", 1.0), rbf_kwargs(16)),
}


def populations(tag, policy, envmodel, data, horizon, finite_horizon):
    """Replays the reference's rollout (its policy, its wrapped model) and sorts the rows into the populations from the recorded
    (state, action) pairs -> ((tag, empty populations) raised as an AssertionError when one has no rows)."""
    o, d, info = data["obs"].clone(), data["done"].clone().bool(), {}
    B = o.shape[0]
    entry = d.clone()
    hit = {k: torch.zeros(B, dtype=torch.bool) for k in ("speed_clamp_above", "speed_clamp_below", "left_wall", "right_bound")}
    first_done = torch.full((B,), -1)
    with torch.no_grad():
        for t in range(horizon):
            a = policy(o, t + 1) if finite_horizon else policy(o)
            tr = mc.trace_step(o.double(), a[:, 0].double().clamp(-1.0, 1.0))
            for k in hit:
                hit[k] |= tr[k] & ~d
            o, _, nd, info = envmodel.forward(o, a, d, info)
            first_done[nd.bool() & ~d & (first_done < 0)] = t
            d = nd.bool()
    pops = dict(hit, done_on_entry=entry, done_inside=(first_done >= 1) & (first_done < horizon - 1) & ~entry)
    pops["none"] = ~entry & (first_done < 0) & ~torch.stack(list(hit.values())).any(0)
    empty = [k for k in mc.POPULATIONS if not bool(pops[k].any())]
    assert not empty, (tag, empty)
    return {k: int(v.sum()) for k, v in pops.items()}


def with_seeds(tag, fn):
    """fn(seed) at the first seed from the tag's checksum on at which every population has rows."""
    base = zlib.crc32(tag.encode()) % 1000
    for seed in range(base, base + 8):
        try:
            return fn(seed)
        except AssertionError as e:
            if not (len(e.args) == 1 and isinstance(e.args[0], tuple) and e.args[0][0] == tag and isinstance(e.args[0][1], list)):
                raise
            print(f"{tag}: seed {seed} leaves {e.args[0][1]} without rows")
    raise AssertionError(tag)


def golden_steps():
    """Six wrapped steps from a crafted batch with actions beyond [-1, 1]; every population is met within them."""
    def one(name, extra, seed):
        B, nsteps = 48, 6
        data, _ = mc.crafted_batch(B, seed)
        model = create_env_model(env_id=mc.ENV_ID, **extra)
        g = torch.Generator().manual_seed(seed + 11)
        acts = [torch.rand(B, 1, generator=g) * 2.6 - 1.3 for _ in range(nsteps)]
        out = {"in/obs": data["obs"].numpy().copy(), "in/done": data["done"].numpy().copy()}
        masked = extra.get("mask_at_done", True)
        o, d = data["obs"], data["done"]
        hit = {k: False for k in ("speed_clamp_above", "speed_clamp_below", "left_wall", "right_bound", "done")}
        for s, a in enumerate(acts):
            x = o.double()
            for _ in range(extra.get("repeat_num") or 1):
                tr = mc.trace_step(x, a[:, 0].double().clamp(-1.0, 1.0))
                live = ~(d != 0) if masked else torch.ones(B, dtype=torch.bool)
                for k in hit:
                    hit[k] = hit[k] or bool((tr[k] & live).any())
                x = mc_next(x, a[:, 0].double().clamp(-1.0, 1.0))
            o, r, d, _ = model.forward(o, a, d, {})
            out[f"s{s}/act"], out[f"s{s}/obs"] = a.numpy(), o.numpy().copy()
            out[f"s{s}/rew"], out[f"s{s}/done"] = r.numpy().copy(), d.numpy().copy()
        empty = [k for k, v in hit.items() if not v]
        assert not empty, (name, empty)
        out["meta/nsteps"] = nsteps
        out["meta/cfg"] = json.dumps(dict(cfg=dict(env_id=mc.ENV_ID), extra=extra, seed=seed))
        mg.save(name, **out)

    def mc_next(x, a):   # float64 next state of the bare model, for the sub-step traces only
        v = (x[:, 1] + 0.0015 * a - 0.0025 * torch.cos(3 * x[:, 0])).clamp(-mc.V_MAX, mc.V_MAX)
        p = (x[:, 0] + v).clamp(mc.P_MIN, mc.P_MAX)
        return torch.stack((p, torch.where((p == mc.P_MIN) & (v < 0), torch.zeros_like(v), v)), 1)

    for name, extra in STEP_CASES.items():
        with_seeds(name, lambda seed: one(name, extra, seed))


def golden_algs(only=()):
    def one(name, cfg, extra, seed):
        alg = mg.build_alg(cfg, seed, **extra)
        if extra.get("policy_func_type") == "GAUSS":
            retouch(alg, cfg, seed)
        fh = cfg["alg"] == "FHADP"
        if not fh:
            mg.perturb_targets(alg, seed)
        data, _ = mc.crafted_batch(cfg["batch"], seed)
        counts = populations(name, alg.networks.policy, alg.envmodel, data, cfg["horizon"], fh)
        out = {"in/" + k: v.numpy().copy() for k, v in data.items()}
        out["meta/cfg"] = json.dumps(dict(cfg=cfg, extra=extra, seed=seed, populations=counts))
        out.update({k: v.copy() for k, v in mg.sd_to_np(alg.networks.state_dict()).items()})
        if fh:
            policy_grads(alg, data, out)
        else:
            infadp_grads(alg, data, out)
        mg.save(name, **out)

    for name, (cfg, extra) in ALG_CASES.items():
        if not only or name in only:
            with_seeds(name, lambda seed: one(name, cfg, extra, seed))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    if not only or "golden_steps" in only:
        golden_steps()
    if not only or "golden_algs" in only or only & set(ALG_CASES):
        golden_algs(only & set(ALG_CASES))
