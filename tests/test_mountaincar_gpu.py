"""GPU: gym_mountaincarconti on the kernels - `gops_env_step` row by row, the MLP rollouts one trajectory at a time (in the manner of
tests/test_per_trajectory_gpu.py), the reference's FHADP / INFADP / POLY / GAUSS fixtures through `create_alg`, bit-identical launches.

Yardstick: the host model in float64 under autograd (tests/mcar_common.py).  Rows that pass within 1e-5 of a threshold in the
float64 run are left out of a comparison (the branch-margin rule there; tests/test_mountaincar_cpu.py asserts the premises of every
batch used here without a device).

Tolerances of the per-trajectory comparisons: for each compared tensor the SAME launch is made with gym_pendulum (same shapes, nets
drawn from the same seed, the oracle's float64 evaluation as its yardstick) in the same test; the new kind is allowed twice the
pendulum kernels' error and not less than 4 fp32 ulp, both as max |error| over the largest compared magnitude.  Both numbers are
printed.  Measured on an MI355X: DESIGN.md, the gym_mountaincarconti subsection."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import (data_from_golden, flat_grads, hip_env_from_oracle, hip_mlp_from_net, one_row_gradients_f64, reference_init_nets,
                     to_device, weighted_gradient_f64)
from oracle import adp_oracle as orc

import mcar_common as mc
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.utils.synthetic import make_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4
ULP4 = 4 * 2.0 ** -23
STREAMED_FP32 = 0x10   # GOPS_VF_STREAMED_FP32
TILE = 16

# name: batch, horizon, hidden, act, gamma, variant flags, wrapper options
CASES = {
    "default_256_b70": dict(batch=70, horizon=10, hidden=(256, 256), act="gelu", gamma=0.99, flags=0, extra={}),
    "fp32_256_b70": dict(batch=70, horizon=10, hidden=(256, 256), act="gelu", gamma=0.99, flags=STREAMED_FP32, extra={}),
    "default_64_b17_nomask": dict(batch=17, horizon=8, hidden=(64, 64), act="elu", gamma=1.0, flags=0, extra=dict(mask_at_done=False)),
    "fp32_64_b17": dict(batch=17, horizon=8, hidden=(64, 64), act="elu", gamma=1.0, flags=STREAMED_FP32, extra={}),
    "repeat2_32_b70": dict(batch=70, horizon=8, hidden=(32, 32), act="tanh", gamma=0.97, flags=0, extra=dict(repeat_num=2)),
}
SEED = 5
_PREPARED = {}


def make_gv(B, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(B, generator=gen) * 10 ** (-3 * torch.rand(B, generator=gen)) / B


def edge_rows(B):
    """First / last row of the first tile, across the first tile edge, the ragged last tile's first and last row."""
    last = (B - 1) // TILE * TILE
    return sorted({0, min(TILE - 1, B - 1), min(TILE, B - 1), last, B - 1})


def prepare(name):
    """A case's inputs and float64 results, mountaincar and its pendulum twin (no GPU)."""
    if name in _PREPARED:
        return _PREPARED[name]
    c = CASES[name]
    B, H, extra = c["batch"], c["horizon"], c["extra"]
    cfg = dict(alg="FHADP", env_id=mc.ENV_ID, batch=B, horizon=H, hidden=c["hidden"], act=c["act"], gamma=c["gamma"])
    data, crafted = mc.crafted_batch(B, SEED)
    model = create_env_model(mc.ENV_ID, **extra)
    policy = reference_init_nets(cfg, SEED, 2, 1)["policy"]
    kw = dict(finite_horizon=True, mask_at_done=extra.get("mask_at_done", True), repeat_num=extra.get("repeat_num") or 1)
    p64 = mc.net_as(policy, torch.float64)
    gv = make_gv(B, SEED)
    ref = mc.weighted_gradient(model, p64, data, H, c["gamma"], gv, **kw)
    rows = sorted(set(edge_rows(B)) | {r for r in crafted if r // TILE in (0, (B - 1) // TILE)})
    rows = [r for r in rows if not bool(ref["left_out"][r])]
    rows64 = mc.one_row_gradients(model, mc.net_as(policy, torch.float64), data, H, c["gamma"], rows, **kw)
    # the pendulum twin: same shapes, nets from the same seed, the oracle in float64
    pcfg = dict(cfg, env_id="gym_pendulum")
    penv = orc.make_env("gym_pendulum", repeat_num=extra.get("repeat_num"), mask_at_done=extra.get("mask_at_done", True))
    pdata = make_batch(pcfg, SEED)
    pdata["done"] = data["done"].clone()
    ppol = reference_init_nets(pcfg, SEED, 3, 1)["policy"]
    pref = weighted_gradient_f64(penv, ppol, pdata, H, c["gamma"], True, gv)
    prows64 = one_row_gradients_f64(penv, ppol, pdata, H, c["gamma"], True, rows)
    out = dict(case=c, cfg=cfg, data=data, crafted=crafted, model=model, policy=policy, gv=gv, ref=ref, rows=rows, rows64=rows64,
               pend=dict(env=penv, data=pdata, policy=ppol, ref=pref, rows64=prows64))
    _PREPARED[name] = out
    return out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


# ---- gops_env_step ---------------------------------------------------------------------------------------------------------------
STEP_B = 70


def step_batch():
    data, rows = mc.crafted_batch(STEP_B, 9)
    gen = torch.Generator().manual_seed(99)
    data["act"] = torch.rand(STEP_B, 1, generator=gen) * 2.6 - 1.3   # beyond [-1, 1]: ClipAction at work
    return data, rows


def step_yardstick(data):
    """The wrapped step (default chain) on the host model in float64, with the branches of every row."""
    base = create_env_model(mc.ENV_ID).unwrapped
    x, a = data["obs"].double(), data["act"].double().clamp(-1.0, 1.0)
    tr = mc.trace_step(x, a[:, 0])
    xn, r, dm, _ = base.forward(x, a, None, {})
    d = data["done"] != 0
    tr.update(obs=torch.where(d.unsqueeze(1), x, xn), rew=torch.where(d, torch.zeros_like(r), r), next_done=d | dm, entry=d)
    return tr


def test_env_step_row_by_row(dev):
    from gops_amd import hip_backend as hb
    data, rows = step_batch()
    want = step_yardstick(data)
    env = create_env_model(mc.ENV_ID).hip_env()
    B, PAD = STEP_B, 32   # sentinels behind the outputs
    nobs = torch.full((B + PAD, 2), 7.5, device=dev)
    io_in = to_device(dict(obs=data["obs"], act=data["act"], done=data["done"]), dev)
    o, r, d, _ = hb.env_step(env, io_in["obs"], io_in["act"], io_in["done"], {})
    o2, r2, d2, _ = hb.env_step(env, io_in["obs"], io_in["act"], io_in["done"], {})
    assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2)
    # the same launch into buffers with sentinels behind them (the ABI call itself)
    rew, nd = torch.full((B + PAD,), 7.5, device=dev), torch.full((B + PAD,), 7.5, device=dev)
    io = hb.GopsStepIO()
    io.obs, io.action, io.done = io_in["obs"].data_ptr(), io_in["act"].data_ptr(), io_in["done"].data_ptr()
    io.next_obs, io.reward, io.next_done = nobs.data_ptr(), rew.data_ptr(), nd.data_ptr()
    assert hb.lib().gops_env_step(ctypes.byref(env), B, ctypes.byref(io), None) == 0
    torch.cuda.synchronize()
    assert bool((nobs[B:] == 7.5).all()) and bool((rew[B:] == 7.5).all()) and bool((nd[B:] == 7.5).all())
    assert torch.equal(nobs[:B], o) and torch.equal(rew[:B], r)
    o, r, d = o.cpu().double(), r.cpu().double(), d.cpu()
    keep = ~want["near"] | want["entry"]
    assert int((~keep).sum()) <= mc.MAX_LEFT_OUT * B and bool(keep[list(rows)].all())
    assert np.array_equal((d != 0).numpy()[keep], want["next_done"].numpy()[keep])
    live = ~want["entry"]
    decided_v = live & (want["speed_clamp_above"] | want["speed_clamp_below"] | want["left_wall"])
    decided_p = live & (want["left_wall"] | want["right_bound"] | (want["obs"][:, 0] == mc.P_MIN))
    assert torch.equal(o[decided_v, 1], want["obs"][decided_v, 1]) and torch.equal(o[decided_p, 0], want["obs"][decided_p, 0])
    assert torch.equal(o[want["entry"]], data["obs"][want["entry"]].double()) and not bool(r[want["entry"]].any())
    err_p = float((o[keep, 0] - want["obs"][keep, 0]).abs().max())
    err_v = float((o[keep, 1] - want["obs"][keep, 1]).abs().max())
    err_r = float((r[keep] - want["rew"][keep]).abs().max())
    print(f"env_step: |pos' error| {err_p:.3e} (bound {ULP4 * 1.2:.3e}), |vel' error| {err_v:.3e} (bound {ULP4 * 0.07:.3e}), "
          f"|reward error| {err_r:.3e} (bound {ULP4 * 100:.3e})")
    assert err_p <= ULP4 * 1.2 and err_v <= ULP4 * 0.07 and err_r <= ULP4 * 100.0


# ---- rollouts, one trajectory at a time ------------------------------------------------------------------------------------------
class _Launch:
    def __init__(self, henv, policy, c, dev):
        from gops_amd import hip_backend as hb
        self.hb, self.dev, self.c = hb, dev, c
        self.pol, self.ws, self.bs = hip_mlp_from_net(policy, dev)
        self.henv = henv

    def rollout(self, B):
        c = self.c
        return self.hb.Rollout(self.henv, self.pol, batch=B, horizon=c["horizon"], gamma=c["gamma"], finite_horizon=True, need_grad=True,
                               variant_flags=c["flags"])

    def backward(self, ro, gv):
        gw, gb = [torch.full_like(w, float("nan")) for w in self.ws], [torch.full_like(b, float("nan")) for b in self.bs]
        ro.backward(gv.to(self.dev).contiguous(), gw, gb)
        torch.cuda.synchronize()
        return [t.cpu() for pair in zip(gw, gb) for t in pair]


def _err(got, want):
    """max |error| over the largest compared magnitude."""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    den = float(want.abs().max())
    return float((got - want).abs().max()) / (den if den > 0 else 1.0)


def _measure(launch, data, gv, keep, rows, ref, rows64, dev):
    """Every compared tensor's error of one kind: forward values over the kept rows, the weighted gradient, one-hot gradients."""
    B = data["obs"].shape[0]
    ro = launch.rollout(B)
    ro.workspace.fill_(0xFF)
    res = {k: v.cpu() for k, v in ro.forward(to_device(data, dev), want_rewards=True, want_final=True).items()}
    m = dict(v_pi=_err(res["v_pi"][keep], ref["v"][keep]), rewards=_err(res["rewards"][:, keep], ref["rewards"][:, keep]),
             final_obs=_err(res["final_obs"][keep], ref["final_obs"][keep]))
    g1 = launch.backward(ro, torch.where(keep, gv, torch.zeros_like(gv)))
    assert all(torch.isfinite(g).all() for g in g1)
    m["grad_weighted"] = _err(flat_grads(g1), flat_grads(ref["grads"]))
    worst = 0.0
    for i in rows:
        hot = torch.zeros(B)
        hot[i] = 1.0
        gi = launch.backward(ro, hot)
        if data["done"][i] != 0 and launch.henv.no_mask_at_done == 0:
            assert all(float(g.abs().max()) == 0.0 for g in gi), (i, "a row that is done on entry has a gradient")
            continue
        worst = max(worst, _err(flat_grads(gi), flat_grads(rows64[i])))
    m["grad_one_row"] = worst
    return m, res, g1, ro


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_per_trajectory(name, dev):
    prep = prepare(name)
    c, data, ref, gv, rows = prep["case"], prep["data"], prep["ref"], prep["gv"], prep["rows"]
    B, H = c["batch"], c["horizon"]
    keep = ~ref["left_out"]
    mc.check_premises(name, ref, prep["crafted"])
    masked = c["extra"].get("mask_at_done", True)
    # the pendulum kernels' own error at these shapes: what the bounds come from
    pend = prep["pend"]
    pl = _Launch(hip_env_from_oracle(pend["env"], pend["policy"]), pend["policy"], c, dev)
    pm, _, _, _ = _measure(pl, pend["data"], gv, torch.ones(B, dtype=torch.bool), rows, pend["ref"], pend["rows64"], dev)
    henv = prep["model"].hip_env(policy_low=prep["policy"]["act_low"], policy_high=prep["policy"]["act_high"])
    launch = _Launch(henv, prep["policy"], c, dev)
    m, res, g1, ro = _measure(launch, data, gv, keep, rows, ref, prep["rows64"], dev)
    # exact parts
    assert np.array_equal(res["final_done"].numpy()[keep] != 0, ref["final_done"].numpy()[keep])
    entry = (data["done"] != 0).nonzero().flatten().tolist()
    if masked:
        assert torch.equal(res["rewards"][:, entry], torch.zeros(H, len(entry))) and torch.equal(res["final_obs"][entry], data["obs"][entry])
        for r in (ref["first_done"] >= 0).nonzero().flatten().tolist():
            if keep[r] and r not in entry:
                t = int(ref["first_done"][r])
                assert torch.equal(res["rewards"][t + 1:, r], torch.zeros(H - t - 1)), r
    bounds = {k: max(2 * pm[k], ULP4) for k in m}
    for k in m:
        print(f"{name}: {k}: mountaincar {m[k]:.3e}, pendulum {pm[k]:.3e}, bound {bounds[k]:.3e}")
    # two launches give identical bits
    res2 = {k: v.cpu() for k, v in ro.forward(to_device(data, dev), want_rewards=True, want_final=True).items()}
    g2 = launch.backward(ro, torch.where(keep, gv, torch.zeros_like(gv)))
    assert all(torch.equal(res[k], res2[k]) for k in res) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    # rows beyond the batch are inert
    extra = TILE + 3
    pad, _ = mc.crafted_batch(B + extra, SEED + 1)
    for k in ("obs", "done"):
        pad[k][:B] = data[k]
    pad["obs"][B:] *= 1.5
    ro_n = launch.rollout(B + extra)
    ro_n.workspace.random_(0, 256)
    out = ro_n.forward(to_device(pad, dev), want_rewards=True, want_final=True)
    assert torch.equal(out["v_pi"][:B].cpu(), res["v_pi"]) and torch.equal(out["rewards"][:, :B].cpu(), res["rewards"])
    gp = launch.backward(ro_n, torch.cat((torch.where(keep, gv, torch.zeros_like(gv)), torch.zeros(extra))))
    assert _err(flat_grads(gp), flat_grads(g1)) <= max(bounds["grad_weighted"], ULP4)
    for k in m:
        assert m[k] <= bounds[k], (name, k, m[k], pm[k], bounds[k])


# ---- the reference's fixtures through create_alg ---------------------------------------------------------------------------------
def _load_alg(name):
    from test_poly_gpu import _kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    g = load_golden(name)
    meta = golden_meta(g)
    cfg = meta["cfg"]
    kw = _kwargs(cfg, meta["extra"], meta["seed"])
    if "policy_func_type" not in kw:
        kw.update(policy_func_type="MLP", policy_hidden_sizes=list(cfg["hidden"]), policy_hidden_activation=cfg["act"])
        if cfg["alg"] == "INFADP":
            kw.update(value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=list(cfg["hidden"]),
                      value_hidden_activation=cfg["act"], value_learning_rate=1e-3)
    alg = create_alg(**kw)
    alg.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")})
    alg.networks.cuda()
    alg.gamma = cfg["gamma"]
    if cfg["alg"] == "INFADP":
        alg.forward_step = cfg["horizon"]
    return alg, g, cfg


def _close(got, want):
    return abs(float(got) - float(want)) <= TOL * max(1.0, abs(float(want)))


@pytest.mark.parametrize("name, rollout_cls", [("fhadp_mountaincar_gelu", "Rollout"), ("fhadp_mountaincar_poly_d2", "PolyRollout"),
                                               ("fhadp_mountaincar_rbf_k16", "RbfRollout")])
def test_fhadp_fixture_through_create_alg(name, rollout_cls, dev):
    from gops_amd import hip_backend as hb
    alg, g, cfg = _load_alg(name)
    tb, info = alg.get_remote_update_info(data_from_golden(g), 0)
    assert _close(tb["Loss/Actor loss-RL iter"], g["loss"])
    assert len(info["grad"]) == len(list(alg.networks.policy.parameters()))
    for i, gr in enumerate(info["grad"]):
        e = rel_l2(gr.cpu(), g[f"grad/{i}"])
        print(f"{name}: grad/{i} rel-L2 {e:.2e}")
        assert e < TOL, i
    assert alg._rollouts and all(type(ro) is getattr(hb, rollout_cls) for ro in alg._rollouts.values())


def test_infadp_fixture_through_create_alg(dev):
    alg, g, cfg = _load_alg("infadp_mountaincar_elu")
    data = data_from_golden(g)
    tb, info = alg.get_remote_update_info(data, 0)       # PEV
    assert _close(tb["Loss/Critic loss-RL iter"], g["pev_loss"]) and _close(tb["Train/Critic avg value-RL iter"], g["pev_vmean"])
    for i, gr in enumerate(info["v"]):
        assert rel_l2(gr.cpu(), g[f"pev_grad/{i}"]) < TOL, i
    tb, info = alg.get_remote_update_info(data, 1)       # PIM
    assert _close(tb["Loss/Actor loss-RL iter"], g["pim_loss"])
    for i, gr in enumerate(info["policy"]):
        assert rel_l2(gr.cpu(), g[f"pim_grad/{i}"]) < TOL, i


def test_device_env_sampler_steps_the_model(dev):
    """DeviceEnvSampler(env_step="model") drives gops_env_step with the new kind from gym's own reset states."""
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    alg, g, cfg = _load_alg("infadp_mountaincar_elu")
    s = DeviceEnvSampler(dict(env_id=mc.ENV_ID), alg.envmodel, n_envs=64, steps_per_sample=3, max_episode_steps=50, seed=2, env_step="model")
    s.networks = alg.networks
    first = s.obs.cpu()
    assert float(first[:, 0].min()) >= -0.6 and float(first[:, 0].max()) <= -0.4 and not first[:, 1].any()
    batch, _ = s.sample()
    obs, obs2 = batch["obs"].cpu(), batch["obs2"].cpu()
    assert obs.shape == (192, 2) and torch.isfinite(obs2).all() and torch.isfinite(batch["rew"]).all()
    assert float(obs2[:, 0].min()) >= mc.P_MIN and float(obs2[:, 0].max()) <= mc.P_MAX and float(obs2[:, 1].abs().max()) <= mc.V_MAX
    assert bool((obs2 != obs).any())
    with pytest.raises(RuntimeError, match="is not restated in the step kernel"):
        DeviceEnvSampler(dict(env_id=mc.ENV_ID), alg.envmodel, n_envs=4, env_step="data")
