"""GPU: POLY approximators (apprfunc/poly.py) on the one-lane-per-trajectory HIP rollout (csrc/rollout_poly.hip), through
`create_alg(...)` and `hb.PolyRollout` / `hb.PolyValueNet`, against the reference fixtures of tests/golden/make_golden_poly.py."""
import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import data_from_golden, hip_env_from_oracle, to_device
from oracle import adp_oracle as orc

from gops_amd import hip_backend as hb
from gops_amd.algorithm.base import poly_grad_buffers
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.utils.synthetic import act_dim_of, make_batch, obs_dim_of

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _kwargs(cfg, extra, seed, lim=None):
    A = act_dim_of(cfg)
    lo, hi = (-np.ones(A, dtype=np.float32), np.ones(A, dtype=np.float32)) if lim is None else \
        (np.array(lim[0], dtype=np.float32), np.array(lim[1], dtype=np.float32))
    kw = dict(algorithm=cfg["alg"], trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=cfg["env_id"],
              obsv_dim=obs_dim_of(cfg), action_dim=A, action_type="continu", action_high_limit=hi, action_low_limit=lo,
              policy_func_name="FiniteHorizonPolicy" if cfg["alg"] == "FHADP" else "DetermPolicy",
              policy_act_distribution="default", policy_learning_rate=1e-3, use_gpu=True)
    if cfg["alg"] == "FHADP":
        kw["pre_horizon"] = cfg.get("pre_horizon", cfg["horizon"])
    if "lq_config" in cfg:
        kw["lq_config"] = cfg["lq_config"]
    kw.update(extra)
    return kw


def _load_alg(name):
    g = load_golden(name)
    meta = golden_meta(g)
    cfg = meta["cfg"]
    alg = create_alg(**_kwargs(cfg, meta["extra"], meta["seed"], meta.get("lim")))
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")}
    alg.load_state_dict(sd)
    alg.networks.cuda()
    alg.gamma = cfg["gamma"]
    if cfg["alg"] == "INFADP":
        alg.forward_step = cfg["horizon"]
    return alg, g, cfg


def _close(got, want):
    return abs(float(got) - float(want)) <= TOL * max(1.0, abs(float(want)))


@pytest.mark.parametrize("name", ["fhadp_poly_lqs2a1_h80", "fhadp_poly_lqs6a3_d2_bias_h30", "fhadp_poly_idp_d1_bias_h20",
                                  "fhadp_poly_lqs3a1_obsscale_repeat2"])
def test_fhadp_poly_matches_reference(name):
    alg, g, cfg = _load_alg(name)
    assert isinstance(next(iter(alg._rollouts.values()), None), (type(None), hb.PolyRollout))
    tb, info = alg.get_remote_update_info(data_from_golden(g), 0)
    assert _close(tb["Loss/Actor loss-RL iter"], g["loss"])
    assert len(info["grad"]) == len(list(alg.networks.policy.parameters()))
    for i, gr in enumerate(info["grad"]):
        assert rel_l2(gr.cpu(), g[f"grad/{i}"]) < TOL, i
    assert all(isinstance(ro, hb.PolyRollout) for ro in alg._rollouts.values())


@pytest.mark.parametrize("name", ["infadp_poly_lqs4a2", "infadp_poly_lqs4a2_fs5", "infadp_trained_poly_lqs4a2"])
def test_infadp_poly_matches_reference(name):
    alg, g, cfg = _load_alg(name)
    data = data_from_golden(g)
    tb, info = alg.get_remote_update_info(data, 0)       # PEV
    assert _close(tb["Loss/Critic loss-RL iter"], g["pev_loss"])
    assert _close(tb["Train/Critic avg value-RL iter"], g["pev_vmean"])
    for i, gr in enumerate(info["v"]):
        assert rel_l2(gr.cpu(), g[f"pev_grad/{i}"]) < TOL, i
    tb, info = alg.get_remote_update_info(data, 1)       # PIM
    assert _close(tb["Loss/Actor loss-RL iter"], g["pim_loss"])
    for i, gr in enumerate(info["policy"]):
        assert rel_l2(gr.cpu(), g[f"pim_grad/{i}"]) < TOL, i


def test_fhadp_poly_five_updates_match_reference():
    """Five `local_update` calls (Adam included; eager, then captured / replayed under the default graph policy) land on the
    reference's weights."""
    g = load_golden("fhadp_poly_lqs2a1_5updates")
    meta = golden_meta(g)
    cfg = meta["cfg"]
    alg = create_alg(**_kwargs(cfg, meta["extra"], meta["seed"]))
    alg.load_state_dict({k[4:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd0/")})
    alg.networks.cuda()
    alg.gamma = cfg["gamma"]
    for k in range(5):
        tb = alg.local_update(data_from_golden(g, f"in{k}/"), k)
        assert _close(tb["Loss/Actor loss-RL iter"], g[f"loss{k}"]), k
    for key, p in alg.networks.state_dict().items():
        want = g["sd5/" + key]
        assert rel_l2(p.cpu().double(), want) < TOL, key


def _poly_rollout(alg, B, device="cuda"):
    return alg._rollout_for(B, torch.device(device))


@pytest.mark.parametrize("B", [1, 300])
def test_poly_gradient_is_bitwise_reproducible(B):
    alg, g, cfg = _load_alg("fhadp_poly_lqs6a3_d2_bias_h30")
    data = {k: v.cuda() for k, v in make_batch(dict(cfg, batch=B), 11).items()}
    ro = _poly_rollout(alg, B)
    gv = torch.full((B,), -1.0 / B, device="cuda")
    outs = []
    for _ in range(2):
        res = ro.forward(data, want_rewards=True, want_final=True)
        gw = [torch.empty_like(alg.networks.policy.pi.weight)]
        gb = [torch.empty_like(alg.networks.policy.pi.bias)]
        ro.backward(gv, gw, gb)
        torch.cuda.synchronize()
        outs.append((res["v_pi"].clone(), gw[0].clone(), gb[0].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][1]).all() and outs[0][1].abs().sum() > 0


def test_poly_batch_slices_are_independent_and_gradients_add_up():
    """Large batch (B = 65 536, H = 80, the s2a1 example's net): each trajectory's return is computed by its own lane, so a slice
    of the batch run on its own gives the same bits; the full gradient is the sum of the slices' gradients."""
    alg, g, cfg = _load_alg("fhadp_poly_lqs2a1_h80")
    B = 65536
    data = {k: v.cuda() for k, v in make_batch(dict(cfg, batch=B), 3).items()}
    ro = _poly_rollout(alg, B)
    v_full = ro.forward(data, want_final=True)["v_pi"]
    W = alg.networks.policy.pi.weight
    gw = [torch.empty_like(W)]
    ro.backward(torch.full((B,), 1.0, device="cuda"), gw, [None])
    S = 4096
    acc = torch.zeros_like(W, dtype=torch.float64)
    ro_s = _poly_rollout(alg, S)
    for s0 in range(0, B, S):
        sl = {k: v[s0:s0 + S].contiguous() for k, v in data.items()}
        v_s = ro_s.forward(sl)["v_pi"]
        assert torch.equal(v_s, v_full[s0:s0 + S])
        gs = [torch.empty_like(W)]
        ro_s.backward(torch.full((S,), 1.0, device="cuda"), gs, [None])
        acc += gs[0].double()
    assert rel_l2(gw[0].cpu().double(), acc.cpu()) < 1e-5
    res = ro.forward(data, want_rewards=True, want_final=True)
    _check_against_f64(alg, data, res, cfg, fh=True)


def _lq_f64(alg, data, n_rows, horizon, gamma, fh, value=None):
    """A float64 restatement of the wrapped pyth_lq rollout with a POLY degree-1 policy on the first n_rows trajectories:
    ScaleAction / ClipAction, x' = inv_IA (x + dt B u), r = rs (rsh - (Q x^2 + R u^2)), ShapingReward, MaskAtDone, ClipObservation,
    and the tail (~done_H) gamma^H V(x_H) of a POLY StateValue (degree 2, no norm_matrix).  -> v, rewards [H, n], x_H, done_H."""
    env = alg.envmodel.hip_env()
    n, m = env.obs_dim, env.act_dim
    f = lambda vals, k: torch.tensor(list(vals)[:k], dtype=torch.float64)
    inv_IA, Bm = f(env.lq_inv_IA, n * n).reshape(n, n), f(env.lq_B, n * m).reshape(n, m)
    Q, R = f(env.lq_Q, n), f(env.lq_R, m)
    amin, amax, alo, ahi = f(env.min_action, m), f(env.max_action, m), f(env.act_low, m), f(env.act_high, m)
    W = alg.networks.policy.pi.weight.detach().cpu().double()
    x = data["obs"][:n_rows].cpu().double()
    done = data["done"][:n_rows].cpu() != 0
    v = torch.zeros(n_rows, dtype=torch.float64)
    rewards = []
    for t in range(horizon):
        a = x @ W[:, :n].T + ((t + 1) * W[:, n] if fh else 0.0)
        u = torch.minimum(torch.maximum(alo + (ahi - alo) * (torch.minimum(torch.maximum(a, amin), amax) - amin) / (amax - amin), alo), ahi)
        r = env.lq_reward_scale * (env.lq_reward_shift - ((Q * x * x).sum(1) + (R * u * u).sum(1)))
        xn = (x + env.lq_dt * u @ Bm.T) @ inv_IA.T
        if env.clip_obs:
            xn = torch.minimum(torch.maximum(xn, f(env.obs_low, n)), f(env.obs_high, n))
        rr = torch.where(done, torch.zeros_like(r), r)
        if env.shaping:
            rr = (rr + env.reward_shift) * env.reward_scale
        rewards.append(rr)
        v += rr * gamma ** t
        x = torch.where(done[:, None], x, xn)
    if value is not None:
        Wv = value.v.weight.detach().cpu().double().reshape(-1)
        feats = torch.stack([x[:, i] * x[:, j] for i in range(n) for j in range(i, n)], 1)
        v += torch.where(done, torch.zeros_like(v), torch.ones_like(v)) * gamma ** horizon * (feats @ Wv)
    return v, torch.stack(rewards), x, done.double()


def _check_against_f64(alg, data, res, cfg, fh, value=None, n_rows=256):
    """v_pi at the 1e-4 bar, rewards and final_obs at 1e-5, final_done exactly, against the float64 restatement."""
    v, rewards, x_H, d_H = _lq_f64(alg, data, n_rows, cfg["horizon"], cfg["gamma"], fh, value)
    assert rel_l2(res["v_pi"][:n_rows].cpu().double(), v) < TOL
    assert rel_l2(res["rewards"][:, :n_rows].cpu().double(), rewards) < 1e-5
    assert rel_l2(res["final_obs"][:n_rows].cpu().double(), x_H) < 1e-5
    assert torch.equal(res["final_done"][:n_rows].cpu().double(), d_H)


def test_infadp_poly_large_batch():
    """INFADP s4a2 (forward_step 5, POLY tail value) at B = 65 536: the policy-improvement rollout against the float64 restatement
    on a slice, its gradient against the sum of the slices' gradients, and the POLY value kernels against float64 autograd."""
    alg, g, cfg = _load_alg("infadp_poly_lqs4a2_fs5")
    B = 65536
    data = {k: v.cuda() for k, v in make_batch(dict(cfg, batch=B), 5).items()}
    data["done"][::97] = 1.0
    ro = alg._rollout_for(B, torch.device("cuda"), need_grad=True)
    res = ro.forward(data, want_rewards=True, want_final=True)
    _check_against_f64(alg, data, res, cfg, fh=False, value=alg.networks.v_target)
    W = alg.networks.policy.pi.weight
    gw = [torch.empty_like(W)]
    ro.backward(torch.full((B,), 1.0, device="cuda"), gw, [None])
    S = 8192
    ro_s = alg._rollout_for(S, torch.device("cuda"), need_grad=True)
    acc = torch.zeros_like(W, dtype=torch.float64)
    for s0 in range(0, B, S):
        sl = {k: v[s0:s0 + S].contiguous() for k, v in data.items()}
        assert torch.equal(ro_s.forward(sl)["v_pi"], res["v_pi"][s0:s0 + S])
        gs = [torch.empty_like(W)]
        ro_s.backward(torch.full((S,), 1.0, device="cuda"), gs, [None])
        acc += gs[0].double()
    assert rel_l2(gw[0].cpu().double(), acc.cpu()) < 1e-5
    # PEV's value net over the whole batch: forward and weight gradient against float64 autograd
    vn = alg._value_for(B, torch.device("cuda"))
    obs = data["obs"]
    gv = torch.linspace(-1.0, 1.0, B, device="cuda")
    v = vn.forward(obs)
    gwv = [torch.empty_like(alg.networks.v.v.weight)]
    vn.backward(obs, gv, gwv, [None])
    Wv = alg.networks.v.v.weight.detach().double().clone().requires_grad_(True)
    o64 = obs.double()
    n = obs.shape[1]
    feats = torch.stack([o64[:, i] * o64[:, j] for i in range(n) for j in range(i, n)], 1)
    v64 = (feats @ Wv.reshape(-1, 1)).squeeze(-1)
    (v64 * gv.double()).sum().backward()
    assert rel_l2(v.double().cpu(), v64.detach().cpu()) < 1e-5
    assert rel_l2(gwv[0].double().cpu(), Wv.grad.cpu()) < 1e-5


def test_poly_value_kernels_match_host_module_and_autograd():
    g = load_golden("poly_features")
    from gops_amd.apprfunc.poly import StateValue
    from gops_amd.utils.act_distribution import DiracDistribution
    for name in ("value_nobias", "value_bias"):
        sd = {k.split("/sd/")[1]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(f"{name}/sd/")}
        net = StateValue(obs_dim=4, degree=2, add_bias="v.bias" in sd, norm_matrix=np.array(g[f"{name}/norm"]).tolist(),
                         action_distribution_cls=DiracDistribution)
        net.load_state_dict(sd)
        net.cuda()
        obs = torch.from_numpy(np.array(g[f"{name}/obs"])).cuda()
        B = obs.shape[0]
        vn = hb.PolyValueNet(net.hip_mlp(), B, 4)
        v = vn.forward(obs)
        assert rel_l2(v.cpu(), g[f"{name}/out"]) < 1e-6
        gv = torch.linspace(-1.0, 1.0, B, device="cuda")
        gw, gb = poly_grad_buffers(net)
        vn.backward(obs, gv, gw, gb)
        got = [p.grad.clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        (net(obs) * gv).sum().backward()
        for a, b in zip(got, [p.grad for p in net.parameters()]):
            assert rel_l2(a.cpu().double(), b.cpu().double()) < 1e-5


@pytest.mark.parametrize("mode", ["fhadp", "infadp"])
def test_poly_update_paths_agree(mode, monkeypatch):
    """Eager, captured and replayed updates give identical weights; get_remote_update_info + remote_update == local_update."""
    name = "fhadp_poly_lqs2a1_h80" if mode == "fhadp" else "infadp_poly_lqs4a2_fs5"
    algs = []
    for flag in ("1", "0", "0"):
        monkeypatch.setenv("GOPS_HIP_GRAPH", flag)
        algs.append(_load_alg(name)[0])
    cfg = golden_meta(load_golden(name))["cfg"]
    for it in range(6):
        data = {k: v.cuda() for k, v in make_batch(cfg, 70 + it).items()}
        monkeypatch.setenv("GOPS_HIP_GRAPH", "1")
        algs[0].local_update(data, it)
        monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
        algs[1].local_update(data, it)
        _, info = algs[2].get_remote_update_info(data, it)
        algs[2].remote_update(info)
    torch.cuda.synchronize()
    for other in algs[1:]:
        for (k, a), b in zip(algs[0].networks.state_dict().items(), other.networks.state_dict().values()):
            assert torch.equal(a, b), k


def test_poly_rollout_refuses_what_it_does_not_run():
    alg, g, cfg = _load_alg("fhadp_poly_lqs2a1_h80")
    env = alg.envmodel.hip_env()
    pol = alg.networks.policy.hip_mlp()
    with pytest.raises(RuntimeError):   # the MLP entry points keep rejecting n_layers = 1
        hb.Rollout(env, pol, batch=8, horizon=4, gamma=1.0, finite_horizon=True)
    bad = hb.GopsEnv.from_buffer_copy(env)
    bad.kind = hb.ENV_VEH
    with pytest.raises(RuntimeError):
        hb.PolyRollout(bad, pol, batch=8, horizon=4, gamma=1.0, finite_horizon=True)
    d = hb.PolyRollout(env, pol, batch=8, horizon=4, gamma=1.0, finite_horizon=True).desc
    d.dtype = 1
    assert hb.lib().gops_poly_rollout_workspace_bytes(d) == 0


# ---- one POLY rollout step against hb.env_step: both inline the same wrapped model step (csrc/env_models.h) --------------------
def _step_env(case):
    lq2 = dict(inv_IA=[[1.0, 0.05], [-0.02, 0.97]], B=[[0.0], [1.0]], Q=[2.0, 1.0], R=[0.5], dt=0.05, reward_scale=0.1,
               reward_shift=1.0)
    lq3 = dict(inv_IA=[[1.0, 0.05, 0.0], [-0.02, 0.97, 0.04], [0.01, -0.03, 0.95]], B=[[0.0], [0.5], [1.0]], Q=[2.0, 1.0, 0.5],
               R=[0.5], dt=0.05, reward_scale=0.1, reward_shift=1.0)
    if case == "lq_s2a1":
        return hb.make_env(hb.ENV_LQ, 2, 1, act_low=[-2.0], act_high=[2.0], lq=lq2)
    if case == "lq_s3a1_obsscale_repeat2_bounds":
        return hb.make_env(hb.ENV_LQ, 3, 1, act_low=[-2.0], act_high=[2.0], lq=lq3, obs_scale=[0.5, 2.0, 1.5],
                           obs_shift=[0.25, -0.125, 0.0], repeat_num=2, obs_low=[-0.2, -0.4, -0.3], obs_high=[0.2, 0.4, 0.3],
                           reward_scale=0.5, reward_shift=0.25)
    kind, n = {"idpendulum": (hb.ENV_IDP, 6), "cartpole": (hb.ENV_CARTPOLE, 4), "pendulum": (hb.ENV_PENDULUM, 3)}[case]
    return hb.make_env(kind, n, 1, act_low=[-1.0], act_high=[1.0])


def _ulp_distance(a, b):
    """Largest distance in units in the last place between two float32 tensors."""
    def ordered(x):
        i = x.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((ordered(a) - ordered(b)).abs().max())


# Largest distance of the two kernels' next observation, in units in the last place, measured on an MI355X at the commit before
# they shared one statement of the step (separate copies then, contracted into fused multiply-adds differently by the compiler).
# The rewards and every other case's observation were bit-equal there; with the shared statement every case measures 0.
ONE_STEP_OBS_ULP_BEFORE_SHARING = {"idpendulum": 130}


@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("case", ["lq_s2a1", "lq_s3a1_obsscale_repeat2_bounds", "idpendulum", "cartpole", "pendulum"])
def test_poly_one_step_equals_env_step(case, B):
    """A PolyRollout of H = 1 and `hb.env_step` fed the policy's own pre-wrapper action give the same bits: rewards, next
    observation and done flag (one lane, a partial wave, one lane past the 256-thread block; every fifth row done).
    Observations are multiples of 1/64 and weights multiples of 1/8, so the float32 feature product formed on the host is exact
    and equals the kernel's in any summation order: the action is identical on both sides by construction.  The bound
    is what the two kernels measured while they were separate copies: bit-equal, except pyth_idpendulum's next observation
    (ONE_STEP_OBS_ULP_BEFORE_SHARING); the figures are printed before they are asserted."""
    env = _step_env(case)
    n = env.obs_dim
    gen = torch.Generator().manual_seed(1000 + B)
    obs = torch.randint(-32, 33, (B, n), generator=gen).float() / 64
    W = torch.randint(-8, 9, (1, n), generator=gen).float() / 8
    bias = torch.randint(-8, 9, (1,), generator=gen).float() / 8
    done = torch.zeros(B)
    done[::5] = 1.0
    action = (obs @ W.T + bias).cuda()          # degree 1: the features are the observation
    obs, done, W, bias = obs.cuda(), done.cuda(), W.cuda(), bias.cuda()
    ro = hb.PolyRollout(env, hb.make_poly(W, bias, hb.POLY_FULL[1]), batch=B, horizon=1, gamma=1.0, finite_horizon=False,
                        need_grad=False)
    res = ro.forward({"obs": obs, "done": done}, want_rewards=True, want_final=True)
    nobs, rew, ndone, _ = hb.env_step(env, obs, action, done)
    torch.cuda.synchronize()
    ulp_r, ulp_o = _ulp_distance(res["rewards"][0], rew), _ulp_distance(res["final_obs"], nobs)
    print(f"{case} B={B}: rewards {ulp_r} ulp, final_obs {ulp_o} ulp")
    assert torch.equal(res["final_done"], ndone)
    assert torch.equal(res["rewards"][0], rew)
    if case in ONE_STEP_OBS_ULP_BEFORE_SHARING:
        assert ulp_o <= ONE_STEP_OBS_ULP_BEFORE_SHARING[case]
    else:
        assert torch.equal(res["final_obs"], nobs)
    assert torch.equal(res["v_pi"], res["rewards"][0])        # gamma^0 = 1, no tail
    assert ndone[::5].all() and torch.isfinite(nobs).all()


# ---- one open-loop step of the tile-form rollout against hb.env_step: both inline the same env phase (csrc/rollout_env.h) ------
_OPEN_LOOP_ENVS = {"veh2dof": "pyth_veh2dofconti_errcstr", "veh3dofconti_p10": "pyth_veh3dofconti",
                   "veh3dof_detour": "pyth_veh3dofconti_detour", "mobilerobot": "pyth_mobilerobot"}


def _open_loop_env_and_batch(case, B):
    """(GopsEnv, CPU batch) of a case.  Every action range is [-1, 1], so that the wrapper chain env_step applies to its action
    is the identity on the multiples of 1/64 the test hands in: the rollout (raw_actions) and env_step step the same action."""
    gen = torch.Generator().manual_seed(77 + B)
    if case == "lq_s4a2_obsscale_clip":
        lq = dict(inv_IA=[[1.0, 0.05, 0.0, 0.01], [-0.02, 0.97, 0.04, 0.0], [0.01, -0.03, 0.95, 0.02], [0.0, 0.02, -0.01, 0.98]],
                  B=[[0.0, 0.1], [0.5, 0.0], [1.0, -0.25], [0.0, 1.0]], Q=[2.0, 1.0, 0.5, 0.25], R=[0.5, 0.125], dt=0.05,
                  reward_scale=0.1, reward_shift=1.0)
        env = hb.make_env(hb.ENV_LQ, 4, 2, act_low=[-1.0, -1.0], act_high=[1.0, 1.0], lq=lq, obs_scale=[0.5, 2.0, 1.5, 1.0],
                          obs_shift=[0.25, -0.125, 0.0, 0.5], obs_low=[-0.2, -0.4, -0.3, -0.5], obs_high=[0.2, 0.4, 0.3, 0.5])
        return env, {"obs": torch.randint(-32, 33, (B, 4), generator=gen).float() / 64}
    if case in ("cartpole", "pendulum", "idpendulum"):
        env = _step_env(case)
        return env, {"obs": torch.randint(-32, 33, (B, env.obs_dim), generator=gen).float() / 64}
    cfg = dict(alg="INFADP", env_id=_OPEN_LOOP_ENVS[case], batch=B, horizon=1, pre_horizon=10)
    env = hip_env_from_oracle(orc.make_env(cfg["env_id"], pre_horizon=10))
    for a in range(env.act_dim):
        env.act_low[a], env.act_high[a], env.min_action[a], env.max_action[a] = -1.0, 1.0, -1.0, 1.0
    data = {k: v for k, v in make_batch(cfg, 5).items() if torch.is_tensor(v)}
    if case == "mobilerobot":
        data["noise"] = (torch.randn(1, B, 2, generator=gen) * torch.tensor(hb.MOBILEROBOT_NOISE_STD)).contiguous()
    return env, data


# Largest distance, in units in the last place, between the open-loop rollout's step and env_step's, measured on an MI355X at the
# commit before the tile-form kernels took their env phase from csrc/rollout_env.h: {case: {output: ulp}}; what is not listed was
# bit-equal there (the forward step of either kernel was contracted into fused multiply-adds in its own way).
OPEN_LOOP_ONE_STEP_ULP_BEFORE_SHARING = {"lq_s4a2_obsscale_clip": {"final_obs": 3}, "idpendulum": {"final_obs": 8},
                                         "veh3dofconti_p10": {"final_obs": 12}, "veh3dof_detour": {"final_obs": 12}}


@pytest.mark.parametrize("case", ["lq_s4a2_obsscale_clip", "cartpole", "pendulum", "idpendulum", "veh2dof", "veh3dofconti_p10",
                                  "veh3dof_detour", "mobilerobot"])
def test_open_loop_rollout_one_step_equals_env_step(case):
    """An open-loop `hb.Rollout` (raw_actions: the actions are handed in) of H = 1, gamma = 1 and `hb.env_step` fed the same
    actions: rewards, next observation, done flag and - where the model has them - the step's constraint values.  B = 33: two
    full 16-row tiles and one row; every fifth row done.  The bound per output is what the two kernels measured before they
    shared the statement of the env phase (OPEN_LOOP_ONE_STEP_ULP_BEFORE_SHARING, 0 where nothing is listed); the figures are
    printed before they are asserted."""
    B = 33
    env, data = _open_loop_env_and_batch(case, B)
    gen = torch.Generator().manual_seed(4242)
    actions = torch.randint(-64, 65, (B, 1, env.act_dim), generator=gen).float() / 64
    data["done"] = torch.zeros(B)
    data["done"][::5] = 1.0
    data = to_device(data, torch.device("cuda", 0))
    actions = actions.cuda()
    ro = hb.Rollout(env, None, batch=B, horizon=1, gamma=1.0, finite_horizon=False, need_grad=False, raw_actions=True)
    res = ro.forward(data, head_pre=actions, want_rewards=True, want_final=True, want_constraints=True)
    info = dict(data, noise=data["noise"][0]) if "noise" in data else data
    nobs, rew, ndone, ninfo = hb.env_step(env, data["obs"], actions[:, 0].contiguous(), data["done"], info)
    torch.cuda.synchronize()
    pairs = {"rewards": (res["rewards"][0], rew), "final_obs": (res["final_obs"], nobs)}
    if hb.has_constraints(env):
        pairs["constraints"] = (res["constraints"][0], ninfo["constraint"])
    ulp = {k: _ulp_distance(a, b) for k, (a, b) in pairs.items()}
    print(f"{case}: " + ", ".join(f"{k} {v} ulp" for k, v in ulp.items()))
    assert torch.equal(res["final_done"], ndone)
    bound = OPEN_LOOP_ONE_STEP_ULP_BEFORE_SHARING.get(case, {})
    for k, v in ulp.items():
        assert v <= bound.get(k, 0), (case, k, v)
    assert torch.equal(res["v_pi"], res["rewards"][0])        # gamma^0 = 1, no tail
    assert ndone[::5].all() and torch.isfinite(nobs).all() and all(torch.isfinite(a).all() for a, _ in pairs.values())
