"""GPU: GAUSS (RBF) policies on the one-lane-per-trajectory HIP rollout (csrc/rollout_rbf.hip), through `create_alg(...)` and
`hb.RbfRollout`, against the reference fixtures of tests/golden/make_golden_rbf.py and the float64 restatement of rbf_helpers.py."""
import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import data_from_golden
from rbf_helpers import PARAMS, load_alg, lq_rollout_f64
from test_poly_gpu import ONE_STEP_OBS_ULP_BEFORE_SHARING, _step_env, _ulp_distance

from gops_amd import hip_backend as hb
from gops_amd.utils.synthetic import make_batch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _close(got, want):
    return abs(float(got) - float(want)) <= TOL * max(1.0, abs(float(want)))


# ---- fixture parity through create_alg --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fhadp_rbf_lqs2a1_k35_h20", "fhadp_rbf_lqs6a3_k64_h10", "fhadp_rbf_idp_k8_h20",
                                  "fhadp_rbf_lqs3a1_k3_obsscale_repeat2"])
def test_fhadp_rbf_matches_reference(name):
    alg, g, cfg = load_alg(name)
    tb, info = alg.get_remote_update_info(data_from_golden(g), 0)
    print(name, "loss", float(tb["Loss/Actor loss-RL iter"]), float(g["loss"]),
          {PARAMS[i]: f"{rel_l2(gr.cpu(), g[f'grad/{i}']):.2e}" for i, gr in enumerate(info["grad"])})
    assert _close(tb["Loss/Actor loss-RL iter"], g["loss"])
    assert len(info["grad"]) == 4
    for i, gr in enumerate(info["grad"]):
        assert rel_l2(gr.cpu(), g[f"grad/{i}"]) < TOL, PARAMS[i]
    assert all(isinstance(ro, hb.RbfRollout) for ro in alg._rollouts.values()) and len(alg._rollouts) == 1


@pytest.mark.parametrize("name", ["infadp_rbf_lqs4a2_k35", "infadp_rbf_lqs4a2_k35_fs5"])
def test_infadp_rbf_matches_reference(name):
    alg, g, cfg = load_alg(name)
    data = data_from_golden(g)
    tb, info = alg.get_remote_update_info(data, 0)       # PEV
    print(name, "pev", float(tb["Loss/Critic loss-RL iter"]), float(g["pev_loss"]),
          [f"{rel_l2(gr.cpu(), g[f'pev_grad/{i}']):.2e}" for i, gr in enumerate(info["v"])])
    assert _close(tb["Loss/Critic loss-RL iter"], g["pev_loss"])
    assert _close(tb["Train/Critic avg value-RL iter"], g["pev_vmean"])
    for i, gr in enumerate(info["v"]):
        assert rel_l2(gr.cpu(), g[f"pev_grad/{i}"]) < TOL, i
    tb, info = alg.get_remote_update_info(data, 1)       # PIM
    print(name, "pim", float(tb["Loss/Actor loss-RL iter"]), float(g["pim_loss"]),
          {PARAMS[i]: f"{rel_l2(gr.cpu(), g[f'pim_grad/{i}']):.2e}" for i, gr in enumerate(info["policy"])})
    assert _close(tb["Loss/Actor loss-RL iter"], g["pim_loss"])
    assert len(info["policy"]) == 4
    for i, gr in enumerate(info["policy"]):
        assert rel_l2(gr.cpu(), g[f"pim_grad/{i}"]) < TOL, PARAMS[i]


def test_fhadp_rbf_five_updates_match_reference():
    """Five `local_update` calls (Adam included; eager, then captured / replayed under the default graph policy) land on the
    reference's weights."""
    alg, g, cfg = load_alg("fhadp_rbf_lqs2a1_5updates", prefix="sd0/")
    for k in range(5):
        tb = alg.local_update(data_from_golden(g, f"in{k}/"), k)
        assert _close(tb["Loss/Actor loss-RL iter"], g[f"loss{k}"]), k
    for key, p in alg.networks.state_dict().items():
        assert rel_l2(p.cpu().double(), g["sd5/" + key]) < TOL, key


# ---- kernel-level checks against the float64 restatement on pyth_lq ----------------------------------------------------------------
_LQ = dict(inv_IA=[[1.0, 0.05, 0.0], [-0.02, 0.97, 0.04], [0.01, -0.03, 0.95]], B=[[0.0, 0.1], [0.5, 0.0], [1.0, -0.25]],
           Q=[2.0, 1.0, 0.5], R=[0.5, 0.125], dt=0.05, reward_scale=0.1, reward_shift=1.0)
_LOW, _HIGH = [-2.0, 0.5], [1.0, 3.0]   # asymmetric limits of the heads


def _lq_env():
    return hb.make_env(hb.ENV_LQ, 3, 2, act_low=[-2.0, -1.0], act_high=[2.0, 1.5], min_action=[-2.0, 0.5], max_action=[1.0, 3.0],
                       policy_low=_LOW, policy_high=_HIGH, lq=_LQ, reward_scale=0.5, reward_shift=0.25)


def _rbf_case(B, H, K, fh, seed=0):
    """(env, the four parameter tensors on the GPU in state_dict order, batch): random parameters with the time coordinate of every
    centre inside [1, H] and every fourth sigma_square negative; every fifth row (4, 9, ...) done on entry."""
    gen = torch.Generator().manual_seed(1000 * K + 10 * B + H + seed)
    n_in = 3 + int(fh)
    Cc = torch.randn(1, K, n_in, generator=gen)
    if fh:
        Cc[0, :, -1] = 1.0 + (H - 1.0) * torch.rand(K, generator=gen)
    s = torch.randn(1, K, generator=gen).abs() + 0.1
    s[0, ::4] *= -1.0
    w, b = torch.randn(1, 2, K, generator=gen) / max(1.0, K ** 0.5), 0.3 * torch.randn(1, 2, 1, generator=gen)
    obs = 0.7 * torch.randn(B, 3, generator=gen)
    done = torch.zeros(B)
    done[4::5] = 1.0
    params = [t.cuda().contiguous() for t in (Cc, s, w, b)]
    return _lq_env(), params, {"obs": obs.cuda(), "done": done.cuda()}


def _rollout(env, params, B, H, fh, gamma=0.97, need_grad=True):
    Cc, s, w, b = params
    mlp = hb.make_rbf(w, b, Cc, s, hb.RBF_TANH if fh else hb.RBF_AFFINE)
    return hb.RbfRollout(env, mlp, batch=B, horizon=H, gamma=gamma, finite_horizon=fh, need_grad=need_grad)


def _f64(env, params, data, H, fh, gamma=0.97, obs=None):
    leaves = [p.detach().cpu().double().clone().requires_grad_(True) for p in params]
    o = data["obs"].cpu().double() if obs is None else obs
    out = lq_rollout_f64(env, leaves, torch.tensor(_LOW), torch.tensor(_HIGH), o, data["done"].cpu(), H, gamma, fh)
    return leaves, out


@pytest.mark.parametrize("fh", [False, True], ids=["affine", "tanh"])
@pytest.mark.parametrize("K", [1, 35, 64])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 65, 257])
def test_rbf_kernels_match_float64(B, H, K, fh):
    """One lane, a partial wave, one lane past the 256-thread block; H = 3 at B = 257 hands the parameter-gradient kernel 771
    samples, across a block edge.  v_pi and every gradient tensor at 1e-4, rewards and final_obs at 1e-5, final_done exactly."""
    env, params, data = _rbf_case(B, H, K, fh)
    ro = _rollout(env, params, B, H, fh)
    res = ro.forward(data, want_rewards=True, want_final=True)
    gv = torch.linspace(-1.0, 0.5, B).cuda() if B > 1 else torch.tensor([0.7]).cuda()
    grads = [torch.full_like(p, float("nan")) for p in params]
    ro.backward(gv, grads)
    leaves, (v, rewards, x_H, d_H) = _f64(env, params, data, H, fh)
    (v * gv.cpu().double()).sum().backward()
    fig = dict(v=rel_l2(res["v_pi"].cpu(), v.detach()), rew=rel_l2(res["rewards"].cpu(), rewards.detach()),
               obs=rel_l2(res["final_obs"].cpu(), x_H.detach()))
    fig.update({PARAMS[i]: rel_l2(gr.cpu(), leaves[i].grad) for i, gr in enumerate(grads)})
    print(f"B={B} H={H} K={K} fh={fh}:", {k: f"{x:.2e}" for k, x in fig.items()})
    assert fig["v"] < TOL and fig["rew"] < 1e-5 and fig["obs"] < 1e-5
    assert torch.equal(res["final_done"].cpu().double(), d_H)
    for k in PARAMS:
        assert fig[k] < TOL, k
    assert all(float(l.grad.abs().max()) > 0 for l in leaves)


@pytest.mark.parametrize("fh", [False, True], ids=["affine", "tanh"])
def test_rbf_one_hot_grad_v(fh):
    """A one-hot grad_v on row 0, on row B - 1 and on a done row: per-trajectory gradients against float64 autograd; the done row's
    gradient is exactly zero in all four tensors."""
    B, H, K = 257, 3, 35
    env, params, data = _rbf_case(B, H, K, fh)
    ro = _rollout(env, params, B, H, fh)
    ro.forward(data)
    for row in (0, B - 1, 4):   # rows 0 and B - 1 = 256 are live, row 4 is done on entry
        gv = torch.zeros(B).cuda()
        gv[row] = 1.0
        grads = [torch.full_like(p, float("nan")) for p in params]
        ro.backward(gv, grads)
        if float(data["done"][row]) != 0.0:
            for gr in grads:
                assert torch.equal(gr, torch.zeros_like(gr))
            continue
        leaves, (v, *_) = _f64(env, params, data, H, fh)
        v[row].backward()
        for i, gr in enumerate(grads):
            assert rel_l2(gr.cpu(), leaves[i].grad) < TOL, (row, PARAMS[i])


@pytest.mark.parametrize("fh", [False, True], ids=["affine", "tanh"])
def test_rbf_grad_final_obs_and_grad_obs(fh):
    """`grad_final_obs` seeds the sweep and `grad_obs` leaves it: against float64 autograd of the restatement, with a random
    grad_final_obs and grad_v zero, then both non-zero."""
    B, H, K = 65, 2, 35
    env, params, data = _rbf_case(B, H, K, fh)
    ro = _rollout(env, params, B, H, fh)
    ro.forward(data)
    gen = torch.Generator().manual_seed(5)
    gfo = torch.randn(B, 3, generator=gen)
    for gv in (torch.zeros(B), torch.linspace(-1.0, 1.0, B)):
        grads = [torch.full_like(p, float("nan")) for p in params]
        g_obs = torch.full((B, 3), float("nan")).cuda()
        ro.backward(gv.cuda(), grads, grad_final_obs=gfo.cuda(), grad_obs=g_obs)
        obs64 = data["obs"].cpu().double().clone().requires_grad_(True)
        leaves, (v, _, x_H, _) = _f64(env, params, data, H, fh, obs=obs64)
        ((v * gv.double()).sum() + (x_H * gfo.double()).sum()).backward()
        assert rel_l2(g_obs.cpu(), obs64.grad) < TOL
        for i, gr in enumerate(grads):
            assert rel_l2(gr.cpu(), leaves[i].grad) < TOL, PARAMS[i]


@pytest.mark.parametrize("B", [1, 300])
def test_rbf_gradient_is_bitwise_reproducible(B):
    env, params, data = _rbf_case(B, 3, 64, True)
    ro = _rollout(env, params, B, 3, True)
    gv = torch.full((B,), -1.0 / B).cuda()
    outs = []
    for _ in range(2):
        res = ro.forward(data)
        grads = [torch.full_like(p, float("nan")) for p in params]
        ro.backward(gv, grads)
        torch.cuda.synchronize()
        outs.append([res["v_pi"].clone()] + grads)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t).all() and t.abs().sum() > 0 for t in outs[0][1:])


def test_rbf_batch_slices_are_independent():
    """Each trajectory's return is computed by its own lane: rows [0, 256) run alone give the bits they have inside B = 300."""
    env, params, data = _rbf_case(300, 3, 35, True)
    v_full = _rollout(env, params, 300, 3, True, need_grad=False).forward(data)["v_pi"]
    sl = {k: v[:256].contiguous() for k, v in data.items()}
    v_s = _rollout(env, params, 256, 3, True, need_grad=False).forward(sl)["v_pi"]
    assert torch.equal(v_s, v_full[:256])


# ---- one RBF rollout step against hb.env_step: both inline the same wrapped model step (csrc/env_models.h) --------------------------
@pytest.mark.parametrize("fh", [False, True], ids=["affine", "tanh"])
@pytest.mark.parametrize("case", ["lq_s2a1", "idpendulum", "cartpole", "pendulum"])
def test_rbf_one_step_equals_env_step(case, fh):
    """An RbfRollout of H = 1 and `hb.env_step` fed the host module's own action give the same bits.  K = 1, w = 1, b = 0, C = 0
    and sigma_square = 2^-22; observations are multiples of 1/64 with a non-zero first coordinate, so r >= 2^-12 and
    r / (2 |s|) >= 2^9: phi underflows to exactly 0 whatever rounds the exponential, y = 0, tanh(0) = 0, and the action is the fixed
    float mid = (high + low) / 2 = -0.25 on both sides.  Rewards and final_done bit-equal; final_obs within the units in the last
    place the POLY test records for that env (the same shared step); every fifth row done."""
    from gops_amd.apprfunc import gauss
    from gops_amd.utils.act_distribution import DiracDistribution
    B = 65
    env = _step_env(case)
    env.policy_low[0], env.policy_high[0] = -0.75, 0.25
    n = env.obs_dim
    gen = torch.Generator().manual_seed(2000 + n)
    obs = torch.randint(-32, 33, (B, n), generator=gen).float() / 64
    obs[:, 0] = torch.where(obs[:, 0] == 0, torch.full((B,), 1.0 / 64), obs[:, 0])   # r >= 2^-12 in every row
    done = torch.zeros(B)
    done[::5] = 1.0
    cls = gauss.FiniteHorizonPolicy if fh else gauss.DetermPolicy
    net = cls(obs_dim=n, act_dim=1, num_kernel=1, act_high_lim=np.array([0.25], dtype=np.float32),
              act_low_lim=np.array([-0.75], dtype=np.float32), action_distribution_cls=DiracDistribution).cuda()
    with torch.no_grad():
        net.pi.C.zero_(); net.pi.b.zero_(); net.pi.w.fill_(1.0); net.pi.sigma_square.fill_(2.0 ** -22)
        obs, done = obs.cuda(), done.cuda()
        action = (net(obs, 1) if fh else net(obs)).contiguous()
    assert torch.equal(action, torch.full_like(action, -0.25))   # r / (2 s) >= 2^-12 / 2^-21 = 512: exp underflows to 0
    ro = hb.RbfRollout(env, net.hip_mlp(), batch=B, horizon=1, gamma=1.0, finite_horizon=fh, need_grad=False)
    res = ro.forward({"obs": obs, "done": done}, want_rewards=True, want_final=True)
    nobs, rew, ndone, _ = hb.env_step(env, obs, action, done)
    torch.cuda.synchronize()
    ulp_r, ulp_o = _ulp_distance(res["rewards"][0], rew), _ulp_distance(res["final_obs"], nobs)
    print(f"{case} fh={fh}: rewards {ulp_r} ulp, final_obs {ulp_o} ulp")
    assert torch.equal(res["final_done"], ndone)
    assert torch.equal(res["rewards"][0], rew)
    assert ulp_o <= ONE_STEP_OBS_ULP_BEFORE_SHARING.get(case, 0)
    assert torch.equal(res["v_pi"], res["rewards"][0])        # gamma^0 = 1, no tail
    assert ndone[::5].all() and torch.isfinite(nobs).all()


# ---- update paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fhadp", "infadp"])
def test_rbf_update_paths_agree(mode, monkeypatch):
    """Eager, captured and replayed updates give identical weights; get_remote_update_info + remote_update == local_update."""
    name = "fhadp_rbf_lqs2a1_k35_h20" if mode == "fhadp" else "infadp_rbf_lqs4a2_k35_fs5"
    algs = []
    for flag in ("1", "0", "0"):
        monkeypatch.setenv("GOPS_HIP_GRAPH", flag)
        algs.append(load_alg(name)[0])
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
    before = load_alg(name)[0].networks.state_dict()
    assert any(not torch.equal(before[k], v) for k, v in algs[0].networks.state_dict().items() if "policy.pi" in k)
    for other in algs[1:]:
        for (k, a), b in zip(algs[0].networks.state_dict().items(), other.networks.state_dict().values()):
            assert torch.equal(a, b), k


def test_fhadp_rbf_takes_no_backward_phases_under_an_overlapping_reducer():
    """With a reducer that overlaps the all-reduce with the backward (more than one rank; here `single_rank_phases`), an MLP policy's
    backward runs as two phases.  A GAUSS policy has four gradient tensors too, but its backward is one call: one
    `_gradient_kernels` call without a phase, no pending all-reduce, and the gradients of the path without a reducer."""
    from gops_amd.trainer.grad_sync import GradAllReducer
    name = "fhadp_rbf_lqs2a1_k35_h20"
    alg, g, cfg = load_alg(name)
    data = data_from_golden(g)
    _, plain = alg.get_remote_update_info(data, 0)
    want = [t.clone() for t in plain["grad"]]
    reducer = GradAllReducer(single_rank_phases=True)
    assert reducer.overlap_enabled()
    calls = []
    inner = alg._gradient_kernels
    alg._gradient_kernels = lambda b, phase=None, fused_opt=None: (calls.append(phase), inner(b, phase=phase, fused_opt=fused_opt))[1]
    for t in plain["grad"]:
        t.fill_(float("nan"))
    _, info = alg.get_remote_update_info(data, 1, reducer=reducer)
    torch.cuda.synchronize()
    assert calls == [None] and "_pending" not in info
    for a, b in zip(info["grad"], want):
        assert torch.equal(a, b)
