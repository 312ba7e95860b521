"""GPU: the plane-split contractions of the register-stationary kernels (csrc/common.h split2h / gemm_split: two half planes per
operand, 22 bits, three f16 MFMAs per block) against the oracle at the 1e-4 bar, and against the
exact-fp32-MFMA kernels of the same library (GOPS_VF_NO_STATIONARY_SPLIT) to see what the 16-bit planes cost: every env kind and
layer-0 chunk count the split kernels are instantiated for, ragged batches, every hidden activation, INFADP's tail value."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import hip_env_from_oracle, hip_mlp_from_net, reference_init_nets, to_device
from oracle import adp_oracle as orc

from gops_amd.utils.synthetic import act_dim_of, make_batch, obs_dim_of

pytestmark = pytest.mark.gpu
TOL = 1e-4

CASES = {
    # name: config (policy 256-256 -> the stationary kernels; at most one 16-trajectory tile per CU)
    "veh_p30_elu": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=200, horizon=12, pre_horizon=30, hidden=(256, 256), act="elu", gamma=0.99),
    "veh_p20_gelu": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=96, horizon=9, pre_horizon=20, hidden=(256, 256), act="gelu", gamma=1.0),
    "veh_p10_tanh": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=77, horizon=10, pre_horizon=10, hidden=(256, 256), act="tanh", gamma=0.95),
    "idp_gelu": dict(alg="FHADP", env_id="pyth_idpendulum", batch=130, horizon=15, hidden=(256, 256), act="gelu", gamma=1.0),
    "idp_selu": dict(alg="FHADP", env_id="pyth_idpendulum", batch=64, horizon=8, hidden=(256, 256), act="selu", gamma=0.9),
    "lq_s4a2_relu": dict(alg="FHADP", env_id="pyth_lq", lq_config="s4a2", batch=100, horizon=20, hidden=(256, 256), act="relu", gamma=0.99),
    "lq_s6a3_sigmoid": dict(alg="FHADP", env_id="pyth_lq", lq_config="s6a3", batch=33, horizon=10, hidden=(256, 256), act="sigmoid", gamma=1.0),
    "lq_s2a1_elu": dict(alg="FHADP", env_id="pyth_lq", lq_config="s2a1", batch=16, horizon=25, hidden=(256, 256), act="elu", gamma=0.97),
    # more than 128 policy inputs: layer 0's planes stream from L2 (StreamQ), 5 .. 8 chunks of 32 inputs
    "veh_p50_elu_stream": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=150, horizon=7, pre_horizon=50, hidden=(256, 256), act="elu", gamma=1.0),
    "veh_p34_gelu_stream": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=64, horizon=6, pre_horizon=34, hidden=(256, 256), act="gelu", gamma=0.98),
    "veh_p45_relu_stream": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=49, horizon=5, pre_horizon=45, hidden=(256, 256), act="relu", gamma=1.0),
    "veh_p60_tanh_stream": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=40, horizon=4, pre_horizon=60, hidden=(256, 256), act="tanh", gamma=0.99),
    "veh_p40_multi_stream": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=4096 + 16 * 5 + 7, horizon=3, pre_horizon=40, hidden=(256, 256), act="elu", gamma=1.0),
    # more tiles than CUs: the workgroups walk their tiles grid-stride with the weights resident (ragged last tile included)
    "lq_s4a2_multi": dict(alg="FHADP", env_id="pyth_lq", lq_config="s4a2", batch=4096 + 16 * 37 + 5, horizon=5, hidden=(256, 256), act="gelu", gamma=0.99),
    "veh_p10_multi": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=4096 + 16 * 9 + 3, horizon=4, pre_horizon=10, hidden=(256, 256), act="elu", gamma=1.0),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _run(cfg, nets, data, env, dev, monkeypatch, split, extra_flags=0):
    """(variant selection goes through GopsRolloutDesc.variant_flags, ABI v10 - `monkeypatch` is kept for the callers' signature)"""
    from gops_amd import hip_backend as hb
    henv = hip_env_from_oracle(env, nets["policy"])
    mlp, ws, bs = hip_mlp_from_net(nets["policy"], dev)
    B = data["obs"].shape[0]
    ro = hb.Rollout(henv, mlp, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=True,
                    variant_flags=(0 if split else hb.VF_NO_STATIONARY_SPLIT) | extra_flags)
    import ctypes
    assert (hb.lib().gops_rollout_variant(ctypes.byref(ro.desc)) == 1) == split, "the launch would not take the kernels under test"
    res = ro.forward(to_device(data, dev), want_rewards=True, want_final=True)
    gw, gb = [torch.empty_like(w) for w in ws], [torch.empty_like(b) for b in bs]
    ro.backward(torch.full((B,), -1.0 / B, device=dev), gw, gb)
    torch.cuda.synchronize()
    return res, [t for pair in zip(gw, gb) for t in pair]


@pytest.mark.parametrize("name", list(CASES))
def test_split_kernels_vs_oracle_and_fp32_mfma(name, dev, monkeypatch):
    cfg = CASES[name]
    data = make_batch(cfg, 3)
    nets = reference_init_nets(cfg, 3, obs_dim_of(cfg), act_dim_of(cfg))
    env = orc.make_env(cfg["env_id"], pre_horizon=cfg.get("pre_horizon", 10), lq_config=cfg.get("lq_config", "s4a2"))
    ref = orc.fhadp_gradient(env, nets["policy"], data, cfg["horizon"], cfg["gamma"])
    res, grads = _run(cfg, nets, data, env, dev, monkeypatch, split=True)
    res0, grads0 = _run(cfg, nets, data, env, dev, monkeypatch, split=False)
    assert rel_l2(res["v_pi"].cpu(), ref["v_pi"]) < TOL
    assert rel_l2(res["rewards"].cpu(), ref["rewards"]) < TOL
    assert rel_l2(res["final_obs"].cpu(), ref["final_obs"]) < TOL
    assert np.array_equal(res["final_done"].cpu().numpy() != 0, ref["final_done"].numpy())
    flat = torch.cat([g.reshape(-1).cpu() for g in grads])
    flat0 = torch.cat([g.reshape(-1).cpu() for g in grads0])
    flat_ref = torch.cat([g.reshape(-1) for g in ref["grads"]])
    err, err0 = rel_l2(flat, flat_ref), rel_l2(flat0, flat_ref)
    worst = max(rel_l2(g.cpu(), w) for g, w in zip(grads, ref["grads"]))
    print(f"{name}: gradient rel-L2 to the oracle: plane-split {err:.2e} (worst tensor {worst:.2e}), fp32 MFMA {err0:.2e}; "
          f"split vs fp32 MFMA {rel_l2(flat, flat0):.2e}; v_pi {rel_l2(res['v_pi'].cpu(), ref['v_pi']):.2e}")
    assert err < TOL and worst < TOL, (name, err, worst)
    assert rel_l2(flat, flat0) < 5e-5, (name, rel_l2(flat, flat0))   # the two arithmetic paths agree far inside the bar


@pytest.mark.parametrize("batch,act", [(90, "gelu"), (4096 + 16 * 11 + 7, "gelu"), (3000, "relu"), (200, "selu")])
def test_split_kernels_with_tail_value(batch, act, dev, monkeypatch):
    """INFADP's policy-improvement gradient (tail value net after the loop: its fp32 tiles alias the plane images); the
    second batch has more tiles than CUs (grid-stride tile walk: the policy biases are re-staged after every tail).  relu / selu:
    the tail value net runs on exact fp32 products in these kernels, which is what such nets need (rollout_fwd.hip: ss_tail_exact)."""
    from gops_amd import hip_backend as hb
    cfg = dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=batch, horizon=8, hidden=(256, 256), act=act, gamma=0.99)
    data = make_batch(cfg, 8)
    nets = reference_init_nets(cfg, 8, obs_dim_of(cfg), act_dim_of(cfg))
    env = orc.make_env("pyth_lq", lq_config="s4a2")
    want = orc.infadp_pim_gradient(env, nets["policy"], nets["v_target"], data, cfg["horizon"], cfg["gamma"])
    out = {}
    for split in (True, False):
        henv = hip_env_from_oracle(env, nets["policy"])
        pol, pw, pb = hip_mlp_from_net(nets["policy"], dev)
        vt, _, _ = hip_mlp_from_net(nets["v_target"], dev)
        B = data["obs"].shape[0]
        # (by default tail + more tiles than CUs stays on the streamed kernels: VF_SPLIT_TAIL_MULTI)
        ro = hb.Rollout(henv, pol, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=False, need_grad=True, value=vt,
                        variant_flags=hb.VF_SPLIT_TAIL_MULTI | (0 if split else hb.VF_NO_STATIONARY_SPLIT))
        import ctypes
        assert (hb.lib().gops_rollout_variant(ctypes.byref(ro.desc)) == 1) == split, "the launch would not take the kernels under test"
        res = ro.forward(to_device(data, dev))
        gw, gb = [torch.empty_like(w) for w in pw], [torch.empty_like(b) for b in pb]
        ro.backward(torch.full((B,), -1.0 / B, device=dev), gw, gb)
        torch.cuda.synchronize()
        out[split] = (res["v_pi"].cpu(), torch.cat([t.reshape(-1).cpu() for pair in zip(gw, gb) for t in pair]))
    flat_ref = torch.cat([g.reshape(-1) for g in want["grads"]])
    for split in (True, False):
        assert abs(-out[split][0].double().mean().item() - float(want["loss"])) <= TOL * max(1.0, abs(float(want["loss"])))
        assert rel_l2(out[split][1], flat_ref) < TOL, (split, rel_l2(out[split][1], flat_ref))
    print(f"tail: split {rel_l2(out[True][1], flat_ref):.2e} fp32 MFMA {rel_l2(out[False][1], flat_ref):.2e}")


def test_weight_gradient_gemm_redoes_saturated_blocks_exactly(dev, monkeypatch):
    """The two-half-plane weight-gradient GEMM saturates beyond |x| = 65504; the converting threads flag it and a guarded
    second launch redoes the GEMM with the exact three-plane split.  A policy whose first layer is scaled up so that H_1
    reaches ~1e5 must still meet the 1e-4 bar against the oracle (and it does not with the guard disabled: that is what
    GOPS_VF_DW_NO_GUARD is for)."""
    cfg = dict(alg="FHADP", env_id="pyth_lq", lq_config="s4a2", batch=64, horizon=3, hidden=(256, 256), act="relu", gamma=0.99)
    data = make_batch(cfg, 21)
    nets = reference_init_nets(cfg, 21, obs_dim_of(cfg), act_dim_of(cfg))
    with torch.no_grad():
        nets["policy"]["w"][0].mul_(2.0e5)
        nets["policy"]["w"][1].mul_(1.0e-5)
    env = orc.make_env("pyth_lq", lq_config="s4a2")
    ref = orc.fhadp_gradient(env, nets["policy"], data, cfg["horizon"], cfg["gamma"])
    h1 = torch.relu(torch.nn.functional.linear(torch.cat((data["obs"], torch.ones(64, 1)), 1), nets["policy"]["w"][0], nets["policy"]["b"][0]))
    assert h1.max().item() > 65504.0 * 1.2   # the premise: H_1 is beyond the half range
    res, grads = _run(cfg, nets, data, env, dev, monkeypatch, split=True)
    worst = max(rel_l2(g.cpu(), w) for g, w in zip(grads, ref["grads"]))
    assert rel_l2(res["v_pi"].cpu(), ref["v_pi"]) < TOL and worst < TOL, worst
    from gops_amd import hip_backend as hb
    _, grads_ng = _run(cfg, nets, data, env, dev, monkeypatch, split=True, extra_flags=hb.VF_DW_NO_GUARD)
    worst_ng = rel_l2(grads_ng[2].cpu(), ref["grads"][2])   # dW of layer 1 = D_2^T H_1
    print(f"saturated H_1: worst tensor with the guard {worst:.2e}; layer-1 weight gradient without it {worst_ng:.2e}")
    assert not (worst_ng <= 10 * TOL)   # wrong by orders of magnitude (round-toward-zero planes, rounds 3-5) or non-finite (round-to-nearest planes: inf)


# ---- streamed-split forward kernels (GOPS_VARIANT_STREAMED_SPLIT_FWD): any number of 256-wide hidden layers, planes of every
#      layer streamed from L2, tail value net on the same routine; the sweep of these launches is the fp32-MFMA one ---------------
SS_CASES = {
    # (relu / selu with a tail value net stay on the exact fp32 kernels: kinked_with_tail in csrc/rollout_fwd.hip)
    "veh_p10_3x256_infadp": dict(alg="INFADP", env_id="pyth_veh3dofconti", batch=300, horizon=6, pre_horizon=10, hidden=(256, 256, 256), act="elu", gamma=0.99),
    # (more than 256 tiles: two workgroups share a CU - the regime the round-3 kernels were not reproducible in)
    "veh_p10_3x256_fhadp_relu": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=4096 + 16 * 37 + 1, horizon=4, pre_horizon=10, hidden=(256, 256, 256), act="relu", gamma=0.99),
    "veh_p10_3x256_infadp_many_tiles": dict(alg="INFADP", env_id="pyth_veh3dofconti", batch=4096 + 16 * 93 + 9, horizon=3, pre_horizon=10, hidden=(256, 256, 256), act="gelu", gamma=0.99),
    "veh_p10_2x256_infadp_many_tiles": dict(alg="INFADP", env_id="pyth_veh3dofconti", batch=4800, horizon=4, pre_horizon=10, hidden=(256, 256), act="elu", gamma=0.99),
    # relu / selu with a tail value net: plane-split step loop and sweep, the tail value net on exact fp32 products (RolloutParams.tail_fp32)
    "veh_p10_3x256_infadp_relu_tail": dict(alg="INFADP", env_id="pyth_veh3dofconti", batch=4096 + 16 * 40 + 5, horizon=4, pre_horizon=10, hidden=(256, 256, 256), act="relu", gamma=0.99),
    "lq_s4a2_3x256_infadp_selu_tail": dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=200, horizon=5, hidden=(256, 256, 256), act="selu", gamma=0.99),
    "veh_p30_4x256_fhadp": dict(alg="FHADP", env_id="pyth_veh3dofconti", batch=70, horizon=5, pre_horizon=30, hidden=(256, 256, 256, 256), act="elu", gamma=1.0),
    "lq_s4a2_infadp_many_tiles": dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=4096 + 16 * 21 + 3, horizon=6, hidden=(256, 256), act="gelu", gamma=0.99),
    "lq_s6a3_3x256_fhadp": dict(alg="FHADP", env_id="pyth_lq", lq_config="s6a3", batch=50, horizon=9, hidden=(256, 256, 256), act="tanh", gamma=0.97),
    # the other env models (the routines do not depend on the model: one instantiation each)
    "idp_3x256_fhadp": dict(alg="FHADP", env_id="pyth_idpendulum", batch=70, horizon=8, hidden=(256, 256, 256), act="gelu", gamma=1.0),
    "surrcstr_2x256_fhadp": dict(alg="FHADP", env_id="pyth_veh3dofconti_surrcstr", batch=60, horizon=6, pre_horizon=10, hidden=(256, 256), act="elu", gamma=1.0),
    "veh2dof_2x256_infadp": dict(alg="INFADP", env_id="pyth_veh2dofconti", batch=90, horizon=7, pre_horizon=10, hidden=(256, 256), act="gelu", gamma=0.99),
    "cartpole_3x256_infadp": dict(alg="INFADP", env_id="gym_cartpoleconti", batch=64, horizon=8, hidden=(256, 256, 256), act="tanh", gamma=0.99),
    "pendulum_2x256_fhadp": dict(alg="FHADP", env_id="gym_pendulum", batch=40, horizon=6, hidden=(256, 256), act="elu", gamma=0.98),
    "mobilerobot_2x256_infadp": dict(alg="INFADP", env_id="pyth_mobilerobot", batch=50, horizon=6, hidden=(256, 256), act="gelu", gamma=0.99),
}


@pytest.mark.parametrize("name", list(SS_CASES))
def test_streamed_split_forward_vs_oracle_and_fp32_mfma(name, dev, monkeypatch):
    import ctypes
    from gops_amd import hip_backend as hb
    cfg = SS_CASES[name]
    data = make_batch(cfg, 5)
    if cfg["env_id"] == "pyth_mobilerobot":
        data["noise"] = torch.randn(cfg["horizon"], cfg["batch"], 2, generator=torch.Generator().manual_seed(3)) * torch.tensor([0.03, 0.02])
    nets = reference_init_nets(cfg, 5, obs_dim_of(cfg), act_dim_of(cfg))
    env = orc.make_env(cfg["env_id"], pre_horizon=cfg.get("pre_horizon", 10), lq_config=cfg.get("lq_config", "s4a2"))
    fh = cfg["alg"] == "FHADP"
    if fh:
        want = orc.fhadp_gradient(env, nets["policy"], data, cfg["horizon"], cfg["gamma"])
    else:
        want = orc.infadp_pim_gradient(env, nets["policy"], nets["v_target"], data, cfg["horizon"], cfg["gamma"])
    flat_ref = torch.cat([g.reshape(-1) for g in want["grads"]])
    out = {}
    for ss in (True, False):
        henv = hip_env_from_oracle(env, nets["policy"])
        pol, pw, pb = hip_mlp_from_net(nets["policy"], dev)
        vt = None if fh else hip_mlp_from_net(nets["v_target"], dev)[0]
        B = data["obs"].shape[0]
        ro = hb.Rollout(henv, pol, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=fh, need_grad=True, value=vt,
                        variant_flags=0 if ss else hb.VF_NO_STREAMED_SPLIT_FWD)
        assert (hb.lib().gops_rollout_variant(ctypes.byref(ro.desc)) == 4) == ss, "the launch would not take the kernels under test"
        res = ro.forward(to_device(data, dev), want_final=True)
        gw, gb = [torch.empty_like(w) for w in pw], [torch.empty_like(b) for b in pb]
        ro.backward(torch.full((B,), -1.0 / B, device=dev), gw, gb)
        torch.cuda.synchronize()
        out[ss] = (res, torch.cat([t.reshape(-1).cpu() for pair in zip(gw, gb) for t in pair]))
    for ss in (True, False):
        res, flat = out[ss]
        assert rel_l2(res["v_pi"].cpu(), want["v_pi"]) < TOL, (name, ss, rel_l2(res["v_pi"].cpu(), want["v_pi"]))
        assert rel_l2(res["final_obs"].cpu(), want["final_obs"]) < TOL
        assert np.array_equal(res["final_done"].cpu().numpy() != 0, want["final_done"].numpy())
        assert rel_l2(flat, flat_ref) < TOL, (name, ss, rel_l2(flat, flat_ref))
    print(f"{name}: gradient rel-L2 to the oracle: streamed-split forward {rel_l2(out[True][1], flat_ref):.2e}, fp32 MFMA {rel_l2(out[False][1], flat_ref):.2e}; "
          f"v_pi {rel_l2(out[True][0]['v_pi'].cpu(), want['v_pi']):.2e}")
    assert rel_l2(out[True][1], out[False][1]) < 5e-5


REPRO_CASES = ["veh_p10_2x256_infadp_many_tiles", "veh_p10_3x256_fhadp_relu", "surrcstr_2x256_fhadp", "lq_s4a2_infadp_many_tiles", "idp_3x256_fhadp",
               "veh2dof_2x256_infadp", "mobilerobot_2x256_infadp"]


@pytest.mark.parametrize("name", REPRO_CASES)
def test_streamed_split_launches_are_reproducible(name, dev):
    """The same forward + backward launch pair TEN times with more tiles than CUs (two workgroups share a CU), the workspace
    filled with other garbage each time (zero bytes, NaN bytes, random bytes): returns AND every parameter gradient are
    bit-identical.  (Round 3: the veh3dofconti forward moved whole tiles by up to 5e-4 and every sweep left a 1e-8 .. 1e-6
    spread - a gfx950 hazard between dependent packed-fp32 instructions, DESIGN_LOG.md, round 4; the library is built without
    those instructions since round 4.)"""
    from gops_amd import hip_backend as hb
    cfg = dict(SS_CASES[name])
    cfg["batch"] = max(cfg["batch"], 4096 + 16 * 40)   # more tiles than CUs: two workgroups share a CU
    data = make_batch(cfg, 5)
    if cfg["env_id"] == "pyth_mobilerobot":
        data["noise"] = torch.randn(cfg["horizon"], cfg["batch"], 2, generator=torch.Generator().manual_seed(3)) * torch.tensor([0.03, 0.02])
    nets = reference_init_nets(cfg, 5, obs_dim_of(cfg), act_dim_of(cfg))
    env = orc.make_env(cfg["env_id"], pre_horizon=cfg.get("pre_horizon", 10), lq_config=cfg.get("lq_config", "s4a2"))
    fh = cfg["alg"] == "FHADP"
    B = data["obs"].shape[0]
    ddev = to_device(data, dev)
    runs = []
    for fill in (0, 255, None, None, 0, None, 255, None, None, None):
        henv = hip_env_from_oracle(env, nets["policy"])
        pol, pw, pb = hip_mlp_from_net(nets["policy"], dev)
        vt = None if fh else hip_mlp_from_net(nets["v_target"], dev)[0]
        ro = hb.Rollout(henv, pol, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=fh, need_grad=True, value=vt)
        if fill is None:
            ro.workspace.random_(0, 256)
        else:
            ro.workspace.fill_(fill)
        res = ro.forward(ddev, want_final=True)
        gw, gb = [torch.empty_like(w) for w in pw], [torch.empty_like(b) for b in pb]
        ro.backward(torch.full((B,), -1.0 / B, device=dev), gw, gb)
        torch.cuda.synchronize()
        runs.append((res["v_pi"].cpu(), res["final_obs"].cpu(), torch.cat([t.reshape(-1).cpu() for pair in zip(gw, gb) for t in pair])))
        del ro
    for v, fo, g in runs[1:]:
        assert torch.isfinite(g).all()
        assert torch.equal(v, runs[0][0])
        assert torch.equal(fo, runs[0][1])
        assert torch.equal(g, runs[0][2]), rel_l2(g, runs[0][2])
