"""CPU: GAUSS approximators (gops_amd/apprfunc/gauss.py) - host modules against the reference's outputs, state_dict layout and
initial draws, get_apprfunc_dict's GAUSS branch, the refusals around it, the library's own descriptor checks (host code, no
launch), the ABI mirrors, and the condition on the fixtures: the reference's fp32 results sit within a quarter of the GPU tests'
bar of a float64 restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import data_from_golden
from rbf_helpers import PARAMS, alg_kwargs, f64_params, load_alg, lq_rollout_f64, policy_limits

from gops_amd.utils.act_distribution import DiracDistribution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_BAR = 2.5e-5   # a quarter of the 1e-4 bar of test_rbf_gpu.py: the kernels keep three quarters for their own rounding

LQ_FHADP = ["fhadp_rbf_lqs2a1_k35_h20", "fhadp_rbf_lqs6a3_k64_h10", "fhadp_rbf_lqs3a1_k3_obsscale_repeat2"]
LQ_INFADP = ["infadp_rbf_lqs4a2_k35", "infadp_rbf_lqs4a2_k35_fs5"]
FEATURE_CASES = (("determ_k1", "DetermPolicy", 4, 1), ("determ_k35", "DetermPolicy", 4, 35), ("fh_k3", "FiniteHorizonPolicy", 3, 3))
LIM = dict(act_high_lim=np.array([1.0, 3.0], dtype=np.float32), act_low_lim=np.array([-2.0, 0.5], dtype=np.float32),
           action_distribution_cls=DiracDistribution)


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)}


def test_host_modules_match_reference_outputs_layout_and_draws():
    from gops_amd.apprfunc import gauss
    assert gauss.__all__ == ["DetermPolicy", "FiniteHorizonPolicy"]
    g = load_golden("rbf_features")
    for name, cls_name, n, K in FEATURE_CASES:
        cls = getattr(gauss, cls_name)
        torch.manual_seed(int(g[f"{name}/seed"]))
        net = cls(obs_dim=n, act_dim=2, num_kernel=K, **LIM)
        sd = _sd(g, f"{name}/sd/")
        assert list(net.state_dict()) == list(sd)   # keys, in the order the reference recorded them
        assert [k for k, _ in net.named_parameters()] == ["pi.C", "pi.sigma_square", "pi.w", "pi.b"]
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
        n_in = n + (cls_name == "FiniteHorizonPolicy")
        assert tuple(net.pi.C.shape) == (1, K, n_in) and tuple(net.pi.sigma_square.shape) == (1, K)
        assert tuple(net.pi.w.shape) == (1, 2, K) and tuple(net.pi.b.shape) == (1, 2, 1)
        for k, v in net.state_dict().items():   # the same seed gives the reference's initial parameters
            assert torch.equal(v, sd[k]), (name, k)
        assert net.is_rbf
        net.load_state_dict(sd)
        x = torch.from_numpy(np.array(g[f"{name}/obs"]))
        if cls_name == "FiniteHorizonPolicy":
            for t in (1, 7):
                assert rel_l2(net(x, t).detach(), g[f"{name}/out_t{t}"]) < 1e-6
        else:
            assert rel_l2(net(x).detach(), g[f"{name}/out"]) < 1e-6


def _fh_kwargs(**over):
    kw = dict(algorithm="FHADP", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_lq", lq_config="s2a1",
              obsv_dim=2, action_dim=1, action_type="continu", action_high_limit=np.ones(1, dtype=np.float32),
              action_low_limit=-np.ones(1, dtype=np.float32), policy_func_type="GAUSS", policy_func_name="FiniteHorizonPolicy",
              policy_num_kernel=35, policy_act_distribution="default", policy_learning_rate=1e-3, pre_horizon=10, use_gpu=False)
    kw.update(over)
    return kw


def _inf_kwargs(**over):
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_lq", lq_config="s4a2",
              obsv_dim=4, action_dim=2, action_type="continu", action_high_limit=np.ones(2, dtype=np.float32),
              action_low_limit=-np.ones(2, dtype=np.float32), policy_func_type="GAUSS", policy_func_name="DetermPolicy",
              policy_num_kernel=35, policy_act_distribution="default", policy_learning_rate=1e-3, value_func_type="MLP",
              value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation="elu", value_learning_rate=1e-3,
              reward_scale=0.1, use_gpu=False)
    kw.update(over)
    return kw


def test_get_apprfunc_dict_gauss_branch_and_create_apprfunc():
    from gops_amd.create_pkg.create_apprfunc import create_apprfunc
    from gops_amd.utils.common_utils import get_apprfunc_dict
    var = get_apprfunc_dict("policy", **_inf_kwargs())
    assert (var["apprfunc"], var["num_kernel"]) == ("GAUSS", 35)
    assert get_apprfunc_dict("value", **_inf_kwargs(value_func_type="GAUSS", value_num_kernel=30))["num_kernel"] == 30
    with pytest.raises(NotImplementedError, match="GAUSS for the policy"):
        get_apprfunc_dict("policy", **_inf_kwargs(policy_func_type="CNN"))
    kw = _inf_kwargs()
    del kw["policy_num_kernel"]
    with pytest.raises(NotImplementedError, match="without policy_num_kernel"):   # the family has no default kernel count
        get_apprfunc_dict("policy", **kw)
    net = create_apprfunc(apprfunc="GAUSS", name="DetermPolicy", obs_dim=4, act_dim=2, num_kernel=5, **LIM)
    assert net.is_rbf and tuple(net.pi.C.shape) == (1, 5, 4)
    with pytest.raises(Exception):   # the family's other classes are unknown keys
        create_apprfunc(apprfunc="GAUSS", name="StateValue", obs_dim=4, num_kernel=5, action_distribution_cls=DiracDistribution)


def test_create_alg_builds_both_algorithms():
    from gops_amd.create_pkg.create_alg import create_alg
    alg = create_alg(**_fh_kwargs())
    assert alg._rbf and not alg._poly and tuple(alg.networks.policy.pi.C.shape) == (1, 35, 3)
    alg = create_alg(**_inf_kwargs())
    assert alg._rbf and not alg._poly and not alg._lips
    assert {k for k in alg.networks.state_dict() if k.startswith("policy.")} == {
        "policy.pi.C", "policy.pi.sigma_square", "policy.pi.w", "policy.pi.b", "policy.act_high_lim", "policy.act_low_lim"}


def test_rbf_refusals_at_create_alg():
    from gops_amd.create_pkg.create_alg import create_alg
    with pytest.raises(NotImplementedError, match="reference itself cannot run"):   # GAUSS value in INFADP
        create_alg(**_inf_kwargs(value_func_type="GAUSS", value_num_kernel=30))
    with pytest.raises(NotImplementedError, match="MLP value"):                     # GAUSS policy with a POLY value
        create_alg(**_inf_kwargs(value_func_type="POLY", value_degree=2, value_add_bias=False))
    for kw in (_fh_kwargs(mlp_dtype="fp16"), _inf_kwargs(mlp_dtype="fp16")):
        with pytest.raises(NotImplementedError, match="fp32"):
            create_alg(**kw)
    for alg_name in ("FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "MAC", "SPIL", "MPG", "DDPG"):
        with pytest.raises(NotImplementedError, match="GAUSS"):
            create_alg(**_inf_kwargs(algorithm=alg_name, pre_horizon=10))
    with pytest.raises(NotImplementedError, match="GAUSS"):                         # an env model outside the list
        create_alg(**_fh_kwargs(env_id="pyth_veh3dofconti", obsv_dim=46, action_dim=2, lq_config=None,
                                action_high_limit=np.ones(2, dtype=np.float32), action_low_limit=-np.ones(2, dtype=np.float32)))
    with pytest.raises(NotImplementedError, match="FiniteHorizonPolicy"):           # a DetermPolicy in FHADP
        create_alg(**_fh_kwargs(policy_func_name="DetermPolicy"))
    with pytest.raises(NotImplementedError, match="DetermPolicy"):                  # a FiniteHorizonPolicy in INFADP
        create_alg(**_inf_kwargs(policy_func_name="FiniteHorizonPolicy"))


def _query(fn="gops_rbf_rollout_workspace_bytes", *, fh=1, code=None, in_dim=4, K=35, tail=0, dtype=0):
    from gops_amd import hip_backend as hb
    env = hb.make_env(hb.ENV_LQ, 3, 1, act_low=-1.0, act_high=1.0,
                      lq=dict(inv_IA=np.eye(3), B=np.ones((3, 1)), Q=np.ones(3), R=np.ones(1), dt=0.1))
    d = hb.GopsRolloutDesc()
    d.batch, d.horizon, d.finite_horizon, d.need_grad, d.gamma, d.env = 64, 8, fh, 1, 1.0, env
    d.tail_value, d.dtype = tail, dtype
    d.policy.n_layers, d.policy.hidden_act = 1, hb.RBF_TANH if code is None else code
    d.policy.sizes[0], d.policy.sizes[1], d.policy.sizes[2] = in_dim, 1, K
    for i in (0, 1):   # (never dereferenced: the size query only checks the description)
        d.policy.weight[i] = d.policy.bias[i] = 256
    return getattr(hb.lib(), fn)(C.byref(d))


def test_rbf_descriptor_is_checked_by_the_library():
    """The ABI's own checks (host code, no launch) through the size query: 0 = refused."""
    from gops_amd import hip_backend as hb
    assert _query() > 0 and _query(K=64) > 0 and _query(K=1) > 0
    assert _query(fh=0, code=hb.RBF_AFFINE, in_dim=3) > 0
    assert _query(K=65) == 0 and _query(K=0) == 0
    assert _query(fh=1, in_dim=3) == 0                           # FiniteHorizonPolicy without the time column
    assert _query(fh=0, code=hb.RBF_AFFINE, in_dim=4) == 0       # DetermPolicy with one
    assert _query(fh=0, code=hb.RBF_TANH, in_dim=4) == 0         # a FiniteHorizonPolicy in an infinite-horizon rollout
    assert _query(fh=1, code=hb.RBF_AFFINE, in_dim=3) == 0       # a DetermPolicy in a finite-horizon one
    assert _query(tail=1) == 0
    assert _query(dtype=1) == 0
    assert _query("gops_poly_rollout_workspace_bytes") == 0      # an RBF net handed to the POLY entry point
    assert _query(code=hb.POLY_FULL[1], in_dim=3, K=4) == 0      # a POLY net handed to the RBF one ...
    assert _query("gops_poly_rollout_workspace_bytes", code=hb.POLY_FULL[1], in_dim=3, K=4) > 0   # ... which POLY's accepts
    assert _query("gops_rollout_workspace_bytes") == 0           # the MLP entry points keep rejecting n_layers = 1


def test_rbf_abi_mirrors():
    from gops_amd import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    for name in ("gops_rbf_rollout_workspace_bytes", "gops_rbf_rollout_forward", "gops_rbf_rollout_backward"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in hb.EXPORTED_SYMBOLS
        assert hasattr(C.CDLL(hb.LIB_PATH), name)
    codes = dict(re.findall(r"(GOPS_RBF_[A-Z]+) = (\d+)", header))
    assert int(codes["GOPS_RBF_AFFINE"]) == hb.RBF_AFFINE == 32 and int(codes["GOPS_RBF_TANH"]) == hb.RBF_TANH == 33
    assert int(re.search(r"#define GOPS_HIP_ABI_VERSION (\d+)", header).group(1)) == 15


def _rel(got, want):
    got, want = float(torch.as_tensor(got).detach()), float(torch.as_tensor(want).detach())
    return abs(got - want) / max(1.0, abs(want))


def _f64_value(value, act):
    """(V, leaves): an MLP StateValue in float64 whose parameters are autograd leaves, in `parameters()` order."""
    act_fn = dict(elu=torch.nn.functional.elu, relu=torch.relu, gelu=torch.nn.functional.gelu, tanh=torch.tanh)[act]
    leaves = [p.detach().double().clone().requires_grad_(True) for p in value.parameters()]
    n_lin = len(value.linear_layers())
    assert len(leaves) == 2 * n_lin

    def V(x):
        for i in range(n_lin):
            x = x @ leaves[2 * i].T + leaves[2 * i + 1]
            if i + 1 < n_lin:
                x = act_fn(x)
        return x.squeeze(-1)
    return V, leaves


@pytest.mark.parametrize("name", LQ_FHADP + LQ_INFADP)
def test_reference_fixtures_sit_inside_the_bar(name):
    """Every loss and every gradient tensor the reference recorded in fp32 is within 2.5e-5 - a quarter of the GPU tests' bar - of
    the float64 restatement (rbf_helpers.lq_rollout_f64) and its float64 autograd."""
    alg, g, cfg = load_alg(name, device="cpu")
    data = data_from_golden(g)
    env = alg._hip_env()
    low, high = policy_limits(alg.networks.policy)
    B, H, gamma = data["obs"].shape[0], cfg["horizon"], cfg["gamma"]
    params = f64_params(alg.networks.policy)
    figures = {}
    if cfg["alg"] == "FHADP":
        v = lq_rollout_f64(env, params, low, high, data["obs"], data["done"], H, gamma, fh=True)[0]
        loss = -v.mean()
        loss.backward()
        figures["loss"] = _rel(g["loss"], loss)
        for i, p in enumerate(params):
            figures[f"grad/{i} ({PARAMS[i]})"] = rel_l2(g[f"grad/{i}"], p.grad.reshape(g[f"grad/{i}"].shape))
    else:
        act = golden_meta(g)["extra"]["value_hidden_activation"]
        Vt, _ = _f64_value(alg.networks.v_target, act)
        V, v_leaves = _f64_value(alg.networks.v, act)
        ret = lq_rollout_f64(env, params, low, high, data["obs"], data["done"], H, gamma, fh=False, value=Vt)[0]
        v_now = V(data["obs"].double())
        loss_v = ((v_now - ret.detach()) ** 2).mean()
        loss_v.backward()
        figures["pev_loss"] = _rel(g["pev_loss"], loss_v)
        figures["pev_vmean"] = _rel(g["pev_vmean"], v_now.mean())
        for i, p in enumerate(v_leaves):
            figures[f"pev_grad/{i}"] = rel_l2(g[f"pev_grad/{i}"], p.grad)
        loss_p = -ret.mean()
        loss_p.backward()
        figures["pim_loss"] = _rel(g["pim_loss"], loss_p)
        for i, p in enumerate(params):
            figures[f"pim_grad/{i} ({PARAMS[i]})"] = rel_l2(g[f"pim_grad/{i}"], p.grad.reshape(g[f"pim_grad/{i}"].shape))
        assert B == 64
    print(name, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < FIXTURE_BAR, (k, v)
    # the cases test something: no gradient tensor is (nearly) zero
    assert all(float(p.grad.abs().max()) > 1e-6 for p in params), [float(p.grad.abs().max()) for p in params]
