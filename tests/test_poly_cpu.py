"""CPU: POLY approximators (gops_amd/apprfunc/poly.py) - host modules against the reference's outputs, state_dict layout, the shipped
checkpoint, get_apprfunc_dict's POLY branch, the refusals around it and the ABI v15 mirrors (header, ctypes, exports)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2

from gops_amd.utils.act_distribution import DiracDistribution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CKPT = "/root/reference/results/INFADP/lqs4a2_poly/apprfunc/apprfunc_115000_opt.pkl"


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)}


def test_host_modules_match_reference_outputs():
    from gops_amd.apprfunc import poly
    g = load_golden("poly_features")
    base = dict(act_high_lim=np.ones(2, dtype=np.float32), act_low_lim=-np.ones(2, dtype=np.float32),
                action_distribution_cls=DiracDistribution)
    for name, cls, n, kw in (("determ_d1", poly.DetermPolicy, 4, dict(degree=1, add_bias=False)),
                             ("determ_d2", poly.DetermPolicy, 4, dict(degree=2, add_bias=True)),
                             ("determ_d3", poly.DetermPolicy, 3, dict(degree=3, add_bias=False)),
                             ("fh_d1_bias", poly.FiniteHorizonPolicy, 3, dict(degree=1, add_bias=True))):
        net = cls(obs_dim=n, act_dim=2, **base, **kw)
        sd = _sd(g, f"{name}/sd/")
        assert set(net.state_dict()) == set(sd)
        net.load_state_dict(sd)
        x = torch.from_numpy(np.array(g[f"{name}/obs"]))
        if cls is poly.FiniteHorizonPolicy:
            for t in (1, 37):
                assert rel_l2(net(x, t).detach(), g[f"{name}/out_t{t}"]) < 1e-6
        else:
            assert rel_l2(net(x).detach(), g[f"{name}/out"]) < 1e-6
    for name in ("value_nobias", "value_bias"):
        sd = _sd(g, f"{name}/sd/")
        net = poly.StateValue(obs_dim=4, degree=2, add_bias="v.bias" in sd, norm_matrix=np.array(g[f"{name}/norm"]).tolist(),
                              action_distribution_cls=DiracDistribution)
        assert set(net.state_dict()) == set(sd)
        net.load_state_dict(sd)
        assert rel_l2(net(torch.from_numpy(np.array(g[f"{name}/obs"]))).detach(), g[f"{name}/out"]) < 1e-6


def _infadp_kwargs(**over):
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_lq", lq_config="s4a2",
              obsv_dim=4, action_dim=2, action_type="continu", action_high_limit=np.full(2, 8.0, dtype=np.float32),
              action_low_limit=np.full(2, -8.0, dtype=np.float32), policy_func_type="POLY", policy_func_name="DetermPolicy",
              policy_degree=1, policy_add_bias=False, policy_act_distribution="default", policy_learning_rate=8e-5,
              value_func_type="POLY", value_func_name="StateValue", value_degree=2, value_add_bias=False, value_learning_rate=3e-4,
              reward_scale=0.1, use_gpu=False)
    kw.update(over)
    return kw


def test_infadp_poly_state_dict_is_the_reference_layout():
    from gops_amd.create_pkg.create_alg import create_alg
    g = load_golden("infadp_trained_poly_lqs4a2")
    alg = create_alg(**_infadp_kwargs())
    want = set(k[3:] for k in g if k.startswith("sd/"))
    assert set(alg.networks.state_dict()) == want
    assert {"policy.pi.weight", "v.v.weight", "policy.act_high_lim", "policy.act_low_lim"} <= want
    alg.load_state_dict(_sd(g, "sd/"))
    assert torch.equal(alg.networks.policy.pi.weight.data, torch.from_numpy(np.array(g["sd/policy.pi.weight"])))


@pytest.mark.skipif(not os.path.exists(REF_CKPT), reason="needs the reference tree (build container only)")
def test_shipped_poly_checkpoint_loads_into_create_alg():
    from gops_amd.create_pkg.create_alg import create_alg
    alg = create_alg(**_infadp_kwargs())
    sd = torch.load(REF_CKPT, map_location="cpu")
    alg.networks.load_state_dict(sd)
    assert tuple(alg.networks.policy.pi.weight.shape) == (2, 4) and tuple(alg.networks.v.v.weight.shape) == (1, 10)


def test_get_apprfunc_dict_poly_branch_and_refusals():
    from gops_amd.utils.common_utils import get_apprfunc_dict
    kw = _infadp_kwargs(norm_matrix=[1.0, 2.0, 3.0, 4.0])
    var = get_apprfunc_dict("value", **kw)
    assert (var["degree"], var["add_bias"], var["norm_matrix"]) == (2, False, [1.0, 2.0, 3.0, 4.0])
    var = get_apprfunc_dict("policy", **_infadp_kwargs())
    assert (var["apprfunc"], var["degree"], var["add_bias"], var["norm_matrix"]) == ("POLY", 1, False, None)
    with pytest.raises(NotImplementedError, match="MLP and POLY only"):
        get_apprfunc_dict("policy", **_infadp_kwargs(policy_func_type="GAUSS"))


def test_poly_refusals_at_create_alg():
    from gops_amd.create_pkg.create_alg import create_alg
    for alg_name in ("MAC", "SPIL", "MPG", "FHADP2", "FHADPExterior"):
        with pytest.raises(NotImplementedError, match="POLY"):
            create_alg(**_infadp_kwargs(algorithm=alg_name, pre_horizon=10))
    with pytest.raises(NotImplementedError, match="POLY"):   # POLY policy with an MLP value
        create_alg(**_infadp_kwargs(value_func_type="MLP", value_hidden_sizes=[64, 64], value_hidden_activation="gelu"))
    with pytest.raises(NotImplementedError, match="POLY"):   # vehicle model
        create_alg(**dict(_infadp_kwargs(algorithm="FHADP", policy_func_name="FiniteHorizonPolicy", env_id="pyth_veh3dofconti",
                                         obsv_dim=46, action_dim=2, pre_horizon=10, lq_config=None)))


def test_fhadp_poly_builds_and_evaluates_on_the_host():
    from gops_amd.create_pkg.create_alg import create_alg
    g = load_golden("fhadp_poly_lqs2a1_h80")
    meta = golden_meta(g)
    kw = dict(algorithm="FHADP", trainer="off_serial_trainer", seed=meta["seed"], cnn_shared=False, env_id="pyth_lq",
              lq_config="s2a1", obsv_dim=2, action_dim=1, action_type="continu", action_high_limit=np.ones(1, dtype=np.float32),
              action_low_limit=-np.ones(1, dtype=np.float32), policy_func_name="FiniteHorizonPolicy",
              policy_act_distribution="default", policy_learning_rate=3e-4, pre_horizon=80, use_gpu=False, **meta["extra"])
    alg = create_alg(**kw)
    alg.load_state_dict(_sd(g, "sd/"))
    assert alg._poly and set(alg.networks.state_dict()) == {"policy.pi.weight", "policy.act_high_lim", "policy.act_low_lim"}
    obs = torch.from_numpy(np.array(g["in/obs"]))
    W = alg.networks.policy.pi.weight.detach()
    assert torch.allclose(alg.networks.policy(obs, 3), obs @ W[:, :2].T + 3 * W[:, 2], atol=1e-6)


def test_poly_abi_mirrors():
    """ABI v15: the POLY entry points are declared, mirrored in hip_backend and exported; the feature-map codes agree."""
    from gops_amd import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    for name in ("gops_poly_rollout_workspace_bytes", "gops_poly_rollout_forward", "gops_poly_rollout_backward",
                 "gops_poly_value_workspace_bytes", "gops_poly_value_forward", "gops_poly_value_backward"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in hb.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(hb.LIB_PATH), name)
    codes = dict(re.findall(r"(GOPS_POLY_[A-Z0-9_]+) = (\d+)", header))
    assert {int(codes[f"GOPS_POLY_FULL_{d}"]) for d in (1, 2, 3)} == set(hb.POLY_FULL.values())
    assert int(codes["GOPS_POLY_SYM_2"]) == hb.POLY_SYM_2
    assert int(re.search(r"#define GOPS_HIP_ABI_VERSION (\d+)", header).group(1)) == 15


def test_mismatched_poly_policies_are_refused():
    """FHADP reads a virtual_t column after the features, INFADP does not: a POLY DetermPolicy in FHADP or a POLY
    FiniteHorizonPolicy in INFADP would be read with the wrong row stride - both are refused at create_alg, and so is
    mlp_dtype fp16 (the POLY kernels are fp32 only)."""
    from gops_amd.create_pkg.create_alg import create_alg
    fh = dict(algorithm="FHADP", pre_horizon=10, policy_func_name="DetermPolicy")
    with pytest.raises(NotImplementedError, match="FiniteHorizonPolicy"):
        create_alg(**_infadp_kwargs(**fh))
    with pytest.raises(NotImplementedError, match="DetermPolicy"):
        create_alg(**_infadp_kwargs(policy_func_name="FiniteHorizonPolicy"))
    for over in (dict(fh, policy_func_name="FiniteHorizonPolicy"), {}):
        with pytest.raises(NotImplementedError, match="fp32"):
            create_alg(**_infadp_kwargs(mlp_dtype="fp16", **over))


def test_poly_descriptor_weight_columns_are_checked_by_the_library():
    """The ABI's own check (host code, no launch): GopsMlp.sizes[2] - the weight's column count - must equal the feature count
    plus the virtual_t column exactly when the rollout is finite-horizon; otherwise the description is rejected."""
    import ctypes as C
    from gops_amd import hip_backend as hb
    env = hb.make_env(hb.ENV_LQ, 3, 1, act_low=-1.0, act_high=1.0,
                      lq=dict(inv_IA=np.eye(3), B=np.ones((3, 1)), Q=np.ones(3), R=np.ones(1), dt=0.1))
    for fh in (0, 1):
        for cols in (12, 13):   # degree 2 on 3 observations: F = 3 + 9
            d = hb.GopsRolloutDesc()
            d.batch, d.horizon, d.finite_horizon, d.need_grad, d.gamma, d.env = 64, 8, fh, 1, 1.0, env
            d.policy.n_layers, d.policy.hidden_act = 1, hb.POLY_FULL[2]
            d.policy.sizes[0], d.policy.sizes[1], d.policy.sizes[2] = 3, 1, cols
            d.policy.weight[0] = 256   # (never dereferenced: the size query only checks the description)
            ok = hb.lib().gops_poly_rollout_workspace_bytes(C.byref(d)) > 0
            assert ok == (cols == 12 + fh), (fh, cols)


_POLY_SCRIPTS = ["example_train/fhadp/fhadp_poly_lqs2a1_serial.py", "example_train/infadp/infadp_poly_lqs4a2_offserial.py"]


@pytest.mark.skipif(not os.path.isdir("/root/reference/gops"), reason="needs the GOPS tree (build container only)")
@pytest.mark.parametrize("script", _POLY_SCRIPTS)
def test_poly_example_scripts_run_unchanged_through_the_overlay(script, tmp_path):
    """The reference's two POLY example scripts, unmodified, through `gops_amd.overlay` (test_host_cpu.py's worker): create_alg
    builds the POLY networks here, the trainer warms its buffer, and the first update fails only for want of a GPU."""
    import subprocess
    import sys
    from test_host_cpu import _PLUMBING
    worker = tmp_path / "plumbing.py"
    worker.write_text(_PLUMBING)
    out = subprocess.run([sys.executable, str(worker), ROOT, os.path.join("/root/reference", script), str(tmp_path / "run")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "plumbing ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
