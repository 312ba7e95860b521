"""LipsNet on the host: the eager module (gops_amd/apprfunc/lipsnet.py) against the reference fixtures of
tests/golden/make_golden_lipsnet.py, the `LipsNet` branch of get_apprfunc_dict / create_apprfunc and create_alg's refusals.

Bounds: relative L2 < 1e-5 in float64 (the reference's own fp32 results lie <= 6e-6 from the float64 restatement - this is the
fixtures' admission check as well), < 1e-4 in float32 (the bar tests/test_poly_gpu.py holds against fixtures)."""
import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import as_f64, data_from_golden, oracle_env

from oracle import adp_oracle as orc

CASES = ("lipsnet_lqs2a1_example", "lipsnet_lqs4a2_gelu_global_squash", "lipsnet_lqs6a3_tanh_local2")
BOUND = {torch.float64: 1e-5, torch.float32: 1e-4}


def policy_kwargs(meta, obs_dim, act_dim):
    from gops_amd.utils.common_utils import get_apprfunc_dict
    cfg, extra = meta["cfg"], meta["extra"]
    kw = dict(obsv_dim=obs_dim, action_dim=act_dim, action_type="continu", action_high_limit=np.ones(act_dim, dtype=np.float32),
              action_low_limit=-np.ones(act_dim, dtype=np.float32), policy_hidden_sizes=list(cfg["hidden"]),
              policy_hidden_activation=cfg["act"], policy_act_distribution="default")
    kw.update(extra)
    return get_apprfunc_dict("policy", **kw)


def load_policy(g, prefix="sd/policy.", dtype=torch.float32):
    from gops_amd.create_pkg.create_apprfunc import create_apprfunc
    meta = golden_meta(g)
    sd = {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)}
    obs_dim, act_dim = sd["pi.mlp.0.weight"].shape[1], sd["act_high_lim"].shape[0]
    torch.manual_seed(0)
    pol = create_apprfunc(**policy_kwargs(meta, obs_dim, act_dim))
    ours = pol.state_dict()
    assert set(ours) == set(sd)
    assert all(tuple(ours[k].shape) == tuple(sd[k].shape) for k in sd)
    pol.load_state_dict(sd, strict=True)
    return pol.to(dtype), meta


def pim_loss(g, pol, dtype):
    """-mean(r + gamma (1 - done') V_target(obs')) of one wrapped model step under `pol` (reference infadp.py:188-213)."""
    meta = golden_meta(g)
    cfg, extra = meta["cfg"], meta["extra"]
    env = oracle_env(cfg, extra, g)
    data = data_from_golden(g)
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")}
    vt = orc.net_from_state_dict(sd, "v_target.v", cfg["act"], requires_grad=False)
    if dtype == torch.float64:
        env, data, vt = as_f64(env), as_f64(data), as_f64(vt)
    a = pol(data["obs"])
    o2, r, d, _ = orc.env_forward(env, data["obs"], a, data["done"].bool(), {})
    v = r + (~d) * cfg["gamma"] * orc.value_forward(vt, o2)
    return -v.mean()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_eager_module_reproduces_reference_actions_and_pim_gradients(name, dtype):
    g = load_golden(name)
    pol, meta = load_policy(g, dtype=dtype)
    obs = torch.from_numpy(g["in/obs"]).to(dtype)
    pol.eval()
    with torch.no_grad():
        act_eval, K, _ = pol.forward_parts(obs)
    pol.train()
    act_train = pol(obs).detach()
    figures = dict(act_eval=rel_l2(act_eval, g["act_eval"]), act_train=rel_l2(act_train, g["act_train"]), K=rel_l2(K, g["K"]))
    pol.zero_grad()
    loss = pim_loss(g, pol, dtype)
    loss.backward()
    figures["pim_loss"] = abs(loss.item() - float(g["pim_loss"])) / abs(float(g["pim_loss"]))
    for i, p in enumerate(pol.parameters()):
        figures[f"pim_grad/{i}"] = rel_l2(p.grad, g[f"pim_grad/{i}"])
    print(name, dtype, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < BOUND[dtype], (k, v)


def test_regular_loss_only_in_training_mode_with_gradients():
    g = load_golden(CASES[0])
    pol, _ = load_policy(g, dtype=torch.float64)
    obs = torch.from_numpy(g["in/obs"]).double()
    w = torch.randn(obs.shape[0], 1, dtype=torch.float64, generator=torch.Generator().manual_seed(3))

    def k_grads(train, lam=None):
        pol.train(train)
        if lam is not None:
            pol.pi.loss_lambda = lam
        pol.zero_grad()
        (pol(obs) * w).sum().backward()
        return torch.cat([p.grad.reshape(-1).clone() for p in pol.lips_parameters()])

    lam = pol.pi.loss_lambda
    g_eval, g_train, g_train0 = k_grads(False), k_grads(True), k_grads(True, 0.0)
    pol.pi.loss_lambda = lam
    assert torch.equal(g_eval, g_train0)            # eval mode: the plain gradient
    assert not torch.allclose(g_eval, g_train, rtol=1e-9, atol=0)
    # the difference is the gradient of lambda * mean K^2
    pol.eval()
    pol.zero_grad()
    (lam * (pol.pi.K(obs) ** 2).mean()).backward()
    reg = torch.cat([p.grad.reshape(-1) for p in pol.lips_parameters()])
    assert rel_l2(g_train - g_eval, reg) < 1e-9
    # under no_grad nothing is recorded, in either mode
    pol.train()
    with torch.no_grad():
        a = pol(obs)
    assert not a.requires_grad
    pol.eval()
    with torch.no_grad():
        assert torch.allclose(a, pol(obs), rtol=1e-12, atol=0)


def test_apprfunc_dict_groups_and_initialisation():
    from gops_amd.create_pkg.create_apprfunc import create_apprfunc, registry
    meta = golden_meta(load_golden(CASES[0]))
    kw = policy_kwargs(meta, 2, 1)
    for key in ("lips_init_value", "lips_auto_adjust", "lips_learning_rate", "lips_hidden_sizes", "eps", "lambda", "local_lips",
                "squash_action", "learning_rate", "hidden_sizes", "hidden_activation", "output_activation"):
        assert key in kw, key
    assert kw["apprfunc"] == "LipsNet" and "lipsnet_DetermPolicy" in registry
    torch.manual_seed(5)
    pol = create_apprfunc(**kw)
    assert not pol.training   # the reference's constructor ends with self.eval()
    groups = pol.param_groups()
    assert [gr["lr"] for gr in groups] == [kw["learning_rate"], kw["lips_learning_rate"]]
    assert [id(p) for gr in groups for p in gr["params"]] == [id(p) for p in pol.parameters()]   # mlp, then K
    assert list(pol.state_dict()) == ["act_high_lim", "act_low_lim", "pi.mlp.0.weight", "pi.mlp.0.bias", "pi.mlp.2.weight", "pi.mlp.2.bias",
                                      "pi.mlp.4.weight", "pi.mlp.4.bias", "pi.K.K.0.weight", "pi.K.K.0.bias", "pi.K.K.2.weight", "pi.K.K.2.bias"]
    # lips_init_value sits on the K head's bias (local) or is the scalar (global): same seed, lips_init_value = 0 gives the bare draw
    torch.manual_seed(5)
    bare = create_apprfunc(**dict(kw, lips_init_value=0.0))
    assert torch.equal(pol.pi.K.K[-2].weight, bare.pi.K.K[-2].weight)
    assert abs((pol.pi.K.K[-2].bias - bare.pi.K.K[-2].bias).item() - kw["lips_init_value"]) < 1e-6
    glob = create_apprfunc(**dict(kw, local_lips=False, lips_hidden_sizes=None, lips_init_value=2.5))
    assert glob.pi.K.K.item() == 2.5 and list(glob.state_dict())[-1] == "pi.K.K"
    with pytest.raises(NotImplementedError, match="StochaPolicy"):
        create_apprfunc(**dict(kw, name="StochaPolicy"))
    with pytest.raises(NotImplementedError, match="output activation"):
        create_apprfunc(**dict(kw, output_activation="tanh"))
    with pytest.raises(NotImplementedError, match="fp16"):
        create_apprfunc(**dict(kw, mlp_dtype="fp16"))


def _infadp_kwargs(**change):
    meta = golden_meta(load_golden(CASES[0]))
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=1, env_id="pyth_lq", lq_config="s2a1", obsv_dim=2, action_dim=1,
              action_type="continu", action_high_limit=np.ones(1, dtype=np.float32), action_low_limit=-np.ones(1, dtype=np.float32),
              policy_hidden_sizes=[64, 64], policy_hidden_activation="relu", policy_act_distribution="default",
              value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation="relu",
              value_learning_rate=8e-5, use_gpu=False)
    kw.update(meta["extra"])
    kw.update(change)
    return kw


@pytest.mark.parametrize("change", [dict(algorithm="FHADP", policy_func_name="DetermPolicy"), dict(algorithm="MAC"), dict(algorithm="MPG"),
                                    dict(value_func_type="LipsNet"), dict(value_func_type="POLY", value_degree=2, value_add_bias=False),
                                    dict(policy_func_name="StochaPolicy"), dict(env_id="pyth_veh3dofconti", pre_horizon=10, obsv_dim=46, action_dim=2,
                                                                                 action_high_limit=np.ones(2, dtype=np.float32),
                                                                                 action_low_limit=-np.ones(2, dtype=np.float32)),
                                    dict(mlp_dtype="fp16")],
                         ids=["fhadp", "mac", "mpg", "lipsnet_value", "poly_value", "stocha", "veh3dof", "fp16"])
def test_create_alg_refuses_lipsnet_outside_its_path(change):
    from gops_amd.create_pkg.create_alg import create_alg
    with pytest.raises(NotImplementedError, match="LipsNet"):
        create_alg(**_infadp_kwargs(**change))


def test_create_alg_builds_infadp_with_a_lipsnet_policy():
    """The one combination that runs: INFADP, LipsNet DetermPolicy, MLP StateValue - two optimizer groups at their own rates."""
    from gops_amd.apprfunc.lipsnet import DetermPolicy
    from gops_amd.create_pkg.create_alg import create_alg
    kw = _infadp_kwargs()
    alg = create_alg(**kw)
    pol = alg.networks.policy
    assert isinstance(pol, DetermPolicy) and isinstance(alg.networks.policy_target, DetermPolicy)
    groups = alg.networks.policy_optimizer.param_groups
    assert [gr["lr"] for gr in groups] == [kw["policy_learning_rate"], kw["policy_lips_learning_rate"]]
    assert [id(p) for gr in groups for p in gr["params"]] == [id(p) for p in pol.parameters()]
    assert not any(p.requires_grad for p in alg.networks.policy_target.parameters())
    alg.set_parameters({"gamma": 0.99, "tau": 0.2, "forward_step": 1})   # the example's call
    with pytest.raises(NotImplementedError, match="forward_step = 1 only"):
        alg.set_parameters({"forward_step": 2})


def test_lips_entry_points_and_ctypes_mirrors(tmp_path):
    """The three entry points are additive (the ABI version stays 15) and the two ctypes mirrors have the header's layout."""
    from abi_helpers import check_abi, layout_probe
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [], ("gops_lips_workspace_bytes", "gops_lips_forward", "gops_lips_backward"), [])
    layout_probe(tmp_path, [("GopsLipsNet", hb.GopsLipsNet), ("GopsLipsGrad", hb.GopsLipsGrad)], c_names={"lam": "lambda"})
