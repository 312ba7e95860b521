"""TRPO without a GPU: registries, construction, the mandatory arguments, refusals, the C ABI of the new entry points, the identity the
HIP Fisher-vector product rests on (Hessian of the KL at theta_old = its Gauss-Newton term) in float64, the whole update restated in
float64 against every fixture of tests/golden/make_golden_trpo.py (how far the fp32 REFERENCE sits from float64: the yardstick of
the GPU tests), the fixtures' distance from the line search's thresholds and their clamp coverage, and the host CG solver."""
import numpy as np
import pytest
import torch

import trpo_helpers as th
from abi_helpers import check_abi
from ac_helpers import REFUSALS, alg_kwargs, check_refusals
from conftest import golden_meta, load_golden

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer


def _kw(**over):
    return alg_kwargs(golden_meta(load_golden("trpo_pend_relu")), False, **over)


def test_the_six_registries():
    assert set(ca.registry) == {"FHADP", "FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "INFADP", "MAC", "MPG", "SPIL"}
    assert {"DDPG", "TD3", "RPI"} == set(ca.loop_registry) and {"DSACT"} == set(ca.soft_registry)
    assert {"SAC", "DSAC"} == set(ca.soft_q_registry) and {"PPO"} == set(ca.on_policy_registry)
    assert {"TRPO"} == set(ca.trust_region_registry)


def test_construction_follows_the_reference():
    """Children in the reference's order, the fixture's state-dict keys, a HipAdam over the value net only with value_learning_rate,
    the constructor's attributes and adjustable parameters; the RNG draws of construction are the reference's: a fresh value net IS
    the fixture's, a fresh policy is up to the maker's shaping of its head."""
    g = load_golden("trpo_pend_relu")
    torch.manual_seed(golden_meta(g)["seed"])
    alg = create_alg(**_kw())
    assert type(alg).__name__ == "TRPO"
    kw = _kw()
    kw.pop("algorithm")
    for nets in (alg.networks, create_approx_contrainer("TRPO", **kw)):
        assert [n for n, _ in nets.named_children()] == ["policy", "value"]
        assert list(nets.state_dict()) == [k[3:] for k in g if k.startswith("sd/")]
    for k, v in alg.networks.value.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g[f"sd/value.{k}"])), k
    assert torch.equal(alg.networks.policy.state_dict()["policy.0.weight"], torch.from_numpy(g["sd/policy.policy.0.weight"]))
    from gops_amd.hip_backend import HipAdam
    opt = alg.value_optimizer
    assert isinstance(opt, HipAdam) and len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == th.CTOR["value_learning_rate"]
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in alg.networks.value.parameters()]
    assert alg.adjustable_parameters == ("delta", "norm_adv", "train_v_iters", "value_learning_rate", "rtol", "atol", "damping_factor", "max_cg",
                                         "alpha", "max_search")
    assert (alg.delta, alg.rtol, alg.atol, alg.damping_factor, alg.max_cg, alg.alpha, alg.max_search, alg.train_v_iters, alg.norm_adv) == (
        0.01, 1e-5, 1e-8, 0.1, 10, 0.8, 10, 5, True)
    assert alg.last_cg_iterations is None and alg.last_search_index is None
    alg.set_parameters({"delta": 0.02})
    assert alg.get_parameters()["delta"] == 0.02


def test_every_missing_mandatory_argument_raises_a_key_error():
    from gops_amd.algorithm.trpo import MANDATORY
    assert MANDATORY == ("delta", "rtol", "atol", "damping_factor", "max_cg", "alpha", "max_search", "train_v_iters", "value_learning_rate")
    for name in MANDATORY:
        with pytest.raises(KeyError, match=name):
            create_alg(**{k: v for k, v in _kw().items() if k != name})


def test_refusals_carry_a_reason():
    own = [(dict(policy_func_name="DetermPolicy"), "stochastic policy"),
           (dict(policy_act_distribution="TanhGaussDistribution"), "Gaussian action distribution"),
           (dict(value_func_name="ActionValue"), "state-value function"),
           (dict(policy_std_type="parameter"), "'parameter' and 'mlp_separated' are not yet supported"),
           (dict(policy_std_type="mlp_separated"), "not yet supported"),
           (dict(trainer="off_serial_trainer"), "on_serial_trainer only"),
           (dict(trainer="on_sync_trainer"), "on_serial_trainer only")]
    generic = [(over, "on_serial" if "trainer" in over else reason) for over, reason in REFUSALS]
    check_refusals(_kw, generic + own)
    assert type(create_alg(**_kw(policy_act_distribution="GaussDistribution"))).__name__ == "TRPO"


def test_abi_of_the_trpo_entry_points(tmp_path):
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsCgState", hb.GopsCgState)],
              ("gops_gauss_fisher_seed", "gops_trpo_surrogate", "gops_cg_init", "gops_cg_step", "gops_cg_finish"),
              [("GOPS_TRPO_STATS_FLOATS", hb.TRPO_STATS_FLOATS), ("GOPS_TRPO_HYPER_FLOATS", hb.TRPO_HYPER_FLOATS),
               ("GOPS_CG_STATE_FLOATS", hb.CG_STATE_FLOATS), ("GOPS_CG_ONE_BLOCK_MAX", hb.CG_ONE_BLOCK_MAX)])
    import ctypes
    assert ctypes.sizeof(hb.GopsCgState) == 4 * hb.CG_STATE_FLOATS


@pytest.mark.parametrize("act", ["relu", "gelu", "tanh"])
def test_the_kl_hessian_at_theta_old_is_its_gauss_newton_term(act, capsys):
    """Float64, autograd on both sides: the reference's double-backward `hvp` of mean KL(pi || pi_old) at theta = theta_old against
    J^T M J v / B with M = diag(1 / sigma^2, 2 inside the closed clamp interval | 0 outside).  Rows below, inside and above the clamp.
    Both sides are float64 evaluations of the same quantity: 1e-10 relative to the largest element."""
    A, B = 2, 48
    seq = th.mlp_stack([5, 16, 32, 2 * A], act, seed=3)
    g = torch.Generator().manual_seed(4)
    obs = torch.randn(B, 5, generator=g, dtype=torch.float64)
    th.spread_log_std(seq, obs, A)
    with torch.no_grad():
        raw = seq(obs)[:, A:]
    below, inside, above = th.clamp_zones(raw)
    assert min(below, inside, above) >= 4, (below, inside, above)
    tangent = [torch.randn(p.shape, generator=g, dtype=torch.float64) for p in seq.parameters()]
    want = th.flat(th.hessian_product(seq, obs, tangent))
    got = th.flat(th.gauss_newton_product(seq, obs, tangent))
    err = th.rel_max(got, want)
    with capsys.disabled():
        print(f"\n{act}: Gauss-Newton form against the double backward {err:.2e} (zones {below}/{inside}/{above})")
    assert err <= 1e-10


@pytest.mark.parametrize("name", th.FIXTURES)
def test_reference_accuracy_against_float64(name, capsys):
    """The whole update restated in float64 against what the fp32 reference recorded: the accepted index and every tried candidate's
    verdict are the same; the relative errors (max |a - b| / max |b|) of g, x, step and the final policy ARE
    tests/golden/trpo_reference_error.json - the GPU tests' bars are 4 x these.  Value parameters and tb values: 1e-4."""
    from ac_helpers import TOL, close
    from conftest import rel_l2
    alg, g, meta = th.load_trpo(name)
    got = th.restate_trpo_update(alg, th.data_of(g))
    assert (-1 if got["index"] is None else got["index"]) == int(g["accepted"])
    assert len(got["cand"]) == len(g["cand_kl"])
    for (s, kl), s32, kl32 in zip(got["cand"], g["cand_surrogate"], g["cand_kl"]):
        assert (s > 0, kl < alg.delta) == (s32 > 0, kl32 < alg.delta)
    after = np.concatenate([g["sd_after/policy." + k].reshape(-1) for k in alg.networks.policy.state_dict() if k.startswith("policy.")])
    errors = dict(g=th.rel_max(g["g_vec"], got["g"]), x=th.rel_max(g["cg_x"], got["x"]), step=th.rel_max(g["trpo_step"], got["step"]),
                  policy=th.rel_max(after, th.flat(got["policy"])))
    with capsys.disabled():
        print(f"\n{name}: fp32 reference against float64 {errors}")
    stored = th.reference_error()[name]
    assert set(stored) == set(th.QUANTITIES)
    for k in th.QUANTITIES:
        assert errors[k] == pytest.approx(stored[k], rel=1e-6, abs=1e-300), k
    for k, v in zip([k for k in alg.networks.state_dict() if k.startswith("value.")], got["value"]):
        assert rel_l2(v, g["sd_after/" + k]) < TOL, k
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(got["tb"][k[3:]], g[k]), k
    if name == "trpo_pend_all_rejected":
        assert int(g["accepted"]) == -1
        for k in [k for k in g if k.startswith("sd/policy.")]:
            assert np.array_equal(g[k], g["sd_after/" + k[3:]]), k


@pytest.mark.parametrize("name", th.FIXTURES)
def test_fixtures_keep_their_distance_from_the_thresholds(name):
    """Every tried candidate: |kl - delta| > 0.02 delta and |surrogate| > 1e-4 (recomputed from the recorded values, and as the maker
    stored them); at least 4 raw log stds below, inside and above the clamp (counted on the float64 restatement)."""
    alg, g, meta = th.load_trpo(name)
    delta = meta["ctor"]["delta"]
    kl_gap = min(abs(float(k) - delta) / delta for k in g["cand_kl"])
    sur_gap = min(abs(float(s)) for s in g["cand_surrogate"])
    assert kl_gap > 0.02 and sur_gap > 1e-4
    assert kl_gap == pytest.approx(meta["kl_margin"]) and sur_gap == pytest.approx(meta["surrogate_margin"])
    zones = th.restate_trpo_update(alg, th.data_of(g))["zones"]
    assert min(zones) >= 4 and list(zones) == meta["zones"]
    B = g["in/obs"].shape[0]
    assert 64 <= B <= 256
    if name == "trpo_pend_backtrack":
        assert int(g["accepted"]) >= 1
    if name == "trpo_pend_no_norm":
        assert meta["ctor"]["norm_adv"] is False


def test_host_conjugate_gradient_matches_the_reference():
    """The static `_conjugate_gradient` on the dense SPD system the reference's own solver was recorded on (float64): after 4
    and after 40 iterations; `x` is updated in place as the reference's is."""
    from gops_amd.algorithm.trpo import TRPO
    g = load_golden("trpo_host_cg")
    A, b = torch.from_numpy(g["A"]), torch.from_numpy(g["b"])
    assert torch.linalg.eigvalsh(A).min() > 0
    for tag in ("few", "converged"):
        x0 = torch.zeros_like(b)
        x, r = TRPO._conjugate_gradient(lambda v: A @ v, b, x0, 1e-5, float(g[f"{tag}/atol"]), int(g[f"{tag}/max_cg"]))
        assert x is x0
        assert th.rel_max(x, g[f"{tag}/x"]) <= 1e-12 and float((r - torch.from_numpy(g[f"{tag}/r"])).abs().max()) <= 1e-12 * float(b.abs().max())
    # (with 40 iterations the residue stalls near 1e-6: the 1e-8 in both quotients damps the steps once p.Ap is that small)
    assert np.abs(g["converged/r"]).max() < 1e-5 < np.abs(g["few/r"]).max()
    x, r, n = th.solve_cg(lambda v: A @ v, b, float(g["few/atol"]), int(g["few/max_cg"]))
    assert n == 4 and th.rel_max(x, g["few/x"]) <= 1e-12   # (the helpers' recurrence, the GPU tests' float64 side)
