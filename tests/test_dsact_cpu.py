"""DSAC-T without a GPU: registries, construction, the two continuous action distributions, refusals, the C ABI of the new entry
points, and the update restated on the host against every fixture of tests/golden/make_golden_dsact.py."""
import os

import pytest
import torch

from abi_helpers import check_abi
from ac_helpers import (DSACT_ONE_UPDATE, REFUSALS, SOFT_REFUSALS, alg_kwargs, batch_of, check_host_restatement, check_refusals,
                        check_soft_tb_and_alpha, q_names, restate_update)
from conftest import ROOT, golden_meta, load_golden, rel_l2

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer

KEYS = ["q1", "q2", "q1_target", "q2_target", "policy", "policy_target"]


def _kw(**over):
    return alg_kwargs(golden_meta(load_golden("dsact_pend_relu")), False, **over)


def test_registries_and_construction():
    """The pinned key sets are untouched; DSACT resolves through create_alg and create_approx_contrainer; children and state-dict
    keys are the reference's (the fixture's), log_alpha included; HipAdam everywhere."""
    assert set(ca.registry) == {"FHADP", "FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "INFADP", "MAC", "MPG", "SPIL"}
    assert {"DDPG", "TD3", "RPI"} == set(ca.loop_registry) and {"DSACT"} == set(ca.soft_registry)
    g = load_golden("dsact_pend_relu")
    alg = create_alg(**_kw())
    assert type(alg).__name__ == "DSACT" and q_names(alg) == ("q1", "q2")
    kw = _kw()
    kw.pop("algorithm")
    for nets in (alg.networks, create_approx_contrainer("DSACT", **kw)):
        assert [n for n, _ in nets.named_children()] == KEYS
        assert list(nets.state_dict()) == [k[3:] for k in g if k.startswith("sd/")]
    assert list(alg.networks.state_dict())[0] == "log_alpha" and alg.networks.log_alpha.item() == 1.0
    from gops_amd.hip_backend import HipAdam
    for n in ("q1", "q2", "policy", "alpha"):
        assert isinstance(getattr(alg.networks, f"{n}_optimizer"), HipAdam)
    assert alg.adjustable_parameters == ("gamma", "tau", "auto_alpha", "alpha", "delay_update")
    assert (alg.gamma, alg.tau, alg.tau_b, alg.auto_alpha, alg.delay_update, alg.target_entropy, alg.fused_target) == (0.97, 0.005, 0.005, True, 2, -1, True)
    assert alg.mean_std1 is None and alg.mean_std2 is None
    assert all(not p.requires_grad for n, p in alg.networks.named_parameters() if "_target." in n)
    with pytest.raises(KeyError):
        create_alg(**_kw(algorithm="SAC"))


@pytest.mark.parametrize("tag,cls", [("gauss", "GaussDistribution"), ("tanh_gauss", "TanhGaussDistribution")])
def test_distributions_against_the_reference(tag, cls):
    from gops_amd.utils import act_distribution as ad
    g, meta = load_golden("dsact_lqs4a2_gelu"), golden_meta(load_golden("dsact_lqs4a2_gelu"))
    t = lambda k: torch.from_numpy(g[f"dist/{tag}/{k}"])   # noqa: E731
    dist = getattr(ad, cls)(t("logits"))
    dist.act_low_lim, dist.act_high_lim = torch.tensor(meta["lim"][0]), torch.tensor(meta["lim"][1])
    act, logp = dist.rsample(t("eps"))
    torch.testing.assert_close(act, t("act"), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(logp, t("logp"), rtol=1e-5, atol=1e-5)
    sa, sl = dist.sample(t("eps"))
    assert torch.equal(sa, act) and torch.equal(sl, logp) and not sa.requires_grad
    torch.testing.assert_close(dist.log_prob(t("at")), t("log_prob"), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dist.mode(), t("mode"), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dist.entropy(), t("entropy"), rtol=1e-6, atol=1e-6)
    a, b = dist.sample(generator=torch.Generator().manual_seed(1)), dist.sample(generator=torch.Generator().manual_seed(1))
    assert torch.equal(a[0], b[0]) and a[0].shape == act.shape


def test_apprfunc_dict_resolves_the_distribution():
    from gops_amd.utils import act_distribution as ad
    from gops_amd.utils.common_utils import get_apprfunc_dict
    var = get_apprfunc_dict("policy", **_kw())
    assert var["action_distribution_cls"] is ad.TanhGaussDistribution
    assert (var["min_log_std"], var["max_log_std"], var["std_type"]) == (-3.0, -0.5, "mlp_shared")
    assert get_apprfunc_dict("policy", **_kw(policy_act_distribution="default"))["action_distribution_cls"] is ad.GaussDistribution
    assert get_apprfunc_dict("policy", **_kw(policy_act_distribution="default", policy_func_name="DetermPolicy"))["action_distribution_cls"] is ad.DiracDistribution
    plain = get_apprfunc_dict("value", **{k: v for k, v in _kw().items() if not k.startswith("policy_m")})
    assert (plain["min_log_std"], plain["max_log_std"]) == (-20.0, 2.0)
    with pytest.raises(NotImplementedError, match="CategoricalDistribution"):
        get_apprfunc_dict("policy", **_kw(policy_act_distribution="CategoricalDistribution"))
    from gops_amd.create_pkg.create_apprfunc import create_apprfunc
    for std_type in ("mlp_separated", "parameter"):
        with pytest.raises(NotImplementedError, match="mlp_shared"):
            create_apprfunc(**dict(var, std_type=std_type))


@pytest.mark.parametrize("name", DSACT_ONE_UPDATE)
def test_host_restatement_matches_the_reference(name, capsys):
    """The fixture's state dict loaded into the networks create_alg built, one update restated on the host in fp32 with the recorded
    draws: targets, the samples, every gradient, log_alpha's gradient, mean_std and the tb values against the reference's, rel-L2 <=
    1e-4.  This is the TEST's restatement (the oracle of the GPU tests at float64): it shows that the modules and distributions are
    the reference's and that the oracle is faithful."""
    keys = ("target_q", "target_q_sample", "a2", "logp_next", "q_targ", "new_act", "new_logp", "mean_std")
    alg, g, meta, got = check_host_restatement(name, keys, "targets / samples", capsys)
    check_soft_tb_and_alpha(alg, g, got)
    # fp32 still resolves 1 + 1e-6 - tanh(u)^2 on these rows: the fp32 log-probabilities are the float64 ones at 1e-5
    ref64 = restate_update(alg, batch_of(g))
    assert rel_l2(got["logp_next"], ref64["logp_next"]) <= 1e-5 and rel_l2(got["new_logp"], ref64["new_logp"]) <= 1e-5


def test_refusals_carry_a_reason():
    check_refusals(_kw, REFUSALS + SOFT_REFUSALS + [(dict(value_func_name="ActionValue"), "distributional action-value")])
    for alg in ("DDPG", "TD3"):   # unchanged: the deterministic algorithms still refuse a stochastic policy
        with pytest.raises(NotImplementedError, match="deterministic policy"):
            create_alg(**_kw(algorithm=alg, value_func_name="ActionValue"))


def test_abi_of_the_dsact_entry_points(tmp_path):
    """Declared in the header (plain C99), mirrored by ctypes field for field, exported by the library; the version stays 15."""
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsSoftBackup", hb.GopsSoftBackup), ("GopsTanhGauss", hb.GopsTanhGauss), ("GopsDsactState", 16)],
              ("gops_soft_backup_workspace_bytes", "gops_soft_backup", "gops_dsact_critic_loss", "gops_tanh_gauss_forward", "gops_tanh_gauss_backward"),
              [("GOPS_DSACT_STATS_FLOATS", hb.DSACT_STATS_FLOATS), ("GOPS_TANH_GAUSS_STATS_FLOATS", hb.TANH_GAUSS_STATS_FLOATS)])
    assert "dsact.hip" in open(os.path.join(ROOT, "gops_amd", "csrc", "Makefile")).read()
