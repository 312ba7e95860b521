"""SAC and DSAC without a GPU: registries, construction, mandatory arguments, refusals, the C ABI of the new entry points, and the
update restated on the host against every fixture of tests/golden/make_golden_sac.py."""
import pytest
import torch

from abi_helpers import check_abi
from ac_helpers import (REFUSALS, SAC_ONE_UPDATE, SOFT_REFUSALS, alg_kwargs, check_host_restatement, check_refusals,
                        check_soft_tb_and_alpha, q_names)
from conftest import golden_meta, load_golden

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer

CHILDREN = {"SAC": ["q1", "q2", "policy", "q1_target", "q2_target"], "DSAC": ["q", "q_target", "policy", "policy_target"]}
FIXTURE = {"SAC": "sac_pend_relu", "DSAC": "dsac_pend_relu_bound"}


def _kw(alg, **over):
    return alg_kwargs(golden_meta(load_golden(FIXTURE[alg])), False, **over)


def test_the_four_registries():
    assert set(ca.registry) == {"FHADP", "FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "INFADP", "MAC", "MPG", "SPIL"}
    assert {"DDPG", "TD3", "RPI"} == set(ca.loop_registry) and {"DSACT"} == set(ca.soft_registry)
    assert {"SAC", "DSAC"} == set(ca.soft_q_registry)


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_construction_follows_the_reference(name):
    """Children in the reference's construction order, the fixture's state-dict keys, HipAdam everywhere, the reference's adjustable
    parameters; the first critic of a fresh object IS the fixture's (same RNG draws)."""
    g = load_golden(FIXTURE[name])
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    alg = create_alg(**_kw(name))
    assert type(alg).__name__ == name
    kw = _kw(name)
    kw.pop("algorithm")
    for nets in (alg.networks, create_approx_contrainer(name, **kw)):
        assert [n for n, _ in nets.named_children()] == CHILDREN[name]
        assert list(nets.state_dict()) == [k[3:] for k in g if k.startswith("sd/")]
    assert q_names(alg) == {"SAC": ("q1", "q2"), "DSAC": ("q",)}[name]
    for n in q_names(alg)[:1]:   # (the fixture's maker shifted q2's output bias)
        for k, v in getattr(alg.networks, n).state_dict().items():
            assert torch.equal(v, torch.from_numpy(g[f"sd/{n}.{k}"])), (n, k)
    assert list(alg.networks.state_dict())[0] == "log_alpha" and alg.networks.log_alpha.item() == 1.0
    from gops_amd.hip_backend import HipAdam
    for n in q_names(alg) + ("policy", "alpha"):
        assert isinstance(getattr(alg.networks, f"{n}_optimizer"), HipAdam)
    assert all(not p.requires_grad for n, p in alg.networks.named_parameters() if "_target." in n)
    if name == "SAC":
        assert alg.adjustable_parameters == ("gamma", "tau", "auto_alpha", "alpha", "target_entropy")
        assert (alg.gamma, alg.tau, alg.auto_alpha, alg.alpha, alg.target_entropy, alg.fused_target) == (0.97, 0.005, True, 0.2, -1, True)
        assert create_alg(**_kw("SAC", target_entropy=-0.5)).target_entropy == -0.5
        assert not hasattr(alg.networks, "policy_target")
    else:
        assert alg.adjustable_parameters == ("gamma", "tau", "auto_alpha", "alpha", "bound", "delay_update")
        assert (alg.gamma, alg.tau, alg.auto_alpha, alg.alpha, alg.bound, alg.delay_update, alg.target_entropy) == (0.97, 0.005, True, 0.2, True, 2, -1)
    alg.set_parameters({"gamma": 0.9})
    assert alg.get_parameters()["gamma"] == 0.9


def test_mandatory_arguments_raise_the_references_key_error():
    """What the reference reads with kwargs[...]: KeyError(name), before any refusal - also for an argument set that a refusal
    would otherwise meet first (DDPG's and DSAC-T's sets carry value_learning_rate, not q_learning_rate)."""
    from gops_amd.algorithm import dsac, sac
    for name, mod in (("SAC", sac), ("DSAC", dsac)):
        for arg in mod.MANDATORY:
            kw = _kw(name)
            kw.pop(arg)
            with pytest.raises(KeyError, match=arg):
                create_alg(**kw)
    kw = _kw("SAC", policy_func_name="DetermPolicy")
    kw.pop("q_learning_rate")
    with pytest.raises(KeyError, match="q_learning_rate"):
        create_alg(**kw)


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_refusals_carry_a_reason(name):
    check_refusals(lambda **over: _kw(name, **over),
                   REFUSALS + SOFT_REFUSALS + [(dict(value_func_name="ActionValueDistri" if name == "SAC" else "ActionValue"),
                                                "an action-value function" if name == "SAC" else "distributional action-value"),
                                               (dict(value_func_name="StateValue"), "action-value")])


def test_abi_of_the_soft_q_entry_points(tmp_path):
    """Declared in the header (plain C99), mirrored by ctypes field for field, exported by the library; the version stays 15."""
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsSoftQBackup", hb.GopsSoftQBackup)], ("gops_soft_q_backup_workspace_bytes", "gops_soft_q_backup", "gops_dsac_critic_loss"),
              [("GOPS_DSAC_STATS_FLOATS", hb.DSAC_STATS_FLOATS)])
    assert [f[0] for f in hb.GopsSoftQBackup._fields_] == ["policy", "q", "n_q", "distri", "act_low", "act_high", "min_log_std", "max_log_std",
                                                           "gamma", "alpha", "log_alpha"]


@pytest.mark.parametrize("name", SAC_ONE_UPDATE)
def test_host_restatement_matches_the_reference(name, capsys):
    """The fixture's state dict loaded into the networks create_alg built, one update restated on the host in fp32 with the recorded
    draws: backup, samples, losses, every gradient, log_alpha's gradient and the tb values against the reference's, rel-L2 <= 1e-4.
    This is the TEST's restatement (the oracle of the GPU tests at float64): it shows that the modules and distributions are the
    reference's and that the oracle is faithful."""
    keys = ("backup", "a2", "logp_next", "q_targ", "new_act", "new_logp", "loss_q", "loss_pi") + (("td_bound",) if name.startswith("dsac") else ())
    alg, g, meta, got = check_host_restatement(name, keys, "backup / samples / losses", capsys)
    assert ("td_bound" in g) == name.startswith("dsac")
    check_soft_tb_and_alpha(alg, g, got)
    if "binds" in got:   # DSAC: the td_bound clamp binds on some rows and is idle on others
        assert got["binds"].any() and (~got["binds"]).any()
