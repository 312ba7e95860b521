"""DDPG / TD3 without a GPU: construction and RNG order, the reference's surface, refusals, registries, the C ABI of the new
entry points, and the update restated on the host against every fixture of tests/golden/make_golden_td3.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

from abi_helpers import check_abi
from ac_helpers import REFUSALS, TD3_ONE_UPDATE, TOL, alg_kwargs, check_host_restatement, check_refusals, close, q_names
from conftest import ROOT, golden_meta, load_golden, rel_l2

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer

TD3_KEYS = ["q1", "q2", "policy", "q1_target", "q2_target", "policy_target"]
DDPG_KEYS = ["q", "policy", "q_target", "policy_target"]


def _fresh(name):
    g = load_golden(name)
    meta = golden_meta(g)
    torch.manual_seed(meta["seed"])
    return create_alg(**alg_kwargs(meta, False)), g, meta


@pytest.mark.parametrize("name", ["td3_pend_relu", "td3_lqs4a2_gelu", "ddpg_pend_relu", "ddpg_lqs4a2_gelu"])
def test_construction_follows_the_reference(name):
    """Network names in construction order, the reference's state-dict keys, and the same RNG draws: the online networks of a fresh
    algorithm ARE the fixture's (the targets were moved by the fixture's maker; they start as copies of the online ones)."""
    alg, g, meta = _fresh(name)
    sd = alg.networks.state_dict()
    assert [n for n, _ in alg.networks.named_children()] == (TD3_KEYS if meta["cfg"]["alg"] == "TD3" else DDPG_KEYS)
    assert list(sd) == [k[3:] for k in g if k.startswith("sd/")]
    assert q_names(alg) == (("q1", "q2") if meta["cfg"]["alg"] == "TD3" else ("q",))
    for n in q_names(alg) + ("policy",):
        for k, v in getattr(alg.networks, n).state_dict().items():
            assert np.array_equal(v.numpy(), g[f"sd/{n}.{k}"]), (n, k)
            assert torch.equal(v, getattr(alg.networks, f"{n}_target").state_dict()[k])
    assert all(not p.requires_grad for n in sd if "_target." in n for p in [dict(alg.networks.named_parameters()).get(n)] if p is not None)
    alg.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")})   # loads unchanged


def test_surface_follows_the_reference():
    td3, _, _ = _fresh("td3_pend_relu")
    assert td3.adjustable_parameters == ("gamma", "tau", "delay_update", "reward_scale")
    assert (td3.gamma, td3.tau, td3.delay_update, td3.reward_scale, td3.per_flag, td3.fused_target) == (0.99, 0.005, 2, 1, False, True)
    kw = alg_kwargs(golden_meta(load_golden("td3_pend_relu")), False)
    kw.pop("target_noise"), kw.pop("noise_clip")
    plain = create_alg(**kw)
    assert (plain.target_noise, plain.noise_clip) == (0.2, 0.5)
    ddpg, _, _ = _fresh("ddpg_pend_relu")
    assert ddpg.adjustable_parameters == ("gamma", "tau", "delay_update")
    assert (ddpg.gamma, ddpg.tau, ddpg.delay_update, ddpg.per_flag) == (0.99, 0.005, 1, False)
    assert _fresh("td3_per_pend_relu")[0].per_flag and _fresh("ddpg_per_lqs4a2_gelu")[0].per_flag
    td3.set_parameters({"reward_scale": 0.1, "delay_update": 3})
    assert td3.get_parameters() == {"gamma": 0.99, "tau": 0.005, "delay_update": 3, "reward_scale": 0.1}
    with pytest.raises(RuntimeError):
        ddpg.set_parameters({"reward_scale": 0.1})
    from gops_amd.hip_backend import HipAdam
    for n in ("q1", "q2", "policy"):
        assert isinstance(getattr(td3.networks, f"{n}_optimizer"), HipAdam)


@pytest.mark.parametrize("alg", ["DDPG", "TD3"])
def test_refusals_carry_a_reason(alg):
    meta = golden_meta(load_golden("td3_pend_relu"))
    check_refusals(lambda **over: alg_kwargs(meta, False, **dict(dict(algorithm=alg), **over)),
                   REFUSALS + [(dict(policy_func_name="StochaPolicy"), "deterministic policy"),
                               (dict(value_func_name="StateValue"), "action-value")])


def test_registries():
    """The pinned key set of `registry` is untouched (tests/test_host_cpu.py); both names resolve through create_alg and
    create_approx_contrainer."""
    assert set(ca.registry) == {"FHADP", "FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "INFADP", "MAC", "MPG", "SPIL"}
    assert {"DDPG", "TD3", "RPI"} == set(ca.loop_registry)
    meta = golden_meta(load_golden("ddpg_pend_relu"))
    for alg in ("DDPG", "TD3"):
        kw = alg_kwargs(meta, False, algorithm=alg)
        assert type(create_alg(**kw)).__name__ == alg
        kw.pop("algorithm")
        nets = create_approx_contrainer(alg, **kw)
        assert [n for n, _ in nets.named_children()] == (TD3_KEYS if alg == "TD3" else DDPG_KEYS)
    with pytest.raises(KeyError):
        create_alg(**alg_kwargs(meta, False, algorithm="SAC"))


@pytest.mark.parametrize("name", TD3_ONE_UPDATE)
def test_host_restatement_matches_the_reference(name, capsys):
    """The fixture's state dict loaded into the networks create_alg built, one update restated on the host in fp32 (autograd over
    the modules' own `forward`): backup, losses and every gradient against the reference's, rel-L2 <= 1e-4.  This is the TEST's
    restatement (ac_helpers.restate_td3, the oracle of the GPU tests at float64): it shows that the modules are the reference's
    and that the oracle is faithful; the algorithm's own update has no host path and is held to the fixtures in test_td3_gpu.py."""
    alg, g, meta, got = check_host_restatement(name, ("backup", "a2", "q_targ"), "backup / a2 / q_targ", capsys)
    for n, l in zip(q_names(alg), got["loss_q"]):
        assert close(l, g[f"loss_{n}"]), n
    assert close(got["loss"], g["tb/Loss/Critic loss-RL iter"]) and close(got["loss_pi"], g["tb/Loss/Actor loss-RL iter"])
    logged = got["loss"] if meta["cfg"]["alg"] == "TD3" else got["q_mean"]   # td3.py:153 logs the mean of the scalar loss
    assert close(logged, g["tb/Train/Critic avg value-RL iter"])
    if meta["per"]:
        assert rel_l2(got["abs_err"], g["abs_err"]) <= TOL


def test_abi_of_the_actor_critic_entry_points(tmp_path):
    """Declared in the header (plain C99), mirrored by ctypes field for field, exported by the library; the version stays 15."""
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsAcBackup", hb.GopsAcBackup)], ("gops_ac_backup_workspace_bytes", "gops_ac_backup", "gops_ac_critic_loss"),
              [("GOPS_AC_LOSS_STATS_FLOATS", hb.AC_LOSS_STATS_FLOATS)])
    assert "actor_critic.hip" in open(os.path.join(ROOT, "gops_amd", "csrc", "Makefile")).read()


_SCRIPTS = ["example_train/td3/td3_mlp_cartpoleconti_offserial.py", "example_train/ddpg/ddpg_mlp_cartpoleconti_offserial.py"]


@pytest.mark.skipif(not os.path.isdir("/root/reference/gops"), reason="needs the GOPS tree (build container only)")
@pytest.mark.parametrize("script", _SCRIPTS)
def test_example_scripts_run_unchanged_through_the_overlay(script, tmp_path):
    """The reference's cartpoleconti example scripts, unmodified, through `gops_amd.overlay` (test_host_cpu.py's worker, existing
    stubs): create_alg builds the algorithm here, set_parameters, the sampler, the replay buffer and OffSerialTrainer run, and the
    first update fails only for want of a GPU."""
    import sys
    from test_host_cpu import _PLUMBING
    worker = tmp_path / "plumbing.py"
    worker.write_text(_PLUMBING)
    out = subprocess.run([sys.executable, str(worker), ROOT, os.path.join("/root/reference", script), str(tmp_path / "run")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "plumbing ok gops_amd.algorithm." in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
