"""PPO without a GPU: registries, construction, the mandatory argument, refusals, the C ABI of the new entry points, the Gaussian's
closed forms, the loss restated on the host against every fixture of tests/golden/make_golden_ppo.py, the branch coverage of the
fixtures and of the GPU tests' synthetic minibatches, and the GAE restatement against the reference's `_finish_trajs`."""
import numpy as np
import pytest
import torch

from abi_helpers import check_abi
from ac_helpers import REFUSALS, TOL, alg_kwargs, check_refusals, close
from conftest import golden_meta, load_golden, rel_l2
from ppo_helpers import (HYPER, KERNEL_SHAPES, LOCAL_UPDATE, MARGIN, MIN_ROWS, ONE_STEP, TERMS, branches, hyper_of, load_ppo, minibatch_of,
                         restate_gae, restate_loss_with_seeds, restate_ppo_step, synthetic_minibatch, ulps32)

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer
from gops_amd.utils.act_distribution import GaussDistribution, TanhGaussDistribution


def _kw(**over):
    return alg_kwargs(golden_meta(load_golden("ppo_pend_relu")), False, **over)


def test_the_five_registries():
    assert set(ca.registry) == {"FHADP", "FHADP2", "FHADPExterior", "FHADPInterior", "FHADPLagrangian", "INFADP", "MAC", "MPG", "SPIL"}
    assert {"DDPG", "TD3", "RPI"} == set(ca.loop_registry) and {"DSACT"} == set(ca.soft_registry)
    assert {"SAC", "DSAC"} == set(ca.soft_q_registry) and {"PPO"} == set(ca.on_policy_registry)


def test_construction_follows_the_reference():
    """Children in the reference's order, the fixture's state-dict keys, ONE HipAdam over policy then value, the reference's
    attribute defaults and adjustable parameters; a fresh policy IS the fixture's up to the maker's shaping of its head."""
    g = load_golden("ppo_pend_relu")
    torch.manual_seed(golden_meta(g)["seed"])
    alg = create_alg(**_kw())
    assert type(alg).__name__ == "PPO"
    kw = _kw()
    kw.pop("algorithm")
    for nets in (alg.networks, create_approx_contrainer("PPO", **kw)):
        assert [n for n, _ in nets.named_children()] == ["policy", "value"]
        assert list(nets.state_dict()) == [k[3:] for k in g if k.startswith("sd/")]
    for k, v in alg.networks.value.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g[f"sd/value.{k}"])), k
    assert torch.equal(alg.networks.policy.state_dict()["policy.0.weight"], torch.from_numpy(g["sd/policy.policy.0.weight"]))
    from gops_amd.hip_backend import HipAdam
    opt = alg.approximate_optimizer
    assert isinstance(opt, HipAdam) and len(opt.param_groups) == 1
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in alg.networks.parameters()]
    assert alg.networks.policy.action_distribution_cls is GaussDistribution
    assert alg.adjustable_parameters == ("gamma", "reward_scale", "clip", "loss_value_clip", "value_clip", "loss_value_norm", "advantage_norm",
                                         "loss_coefficient_kl", "loss_coefficient_value", "loss_coefficient_entropy", "schedule_adam",
                                         "schedule_clip")
    assert (alg.clip, alg.clip_now, alg.EPS, alg.gamma, alg.reward_scale, alg.loss_coefficient_kl, alg.loss_coefficient_value,
            alg.loss_coefficient_entropy, alg.schedule_adam, alg.schedule_clip, alg.advantage_norm, alg.loss_value_clip, alg.value_clip,
            alg.loss_value_norm) == (0.2, 0.2, 1e-8, 0.99, 0.1, 0.2, 1.0, 0.0, "none", "none", True, True, 10.0, False)
    assert (alg.max_iteration, alg.num_repeat, alg.num_mini_batch, alg.mini_batch_size, alg.sample_batch_size) == (10, 1, 1, 70, 70)
    assert np.array_equal(alg.indices, np.arange(70)) and alg.learning_rate == 1e-3
    alg.set_parameters({"clip": 0.1})
    assert alg.get_parameters()["clip"] == 0.1


def test_a_missing_learning_rate_raises_the_references_key_error():
    kw = _kw()
    kw.pop("learning_rate")
    with pytest.raises(KeyError, match="learning_rate"):
        create_alg(**kw)
    with pytest.raises(TypeError):   # the five sizes are keyword-only without defaults, as in the reference
        create_alg(**{k: v for k, v in _kw().items() if k != "num_repeat"})


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
    assert type(create_alg(**_kw(policy_act_distribution="GaussDistribution"))).__name__ == "PPO"


def test_abi_of_the_ppo_entry_points(tmp_path):
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsPpoLoss", hb.GopsPpoLoss)], ("gops_ppo_loss", "gops_adv_normalize", "gops_gae"),
              [("GOPS_PPO_STATS_FLOATS", hb.PPO_STATS_FLOATS), ("GOPS_PPO_HYPER_FLOATS", hb.PPO_HYPER_FLOATS),
               ("GOPS_ADV_STATS_FLOATS", hb.ADV_STATS_FLOATS)])
    assert [f[0] for f in hb.GopsPpoLoss._fields_] == ["act_dim", "loss_value_clip", "loss_value_norm", "reserved", "min_log_std", "max_log_std"]


@pytest.mark.parametrize("name", ONE_STEP)
def test_kl_divergence_and_entropy_match_the_reference(name):
    """The closed forms against what the reference's distributions returned on the fixture's logits (make_golden_ppo.one_step_at)."""
    g = load_golden(name)
    logits = torch.from_numpy(g["in/logits"])
    new, old = GaussDistribution(logits), GaussDistribution(torch.flip(logits, dims=[0]))
    assert rel_l2(new.entropy(), g["dist/entropy"]) <= 1e-6 and rel_l2(old.kl_divergence(new), g["dist/kl"]) <= 1e-5
    assert torch.equal(TanhGaussDistribution(logits).kl_divergence(new), torch.zeros(logits.shape[0]))   # (inherited, as in the reference)
    assert (old.kl_divergence(new) >= 0).all()


@pytest.mark.parametrize("name", ONE_STEP + [LOCAL_UPDATE])
def test_host_restatement_matches_the_reference(name, capsys):
    """The fixture's state dict loaded into the networks create_alg built, the loss restated on the host in fp32: the six terms and
    every gradient against the reference's, rel-L2 <= 1e-4.  The local-update fixture is restated whole: the columns permuted by the
    recorded permutations, torch's Adam, both schedules - the state dict after the update, the last minibatch's gradients and tb
    values, the learning rate and clip_now."""
    alg, g, meta = load_ppo(name)
    if name != LOCAL_UPDATE:
        got = restate_ppo_step(alg, minibatch_of(g), dtype=torch.float32)
        worst = max([abs(got["terms"][k] - float(g["loss/" + k])) / max(1.0, abs(float(g["loss/" + k]))) for k in TERMS]
                    + [rel_l2(gr, g[f"{n}_grad/{i}"]) for n in ("policy", "value") for i, gr in enumerate(got["grads"][n])])
    else:
        nets = alg.networks
        opt = torch.optim.Adam(nets.parameters(), lr=meta["lr"])
        it, data = meta["iteration"], {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("in/")}
        data["adv"] = (data["adv"] - data["adv"].mean()) / (data["adv"].std() + alg.EPS)
        with torch.no_grad():
            data["val"], data["logits"] = nets.value(data["obs"]), nets.policy(data["obs"])
        for perm in data.pop("perm"):
            for n in range(alg.num_mini_batch):
                idx = perm[alg.mini_batch_size * n:alg.mini_batch_size * (n + 1)]
                got = restate_ppo_step(alg, {k: v[idx] for k, v in data.items()}, dtype=torch.float32)
                alg.clip_now = alg.clip * (1 - it / alg.max_iteration)
                for p, gr in zip(nets.parameters(), got["grads"]["policy"] + got["grads"]["value"]):
                    p.grad = gr
                opt.step()
                for group in opt.param_groups:
                    group["lr"] = alg.learning_rate * (1 - it / alg.max_iteration)
        worst = max([rel_l2(v, g["sd_after/" + k]) for k, v in nets.state_dict().items()]
                    + [rel_l2(gr, g[f"{n}_grad/{i}"]) for n in ("policy", "value") for i, gr in enumerate(got["grads"][n])])
        assert close(got["terms"]["loss_surrogate"], g["tb/Loss/Actor loss-RL iter"]) and close(got["terms"]["loss_value"], g["tb/Loss/Critic loss-RL iter"])
        assert close(got["terms"]["approximate_kl"], g["tb/PPO/KL_divergence-RL iter"])
        assert opt.param_groups[0]["lr"] == float(g["lr_after"]) and alg.clip_now == float(g["clip_now_after"])
    with capsys.disabled():
        print(f"\n{name}: worst rel-L2 of losses / gradients / parameters against the reference {worst:.2e}")
    assert worst <= TOL


def _assert_branches(got, adv, clip, value_clip, value, min_rows=MIN_ROWS):
    rows, gap = branches(got, adv, clip, value_clip, value=value)
    assert all(n >= min_rows for n in rows.values()), rows
    assert gap >= MARGIN, gap


@pytest.mark.parametrize("name", ONE_STEP + [LOCAL_UPDATE])
def test_fixtures_populate_every_branch(name):
    """Ratio below / inside / above the clip x advantage sign, value clipped / not, l2 > l1 / not, log std below / inside / above the
    clamp: at least 4 rows each on the float64 restatement, none within 1e-3 of a boundary.  The value branches exist where the
    fixture clips the value loss; the local-update fixture is counted on its whole sample batch at the parameters it starts from,
    where val_old is the value net's own output (no value branch to populate)."""
    alg, g, meta = load_ppo(name)
    if name == LOCAL_UPDATE:
        mb = {k: torch.from_numpy(np.array(g["in/" + k])) for k in ("obs", "act", "logp", "adv", "ret")}
        mb["adv"] = (mb["adv"] - mb["adv"].mean()) / (mb["adv"].std() + alg.EPS)
        with torch.no_grad():
            mb["val"], mb["logits"] = alg.networks.value(mb["obs"]), alg.networks.policy(mb["obs"])
    else:
        mb = minibatch_of(g)
    got = restate_ppo_step(alg, mb, dtype=torch.float64)
    _assert_branches(got, mb["adv"], alg.clip_now, alg.value_clip, value=alg.loss_value_clip and name != LOCAL_UPDATE)


@pytest.mark.parametrize("M,A", KERNEL_SHAPES)
def test_synthetic_minibatches_populate_every_branch(M, A):
    """The GPU tests' minibatches: no row within 1e-3 of a boundary at any size; every branch with at least 4 rows from 70 rows on
    (one and two rows cannot hold them)."""
    t = synthetic_minibatch(M, A)
    for norm in (False, True) if M > 1 else (False,):
        _, _, _, got = restate_loss_with_seeds(t, dict(HYPER, loss_value_clip=True, loss_value_norm=norm))
        _assert_branches(got, t["adv"], HYPER["clip"], HYPER["value_clip"], value=True, min_rows=MIN_ROWS if M >= 70 else 0)


def test_gae_restatement_meets_the_references_finish_trajs():
    """restate_gae against what `OnSampler._finish_trajs` wrote (float64 numpy stored to float32 arrays): within 2 fp32 ulp.  The
    fixture has segments ended by done, by the time limit and by the horizon, an environment with several ends and one with none."""
    g = load_golden("gae_segments")
    end, done = g["end"], g["done"]
    T, N = end.shape
    assert (T, N) == (12, 5) and (end[T - 1] == 1).all()
    inner = end[:T - 1]
    assert (inner.sum(axis=0) >= 3).any() and (inner.sum(axis=0) == 0).any()
    assert ((inner == 1) & (done[:T - 1] == 1)).any() and ((inner == 1) & (done[:T - 1] == 0)).any() and (done[T - 1] == 1).any()
    ret, adv = restate_gae(g["rew"], g["val"], g["val_next"], done, end, float(g["gamma"]), float(g["gae_lambda"]))
    assert ulps32(ret, g["ret"]) <= 2 and ulps32(adv, g["adv"]) <= 2
