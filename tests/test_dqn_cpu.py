"""DQN without a GPU: registries, construction and RNG order, the reference's surface, mandatory arguments and refusals, the C ABI of
the new entry points, the discrete branch of get_apprfunc_dict with its two distributions, the update restated on the host against
every fixture of tests/golden/make_golden_dqn.py, and DeviceEnvSampler's epsilon-greedy index selection."""
import os

import numpy as np
import pytest
import torch

from abi_helpers import check_abi
from ac_helpers import TOL, check_refusals, close
from conftest import ROOT, rel_l2
from dqn_helpers import DQN_FIVE_UPDATES, DQN_ONE_UPDATE, dqn_kwargs, fresh, load_dqn, restate_dqn
from helpers import data_from_golden

from gops_amd.create_pkg import create_alg as ca
from gops_amd.create_pkg.create_alg import create_alg, create_approx_contrainer


def test_registries():
    """DQN sits in a side registry that states MANDATORY / refusal itself; its stem is kept out of `registry` (whose key set
    tests/test_host_cpu.py pins).  The new registry's own key set is NOT pinned: the next algorithm joins it."""
    assert "DQN" in ca.value_based_registry
    assert ca.value_based_registry in ca._SIDE_REGISTRIES and ca.value_based_registry in ca._SELF_DESCRIBED
    assert "dqn" in ca._ELSEWHERE and "DQN" not in ca.registry
    assert ca._registry_of("DQN") is ca.value_based_registry
    with pytest.raises(KeyError):
        create_alg(**dqn_kwargs(3, 2, [32], "relu", algorithm="DQN2"))


@pytest.mark.parametrize("name", DQN_ONE_UPDATE + [DQN_FIVE_UPDATES])
def test_construction_follows_the_reference(name):
    """Network names in construction order, the reference's state-dict keys, and the same RNG draws: the online network of a fresh
    algorithm IS the fixture's (the target was moved by the fixture's maker; it starts as a copy of the online one)."""
    alg, g, meta = fresh(name)
    prefix = "sd0/" if name == DQN_FIVE_UPDATES else "sd/"
    sd = alg.networks.state_dict()
    assert [n for n, _ in alg.networks.named_children()] == ["q", "q_target"]
    assert list(sd) == [k[len(prefix):] for k in g if k.startswith(prefix)]
    for k, v in alg.networks.q.state_dict().items():
        assert np.array_equal(v.numpy(), g[f"{prefix}q.{k}"]), k
        assert torch.equal(v, alg.networks.q_target.state_dict()[k])
    assert all(not p.requires_grad for p in alg.networks.q_target.parameters()) and all(p.requires_grad for p in alg.networks.q.parameters())
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})   # loads unchanged
    nets = create_approx_contrainer("DQN", **{k: v for k, v in dqn_kwargs(3, 2, [32, 16], "relu").items() if k != "algorithm"})
    assert [n for n, _ in nets.named_children()] == ["q", "q_target"]


def test_surface_follows_the_reference():
    from gops_amd.apprfunc.mlp import ActionValueDis
    from gops_amd.hip_backend import HipAdam
    from gops_amd.utils.act_distribution import ValueDiracDistribution
    # the arguments of example_train/dqn/dqn_mlp_cartpole_offserial.py: gym_cartpole's four observations and two actions
    alg = create_alg(**dqn_kwargs(4, 2, [64, 64], "relu", seed=None, cnn_shared=None))
    assert alg.adjustable_parameters == ("gamma", "tau")
    assert (alg.gamma, alg.tau, alg.reward_scale, alg.per_flag, alg.fused_target, alg.backup_path) == (0.99, 0.005, 1, False, True, None)
    alg.set_parameters({"gamma": 0.99, "tau": 0.2})
    assert alg.get_parameters() == {"gamma": 0.99, "tau": 0.2}
    nets = alg.networks
    assert type(nets.q) is ActionValueDis and type(nets.q_target) is ActionValueDis and isinstance(nets.q_optimizer, HipAdam)
    assert [tuple(l.weight.shape) for l in nets.q.linear_layers()] == [(64, 4), (64, 64), (2, 64)]
    obs = torch.randn(5, 4)
    values = nets.policy(obs)   # the policy is the no-grad forward of q
    assert not values.requires_grad and torch.equal(values, nets.q(obs).detach())
    dist = nets.create_action_distributions(values)
    assert type(dist) is ValueDiracDistribution and torch.equal(dist.mode(), values.argmax(dim=-1))
    assert create_alg(**dqn_kwargs(4, 2, [64, 64], "relu", buffer_name="prioritized_replay_buffer")).per_flag
    for hook in ("local_update", "get_remote_update_info", "remote_update"):
        assert callable(getattr(alg, hook))


def test_mandatory_arguments_and_refusals():
    from gops_amd.algorithm import dqn
    assert dqn.MANDATORY == ("value_learning_rate", "buffer_name")
    for name in dqn.MANDATORY:
        kw = dqn_kwargs(3, 2, [32], "relu")
        kw.pop(name)
        with pytest.raises(KeyError, match=name):
            create_alg(**kw)
    check_refusals(lambda **over: dqn_kwargs(3, 2, [32], "relu", **over),
                   [(dict(value_func_type="POLY", value_degree=2, value_add_bias=False), "POLY"),
                    (dict(value_func_type="CNN"), "MLP value network only"),
                    (dict(value_func_name="ActionValue"), "ActionValueDis"),
                    (dict(value_func_name="StateValue"), "ActionValueDis"),
                    (dict(action_type="continu", action_dim=1, action_low_limit=-np.ones(1, np.float32),
                          action_high_limit=np.ones(1, np.float32)), "discrete action space"),
                    (dict(value_output_activation="tanh"), "linear output"),
                    (dict(mlp_dtype="fp16"), "fp32 only"),
                    (dict(trainer="off_sync_trainer"), "off_serial"),
                    (dict(trainer="off_async_trainer"), "off_serial")])


def test_abi_of_the_dqn_entry_points(tmp_path):
    """Declared in the header (plain C99), mirrored by ctypes field for field, exported by the library; the version stays 15."""
    from gops_amd import hip_backend as hb
    check_abi(tmp_path, [("GopsDqnBackup", hb.GopsDqnBackup)], ("gops_dqn_backup_workspace_bytes", "gops_dqn_backup", "gops_dqn_loss"),
              [("GOPS_DQN_MAX_ACTIONS", hb.DQN_MAX_ACTIONS), ("GOPS_DQN_LOSS_STATS_FLOATS", hb.DQN_LOSS_STATS_FLOATS)])
    assert "actor_critic.hip" in open(os.path.join(ROOT, "gops_amd", "csrc", "Makefile")).read()


def test_discrete_apprfunc_dict_and_distributions():
    from gops_amd.utils import act_distribution as ad
    from gops_amd.utils.common_utils import get_apprfunc_dict
    kw = dqn_kwargs(4, 5, [64, 48], "gelu")
    var = get_apprfunc_dict("value", **kw)
    assert (var["apprfunc"], var["name"], var["obs_dim"], var["act_num"]) == ("MLP", "ActionValueDis", 4, 5)
    assert (var["hidden_sizes"], var["hidden_activation"], var["output_activation"]) == ([64, 48], "gelu", "linear")
    assert "act_dim" not in var and "act_high_lim" not in var
    assert var["action_distribution_cls"] is ad.ValueDiracDistribution
    assert get_apprfunc_dict("value", **dict(kw, policy_func_name="StochaPolicyDis"))["action_distribution_cls"] is ad.CategoricalDistribution
    assert get_apprfunc_dict("value", **dict(kw, policy_act_distribution="CategoricalDistribution"))["action_distribution_cls"] is ad.CategoricalDistribution
    with pytest.raises(NotImplementedError, match="discrete actions"):
        get_apprfunc_dict("value", **dict(kw, policy_act_distribution="GaussDistribution"))
    with pytest.raises(KeyError):
        get_apprfunc_dict("value", **{k: v for k, v in kw.items() if k != "action_num"})
    # the continuous branch is as it was
    cont = dict(kw, action_type="continu", action_dim=2, action_low_limit=[-1.0, -2.0], action_high_limit=[1.0, 2.0], policy_func_name="DetermPolicy")
    var = get_apprfunc_dict("value", **cont)
    assert var["act_dim"] == 2 and "act_num" not in var and var["action_distribution_cls"] is ad.DiracDistribution

    logits = torch.tensor([[0.5, 2.0, -1.0], [3.0, 3.0, 1.0], [-2.0, -3.0, -1.0]])
    vd = ad.ValueDiracDistribution(logits)
    act, logp = vd.sample()
    assert torch.equal(act, torch.tensor([1, 0, 2])) and torch.equal(vd.mode(), act) and torch.equal(logp, torch.tensor([0.0]))
    cat = ad.CategoricalDistribution(logits)
    logsm = torch.log_softmax(logits, dim=-1)
    a = torch.tensor([[2], [0], [1]])
    assert torch.allclose(cat.log_prob(a), logsm.gather(1, a).squeeze(1)) and torch.allclose(cat.log_prob(a.squeeze(1)), cat.log_prob(a))
    assert torch.allclose(cat.entropy(), -(logsm.exp() * logsm).sum(-1)) and torch.equal(cat.mode(), torch.tensor([1, 0, 2]))
    other = ad.CategoricalDistribution(logits.flip(-1))
    assert torch.allclose(cat.kl_divergence(other), (logsm.exp() * (logsm - torch.log_softmax(logits.flip(-1), dim=-1))).sum(-1))
    torch.manual_seed(0)
    act, logp = cat.sample()
    assert act.shape == (3,) and act.dtype == torch.long and torch.allclose(logp, logsm.gather(1, act[:, None]).squeeze(1))


@pytest.mark.parametrize("name", DQN_ONE_UPDATE)
def test_host_restatement_matches_the_reference(name, capsys):
    """The fixture's state dict loaded into the networks create_alg built, one update restated on the host in fp32 (autograd over
    the modules' own `forward`): backup, q_targ, the loss and every gradient against the reference's, rel-L2 <= 1e-4.  This is the
    TEST's restatement (dqn_helpers.restate_dqn, the oracle of the GPU tests at float64); the algorithm's own update has no host
    path and is held to the fixtures in test_dqn_gpu.py."""
    alg, g, meta = load_dqn(name)
    got = restate_dqn(alg, data_from_golden(g), dtype=torch.float32)
    worst = max([rel_l2(got[k], g[k]) for k in ("backup", "q_targ")] + [rel_l2(gr, g[f"q_grad/{i}"]) for i, gr in enumerate(got["grads"]["q"])])
    with capsys.disabled():
        print(f"\n{name}: worst rel-L2 of backup / q_targ / gradients against the reference {worst:.2e}")
    assert worst <= TOL and close(got["loss"], g["loss_q"])
    # what the maker asserted is in the batch: every action the arg-max somewhere, every action taken, both values of done
    N = meta["case"]["act_num"]
    assert set(got["a_star"].tolist()) == set(range(N)) == set(g["in/act"].astype(int).reshape(-1).tolist())
    assert set(g["in/done"].tolist()) == {0.0, 1.0}


def _cpu_sampler(**kw):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    model = create_env_model(env_id="gym_cartpoleconti")
    return DeviceEnvSampler(dict(env_id="gym_cartpoleconti"), model, n_envs=8, device="cpu", seed=3, **kw)


def test_sampler_selects_indices_epsilon_greedy():
    """The index selection runs on whatever device the sampler's generator lives on: with epsilon 0 the arg-max; with epsilon 1 a
    uniform index whatever the values say; in between, exploration replaces about that share of the rows - and only those can differ
    from the arg-max.  Without a table nothing changes: no attribute of the continuous path depends on the new arguments."""
    values = torch.tensor([[0.0, 1.0, -1.0]]).repeat(4096, 1)
    greedy = _cpu_sampler(action_table=[[-1.0], [0.0], [1.0]])
    assert greedy.epsilon == 0.0 and torch.equal(greedy.select_index(values), torch.ones(4096, dtype=torch.long))
    uniform = _cpu_sampler(action_table=[[-1.0], [0.0], [1.0]], epsilon=1.0).select_index(values)
    counts = torch.bincount(uniform, minlength=3)
    assert counts.sum() == 4096 and (counts > 4096 / 3 - 5 * 31).all() and (counts < 4096 / 3 + 5 * 31).all()   # 5 sigma of Binomial(4096, 1/3)
    smp = _cpu_sampler(action_table=[[-1.0], [0.0], [1.0]], epsilon=0.25)
    picked = smp.select_index(values)
    off = (picked != 1).float().mean().item()   # explored AND drew another index: 0.25 * 2 / 3, 5 sigma = 0.029
    assert abs(off - 0.25 * 2 / 3) < 0.03
    again = _cpu_sampler(action_table=[[-1.0], [0.0], [1.0]], epsilon=0.25).select_index(values)
    assert torch.equal(picked, again)   # the sampler's own seeded generator
    assert smp.action_table.shape == (3, 1) and smp.action_table.dtype == torch.float32
    plain = _cpu_sampler()
    assert plain.action_table is None and plain.epsilon == 0.0
    with pytest.raises(ValueError, match="action_table"):
        _cpu_sampler(action_table=[-1.0, 1.0])


def test_evaluator_refuses_a_discrete_policy():
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.evaluator import Evaluator
    alg = create_alg(**dqn_kwargs(4, 2, [32], "relu"))
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        Evaluator(env_model=create_env_model(env_id="gym_cartpoleconti"), networks=alg.networks, cfg=dict(env_id="gym_cartpoleconti"),
                  num_eval_episode=2, eval_save=False)
