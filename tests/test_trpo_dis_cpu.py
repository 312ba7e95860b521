"""TRPO on discrete actions without a GPU: the StochaPolicyDis approximator and its construction through create_alg, the refusals, the
C ABI and the refusal codes of the two categorical entry points, the identity the HIP Fisher-vector product rests on (Hessian of
the categorical KL at theta_old = J^T (diag p - p p^T) J / B) in float64, the whole update restated in float64 against every fixture
of tests/golden/make_golden_trpo_dis.py, and the sampler's categorical draw."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import trpo_dis_helpers as td
import trpo_helpers as th
from abi_helpers import check_abi
from ac_helpers import TOL, check_refusals, close
from conftest import rel_l2
from desc_helpers import BAD, ODD, UNS, P, mlp_desc

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg


def _kw(**over):
    return td.dis_kwargs(4, 2, [64, 64], "relu", **over)


# ---- approximator and construction -----------------------------------------------------------------------------------------------
def test_stocha_policy_dis_is_an_action_value_dis_under_another_name():
    from gops_amd.apprfunc import mlp
    from gops_amd.create_pkg.create_apprfunc import registry
    assert "StochaPolicyDis" in mlp.__all__ and "mlp_StochaPolicyDis" in registry
    assert issubclass(mlp.StochaPolicyDis, mlp.ActionValueDis)
    alg = create_alg(**_kw(action_num=3))
    pol = alg.networks.policy
    assert type(pol) is mlp.StochaPolicyDis and pol.act_num == 3
    assert list(pol.state_dict()) == ["q.0.weight", "q.0.bias", "q.2.weight", "q.2.bias", "q.4.weight", "q.4.bias"]
    logits = pol(torch.zeros(5, 4))
    assert logits.shape == (5, 3)
    from gops_amd.utils.act_distribution import CategoricalDistribution
    assert isinstance(alg.networks.create_action_distributions(logits), CategoricalDistribution)


@pytest.mark.parametrize("name", td.FIXTURES)
def test_fixtures_load_with_the_references_key_set(name):
    """The host StochaPolicyDis takes each fixture's `sd/` (the reference's keys, `policy.q.<i>.weight` ...), and construction through
    create_alg consumes the reference's RNG draws: the value net and the policy's hidden layers ARE the fixture's (the maker scales
    the policy's output layer only)."""
    alg, g, meta = td.fresh(name)
    keys = [k[3:] for k in g if k.startswith("sd/")]
    assert list(alg.networks.state_dict()) == keys and [n for n, _ in alg.networks.named_children()] == ["policy", "value"]
    n_lin = len(meta["cfg"]["hidden"]) + 1
    assert [k for k in keys if k.startswith("policy.")] == [f"policy.q.{2 * i}.{w}" for i in range(n_lin) for w in ("weight", "bias")]
    sd = alg.networks.state_dict()
    for k in keys:
        if k.startswith("value.") or (k.startswith("policy.") and not k.startswith(f"policy.q.{2 * (n_lin - 1)}.")):
            assert torch.equal(sd[k], torch.from_numpy(g["sd/" + k])), k
    alg.load_state_dict({k: torch.from_numpy(np.array(g["sd/" + k])) for k in keys})
    assert set(g["in/act"].reshape(-1).tolist()) == set(float(a) for a in range(meta["cfg"]["act_num"]))   # every action occurs
    assert g["in/obs"].shape[0] == 96 and g["in/act"].shape == (96, 1)
    if name == "trpo_dis_backtrack":
        assert int(g["accepted"]) >= 1
    if name == "trpo_dis_all_rejected":
        assert int(g["accepted"]) == -1


def test_refusals_carry_a_reason():
    new = [(dict(action_type="continu", action_dim=1, action_low_limit=np.array([-1.0], dtype=np.float32),
                 action_high_limit=np.array([1.0], dtype=np.float32)), "action_type 'discret' only"),
           (dict(action_num=1), "2 .. 16 discrete actions"),
           (dict(action_num=17), "2 .. 16 discrete actions"),
           (dict(policy_act_distribution="ValueDiracDistribution"), "categorical action distribution"),
           (dict(policy_act_distribution="GaussDistribution"), "categorical action distribution")]
    kept = [(dict(policy_func_name="DetermPolicyDis"), "stochastic policy with a Gaussian action distribution"),
            (dict(value_func_name="ActionValue"), "state-value function"),
            (dict(trainer="off_serial_trainer"), "on_serial_trainer only"),
            (dict(policy_func_type="POLY", policy_degree=1, policy_add_bias=False), "POLY"),
            (dict(policy_func_type="LipsNet"), "LipsNet"),
            (dict(mlp_dtype="fp16"), "fp32 only"),
            (dict(policy_output_activation="tanh"), "linear output")]
    check_refusals(_kw, new + kept)
    for over in (dict(), dict(policy_act_distribution="CategoricalDistribution"), dict(policy_std_type="mlp_shared"), dict(action_num=16)):
        assert type(create_alg(**_kw(**over))).__name__ == "TRPO"
    # PPO keeps refusing the combination, with its present reason: gops_ppo_loss is Gaussian
    ppo = dict(algorithm="PPO", learning_rate=1e-3, max_iteration=10, num_repeat=2, num_mini_batch=2, mini_batch_size=8, sample_batch_size=16)
    with pytest.raises(NotImplementedError, match="PPO takes a stochastic policy with a Gaussian action distribution"):
        create_alg(**_kw(**ppo))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_categorical_entry_points(tmp_path):
    check_abi(tmp_path, [], ("gops_cat_fisher_seed", "gops_cat_trpo_surrogate"),
              [("GOPS_TRPO_STATS_FLOATS", hb.TRPO_STATS_FLOATS), ("GOPS_TRPO_HYPER_FLOATS", hb.TRPO_HYPER_FLOATS),
               ("GOPS_DQN_MAX_ACTIONS", 16)])
    assert hb.lib().gops_hip_version() == 15
    assert hb.CatFisherSeed.run is hb.FisherSeed.run and hb.CatTrpoSurrogate.set_delta is hb.TrpoSurrogate.set_delta


def _mlp(sizes, **fields):
    return mlp_desc(sizes, act=hb.ACT_IDS["relu"], **fields)


def _grad(weight0=P, bias1=P):
    g = hb.GopsMlpGrad()
    for j in range(hb.MAX_LAYERS):
        g.weight[j] = g.bias[j] = P
    g.weight[0], g.bias[1] = weight0, bias1
    return g


def _seed_call(m=None, g=None, B=4, x=P, seed=P):
    m = _mlp([4, 64, 64, 2]) if m is None else m
    g = _grad() if g is None else g
    return hb.lib().gops_cat_fisher_seed(None if m == 0 else C.byref(m), None if g == 0 else C.byref(g), B, x, seed, None)


def _sur_call(n=2, M=4, new=P, old=P, act=P, adv=P, hyper=P, seed=None, stats=P):
    return hb.lib().gops_cat_trpo_surrogate(n, M, new, old, act, adv, hyper, seed, stats, None)


def test_refusal_codes_of_the_categorical_entry_points():
    """Every call is refused by an argument check in the entry point, before any HIP call: no device is needed (the pointers are never
    followed)."""
    assert _seed_call(m=0) == BAD and _seed_call(g=0) == BAD and _seed_call(x=None) == BAD and _seed_call(seed=None) == BAD
    assert _seed_call(B=0) == BAD
    assert _seed_call(g=_grad(weight0=None)) == BAD and _seed_call(g=_grad(bias1=None)) == BAD
    assert _seed_call(m=_mlp([4, 64, 2], n_layers=0)) == BAD and _seed_call(m=_mlp([4, 64, 2], n_layers=hb.MAX_LAYERS + 1)) == BAD
    assert _seed_call(m=_mlp([4, 64, 1])) == UNS and _seed_call(m=_mlp([4, 64, 17])) == UNS
    assert _seed_call(m=_mlp([4, 272, 2])) == UNS and _seed_call(m=_mlp([4, 24, 2])) == UNS
    assert _seed_call(m=_mlp([65, 64, 2])) == UNS
    assert _seed_call(m=_mlp([4, 2])) == UNS                                   # n_layers = 1: no hidden layer
    assert _seed_call(m=_mlp([4, 16, 16, 16, 16, 2])) == UNS                   # four hidden layers
    assert _seed_call(m=_mlp([4, 64, 1]), x=None) == BAD                       # (the pointers are checked first)
    for null in ("new", "old", "act", "adv", "hyper", "stats"):
        assert _sur_call(**{null: None}) == BAD, null
    assert _sur_call(M=0) == BAD and _sur_call(n=0) == BAD and _sur_call(stats=ODD) == BAD
    assert _sur_call(n=1) == UNS and _sur_call(n=17) == UNS
    assert _sur_call(n=17, M=0) == BAD


# ---- the identity the kernels rest on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[3, 16, 5], [4, 64, 64, 2]])
@pytest.mark.parametrize("act", ["relu", "gelu", "tanh"])
def test_the_categorical_kl_hessian_at_theta_old_is_its_gauss_newton_term(sizes, act, capsys):
    """Float64, autograd on both sides: the reference's double-backward `hvp` of mean KL(pi || pi_old) at theta = theta_old against
    J^T (diag p - p p^T) J v / B.  Both sides are float64 evaluations of the same quantity: 1e-10 relative to the largest element."""
    seq = th.mlp_stack(sizes, act, seed=3)
    g = torch.Generator().manual_seed(4)
    obs = torch.randn(48, sizes[0], generator=g, dtype=torch.float64)
    with torch.no_grad():   # logits of a spread that moves the probabilities well away from uniform
        head = [m for m in seq if isinstance(m, torch.nn.Linear)][-1]
        scale = 2.0 / seq(obs).std()
        head.weight.mul_(scale), head.bias.mul_(scale)
    tangent = [torch.randn(p.shape, generator=g, dtype=torch.float64) for p in seq.parameters()]
    want = th.flat(td.hessian_product(seq, obs, tangent))
    got = th.flat(td.gauss_newton_product(seq, obs, tangent))
    err = th.rel_max(got, want)
    with capsys.disabled():
        print(f"\n{sizes} {act}: softmax Gauss-Newton form against the double backward {err:.2e}")
    assert want.abs().max() > 0 and err <= 1e-10
    seed, _ = td.metric_seed(seq, obs, tangent)
    assert seed.sum(dim=-1).abs().max() <= 1e-12 * seed.abs().max()   # the rows of diag p - p p^T sum to zero


@pytest.mark.parametrize("name", td.FIXTURES)
def test_reference_accuracy_against_float64(name, capsys):
    """The whole update restated in float64 against what the fp32 reference recorded: the accepted index and every tried candidate's
    verdict are the same; the relative errors of g, x, step and the final policy ARE tests/golden/trpo_dis_reference_error.json - the
    GPU tests' bars are 4 x these.  Value parameters and tb values: 1e-4.  Every candidate keeps its distance from both thresholds."""
    alg, g, meta = td.load_trpo_dis(name)
    got = td.restate_trpo_update(alg, th.data_of(g))
    assert (-1 if got["index"] is None else got["index"]) == int(g["accepted"])
    assert len(got["cand"]) == len(g["cand_kl"])
    for (s, kl), s32, kl32 in zip(got["cand"], g["cand_surrogate"], g["cand_kl"]):
        assert (s > 0, kl < alg.delta) == (s32 > 0, kl32 < alg.delta)
    delta = meta["ctor"]["delta"]
    assert min(abs(float(k) - delta) / delta for k in g["cand_kl"]) > 0.02 and min(abs(float(s)) for s in g["cand_surrogate"]) > 1e-4
    after = np.concatenate([g["sd_after/policy." + k].reshape(-1) for k in alg.networks.policy.state_dict()])
    errors = dict(g=th.rel_max(g["g_vec"], got["g"]), x=th.rel_max(g["cg_x"], got["x"]), step=th.rel_max(g["trpo_step"], got["step"]),
                  policy=th.rel_max(after, th.flat(got["policy"])))
    with capsys.disabled():
        print(f"\n{name}: fp32 reference against float64 {errors}")
    stored = td.reference_error()[name]
    assert set(stored) == set(th.QUANTITIES)
    for k in th.QUANTITIES:
        assert errors[k] == pytest.approx(stored[k], rel=1e-6, abs=1e-300), k
    for k, v in zip([k for k in alg.networks.state_dict() if k.startswith("value.")], got["value"]):
        assert rel_l2(v, g["sd_after/" + k]) < TOL, k
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(got["tb"][k[3:]], g[k]), k
    if name == "trpo_dis_all_rejected":
        for k in [k for k in g if k.startswith("sd/policy.")]:
            assert np.array_equal(g[k], g["sd_after/" + k[3:]]), k


# ---- sampler -----------------------------------------------------------------------------------------------------------------------
def _cpu_sampler(**kw):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    model = create_env_model(env_id="gym_cartpoleconti")
    return DeviceEnvSampler(dict(env_id="gym_cartpoleconti"), model, n_envs=8, device="cpu", seed=3, action_table=[[-1.0], [1.0]], **kw)


def test_sampler_draws_the_index_from_the_softmax():
    """Fixed logits favouring action 1 with 0.9 / 0.1 over 4096 rows: the empirical frequency within 5 standard deviations of
    Binomial(4096, 0.9); the returned logp is the log-softmax at the drawn index; the draw is the sampler's own seeded generator's."""
    logits = torch.tensor([[0.0, math.log(9.0)]]).repeat(4096, 1)
    smp = _cpu_sampler()
    index, logp = smp.sample_index(logits)
    assert index.shape == (4096,) and index.dtype == torch.long and set(index.tolist()) == {0, 1}
    sigma = math.sqrt(4096 * 0.9 * 0.1)
    assert abs(int((index == 1).sum()) - 4096 * 0.9) <= 5 * sigma
    assert torch.equal(logp, torch.log_softmax(logits, dim=-1).gather(1, index[:, None]).squeeze(1))
    assert torch.allclose(logp.exp(), torch.where(index == 1, torch.tensor(0.9), torch.tensor(0.1)), rtol=1e-6, atol=0)
    again, _ = _cpu_sampler().sample_index(logits)
    assert torch.equal(index, again)


def test_sampler_refuses_epsilon_with_a_categorical_policy():
    """The first step with a StochaPolicyDis and epsilon > 0 raises before anything is stepped; an ActionValueDis (DQN) keeps its
    epsilon-greedy path."""
    from gops_amd.apprfunc.mlp import ActionValueDis
    alg = create_alg(**_kw())
    smp = _cpu_sampler(epsilon=0.1)
    smp.networks = alg.networks
    with pytest.raises(ValueError, match="epsilon > 0 with a StochaPolicyDis"):
        smp.sample()
    assert not isinstance(alg.networks.policy, type(None)) and isinstance(alg.networks.policy, ActionValueDis)
    values = torch.tensor([[0.0, 1.0]]).repeat(64, 1)
    assert torch.equal(_cpu_sampler().select_index(values), torch.ones(64, dtype=torch.long))
