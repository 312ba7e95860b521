"""The LipsNet tangent-propagation kernels (csrc/rollout_lips.hip through hip_backend.LipsPolicy) against the float64 eager
module (gops_amd/apprfunc/lipsnet.py `.double()`), tensor by tensor.

Bounds (the issue's): actions, K and N < 1e-5, every mlp and K gradient < 1e-4, relative L2.  Shapes: B = 1 / 64 / 65 / 300 are the
smallest that give one sample, whole tiles (16 samples per workgroup), a partial tile and - at 300 - several row slabs of the
weight-gradient GEMM (64 samples each); obs / act dims 2/1, 4/2, 6/3 and the 8/4 bound."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def make_policy(n, m, hidden, act, lips_hidden, squash, seed, lam=1e-3, eps=1e-4, init=1.0):
    from gops_amd.apprfunc.lipsnet import DetermPolicy
    from gops_amd.utils.act_distribution import DiracDistribution
    torch.manual_seed(seed)
    lo = -np.linspace(1.0, 2.0, m).astype(np.float32)
    hi = np.linspace(0.5, 1.5, m).astype(np.float32)
    pol = DetermPolicy(obs_dim=n, act_dim=m, hidden_sizes=hidden, hidden_activation=act, output_activation="linear",
                       lips_init_value=init, lips_auto_adjust=True, lips_learning_rate=1e-5, lips_hidden_sizes=lips_hidden, eps=eps,
                       **{"lambda": lam}, local_lips=lips_hidden is not None, squash_action=squash, learning_rate=3e-5,
                       act_high_lim=hi, act_low_lim=lo, action_distribution_cls=DiracDistribution)
    with torch.no_grad():   # biases away from zero (the initialisation leaves nn.Linear's small uniform draw)
        for p in pol.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return pol


def reference(pol, obs, grad_action, training):
    ref = copy.deepcopy(pol).cpu().double()
    ref.train(training)
    ref.zero_grad()
    act, K, N = ref.forward_parts(obs.cpu().double())
    (act * grad_action.cpu().double()).sum().backward()
    return act.detach(), K.detach(), N.detach(), [p.grad.clone() for p in ref.parameters()]


def run_kernel(pol, obs, grad_action, training):
    from gops_amd import hip_backend as hb
    lp = hb.LipsPolicy(pol, obs.shape[0])
    act, K, N = lp.forward(obs, training=training)
    grads = [g.clone() for g in lp.backward(grad_action)]
    torch.cuda.synchronize()
    return lp, act, K, N, grads


def check(pol, B, training, seed, grad_action=None):
    g = torch.Generator().manual_seed(seed)
    n = pol.pi.linear_layers()[0].in_features
    m = pol.pi.linear_layers()[-1].out_features
    obs = torch.randn(B, n, generator=g).cuda()
    ga = (torch.randn(B, m, generator=g) if grad_action is None else grad_action).cuda()
    pol = pol.cuda()
    _, act, K, N, grads = run_kernel(pol, obs, ga, training)
    r_act, r_K, r_N, r_grads = reference(pol, obs, ga, training)
    names = [k for k, _ in pol.named_parameters()]
    figures = dict(action=rel_l2(act.cpu(), r_act), K=rel_l2(K.cpu(), r_K), N=rel_l2(N.cpu(), r_N))
    figures.update({nm: rel_l2(gk.cpu(), gr) for nm, gk, gr in zip(names, grads, r_grads)})
    print({k: f"{v:.1e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < (1e-5 if k in ("action", "K", "N") else 1e-4), (k, v)
    return obs, ga, grads


# (n, m, hidden, act, lips_hidden, squash, B, training): each activation once, global and local K, squash and training on and off
KERNEL_CASES = [
    (2, 1, [64, 64], "relu", [32], False, 64, True),
    (2, 1, [64, 64], "relu", [32], False, 1, False),
    (4, 2, [64, 64], "gelu", None, True, 65, True),
    (6, 3, [32, 32, 32], "tanh", [16, 16], False, 300, True),
    (4, 2, [48], "elu", None, False, 65, False),
    (6, 3, [16, 256], "selu", [256], True, 64, True),
    # (no squash here: three sigmoid layers have a Jacobian norm of ~1e-3, y = K f / N is in the hundreds and tanh(y) is +-1 to the
    #  last bit - action and gradient of a saturated squash test nothing)
    (8, 4, [256, 256, 256], "sigmoid", [32, 16], False, 300, False),
    (2, 1, [64, 64], "gelu", [32], True, 300, True),
]


@pytest.mark.parametrize("n,m,hidden,act,lips_hidden,squash,B,training", KERNEL_CASES,
                         ids=[f"n{c[0]}m{c[1]}_{c[3]}_{'local' if c[4] else 'global'}_B{c[6]}" for c in KERNEL_CASES])
def test_kernels_match_float64_module(n, m, hidden, act, lips_hidden, squash, B, training):
    pol = make_policy(n, m, hidden, act, lips_hidden, squash, seed=11 + B + n)
    check(pol, B, training, seed=5 + B)


def test_zero_jacobian_rows():
    """relu with a first-layer bias of -10: J = 0 on every row, the action is K f / eps, gradients finite and equal to torch's."""
    pol = make_policy(2, 1, [32, 32], "relu", [16], False, seed=3)
    with torch.no_grad():
        pol.pi.mlp[0].bias.fill_(-10.0)
    obs, ga, grads = check(pol, 65, True, seed=9)
    from gops_amd import hip_backend as hb
    act, K, N = hb.LipsPolicy(pol, 65).forward(obs)
    assert torch.all(N == 0)
    f = pol.pi.mlp(obs)
    assert rel_l2(act.cpu(), (K.unsqueeze(1) * f / pol.pi.eps).detach().cpu()) < 1e-5
    assert all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("B,row", [(64, 0), (64, 15), (64, 16), (65, 64), (300, 299)])
def test_one_hot_grad_action(B, row):
    """One seeded row: first and last row of a tile, the last valid row of a partial tile - nothing leaks from rows beyond the batch."""
    pol = make_policy(4, 2, [64, 32], "tanh", [16], True, seed=21)
    ga = torch.zeros(B, 2)
    ga[row, 1] = 1.0
    check(pol, B, False, seed=31, grad_action=ga)


@pytest.mark.parametrize("B", [1, 300])
def test_backward_is_bitwise_reproducible(B):
    pol = make_policy(6, 3, [64, 64], "gelu", [32], False, seed=7).cuda()
    g = torch.Generator().manual_seed(B)
    obs, ga = torch.randn(B, 6, generator=g).cuda(), torch.randn(B, 3, generator=g).cuda()
    lp, _, _, _, first = run_kernel(pol, obs, ga, True)
    lp.forward(obs, training=True)
    second = [x.clone() for x in lp.backward(ga)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert any(a.abs().max() > 0 for a in first)


def test_entry_points_refuse_what_they_do_not_run():
    from gops_amd import hip_backend as hb
    for kw in (dict(n=9, m=1, hidden=[64]), dict(n=2, m=1, hidden=[24]), dict(n=2, m=1, hidden=[64] * 4), dict(n=2, m=5, hidden=[64])):
        pol = make_policy(kw["n"], kw["m"], kw["hidden"], "relu", None, False, seed=1).cuda()
        with pytest.raises(RuntimeError, match="gops_lips_workspace_bytes"):
            hb.LipsPolicy(pol, 8)
    pol = make_policy(2, 1, [64], "relu", [16, 16, 16], False, seed=1).cuda()
    with pytest.raises(RuntimeError, match="gops_lips_workspace_bytes"):
        hb.LipsPolicy(pol, 8)


# ---- INFADP through create_alg, against the reference fixtures (tests/golden/make_golden_lipsnet.py), bound 1e-4 ----------------
TOL = 1e-4
ALG_CASES = ("lipsnet_lqs2a1_example", "lipsnet_lqs4a2_gelu_global_squash", "lipsnet_lqs6a3_tanh_local2")


def alg_kwargs(cfg, extra, seed, use_gpu=True):
    from gops_amd.utils.synthetic import act_dim_of, obs_dim_of
    A = act_dim_of(cfg)
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=cfg["env_id"], lq_config=cfg["lq_config"],
              obsv_dim=obs_dim_of(cfg), action_dim=A, action_type="continu", action_high_limit=np.ones(A, dtype=np.float32),
              action_low_limit=-np.ones(A, dtype=np.float32), policy_hidden_sizes=list(cfg["hidden"]), policy_hidden_activation=cfg["act"],
              policy_act_distribution="default", value_func_type="MLP", value_func_name="StateValue",
              value_hidden_sizes=list(cfg["hidden"]), value_hidden_activation=cfg["act"], use_gpu=use_gpu)
    kw.update(extra)
    return kw


def load_alg(name, prefix="sd/"):
    from conftest import golden_meta, load_golden
    from gops_amd.create_pkg.create_alg import create_alg
    g = load_golden(name)
    meta = golden_meta(g)
    cfg = meta["cfg"]
    alg = create_alg(**alg_kwargs(cfg, meta["extra"], meta["seed"]))
    alg.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)})
    alg.networks.cuda()
    alg.set_parameters({"gamma": cfg["gamma"], "forward_step": cfg["horizon"], "tau": meta.get("tau", 0.005)})
    alg.train()   # the fixtures were recorded with alg.networks.train(): the regular loss is part of the PIM gradient
    return alg, g, cfg


def close(got, want):
    got, want = float(got), float(want)
    print(f"scalar {got:.8g} vs {want:.8g}")
    return abs(got - want) <= TOL * max(1.0, abs(want))


@pytest.mark.parametrize("name", ALG_CASES)
def test_infadp_lipsnet_matches_reference(name):
    from helpers import data_from_golden
    alg, g, cfg = load_alg(name)
    data = data_from_golden(g)
    tb, info = alg.get_remote_update_info(data, 0)       # PEV
    figures = {f"pev_grad/{i}": rel_l2(gr.cpu(), g[f"pev_grad/{i}"]) for i, gr in enumerate(info["v"])}
    assert close(tb["Loss/Critic loss-RL iter"], g["pev_loss"])
    assert close(tb["Train/Critic avg value-RL iter"], g["pev_vmean"])
    tb, info = alg.get_remote_update_info(data, 1)       # PIM
    assert len(info["policy"]) == len(list(alg.networks.policy.parameters()))   # reference parameter order: mlp, then K
    figures.update({f"pim_grad/{i}": rel_l2(gr.cpu(), g[f"pim_grad/{i}"]) for i, gr in enumerate(info["policy"])})
    print({k: f"{v:.1e}" for k, v in figures.items()})
    assert close(tb["Loss/Actor loss-RL iter"], g["pim_loss"])
    for k, v in figures.items():
        assert v < TOL, (k, v)


def test_infadp_lipsnet_five_updates_match_reference():
    """Five alternating PEV / PIM `local_update` calls (two Adam groups at their own learning rates, Polyak over all tensors) land on
    the reference's weights: policy, value and both targets."""
    from helpers import data_from_golden
    alg, g, cfg = load_alg("lipsnet_lqs2a1_5updates", prefix="sd0/")
    for k in range(5):
        tb = alg.local_update(data_from_golden(g, f"in{k}/"), k)
        assert close(tb["Loss/Critic loss-RL iter" if k % 2 == 0 else "Loss/Actor loss-RL iter"], g[f"loss{k}"]), k
    figures = {key: rel_l2(p.cpu().double(), g["sd5/" + key]) for key, p in alg.networks.state_dict().items()}
    moved = {key: rel_l2(g["sd0/" + key], g["sd5/" + key]) for key in figures}
    print({k: f"{v:.1e} (moved {moved[k]:.1e})" for k, v in figures.items()})
    assert moved["policy.pi.mlp.0.weight"] > 1e-3 and moved["policy.pi.K.K.0.weight"] > 1e-4 and moved["policy_target.pi.K.K.0.weight"] > 1e-5
    for k, v in figures.items():
        assert v < TOL, (k, v)


def test_infadp_lipsnet_refuses_longer_rollouts():
    alg, g, cfg = load_alg(ALG_CASES[0])
    with pytest.raises(NotImplementedError, match="forward_step = 1 only"):
        alg.set_parameters({"forward_step": 2})
    from helpers import data_from_golden
    alg.forward_step = 2   # (set behind set_parameters' back: the first update refuses)
    with pytest.raises(NotImplementedError, match="forward_step = 1 only"):
        alg.local_update(data_from_golden(g), 1)
