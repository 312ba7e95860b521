"""CPU-only checks of the recurrent family: the modules' parameter names and shapes, the factory, the ABI of gops_rnn_*, the codes the
entry points refuse with before any HIP call, and create_alg's refusals."""
import ctypes as C

import pytest
import torch

from rnn_helpers import apprfunc_kwargs, ppo_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_apprfunc import create_apprfunc

ENTRY_POINTS = ("gops_rnn_workspace_bytes", "gops_rnn_forward", "gops_rnn_backward")
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x1000   # a non-null pointer: every call below is refused before anything reads it


@pytest.mark.parametrize("name, heads, out", [("DetermPolicy", ("pi",), 2), ("StochaPolicy", ("mean", "log_std"), 2),
                                              ("StateValue", ("v",), 1), ("ActionValueDis", ("q",), 2)])
def test_parameter_names_and_shapes_are_the_reference_s(name, heads, out):
    """`rnn.*_l0` of nn.RNN(O = 4, 16), then `mlp([16, 32, out])` per head, in this order: the reference's checkpoints load unchanged.
    The eager forward takes a stack [B, L, O] for any L."""
    net = create_apprfunc(**apprfunc_kwargs(name, (16, 32)))
    want = [("rnn.weight_ih_l0", (16, 4)), ("rnn.weight_hh_l0", (16, 16)), ("rnn.bias_ih_l0", (16,)), ("rnn.bias_hh_l0", (16,))]
    for h in heads:
        want += [(f"{h}.0.weight", (32, 16)), (f"{h}.0.bias", (32,)), (f"{h}.2.weight", (out, 32)), (f"{h}.2.bias", (out,))]
    assert [(k, tuple(p.shape)) for k, p in net.named_parameters()] == want
    y = net(torch.randn(3, 7, 4))
    assert tuple(y.shape) == {"StateValue": (3,), "StochaPolicy": (3, 4)}.get(name, (3, 2))
    if name == "StochaPolicy":
        assert (y[:, 2:] > 0).all() and torch.equal(net.policy(torch.zeros(1, 2, 4))[:, 2:].exp(), net(torch.zeros(1, 2, 4))[:, 2:])


def test_classes_outside_the_recurrent_kernels_say_so():
    with pytest.raises(NotImplementedError):
        create_apprfunc(**apprfunc_kwargs("FiniteHorizonPolicy", (16,)))
    with pytest.raises(NotImplementedError, match="h_L \\|\\| act"):
        create_apprfunc(**apprfunc_kwargs("ActionValue", (16,)))


def test_abi_of_the_rnn_entry_points(tmp_path):
    from abi_helpers import check_abi
    check_abi(tmp_path, [("GopsRnn", hb.GopsRnn), ("GopsRnnGrad", hb.GopsRnnGrad)], ENTRY_POINTS)


def _desc(seq_len=5, obs_dim=4, hidden=16, n_heads=1, dtype=0, null=None):
    r = hb.GopsRnn()
    r.seq_len, r.obs_dim, r.hidden, r.n_heads = seq_len, obs_dim, hidden, n_heads
    for name in hb.RNN_PARAMS:
        setattr(r, name, None if name == null else FAKE)
    for h in range(hb.RNN_MAX_HEADS):
        m = r.head[h]
        m.n_layers, m.hidden_act, m.dtype = 2, hb.ACT_IDS["tanh"], dtype
        m.sizes[0], m.sizes[1], m.sizes[2] = hidden, 32, 1
        for l in range(2):
            m.weight[l] = m.bias[l] = FAKE
    return r


@pytest.mark.parametrize("desc, call, code", [
    (dict(), dict(net=None), BAD_ARG), (dict(), dict(x=None), BAD_ARG), (dict(), dict(y=None), BAD_ARG), (dict(null="weight_hh"), dict(), BAD_ARG),
    (dict(), dict(batch=0), BAD_ARG), (dict(seq_len=0), dict(), BAD_ARG), (dict(seq_len=33), dict(), UNSUPPORTED),
    (dict(hidden=24), dict(), UNSUPPORTED), (dict(hidden=144), dict(), UNSUPPORTED), (dict(obs_dim=65), dict(), UNSUPPORTED),
    (dict(n_heads=3), dict(), BAD_ARG), (dict(dtype=1), dict(), UNSUPPORTED), (dict(), dict(ws=None), WORKSPACE), (dict(), dict(nbytes=64), WORKSPACE)])
def test_refusals_come_before_any_hip_call(desc, call, code):
    """Forward and backward refuse with the same code (`y` is the backward's grad_y), and a refused description has no workspace."""
    lib, r, g = hb.lib(), _desc(**desc), hb.GopsRnnGrad()
    for name in hb.RNN_PARAMS:
        setattr(g, name, FAKE)
    for l in range(2):
        g.head[0].weight[l] = g.head[0].bias[l] = g.head[1].weight[l] = g.head[1].bias[l] = FAKE
    a = dict(dict(net=C.byref(r), batch=17, x=FAKE, y=FAKE, ws=FAKE, nbytes=1 << 30), **call)
    assert lib.gops_rnn_forward(a["net"], a["batch"], a["x"], a["y"], a["ws"], a["nbytes"], None) == code
    assert lib.gops_rnn_backward(a["net"], a["batch"], a["x"], a["y"], C.byref(g), a["ws"], a["nbytes"], None) == code
    assert lib.gops_rnn_backward(a["net"], a["batch"], a["x"], a["y"], None, a["ws"], a["nbytes"], None) == (code if a["net"] is None else BAD_ARG)
    described = not desc and a["net"] is not None and a["batch"] > 0   # (what is wrong lies in the call's pointers alone)
    assert (lib.gops_rnn_workspace_bytes(a["net"], a["batch"]) > 0) == described


@pytest.mark.parametrize("over, reason", [
    (dict(value_func_type="MLP"), "as a pair"), (dict(policy_func_type="MLP"), "as a pair"),
    (dict(algorithm="TRPO", delta=0.01, rtol=1e-5, atol=1e-8, damping_factor=0.1, max_cg=10, alpha=0.8, max_search=10, train_v_iters=2,
          value_learning_rate=1e-3), "TRPO runs MLP networks only"), (dict(obsv_dim=4), r"pair \(L, O\)"), (dict(obsv_dim=(33, 4)), "L in 1 .. 32"),
    (dict(policy_hidden_sizes=[24, 16]), "multiple of 16 in 16 .. 128"), (dict(value_hidden_sizes=[144]), "multiple of 16 in 16 .. 128"),
    (dict(value_func_name="ActionValue"), "state-value function"), (dict(action_dim=17), "1 .. 16 outputs"),
    (dict(algorithm="INFADP"), "supported by PPO only, not by INFADP"), (dict(algorithm="MPG", obsv_dim=4), "supported by PPO only, not by MPG"),
    (dict(algorithm="RPI", policy_func_type="MLP"), r"RNN \(value\) is supported by PPO only")])
def test_create_alg_refusals_carry_the_reason(over, reason):
    with pytest.raises(NotImplementedError, match=reason):
        create_alg(**ppo_kwargs(**over))


def test_create_alg_builds_ppo_on_the_recurrent_pair():
    from gops_amd.apprfunc import rnn
    nets = create_alg(**ppo_kwargs()).networks
    assert type(nets.policy) is rnn.StochaPolicy and type(nets.value) is rnn.StateValue
    assert len(list(nets.parameters())) == 12 + 8
