"""CPU-only checks of the convolutional family: the modules' parameter names and shapes, the factory and get_apprfunc_dict's CNN branch,
the ABI of gops_conv_*, the codes the entry points refuse with before any HIP call, and create_alg's refusals."""
import ctypes as C
import inspect

import pytest
import torch

from cnn_helpers import apprfunc_kwargs, ppo_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict

ENTRY_POINTS = ("gops_conv_workspace_bytes", "gops_conv_forward", "gops_conv_backward")
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x1000   # a non-null pointer: every call below is refused before anything reads it

# conv_type -> the image, the convolutions (C_out, C_in, k), F, the heads' widths after F (long: policies; short: StateValue, ActionValueDis)
TABLES = {"type_1": ((3, 44, 52), ((32, 3, 8), (64, 32, 4), (64, 64, 3)), 384, (512, 256), (512,)),
          "type_2": ((4, 96, 96), ((8, 4, 4), (16, 8, 3), (32, 16, 3), (64, 32, 3), (128, 64, 3), (256, 128, 3)), 256, (256, 256, 256), (256, 256, 256))}


@pytest.mark.parametrize("conv_type", sorted(TABLES))
@pytest.mark.parametrize("name, heads, out, short", [("DetermPolicy", ("mlp",), 2, False), ("StochaPolicy", ("mean", "log_std"), 2, False),
                                                     ("StateValue", ("mlp",), 1, True), ("ActionValueDis", ("mlp",), 2, True),
                                                     ("StochaPolicyDis", ("mlp",), 2, True)])
def test_parameter_names_and_shapes_are_the_reference_s(conv_type, name, heads, out, short):
    """`conv.{0,2,..}` then `mlp.*` (`mean.*`, `log_std.*`), in this order: the reference's checkpoints load unchanged."""
    shape, convs, F, long_head, short_head = TABLES[conv_type]
    net = create_apprfunc(**apprfunc_kwargs(name, conv_type, shape))
    want = []
    for l, (n, c, k) in enumerate(convs):
        want += [(f"conv.{2 * l}.weight", (n, c, k, k)), (f"conv.{2 * l}.bias", (n,))]
    widths = (F,) + (short_head if short else long_head) + (out,)
    for h in heads:
        for j, (a, b) in enumerate(zip(widths, widths[1:])):
            want += [(f"{h}.{2 * j}.weight", (b, a)), (f"{h}.{2 * j}.bias", (b,))]
    assert [(k, tuple(p.shape)) for k, p in net.named_parameters()] == want
    y = net(torch.randn((3,) + shape))
    assert tuple(y.shape) == {"StateValue": (3,), "StochaPolicy": (3, 4)}.get(name, (3, 2))
    if name == "StochaPolicy":
        assert (y[:, 2:] > 0).all() and torch.equal(net.policy(torch.zeros((1,) + shape))[:, 2:].exp(), net(torch.zeros((1,) + shape))[:, 2:])


@pytest.mark.parametrize("name", ["FiniteHorizonPolicy", "ActionValue", "ActionValueDistri"])
def test_classes_outside_the_convolution_path_say_so(name):
    with pytest.raises(NotImplementedError, match=None if name == "FiniteHorizonPolicy" else "features \\|\\| act"):
        create_apprfunc(**apprfunc_kwargs(name))


def test_get_apprfunc_dict_takes_the_cnn_branch_with_a_conv_type_only():
    kw = ppo_kwargs()
    var = get_apprfunc_dict("value", **kw)
    assert (var["apprfunc"], var["conv_type"], var["hidden_activation"], var["output_activation"], var["obs_dim"]) == ("CNN", "type_2", "tanh", "linear", (4, 96, 96))
    del kw["value_conv_type"]
    with pytest.raises(NotImplementedError, match="apprfunc type CNN is outside the MI355X ADP path"):
        get_apprfunc_dict("value", **kw)


def test_abi_of_the_conv_entry_points(tmp_path):
    from abi_helpers import check_abi
    check_abi(tmp_path, [("GopsConv", hb.GopsConv), ("GopsConvGrad", hb.GopsConvGrad)], ENTRY_POINTS)


def _desc(n_conv=2, shape=(4, 20, 20), layers=((8, 4, 2), (16, 3, 2)), null=None):
    c = hb.GopsConv()
    c.n_conv, (c.in_channels, c.in_h, c.in_w) = n_conv, shape
    for l in range(hb.CONV_MAX_LAYERS):
        c.channels[l], c.kernel[l], c.stride[l] = layers[l] if l < len(layers) else (8, 1, 1)
        c.weight[l], c.bias[l] = (None if null == ("weight", l) else FAKE), FAKE
    return c


@pytest.mark.parametrize("desc, call, code", [
    (dict(), dict(net=None), BAD_ARG), (dict(), dict(x=None), BAD_ARG), (dict(), dict(y=None), BAD_ARG), (dict(null=("weight", 1)), dict(), BAD_ARG),
    (dict(), dict(batch=0), BAD_ARG), (dict(n_conv=0), dict(), BAD_ARG), (dict(n_conv=7), dict(), UNSUPPORTED),
    (dict(layers=((8, 9, 2), (16, 3, 2))), dict(), UNSUPPORTED), (dict(layers=((8, 4, 5), (16, 3, 2))), dict(), UNSUPPORTED),
    (dict(layers=((8, 2, 3), (16, 3, 2))), dict(), UNSUPPORTED), (dict(layers=((257, 4, 2), (16, 3, 2))), dict(), UNSUPPORTED),
    (dict(layers=((8, 4, 0), (16, 3, 2))), dict(), UNSUPPORTED), (dict(shape=(4, 129, 20)), dict(), UNSUPPORTED),
    (dict(shape=(0, 20, 20)), dict(), UNSUPPORTED), (dict(shape=(4, 20, 3)), dict(), UNSUPPORTED),   # (narrower than the first kernel)
    (dict(shape=(4, 6, 20)), dict(), UNSUPPORTED),                                                   # (6 -> 2: below the second kernel)
    (dict(), dict(batch=1 << 20), UNSUPPORTED),                                                      # (2^20 x 8 x 10 x 10 elements)
    (dict(), dict(ws=None), WORKSPACE), (dict(), dict(nbytes=64), WORKSPACE)])
def test_refusals_come_before_any_hip_call(desc, call, code):
    """Forward and backward refuse with the same code (`y` is the forward's features and the backward's grad_features_a; grad_features_b
    may be NULL), and a refused description has no workspace."""
    lib, c, g = hb.lib(), _desc(**desc), hb.GopsConvGrad()
    for l in range(hb.CONV_MAX_LAYERS):
        g.weight[l] = g.bias[l] = FAKE
    a = dict(dict(net=C.byref(c), batch=17, x=FAKE, y=FAKE, ws=FAKE, nbytes=1 << 40), **call)
    assert lib.gops_conv_forward(a["net"], a["batch"], a["x"], a["y"], a["ws"], a["nbytes"], None) == code
    for gb in (None, FAKE):
        assert lib.gops_conv_backward(a["net"], a["batch"], a["x"], a["y"], gb, C.byref(g), a["ws"], a["nbytes"], None) == code
    assert lib.gops_conv_backward(a["net"], a["batch"], a["x"], a["y"], None, None, a["ws"], a["nbytes"], None) == (code if a["net"] is None else BAD_ARG)
    described = not desc and a["net"] is not None and 0 < a["batch"] < 1 << 20   # (what is wrong lies in the call's pointers alone)
    assert (lib.gops_conv_workspace_bytes(a["net"], a["batch"]) > 0) == described


OTHERS = dict(policy_hidden_sizes=[16, 16], value_hidden_sizes=[16, 16], policy_learning_rate=1e-3, value_learning_rate=1e-3, buffer_name="replay_buffer")


@pytest.mark.parametrize("over, reason", [
    (dict(value_func_type="MLP"), "as a pair"), (dict(policy_func_type="MLP"), "as a pair"), (dict(policy_func_type="CNN_SHARED"), "as a pair"),
    (dict(cnn_shared=True), "cnn_shared feature networks are outside"), (dict(obsv_dim=4), r"triple \(C, H, W\)"), (dict(obsv_dim=(96, 96)), r"triple \(C, H, W\)"),
    (dict(obsv_dim=(4, 129, 96)), "H and W up to 128"), (dict(obsv_dim=(4, 40, 96)), "large enough for every layer"),
    (dict(obsv_dim=(4, 84, 84), policy_conv_type="type_1", value_conv_type="type_1"), "feature width of 3136"),
    (dict(policy_conv_type="type_3"), "type_1, type_2 only"), (dict(value_func_name="ActionValue"), "state-value function"),
    (dict(action_dim=5), "1 .. 4 actions"), (dict(policy_func_type="CNN_SHARED", value_func_type="CNN_SHARED"), "PPO runs MLP networks only")] + [
    (dict(OTHERS, algorithm=alg), f"CNN \\({'value' if alg == 'RPI' else 'policy, value'}\\) is supported by PPO only, not by {alg}")
    for alg in ("TRPO", "INFADP", "FHADP", "MPG", "RPI", "DDPG", "TD3", "SAC", "DSAC", "DSACT", "DQN")])
def test_create_alg_refusals_carry_the_reason(over, reason):
    from gops_amd.create_pkg import create_alg as ca
    module = inspect.getmodule(ca._registry_of(over.get("algorithm", "PPO")).lookup(over.get("algorithm", "PPO")).entry_point)
    mandatory = {name: 1 for name in getattr(module, "MANDATORY", ())}   # (their absence is a KeyError before any refusal)
    with pytest.raises(NotImplementedError, match=reason):
        create_alg(**dict(mandatory, **ppo_kwargs(**over)))


def test_create_alg_builds_ppo_on_the_convolutional_pair():
    from gops_amd.apprfunc import cnn
    nets = create_alg(**ppo_kwargs()).networks
    assert type(nets.policy) is cnn.StochaPolicy and type(nets.value) is cnn.StateValue
    assert len(list(nets.parameters())) == (12 + 2 * 8) + (12 + 8)
