"""gops_conv_forward / _backward and hb.CnnNet against plain torch in float64 with autograd on the host (F.conv2d; the module itself), and
PPO on the convolutional pair.  Bounds: the project's own, as relative L2 against float64 (tests/test_rnn_gpu.py) - outputs < 1e-5,
every gradient tensor < 1e-4."""
import copy

import pytest
import torch
import torch.nn.functional as F

import ac_helpers as ah
from cnn_helpers import apprfunc_kwargs, ppo_kwargs
from conftest import rel_l2
from ppo_helpers import TERMS, restate_ppo_step

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_apprfunc import create_apprfunc

pytestmark = pytest.mark.gpu

# (B, (C, H, W), ((C_out, k, stride), ...), two feature gradients)
STACKS = [
    (1, (3, 9, 11), ((8, 3, 2),), False),                  # K = 27: no multiple of 4; C_out = 8 < 16; one ragged M tile (20 pixels)
    (2, (4, 13, 12), ((8, 4, 2), (16, 3, 2)), True),       # stride 2 through a data gradient; 13 -> 5 drops a row
    (2, (4, 15, 14), ((8, 4, 2), (16, 3, 2)), False),      # ... and the second layer's floor (6 -> 2) drops a row AND a column of dZ's target
    (5, (3, 20, 24), ((32, 8, 4), (64, 4, 2)), True),      # k = 8, stride 4, then k = 4, stride 2 down to 1 x 1: type_1's front
    (17, (16, 7, 7), ((48, 3, 1), (80, 3, 1)), True),      # stride 1; C_out 48 and 80: partial N tiles, 3 and 5 column blocks; M tiles straddle samples
    (130, (4, 20, 20), ((8, 4, 2),), False),               # M = 10530 > 512: the weight gradient runs in 21 slices, the last one ragged (290 rows)
    (3, (4, 5, 5), ((8, 3, 1), (16, 3, 1)), True),         # a 3 x 3 input to a k = 3 layer: output 1 x 1, type_2's tail
    (2, (3, 8, 8), ((6, 3, 1), (5, 2, 2)), True),          # inner channel counts 6 and 5: the scalar gathers of the channels-last tensors
]


def _grow(module, by=2.0):
    """torch's default initialisation with the convolutions' weights scaled up: with randn inputs every layer then has both signs
    before its ReLU (asserted where the reference is formed)."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(by)
    return module


def _mixed(h):
    assert 0.02 < float((h > 0).double().mean()) < 0.98   # neither all dead nor all alive


@pytest.mark.parametrize("case", STACKS, ids=lambda c: "B{}-{}-{}".format(c[0], "x".join(map(str, c[1])), "_".join("c{}k{}s{}".format(*l) for l in c[2])))
def test_conv_stack_features_and_gradients(case):
    B, shape, layers, two = case
    torch.manual_seed(100 * B + shape[1])
    convs, c_in = [], shape[0]
    for n, k, s in layers:
        convs.append(_grow(torch.nn.Conv2d(c_in, n, k, s)))
        c_in = n
    x = torch.randn((B,) + shape)
    ref = [copy.deepcopy(c).double() for c in convs]
    h = x.double()
    for c in ref:
        h = F.relu(c(h))
        _mixed(h)
    feat = h.reshape(B, -1)
    ga, gb = torch.randn(feat.shape), (torch.randn(feat.shape) if two else None)
    feat.backward(ga.double() + (gb.double() if two else 0.0))

    dev = [c.cuda() for c in convs]
    stack = hb.ConvStack(hb.make_conv([c.weight.data for c in dev], [c.bias.data for c in dev], [l[2] for l in layers], shape[1:]), B)
    got = stack.forward(x.cuda())
    gw, gbias = [torch.full_like(c.weight, float("nan")) for c in dev], [torch.full_like(c.bias, float("nan")) for c in dev]   # (all overwritten)
    stack.backward(x.cuda(), ga.cuda(), gb.cuda() if two else None, hb.make_conv_grad(gw, gbias))
    assert rel_l2(got.cpu(), feat.detach()) < 1e-5
    for l, c in enumerate(ref):
        assert rel_l2(gw[l].cpu(), c.weight.grad) < 1e-4, ("weight", l, rel_l2(gw[l].cpu(), c.weight.grad))
        assert rel_l2(gbias[l].cpu(), c.bias.grad) < 1e-4, ("bias", l, rel_l2(gbias[l].cpu(), c.bias.grad))


def _setup(name, conv_type, shape, B):
    """Module (device), x, grad_y, and the float64 reference (y, gradients in parameters() order)."""
    torch.manual_seed(100 * B + shape[2])
    net = _grow(create_apprfunc(**apprfunc_kwargs(name, conv_type, shape)), 1.5)
    x = torch.randn((B,) + shape)
    ref = copy.deepcopy(net).double()
    h = x.double()
    for m in ref.conv:
        h = m(h)
        if isinstance(m, torch.nn.ReLU):
            _mixed(h)
    y = ref.policy(x.double()) if name == "StochaPolicy" else ref(x.double()).reshape(B, -1)
    gy = torch.randn(y.shape)
    y.backward(gy.double())
    return net.cuda(), x.cuda(), gy.cuda(), y.detach(), [p.grad for p in ref.parameters()]


def _backward(net, cnn_net, x, gy):
    for p in net.parameters():
        p.grad = torch.full_like(p, float("nan"))   # (every element is overwritten)
    cnn_net.backward(x, gy, net.hip_cnn_grad())
    return [p.grad.clone() for p in net.parameters()]


# type_2 on the reference's 96 x 96 and on a non-square image whose extents go through floors; type_1 with F = 64 x 2 x 3 (a wrong
# flatten order shows); B: one row, a ragged tile
NETS = [("type_2", (4, 96, 96), 1), ("type_2", (4, 96, 96), 17), ("type_2", (4, 97, 99), 1), ("type_2", (4, 97, 99), 17), ("type_1", (3, 44, 52), 3)]


@pytest.mark.parametrize("name", ["StateValue", "StochaPolicy"])
@pytest.mark.parametrize("conv_type, shape, B", NETS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_cnn_net_output_and_every_parameter_gradient(name, conv_type, shape, B):
    net, x, gy, y_ref, g_ref = _setup(name, conv_type, shape, B)
    cnn_net = hb.CnnNet(*net.hip_cnn(), B, x.device)
    y = cnn_net.forward(x)
    grads = _backward(net, cnn_net, x, gy)
    assert rel_l2(y.cpu(), y_ref) < 1e-5
    for (k, _), g, r in zip(net.named_parameters(), grads, g_ref):   # (the convolutions' take the sum of both heads' feature gradients)
        assert rel_l2(g.cpu(), r) < 1e-4, (k, rel_l2(g.cpu(), r))


def test_rows_beyond_the_batch_and_reproducible_gradients():
    """B = 17: nothing behind row 17 of y is written; two backward calls on the same inputs give bit-equal gradients."""
    net, x, gy, _, _ = _setup("StochaPolicy", "type_2", (4, 96, 96), 17)
    cnn_net = hb.CnnNet(*net.hip_cnn(), 17, x.device)
    ah.check_rows_beyond_the_batch(lambda out: cnn_net.forward(x, out=out["y"]), {"y": 17 * 4})
    first, second = _backward(net, cnn_net, x, gy), _backward(net, cnn_net, x, gy)
    assert all(torch.equal(a, b) and torch.isfinite(a).all() for a, b in zip(first, second))


def _ppo(**over):
    torch.manual_seed(7)
    alg = create_alg(**ppo_kwargs(use_gpu=True, **over))
    alg.networks.cuda()
    return alg


def _columns(alg, S):
    """On-policy columns around the policy as it stands: ratios within exp(+-0.3) on both sides of the clip range."""
    g = torch.Generator().manual_seed(S)
    obs = torch.randn(S, 4, 96, 96, generator=g)
    nets = copy.deepcopy(alg.networks).cpu()
    with torch.no_grad():
        logits = nets.policy(obs)
        val = nets.value(obs) + 0.3 * torch.randn(S, generator=g)
    dist = alg.networks.create_action_distributions(logits)
    act = logits[:, :1] + logits[:, 1:] * torch.randn(S, 1, generator=g)
    return dict(obs=obs, act=act, logp=dist.log_prob(act) + 0.3 * (torch.rand(S, generator=g) - 0.5), adv=torch.randn(S, generator=g),
                ret=val + torch.randn(S, generator=g), val=val, logits=logits)


def test_ppo_minibatch_step_against_float64():
    """One minibatch_gradients on the type_2 pair at M = 17 against the float64 restatement through the modules
    (ppo_helpers.restate_ppo_step): the six loss terms, every gradient tensor."""
    alg = _ppo()
    mb = {k: v.cuda() for k, v in _columns(alg, 17).items()}
    out = alg.minibatch_gradients(mb).cpu()
    want = restate_ppo_step(alg, mb)
    for i, k in enumerate(TERMS):
        assert ah.close(out[i], want["terms"][k]), (k, float(out[i]), want["terms"][k])
    for n in ("policy", "value"):
        for (k, p), r in zip(getattr(alg.networks, n).named_parameters(), want["grads"][n]):
            assert rel_l2(p.grad.cpu(), r) < 1e-4, (n, k, rel_l2(p.grad.cpu(), r))


def test_ppo_local_update_is_captured_and_reproducible():
    """One local_update of 3 repeats x 2 minibatches of 17: every parameter tensor moves, the minibatch steps replay a captured graph,
    and a second run from the same state is bit-equal."""
    def run():
        alg = _ppo()
        before = [p.detach().clone() for p in alg.networks.parameters()]
        data = {k: v for k, v in _columns(alg, 34).items() if k not in ("val", "logits")}
        data["perm"] = torch.stack([torch.randperm(34, generator=torch.Generator().manual_seed(r)) for r in range(3)])
        alg.local_update(data, 1)
        return alg, before

    a, before = run()
    b, _ = run()
    assert all(not torch.equal(p, q) for p, q in zip(a.networks.parameters(), before))
    assert a.graph_replays == b.graph_replays > 0
    for (k, p), q in zip(a.networks.named_parameters(), b.networks.parameters()):
        assert torch.equal(p, q) and torch.isfinite(p).all(), k
