"""gops_rnn_forward / _backward against the module itself in float64 with autograd on the host (nn.RNN + nn.Linear), and PPO on the
recurrent pair.  Bounds: the project's own, as relative L2 against float64 (tests/test_lipsnet_gpu.py) - outputs < 1e-5, every
gradient tensor < 1e-4."""
import copy

import pytest
import torch

import ac_helpers as ah
from conftest import rel_l2
from ppo_helpers import TERMS, restate_ppo_step
from rnn_helpers import apprfunc_kwargs, ppo_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_apprfunc import create_apprfunc

pytestmark = pytest.mark.gpu

# (B, L, O, H, head hidden, class, hidden activation).  B: one row, a full tile, a tile edge, several tiles with a ragged last one;
# L: no recurrence, the smallest with one, the reference env's stack; O: k padding of the MFMA; H: one column block on one wave, three
# dealt unevenly over four waves, the register-budget case (two blocks per wave); StateValue: one head of 1, StochaPolicy: 2 + 2.
CASES = [(1, 1, 3, 16, (), "StateValue", "tanh"), (16, 2, 4, 16, (32,), "StochaPolicy", "gelu"), (17, 5, 4, 48, (32,), "StateValue", "gelu"),
         (50, 5, 3, 128, (32,), "StochaPolicy", "tanh"), (17, 1, 4, 128, (), "StochaPolicy", "tanh"), (50, 2, 3, 48, (), "StateValue", "gelu"),
         (16, 5, 3, 16, (32,), "StateValue", "tanh"), (1, 2, 4, 128, (32,), "StochaPolicy", "gelu"),
         # 258 tiles, past the sweep's cap of 256 workgroups: two of them walk a second tile (the last one ragged) - register
         # accumulators carried across tiles, head gradients added into the slot
         (4113, 2, 3, 16, (32,), "StochaPolicy", "tanh")]


def _setup(B, L, O, H, head, name, activation):
    """Module (device), x [B, L, O], grad_y, and the float64 reference (y, gradients in parameters() order).  x ~ N(0, 1) on torch's
    default U(+-1 / sqrt(H)) init with the recurrent weights doubled: over CASES 99 % of the |tanh arguments| lie within 1.8 and the
    largest is 3.4 (H = 16, B = 4113; evaluated on the host with these seeds) - away from saturation, with a recurrence that matters."""
    torch.manual_seed(100 * B + L)
    net = create_apprfunc(**apprfunc_kwargs(name, (H,) + head, activation, O=O))
    with torch.no_grad():
        net.rnn.weight_hh_l0.mul_(2.0)
        net.rnn.weight_ih_l0.mul_(2.0)
    x = torch.randn(B, L, O)
    ref = copy.deepcopy(net).double()
    y = ref.policy(x.double()) if name == "StochaPolicy" else ref(x.double()).reshape(B, -1)
    gy = torch.randn(y.shape)
    y.backward(gy.double())
    return net.cuda(), x.cuda(), gy.cuda(), y.detach(), [p.grad for p in ref.parameters()]


def _backward(net, rnn_net, x, gy):
    for p in net.parameters():
        p.grad = torch.full_like(p, float("nan"))   # (every element is overwritten)
    rnn_net.backward(x, gy, net.hip_rnn_grad())
    return [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-L{}-O{}-H{}-{}-{}-{}".format(*c))
def test_forward_and_backward_per_tensor(case):
    B, L = case[:2]
    net, x, gy, y_ref, g_ref = _setup(*case)
    rnn_net = hb.RnnNet(net.hip_rnn(L), B, x.device)
    y = rnn_net.forward(x)
    grads = _backward(net, rnn_net, x, gy)
    assert rel_l2(y.cpu(), y_ref) < 1e-5
    for (k, _), g, r in zip(net.named_parameters(), grads, g_ref):
        assert rel_l2(g.cpu(), r) < 1e-4, k
    if L == 1:
        assert (net.rnn.weight_hh_l0.grad == 0).all()   # h_0 = 0: exactly


def test_rows_beyond_the_batch_and_reproducible_gradients():
    """B = 17: nothing behind row 17 of y is written; two backward calls on the same inputs give bit-equal gradients."""
    net, x, gy, _, _ = _setup(17, 5, 4, 48, (32,), "StochaPolicy", "tanh")
    rnn_net = hb.RnnNet(net.hip_rnn(5), 17, x.device)
    ah.check_rows_beyond_the_batch(lambda out: rnn_net.forward(x, out=out["y"]), {"y": 17 * 4})
    first, second = _backward(net, rnn_net, x, gy), _backward(net, rnn_net, x, gy)
    assert all(torch.equal(a, b) and torch.isfinite(a).all() for a, b in zip(first, second))


def _ppo(**over):
    torch.manual_seed(7)
    alg = create_alg(**ppo_kwargs(use_gpu=True, **over))
    alg.networks.cuda()
    return alg


def _columns(alg, S, stacked=True):
    """On-policy columns around the policy as it stands: ratios within exp(+-0.3) on both sides of the clip range."""
    g = torch.Generator().manual_seed(S)
    obs = torch.randn(S, 5, 4, generator=g)
    obs = obs if stacked else obs[:, -1].contiguous()
    nets = copy.deepcopy(alg.networks).cpu()
    with torch.no_grad():
        logits = nets.policy(obs)
        val = nets.value(obs) + 0.3 * torch.randn(S, generator=g)
    dist = alg.networks.create_action_distributions(logits)
    act = logits[:, :1] + logits[:, 1:] * torch.randn(S, 1, generator=g)
    return dict(obs=obs, act=act, logp=dist.log_prob(act) + 0.3 * (torch.rand(S, generator=g) - 0.5), adv=torch.randn(S, generator=g),
                ret=val + torch.randn(S, generator=g), val=val, logits=logits)


def test_ppo_minibatch_step_against_float64():
    """One minibatch_gradients at L = 5, O = 4, H = 16, head hidden (16,), A = 1, M = 17 against the float64 restatement through the
    modules (ppo_helpers.restate_ppo_step): the six loss terms, every gradient tensor."""
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
    """One local_update of 3 repeats x 2 minibatches of 17: parameters move, the minibatch steps replay a captured graph as often as
    they do for the MLP pair of the same sizes, and a second run from the same state is bit-equal."""
    def run(**over):
        alg = _ppo(**over)
        before = [p.detach().clone() for p in alg.networks.parameters()]
        data = {k: v for k, v in _columns(alg, 34, stacked="obsv_dim" not in over).items() if k not in ("val", "logits")}
        data["perm"] = torch.stack([torch.randperm(34, generator=torch.Generator().manual_seed(r)) for r in range(3)])
        alg.local_update(data, 1)
        return alg, before

    a, before = run()
    b, _ = run()
    mlp, _ = run(policy_func_type="MLP", value_func_type="MLP", obsv_dim=4)
    assert all(not torch.equal(p, q) for p, q in zip(a.networks.parameters(), before))
    assert a.graph_replays == mlp.graph_replays > 0
    for (k, p), q in zip(a.networks.named_parameters(), b.networks.parameters()):
        assert torch.equal(p, q) and torch.isfinite(p).all(), k
