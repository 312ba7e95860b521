"""gops_rnn_dqn_step against the modules in float64 on the host (apprfunc.rnn.ActionValueDis cast to double, torch.max, the seam's
formulas, autograd), bit for bit against the composed path (RnnNet.forward, RnnNet.backward), and DQN on recurrent networks fused
against composed.  Bounds: the project's own for this arithmetic (tests/test_rnn_gpu.py) - an output within 1e-5 of the tensor's
largest element, every gradient tensor's relative L2 below 1e-4."""
import copy

import pytest
import torch

from conftest import rel_l2
from dqn_helpers import dqn_kwargs
from rnn_helpers import apprfunc_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_apprfunc import create_apprfunc

pytestmark = pytest.mark.gpu

GAMMA, RSCALE, GAP = 0.97, 0.5, 1e-4
# (B, L, O, H, head hidden, N, extras).  1: L = 1 skips the W_hh chain, O no multiple of 4, fewer H blocks than waves, the output layer
# alone, 15 rows beyond B; 2: a second tile with one row, NB = 1 full, a hidden head layer; 3: NB = 2 with a ragged last block, two
# hidden head layers, the widest head; 4: H at the limit, weights, done rows, one index out of range, ties from a duplicated output
# unit; 5: 513 tiles - the fold past one workgroup's worth of partials.
CASES = [(1, 1, 3, 16, (), 2, False), (17, 2, 4, 64, (32,), 5, False), (33, 5, 4, 80, (16, 48), 16, False), (40, 3, 7, 128, (128,), 3, True),
         (8200, 2, 4, 16, (), 2, False)]
IDS = ["B{}-L{}-O{}-H{}-{}-N{}".format(*c[:6]) for c in CASES]


def _setup(B, L, O, H, head, N, extras):
    """Online and target modules (device), the batch, and the float64 reference.  The target's output layer is scaled up so that the
    top two of every row lie at least GAP apart in float64 (asserted: no row is left out); `extras`: importance weights, done rows
    at both ends, row 3 with the index N, and target unit 2 a copy of unit 1 - every row whose maximum they hold is a tie."""
    torch.manual_seed(1000 * L + B)
    q = create_apprfunc(**apprfunc_kwargs("ActionValueDis", (H,) + head, "tanh", O=O, out=N))
    qt = create_apprfunc(**apprfunc_kwargs("ActionValueDis", (H,) + head, "tanh", O=O, out=N))
    with torch.no_grad():
        for net in (q, qt):
            net.rnn.weight_hh_l0.mul_(2.0)
            net.rnn.weight_ih_l0.mul_(2.0)
        out = [m for m in qt.q if isinstance(m, torch.nn.Linear)][-1]
        out.weight.mul_(40.0)
        if extras:
            out.weight[2], out.bias[2] = out.weight[1], out.bias[1]
    d = dict(obs=torch.randn(B, L, O), obs2=torch.randn(B, L, O), act=torch.randint(N, (B,)).float(), rew=torch.randn(B),
             done=torch.zeros(B))
    if extras:
        d["weight"] = 0.2 + 0.8 * torch.rand(B)
        d["done"][[0, B - 1]] = 1.0
        d["act"][3] = float(N)
    w = d.get("weight", torch.ones(B)).double()
    ref_q = copy.deepcopy(q).double()
    with torch.no_grad():
        q_t = copy.deepcopy(qt).double()(d["obs2"].double())
    q_max = q_t.max(dim=1).values
    a_star = torch.where(q_t == q_max[:, None], torch.arange(N), N).min(dim=1).values   # the lowest index attaining the maximum
    distinct = q_t[:, :2] if extras else q_t   # (units 1 and 2 are one value)
    top = distinct.topk(2, dim=1).values
    assert (top[:, 0] - top[:, 1]).min() >= GAP
    backup = d["rew"].double() * RSCALE + GAMMA * (1 - d["done"].double()) * q_max
    q_all = ref_q(d["obs"].double())
    ok = d["act"] < N
    a = torch.where(ok, d["act"].long(), 0)
    delta = (q_all.gather(1, a[:, None]).squeeze(1) - backup) * ok
    loss = (w * delta ** 2).sum() / B
    loss.backward()
    seed = torch.zeros(B, N, dtype=torch.float64).scatter_(1, a[:, None], (2.0 / B * w * delta.detach())[:, None])
    ref = dict(q_all=q_all.detach(), backup=backup, a_star=a_star, seed=seed, abs_err=delta.detach().abs(),
               stats=torch.stack([loss.detach(), (q_all.detach().gather(1, a[:, None]).squeeze(1) * ok).sum() / B]),
               bad=int((~ok).sum()), tie=extras and bool((a_star == 1).any()), grads=[p.grad for p in ref_q.parameters()])
    return q.cuda(), qt.cuda(), {k: v.cuda() for k, v in d.items()}, ref


def _backward(net, rnn_net, x, seed):
    for p in net.parameters():
        p.grad = torch.full_like(p, float("nan"))   # (every element is overwritten)
    rnn_net.backward(x, seed, net.hip_rnn_grad())
    return [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_launch_against_float64_and_the_composed_path(case):
    B, L = case[:2]
    q, qt, d, ref = _setup(*case)
    step = hb.RnnDqnStep(q.hip_rnn(L), qt.hip_rnn(L), B, d["obs"].device)
    composed = hb.RnnNet(q.hip_rnn(L), B, d["obs"].device)
    assert step.supported
    step.net.workspace.zero_()
    composed.workspace.zero_()   # (the padding between the stash sections, and the sweep's slots, which no forward writes)
    args = (d["obs"], d["obs2"], d["act"], d["rew"], d["done"], d.get("weight"))
    res = {k: v.clone() for k, v in step.run(*args, reward_scale=RSCALE, gamma=GAMMA).items()}
    # float64
    for k in ("q_all", "backup", "abs_err", "seed"):
        err, top = float((res[k].cpu().double() - ref[k]).abs().max()), float(ref[k].abs().max())
        print(k, err, top)
        assert err <= 1e-5 * top, k
    err, top = float((res["stats"][:2].cpu().double() - ref["stats"]).abs().max()), float(ref["stats"].abs().max())
    print("stats", err, top)
    assert err <= 1e-5 * top and int(res["stats"][2]) == ref["bad"] == int(case[6])
    assert torch.equal(res["a_star"].cpu().long(), ref["a_star"]) and ref["tie"] == case[6]
    assert torch.equal(res["seed"] != 0, (ref["seed"] != 0).cuda())   # the taken column, and only it
    # the composed path, bit for bit
    assert torch.equal(res["q_all"], composed.forward(d["obs"])) and torch.equal(step.net.workspace, composed.workspace)
    grads = _backward(q, step.net, d["obs"], res["seed"])
    assert all(torch.equal(g, c) for g, c in zip(grads, _backward(q, composed, d["obs"], res["seed"])))
    for (k, _), g, r in zip(q.named_parameters(), grads, ref["grads"]):
        print(k, rel_l2(g.cpu(), r))
        assert rel_l2(g.cpu(), r) < 1e-4, k
    # a second launch, after the sweep has written its slots behind the stash
    again = step.run(*args, reward_scale=RSCALE, gamma=GAMMA)
    assert all(torch.equal(again[k], res[k]) for k in res)


def _dqn(per=False, **over):
    torch.manual_seed(11)
    alg = create_alg(**dqn_kwargs((2, 4), 5, [64, 32], "tanh", use_gpu=True, value_func_type="RNN", env_id="gym_cartpolecontiwithstack",
                                  buffer_name="prioritized_replay_buffer" if per else "replay_buffer", **over))
    with torch.no_grad():
        for p in alg.networks.q_target.parameters():
            p.add_(0.3 * (torch.rand(p.shape) - 0.5))
    alg.networks.cuda()
    alg.gamma, alg.reward_scale = GAMMA, RSCALE
    return alg


def _batch(B=17, per=False):
    g = torch.Generator().manual_seed(3)
    d = dict(obs=torch.randn(B, 2, 4, generator=g), obs2=torch.randn(B, 2, 4, generator=g), act=torch.randint(5, (B, 1), generator=g).float(),
             rew=torch.randn(B, generator=g), done=(torch.rand(B, generator=g) < 0.2).float())
    if per:
        d.update(weight=0.2 + 0.8 * torch.rand(B, generator=g), idx=torch.arange(B, dtype=torch.int32))
    return d


def test_dqn_fused_against_composed_and_graph_against_eager(monkeypatch):
    """(17, 2, 4, 64, (32,), 5): the same initial weights.  Fused and composed agree after three local_updates and after seven.  With
    capture on, StepGraphCache runs two eager calls per signature before it captures and the first update changes the signature (it
    allocates the workspaces): the fourth update is the capture, the fifth to seventh are replays - and walk the eager launches'
    parameter trajectory bit for bit."""
    def run(fused_target, mode, snapshots):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        alg, seen = _dqn(fused_target=fused_target), []
        for it in range(7):
            alg.local_update(_batch(), it)
            if it in snapshots:
                seen.append([p.detach().clone() for p in alg.networks.parameters()])
        g = alg._graphs["update"]
        assert alg.backup_path == ("fused" if fused_target else "composed") and not g.failed and (g.graph is not None) == (mode == "1")
        return seen

    fused, eager, composed = run(True, "1", (2, 6)), run(True, "0", (2, 6)), run(False, "1", (2, 6))
    for f, e, c in zip(fused, eager, composed):
        assert all(torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(f, e))
        assert all(rel_l2(p.cpu(), q.cpu()) < 1e-4 for p, q in zip(f, c))


def test_dqn_prioritized_replay_returns_the_kernel_s_abs_err():
    alg, data = _dqn(per=True), _batch(per=True)
    dev = {k: v.cuda() for k, v in data.items()}
    nets = alg.networks
    want = hb.RnnDqnStep(nets.q.hip_rnn(2), nets.q_target.hip_rnn(2), 17, dev["obs"].device).run(
        dev["obs"], dev["obs2"], dev["act"].reshape(-1), dev["rew"], dev["done"], dev["weight"], reward_scale=RSCALE, gamma=GAMMA)
    want = {k: v.clone() for k, v in want.items()}
    tb_info, idx, abs_err = alg.local_update(data, 0)
    assert alg.backup_path == "fused" and idx is data["idx"]
    assert torch.equal(abs_err, want["abs_err"]) and float(abs_err.max()) > 0
    assert float(alg._last[0]) == float(want["stats"][0])
