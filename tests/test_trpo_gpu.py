"""TRPO on the MI355X: the kernels of csrc/trpo.hip against float64 restatements (the bars are multiples of what an fp32 evaluation
of the same case on the host loses against float64), the fixtures of tests/golden/make_golden_trpo.py through `local_update`, graph
replay against eager launches, and a short OnSerialTrainer run."""
import copy

import numpy as np
import pytest
import torch

import trpo_helpers as th
from ac_helpers import EPS32, TOL, check_rows_beyond_the_batch, close
from conftest import rel_l2
from ppo_helpers import KERNEL_SHAPES

pytestmark = pytest.mark.gpu

NETS = {"n1": [3, 16, 2], "n2": [4, 64, 64, 4], "n3": [6, 16, 32, 48, 6], "wide": [3, 256, 2]}
# every activation of act_dispatch, every net, every row count of the issue; the 256-wide net once
SEED_CASES = ([("n1", a, B) for a in ("relu", "elu") for B in (1, 2, 17, 70, 257)]
              + [("n2", a, B) for a in ("gelu", "selu", "tanh") for B in (1, 17, 70, 257)] + [("n2", "gelu", 2)]
              + [("n3", a, B) for a in ("sigmoid", "linear") for B in (2, 70, 257)] + [("n3", "relu", B) for B in (1, 17)]
              + [("wide", "relu", 70)])


def _case(net, act, B, seed=0):
    """(float64 stack with log stds on both sides of the clamp, obs float64 [B, in]) - the same stack for every B of a net."""
    sizes = NETS[net]
    A = sizes[-1] // 2
    seq = th.mlp_stack(sizes, act, seed=11 + seed)
    g = torch.Generator().manual_seed(5 + seed)
    probe = torch.randn(257, sizes[0], generator=g, dtype=torch.float64)
    th.spread_log_std(seq, probe[:70], A)
    seq = seq.float().double()   # (the parameters are fp32 numbers on every side)
    return seq, probe[:B].float().double(), A


def _device_net(seq, act, B):
    from gops_amd import hip_backend as hb
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    ws, bs = [m.weight.detach().float().cuda().contiguous() for m in lin], [m.bias.detach().float().cuda().contiguous() for m in lin]
    mlp = hb.make_mlp(ws, bs, act)
    return mlp, ws, bs


def _tangents(seq, kind, seed=1):
    g = torch.Generator().manual_seed(seed)
    params = list(seq.parameters())
    full = [torch.randn(p.shape, generator=g, dtype=torch.float64).float().double() for p in params]
    if kind == "full":
        return full
    which, layer = kind.split(":")
    idx = 2 * int(layer) + (1 if which == "bias" else 0)
    return [t if i == idx else torch.zeros_like(t) for i, t in enumerate(full)]


def _seed_errors(seq, obs, tangent):
    want, head = th.metric_seed(seq, obs, tangent)
    seq32 = copy.deepcopy(seq).float()
    comp, _ = th.metric_seed(seq32, obs.float(), [t.float() for t in tangent])
    scale = want.abs().max().item()
    return want, head, (comp.double() - want).abs().max().item() / scale, scale


def _run_seed(seq, act, obs, tangent, out=None):
    from gops_amd import hip_backend as hb
    mlp, ws, bs = _device_net(seq, act, obs.shape[0])
    fs = hb.FisherSeed(mlp, th.MIN_LS, th.MAX_LS, "cuda")
    tw, tb = [t.float().cuda().contiguous() for t in tangent[0::2]], [t.float().cuda().contiguous() for t in tangent[1::2]]
    return fs.run(obs.float().cuda().contiguous(), tw, tb, seed=out)


@pytest.mark.parametrize("net,act,B", SEED_CASES)
def test_fisher_seed_against_float64(net, act, B):
    """seed = (1/B) M (J v) against torch.func.jvp plus the metric in float64.  Bar: 4 x the error of the same evaluation in fp32 on
    the host, relative to the seed's largest element (a different but equally long summation order).  The kernel writes the batch's
    rows and nothing behind them; a second launch gives the same bits; the log-std column is exactly zero outside the clamp."""
    seq, obs, A = _case(net, act, B)
    tangent = _tangents(seq, "full")
    want, head, err32, scale = _seed_errors(seq, obs, tangent)
    got = check_rows_beyond_the_batch(lambda out: _run_seed(seq, act, obs, tangent, out=out["seed"].view(B, 2 * A)), dict(seed=2 * A * B))
    again = _run_seed(seq, act, obs, tangent)
    torch.cuda.synchronize()
    err = (got.double().cpu().view(B, 2 * A) - want).abs().max().item() / scale
    print(f"fisher_seed {net} {act} B={B}: kernel {err:.3e} fp32 host {err32:.3e} bar {4 * err32:.3e}")
    raw = head[:, A:]
    below, inside, above = th.clamp_zones(raw)
    assert B < 70 or min(below, inside, above) >= 4, (below, inside, above)
    outside = ((raw < th.MIN_LS) | (raw > th.MAX_LS)).cuda()
    assert (got.view(B, 2 * A)[:, A:][outside] == 0.0).all()
    assert torch.equal(got.view(-1), again.view(-1))
    assert err <= 4 * err32, (err, err32)


@pytest.mark.parametrize("kind", [f"{w}:{j}" for j in range(4) for w in ("bias", "weight")])
def test_fisher_seed_takes_every_layers_tangent(kind):
    """A tangent that is zero except in ONE layer's bias, or ONE layer's weight (three hidden layers of different widths): a missing
    V h + c term of that layer shows as a zero or wrong seed.  Same bar."""
    seq, obs, A = _case("n3", "tanh", 17)
    tangent = _tangents(seq, kind)
    want, _, err32, scale = _seed_errors(seq, obs, tangent)
    got = _run_seed(seq, "tanh", obs, tangent)
    err = (got.double().cpu() - want).abs().max().item() / scale
    print(f"fisher_seed one-hot tangent {kind}: kernel {err:.3e} fp32 host {err32:.3e}")
    assert scale > 0 and err <= 4 * err32, (kind, err, err32)


def test_fisher_seed_rows_do_not_depend_on_the_tile():
    """The same rows inside batches of 70, 2048 and 16384 rows, which run on tiles of 16, 32 and 64 rows: bit-identical up to 1 / B,
    which is a power of two apart for 2048 and 16384 (and is divided out exactly for 70 against a 70-row prefix run at B = 70)."""
    seq, obs, A = _case("n2", "elu", 257)
    tangent = _tangents(seq, "full")
    g = torch.Generator().manual_seed(9)
    big = torch.cat((obs, torch.randn(16384 - 257, obs.shape[1], generator=g, dtype=torch.float64)))
    s2048 = _run_seed(seq, "elu", big[:2048], tangent)
    s16384 = _run_seed(seq, "elu", big, tangent)
    assert torch.equal(s2048[:257] * (1.0 / 8), s16384[:257])          # R = 32 against R = 64: 1 / B differs by exactly 8
    s256 = _run_seed(seq, "elu", big[:256], tangent)                     # R = 16, 1 / B a power of two
    assert torch.equal(s256 * (1.0 / 8), s2048[:256])
    s70, s257 = _run_seed(seq, "elu", big[:70], tangent), _run_seed(seq, "elu", big[:257], tangent)
    ratio = (s70.double() * 70) - (s257[:70].double() * 257)            # same tile size, other partial tiles: equal up to the division's rounding
    assert ratio.abs().max().item() <= 4 * EPS32 * (s70.double().abs().max().item() * 70)


def test_fisher_product_against_the_double_backward():
    """seed, then gops_mlp_backward: the whole product against the float64 `hvp` of the reference's form.  Bar: 4 x the fp32 `hvp` on
    the host.  Symmetry: u.(F v) = v.(F u) to that bar.  The stash of ONE forward serves every backward: a second product of the same
    tangent has the same bits, with another product in between."""
    from gops_amd import hip_backend as hb
    seq, obs, A = _case("n2", "tanh", 70)
    u, v = _tangents(seq, "full", seed=1), _tangents(seq, "full", seed=2)
    want_v, want_u = th.flat(th.hessian_product(seq, obs, v)), th.flat(th.hessian_product(seq, obs, u))
    seq32 = copy.deepcopy(seq).float()
    err32 = th.rel_max(th.flat(th.hessian_product(seq32, obs.float(), [t.float() for t in v])), want_v)
    mlp, ws, bs = _device_net(seq, "tanh", 70)
    net, fs = hb.MlpNet(mlp, 70), hb.FisherSeed(mlp, th.MIN_LS, th.MAX_LS, "cuda")
    x = obs.float().cuda().contiguous()
    net.forward(x)

    def product(t):
        out = torch.zeros(sum(w.numel() + b.numel() for w, b in zip(ws, bs)), device="cuda")
        views = hb.flat_views(out, [s for w, b in zip(ws, bs) for s in (tuple(w.shape), tuple(b.shape))])
        tw, tb = [a.float().cuda().contiguous() for a in t[0::2]], [a.float().cuda().contiguous() for a in t[1::2]]
        net.backward(x, fs.run(x, tw, tb), views[0::2], views[1::2])
        return out

    fv, fu, fv2 = product(v), product(u), product(v)
    torch.cuda.synchronize()
    err = th.rel_max(fv.cpu(), want_v)
    print(f"fisher product: kernels {err:.3e} fp32 host hvp {err32:.3e} bar {4 * err32:.3e}")
    assert torch.equal(fv, fv2)
    assert err <= 4 * err32 and th.rel_max(fu.cpu(), want_u) <= 4 * err32
    ufv, vfu = torch.dot(th.flat(u), fv.double().cpu()).item(), torch.dot(th.flat(v), fu.double().cpu()).item()
    size = th.flat(u).abs().max().item() * want_v.abs().max().item() * want_v.numel()
    assert abs(ufv - vfu) <= 4 * err32 * size, (ufv, vfu)
    assert abs(ufv - torch.dot(th.flat(u), want_v).item()) <= 4 * err32 * size


def test_fisher_seed_refuses_what_it_does_not_hold():
    from gops_amd import hip_backend as hb
    for sizes, reason in (([3, 24, 2], "GOPS_ERR_UNSUPPORTED"), ([3, 16, 3], "GOPS_ERR_BAD_ARG"), ([3, 16, 16, 16, 16, 2], "GOPS_ERR_UNSUPPORTED")):
        seq = th.mlp_stack(sizes, "relu", seed=0)
        mlp, ws, bs = _device_net(seq, "relu", 4)
        fs = hb.FisherSeed(mlp, th.MIN_LS, th.MAX_LS, "cuda")
        with pytest.raises(RuntimeError, match=reason):
            fs.run(torch.zeros(4, 3, device="cuda"), [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs],
                   seed=torch.zeros(4, sizes[-1], device="cuda"))


# ---- gops_trpo_surrogate ---------------------------------------------------------------------------------------------------------
def _bound_check(label, got, comp, want):
    """test_ppo_gpu.py's rule for gops_ppo_loss: the same formulas composed from fp32 torch ops on the device are measured first; the
    kernel may use twice their max error, and not less than 4 fp32 ulp of the tensor's largest magnitude."""
    want = want.reshape(got.shape)
    err_c = (comp.double().cpu().reshape(got.shape) - want).abs().max().item()
    err_k = (got.double().cpu() - want).abs().max().item()
    bound = max(2 * err_c, 4 * EPS32 * want.abs().max().item())
    print(f"{label}: kernel {err_k:.3e} composed {err_c:.3e} bound {bound:.3e}")
    assert err_k <= bound, (label, err_k, err_c, bound)


@pytest.mark.parametrize("M,A", KERNEL_SHAPES)
def test_trpo_surrogate_kernel_against_float64(M, A):
    from gops_amd import hip_backend as hb
    host = th.synthetic_heads(M, A)
    sur64, kl64, seed64 = th.restate_surrogate(host)
    sur32, kl32, seed32 = th.restate_surrogate(host, dtype=torch.float32, device="cuda")
    t = {k: v.cuda() for k, v in host.items()}
    ts = hb.TrpoSurrogate(A, th.MIN_LS, th.MAX_LS, "cuda")
    # the verdict on both sides of both thresholds, each at least 1e-3 away
    for delta, want_verdict in ((float(kl64) + 1e-3 + 0.1, float(sur64) > 0), (max(float(kl64) - 1e-3 - 0.1 * float(kl64), 0.0), False)):
        assert abs(float(kl64) - delta) >= 1e-3 and abs(float(sur64)) >= 1e-3
        ts.set_delta(delta)

        def run(out=None):
            seed, st = ts.run(t["head_new"], t["head_old"], t["act"], t["adv"], seed_head=None if out is None else out["seed"].view(M, 2 * A))
            return dict(seed=seed.clone(), stats=st.clone(), verdict=ts.verdict.clone())

        got = check_rows_beyond_the_batch(run, dict(seed=2 * M * A))
        again = run()
        torch.cuda.synchronize()
        label = f"trpo_surrogate M={M} A={A}"
        _bound_check(label + " seed", got["seed"], seed32, seed64)
        _bound_check(label + " surrogate", got["stats"][0], sur32, sur64)
        _bound_check(label + " kl", got["stats"][1], kl32, kl64)
        assert int(got["verdict"].item()) == int(want_verdict)
        for k in got:
            assert torch.equal(got[k], again[k]), k
        assert int(ts.buf.view(torch.int32)[4 + 2 * 2 * 64].item()) == 0   # the ticket
    raw = t["head_new"][:, A:]
    outside = (raw < th.MIN_LS) | (raw > th.MAX_LS)
    assert (got["seed"].view(M, 2 * A)[:, A:][outside] == 0.0).all() and (M < 70 or outside.any() and (~outside).any())
    # aliased heads (the evaluation at theta_old): the ratio is exactly 1 - the surrogate is mean(adv) in double, rounded once - and
    # the KL exactly 0; no seed is written when none is asked for
    _, st = ts.run(t["head_new"], t["head_new"], t["act"], t["adv"], want_seed=False)
    torch.cuda.synchronize()
    mean_adv = host["adv"].double().mean().item()
    assert float(st[1]) == 0.0 and abs(float(st[0]) - mean_adv) <= EPS32 * abs(mean_adv)   # (one rounding of a double sum in another order)
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        hb.TrpoSurrogate(5, th.MIN_LS, th.MAX_LS, "cuda").run(torch.zeros(2, 10, device="cuda"), torch.zeros(2, 10, device="cuda"),
                                                               torch.zeros(2, 5, device="cuda"), torch.zeros(2, device="cuda"))


# ---- conjugate gradients -----------------------------------------------------------------------------------------------------------
def _spd(P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if P <= 512:
        q = torch.randn(P, P, generator=g, device="cuda", dtype=torch.float64)
        return (q @ q.T / P + torch.eye(P, device="cuda", dtype=torch.float64)).float()
    u = torch.randn(P, 8, generator=g, device="cuda", dtype=torch.float64) / P ** 0.5   # identity plus rank 8: dense all the same
    return (u @ u.T + torch.eye(P, device="cuda", dtype=torch.float64)).float()


@pytest.mark.parametrize("P", [1, 5, 257, 8193])
def test_cg_kernels_against_the_float64_recurrence(P):
    """A dense SPD matrix through torch.matmul is the operator.  Iteration by iteration: from the vectors the kernels hold before a
    step (fp32) and the product handed in, the float64 recurrence gives what they must hold after it - 4 fp32 ulp of each vector's
    largest element, the scalars to 1e-12 relative (they are doubles over fp32 data in another order).  8193: the first size on 64
    workgroups and three launches per step."""
    from gops_amd import hip_backend as hb
    A = _spd(P, P)
    damping, atol = 0.1, 1e-10
    cg = hb.CgSolver(P, "cuda")
    cg.hyper[:1].copy_(torch.tensor([0.01]))
    cg.g.copy_(torch.randn(P, generator=torch.Generator().manual_seed(P)).cuda())
    cg.init(atol)
    st = cg.state()
    assert torch.equal(cg.r, cg.g) and torch.equal(cg.p, cg.g) and (cg.x == 0).all() and st["done"] == 0 and st["calls"] == 0
    assert st["r_dot"] == pytest.approx(torch.dot(cg.g.double(), cg.g.double()).item(), rel=1e-12)
    for it in range(4):
        before = {k: getattr(cg, k).clone() for k in ("x", "r", "p")}
        r_dot = cg.state()["r_dot"]
        torch.matmul(A, cg.p, out=cg.Ap)
        want = th.cg_recurrence_step(before["x"], before["r"], before["p"], cg.Ap, r_dot, damping, atol)
        cg.step(damping, atol)
        st = cg.state()
        assert st["calls"] == it + 1 and st["iterations"] == it + 1 and st["done"] == int(want["done"])
        for k in ("x", "r", "p", "Ap"):   # (x, r, p are sums of two vectors of the size they had before: the stored Ap is an fp32 number)
            err = (getattr(cg, k).double() - want[k]).abs().max().item()
            size = max(want[k].abs().max().item(), before[k].abs().max().item() if k in before else 0.0)
            assert err <= 4 * EPS32 * size, (P, it, k, err, size)
        assert st["alpha"] == pytest.approx(want["alpha"], rel=1e-6) and st["r_dot"] == pytest.approx(want["r_dot"], rel=1e-4, abs=1e-30)
        if want["done"]:
            break
    cg.finish()
    st = cg.state()
    gx = torch.dot(cg.g.double(), cg.x.double()).item()
    assert st["g_x"] == pytest.approx(gx, rel=1e-10, abs=1e-30)
    want_step = np.sqrt(2 * float(np.float32(0.01)) / (gx + 1e-8)) * cg.x.double()
    assert (cg.step_vec.double() - want_step).abs().max().item() <= 2 * EPS32 * want_step.abs().max().item()
    assert int(cg._state.view(torch.int32)[15].item()) == 0   # the ticket


def test_cg_stops_at_the_tolerance_and_stays_stopped():
    """A diagonal 5 x 5 system with atol = 1e-4 sets `done` within 5 steps; every further gops_cg_step leaves x, r, p bitwise as they
    are and the iteration count still, while the call count goes on."""
    from gops_amd import hip_backend as hb
    diag = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], device="cuda")
    cg = hb.CgSolver(5, "cuda")
    cg.g.copy_(torch.tensor([1.0, -2.0, 0.5, 3.0, -1.0]))
    cg.init(1e-4)
    for k in range(5):
        torch.mul(diag, cg.p, out=cg.Ap)
        cg.step(0.0, 1e-4)
    st = cg.state()
    assert st["done"] == 1 and 1 <= st["iterations"] <= 5 and st["calls"] == 5
    assert (cg.x.double().cpu() - torch.tensor([1.0, -1.0, 1 / 6, 0.75, -0.2], dtype=torch.float64)).abs().max() < 1e-3
    frozen = {k: getattr(cg, k).clone() for k in ("x", "r", "p")}
    for k in range(3):
        torch.mul(diag, cg.p, out=cg.Ap)
        ap = cg.Ap.clone()
        cg.step(0.5, 1e-4)
        assert torch.equal(cg.Ap, ap)   # not even the damping is added
    after = cg.state()
    assert after["iterations"] == st["iterations"] and after["calls"] == 8 and after["done"] == 1
    for k, v in frozen.items():
        assert torch.equal(getattr(cg, k), v), k


def test_cg_with_a_gradient_within_the_tolerance():
    from gops_amd import hip_backend as hb
    cg = hb.CgSolver(7, "cuda")
    cg.hyper[:1].copy_(torch.tensor([0.01]))
    cg.x.fill_(3.0)
    cg.g.copy_(torch.tensor([1e-9, -1e-9, 0.0, 5e-10, -1e-9, 1e-9, 0.0]))
    cg.init(1e-9)
    assert cg.state()["done"] == 1
    cg.Ap.fill_(1.0)
    cg.step(0.1, 1e-9)
    cg.finish()
    assert (cg.x == 0).all() and (cg.step_vec == 0).all() and cg.state()["iterations"] == 0 and cg.state()["calls"] == 1


# ---- local_update ------------------------------------------------------------------------------------------------------------------
def _policy_flat(alg):
    return th.flat([p.detach() for p in alg.networks.policy.parameters()]).double().cpu()


@pytest.mark.parametrize("name", th.FIXTURES)
def test_local_update_against_float64(name, monkeypatch):
    """One local_update per fixture: the accepted index is the fixture's; g, x, step and the final policy within 4 x the fp32
    REFERENCE's own error against the float64 restatement (tests/golden/trpo_reference_error.json), measured against that restatement;
    value parameters and tb values to the bars of PPO's step (rel-L2 1e-4 against the reference, `close`)."""
    monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
    alg, g, meta = th.load_trpo(name, use_gpu=True)
    want = th.restate_trpo_update(alg, th.data_of(g))
    before = _policy_flat(alg)
    tb = alg.local_update(th.data_of(g), 0)
    cg = alg._cache["cg"]
    got = dict(g=cg.g.cpu(), x=cg.x.cpu(), step=cg.step_vec.cpu(), policy=_policy_flat(alg))
    bars = th.reference_error()[name]
    errs = {k: th.rel_max(got[k], th.flat(want[k]) if k == "policy" else want[k]) for k in th.QUANTITIES}
    print(f"{name}: kernels against float64 {errs}; fp32 reference against float64 {bars}")
    assert (-1 if alg.last_search_index is None else alg.last_search_index) == int(g["accepted"])
    assert alg.last_cg_iterations == want["cg_iterations"]
    for k, v in alg.networks.value.state_dict().items():
        assert rel_l2(v.cpu(), g["sd_after/value." + k]) < TOL, k
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), (k, float(tb[k[3:]]), float(g[k]))
    if int(g["accepted"]) == -1:
        assert torch.equal(_policy_flat(alg), before)   # every candidate failed: the policy comes back bit-identical
    for k in th.QUANTITIES:
        assert errs[k] <= 4 * bars[k], (k, errs[k], bars[k])


def test_graph_replay_matches_eager_launches(monkeypatch):
    """GOPS_HIP_GRAPH=1 against 0 over 5 local_updates with new data each: x, the step and every parameter bit-equal; the CG loop and
    the value step are each captured once and replayed from then on (both replay counters rise with further updates)."""
    def run(mode):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        alg, g, meta = th.load_trpo("trpo_pend_relu", use_gpu=True)
        xs, replays = [], []
        for it in range(5):
            data = th.data_of(g)
            data["ret"] = data["ret"] + 0.1 * it
            data["adv"] = data["adv"] * (1 + 0.05 * it)
            alg.local_update(data, it)
            xs.append(alg._cache["cg"].x.clone())
            replays.append((alg.cg_graph_replays, alg.value_graph_replays))
        return alg, xs, replays

    eager, x_e, rep_e = run("0")
    graph, x_g, rep_g = run("1")
    assert rep_e[-1] == (0, 0) and eager._cg_graph.graph is None and eager._v_graph.graph is None
    assert graph._cg_graph.graph is not None and graph._v_graph.graph is not None
    assert rep_g[-1][0] > rep_g[-2][0] >= 1 and rep_g[-1][1] >= rep_g[-2][1] + graph.train_v_iters
    for a, b in zip(x_e, x_g):
        assert torch.equal(a, b)
    for (ne, pe), (ng, pg) in zip(eager.networks.named_parameters(), graph.networks.named_parameters()):
        assert ne == ng and torch.equal(pe, pg), ne


def test_on_serial_trainer_runs_trpo(tmp_path):
    """Five iterations of OnSerialTrainer with TRPO on the on-policy device sampler and the pendulum model: tb_info stays finite."""
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    import ac_helpers as ah
    torch.manual_seed(0)
    args = ah._common_kwargs("TRPO", "gym_pendulum", 3, 1, ([-2.0], [2.0]), [64, 64], "relu", 0, True)
    args.update(th.CTOR, max_iteration=8, sample_batch_size=128, policy_min_log_std=-3.0, policy_max_log_std=-0.5,
                log_save_interval=1000, apprfunc_save_interval=1000, eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    alg = create_alg(**args)
    alg.networks.to("cuda")
    model = create_env_model(**args)
    smp = OnPolicyDeviceSampler(dict(env_id="gym_pendulum"), model, n_envs=8, steps_per_sample=16, max_episode_steps=50, seed=3, env_step="model")
    smp.networks = alg.networks
    trainer = create_trainer(alg, smp, None, None, **args)
    for _ in range(5):
        trainer.step()
        trainer.iteration += 1
        assert all(np.isfinite(float(v)) for v in alg.tb_info.values()), dict(alg.tb_info)
    assert all(torch.isfinite(p).all() for p in alg.networks.state_dict().values())
