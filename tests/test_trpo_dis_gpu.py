"""TRPO on discrete actions on the MI355X: gops_cat_fisher_seed and gops_cat_trpo_surrogate against float64 restatements (the bars are
multiples of what an fp32 evaluation of the same case loses against float64), the fixtures of tests/golden/make_golden_trpo_dis.py
through `local_update`, graph replay against eager launches, and a short OnSerialTrainer run on the two-action cartpole."""
import copy

import numpy as np
import pytest
import torch

import trpo_dis_helpers as td
import trpo_helpers as th
from ac_helpers import EPS32, S, TOL, check_rows_beyond_the_batch, close
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NETS = {"n1": [3, 16, 2], "n2": [4, 64, 64, 5], "n3": [6, 16, 32, 48, 16], "wide": [3, 256, 3]}
SEED_CASES = ([("n1", a, B) for a in ("relu", "elu") for B in (1, 2, 17, 70, 257)]
              + [("n2", a, B) for a in ("gelu", "tanh") for B in (1, 17, 70, 257)]
              + [("n3", a, B) for a in ("sigmoid", "linear") for B in (2, 70, 257)] + [("wide", "relu", 70)])


def _case(net, act, B, seed=0, gap=None):
    """(float64 stack whose logits have spread 2 over the probe - `gap`: the output layer scaled further, so that the largest gap within
    a row exceeds it -, obs float64 [B, in]) - the same stack for every B of a net; the parameters are fp32 numbers on every side."""
    sizes = NETS[net]
    seq = th.mlp_stack(sizes, act, seed=11 + seed)
    g = torch.Generator().manual_seed(5 + seed)
    probe = torch.randn(257, sizes[0], generator=g, dtype=torch.float64)
    with torch.no_grad():
        head = [m for m in seq if isinstance(m, torch.nn.Linear)][-1]
        z = seq(probe[:70])
        scale = 2.0 / z.std() if gap is None else 1.5 * gap / (z.max(dim=1).values - z.min(dim=1).values).max()
        head.weight.mul_(scale), head.bias.mul_(scale)
    return seq.float().double(), probe[:B].float().double()


def _device_net(seq, act):
    from gops_amd import hip_backend as hb
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    ws, bs = [m.weight.detach().float().cuda().contiguous() for m in lin], [m.bias.detach().float().cuda().contiguous() for m in lin]
    return hb.make_mlp(ws, bs, act), ws, bs


def _tangents(seq, kind, seed=1):
    g = torch.Generator().manual_seed(seed)
    full = [torch.randn(p.shape, generator=g, dtype=torch.float64).float().double() for p in seq.parameters()]
    if kind == "full":
        return full
    which, layer = kind.split(":")
    idx = 2 * int(layer) + (1 if which == "bias" else 0)
    return [t if i == idx else torch.zeros_like(t) for i, t in enumerate(full)]


def _seed_errors(seq, obs, tangent):
    """(float64 seed, logits, the fp32 host evaluation's error relative to the seed's largest element, that element)."""
    want, logits = td.metric_seed(seq, obs, tangent)
    comp, _ = td.metric_seed(copy.deepcopy(seq).float(), obs.float(), [t.float() for t in tangent])
    scale = want.abs().max().item()
    return want, logits, (comp.double() - want).abs().max().item() / scale, scale


def _run_seed(seq, act, obs, tangent, out=None):
    from gops_amd import hip_backend as hb
    mlp, ws, bs = _device_net(seq, act)
    fs = hb.CatFisherSeed(mlp, "cuda")
    tw, tb = [t.float().cuda().contiguous() for t in tangent[0::2]], [t.float().cuda().contiguous() for t in tangent[1::2]]
    return fs.run(obs.float().cuda().contiguous(), tw, tb, seed=out)


# ---- gops_cat_fisher_seed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,act,B", SEED_CASES)
def test_cat_fisher_seed_against_float64(net, act, B):
    """seed = (1/B) (diag p - p p^T) (J v) against torch.func.jvp plus the metric in float64.  Bar: 4 x the error of the same evaluation
    in fp32 on the host, relative to the seed's largest element.  The kernel writes the batch's rows and nothing behind them; a second
    launch gives the same bits; each row sums to zero within 4 eps32 n max|seed| (every element is one rounding of a double whose row
    sum is zero to double precision)."""
    seq, obs = _case(net, act, B)
    n = NETS[net][-1]
    tangent = _tangents(seq, "full")
    want, _, err32, scale = _seed_errors(seq, obs, tangent)
    got = check_rows_beyond_the_batch(lambda out: _run_seed(seq, act, obs, tangent, out=out["seed"].view(B, n)), dict(seed=n * B))
    again = _run_seed(seq, act, obs, tangent)
    torch.cuda.synchronize()
    got64 = got.double().cpu().view(B, n)
    err = (got64 - want).abs().max().item() / scale
    row_sum = got64.sum(dim=1).abs().max().item()
    print(f"cat_fisher_seed {net} {act} B={B}: kernel {err:.3e} fp32 host {err32:.3e} bar {4 * err32:.3e}; row sums {row_sum:.3e}")
    assert torch.equal(got.view(-1), again.view(-1))
    assert row_sum <= 4 * EPS32 * n * got64.abs().max().item()
    assert err <= 4 * err32, (err, err32)


@pytest.mark.parametrize("kind", [f"{w}:{j}" for j in range(4) for w in ("bias", "weight")])
def test_cat_fisher_seed_takes_every_layers_tangent(kind):
    """A tangent that is zero except in ONE layer's bias, or ONE layer's weight (three hidden layers of different widths, 16 logits):
    a dropped V h or c term of that layer shows as a zero or wrong seed.  Same bar."""
    seq, obs = _case("n3", "tanh", 17)
    tangent = _tangents(seq, kind)
    want, _, err32, scale = _seed_errors(seq, obs, tangent)
    got = _run_seed(seq, "tanh", obs, tangent)
    err = (got.double().cpu() - want).abs().max().item() / scale
    print(f"cat_fisher_seed one-hot tangent {kind}: kernel {err:.3e} fp32 host {err32:.3e}")
    assert scale > 0 and err <= 4 * err32, (kind, err, err32)


def test_cat_fisher_seed_has_the_softmax_metrics_null_direction():
    """What only diag(p) - p p^T satisfies: a tangent that is zero except for the output layer's bias, equal to a constant c in every
    component, moves every logit alike and no probability - |seed| <= 4 eps32 |c| / B (u_k = c exactly, pu = c sum p_k = c within a few
    double roundings).  The diagonal-only metric p u / B fails this bound and the zero row sums by orders of magnitude."""
    seq, obs = _case("n2", "gelu", 70)
    c, B, n = 0.75, 70, 5
    tangent = [torch.zeros_like(p) for p in seq.parameters()]
    tangent[-1] = torch.full_like(tangent[-1], c)
    got = _run_seed(seq, "gelu", obs, tangent).double().cpu()
    diag = td.diagonal_seed(seq, obs, tangent)
    print(f"cat_fisher_seed constant bias tangent: max |seed| {got.abs().max().item():.3e} bound {4 * EPS32 * c / B:.3e}; "
          f"diagonal-only metric {diag.abs().max().item():.3e}")
    assert got.abs().max().item() <= 4 * EPS32 * c / B
    assert diag.abs().max().item() > 1e3 * 4 * EPS32 * c / B
    full = td.diagonal_seed(seq, obs, _tangents(seq, "full"))
    assert full.sum(dim=1).abs().max().item() > 4 * EPS32 * n * full.abs().max().item()


def test_cat_fisher_seed_with_large_logit_gaps():
    """The output layer scaled until the gap within a row exceeds 1000 on some rows: exp(z - max) underflows to zero there, every value
    stays finite, and the result keeps the 4 x fp32 bar against the float64 restatement (which shifts by the maximum as well)."""
    seq, obs = _case("n2", "tanh", 70, gap=1000.0)
    tangent = _tangents(seq, "full")
    want, logits, err32, scale = _seed_errors(seq, obs, tangent)
    gaps = logits.max(dim=1).values - logits.min(dim=1).values
    assert (gaps > 1000).any()
    got = _run_seed(seq, "tanh", obs, tangent).double().cpu()
    err = (got - want).abs().max().item() / scale
    print(f"cat_fisher_seed large gaps (max {gaps.max().item():.0f}): kernel {err:.3e} fp32 host {err32:.3e} bar {4 * err32:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 4 * err32, (err, err32)


def test_cat_fisher_seed_rows_do_not_depend_on_the_tile():
    """The same rows inside batches of 256, 2048 and 16384 rows, which run on tiles of 16, 32 and 64 rows: bit-identical up to 1 / B,
    a power of two apart.  And the rows of B = 257 against the same rows run in a batch of 1 and of 17: 1 / B is no power of two apart
    there, so seed * B is equal up to the one rounding of the division on each side (2 eps32 of the value)."""
    seq, obs = _case("n2", "elu", 257)
    tangent = _tangents(seq, "full")
    g = torch.Generator().manual_seed(9)
    big = torch.cat((obs, torch.randn(16384 - 257, obs.shape[1], generator=g, dtype=torch.float64)))
    s256, s2048, s16384 = (_run_seed(seq, "elu", big[:B], tangent) for B in (256, 2048, 16384))
    assert torch.equal(s256 * (1.0 / 8), s2048[:256]) and torch.equal(s2048[:257] * (1.0 / 8), s16384[:257])
    s257 = _run_seed(seq, "elu", big[:257], tangent).double() * 257
    for B in (1, 17):
        sB = _run_seed(seq, "elu", big[:B], tangent).double() * B
        assert ((sB - s257[:B]).abs() <= 2 * EPS32 * sB.abs()).all(), B


def test_cat_fisher_product_against_the_double_backward():
    """seed, then gops_mlp_backward: the whole product against the float64 `hvp` of the reference's form (double backward of the
    categorical KL).  Bar: 4 x the fp32 `hvp` on the host, the Gaussian product test's bound."""
    from gops_amd import hip_backend as hb
    seq, obs = _case("n2", "gelu", 70)
    v = _tangents(seq, "full", seed=2)
    want = th.flat(td.hessian_product(seq, obs, v))
    err32 = th.rel_max(th.flat(td.hessian_product(copy.deepcopy(seq).float(), obs.float(), [t.float() for t in v])), want)
    mlp, ws, bs = _device_net(seq, "gelu")
    net, fs = hb.MlpNet(mlp, 70), hb.CatFisherSeed(mlp, "cuda")
    x = obs.float().cuda().contiguous()
    net.forward(x)
    out = torch.zeros(sum(w.numel() + b.numel() for w, b in zip(ws, bs)), device="cuda")
    views = hb.flat_views(out, [s for w, b in zip(ws, bs) for s in (tuple(w.shape), tuple(b.shape))])
    tw, tb = [a.float().cuda().contiguous() for a in v[0::2]], [a.float().cuda().contiguous() for a in v[1::2]]
    net.backward(x, fs.run(x, tw, tb), views[0::2], views[1::2])
    torch.cuda.synchronize()
    err = th.rel_max(out.cpu(), want)
    print(f"cat fisher product: kernels {err:.3e} fp32 host hvp {err32:.3e} bar {4 * err32:.3e}")
    assert err <= 4 * err32


# ---- gops_cat_trpo_surrogate -------------------------------------------------------------------------------------------------------
def _bound_check(label, got, comp, want):
    """test_trpo_gpu.py's rule: the same formulas composed from fp32 torch ops on the device are measured first; the kernel may use
    twice their max error, and not less than 4 fp32 ulp of the tensor's largest magnitude."""
    want = want.reshape(got.shape)
    err_c = (comp.double().cpu().reshape(got.shape) - want).abs().max().item()
    err_k = (got.double().cpu() - want).abs().max().item()
    bound = max(2 * err_c, 4 * EPS32 * want.abs().max().item())
    print(f"{label}: kernel {err_k:.3e} composed {err_c:.3e} bound {bound:.3e}")
    assert err_k <= bound, (label, err_k, err_c, bound)


@pytest.mark.parametrize("M,n", [(1, 2), (2, 5), (70, 16), (257, 2), (8192, 5), (8193, 16)])
def test_cat_surrogate_kernel_against_float64(M, n):
    from gops_amd import hip_backend as hb
    host = td.synthetic_logits(M, n)
    gaps = host["head_new"].max(dim=1).values - host["head_new"].min(dim=1).values
    assert gaps.max() <= 30
    sur64, kl64, seed64 = td.restate_surrogate(host)
    sur32, kl32, seed32 = td.restate_surrogate(host, dtype=torch.float32, device="cuda")
    t = {k: v.cuda() for k, v in host.items()}
    ts = hb.CatTrpoSurrogate(n, "cuda")
    # the verdict on both sides of both thresholds, each at least 1e-3 away
    for delta, want_verdict in ((float(kl64) + 1e-3 + 0.1, float(sur64) > 0), (max(float(kl64) - 1e-3 - 0.1 * float(kl64), 0.0), False)):
        assert abs(float(kl64) - delta) >= 1e-3 and abs(float(sur64)) >= 1e-3
        ts.set_delta(delta)

        def run(out=None):
            seed, st = ts.run(t["head_new"], t["head_old"], t["act"], t["adv"], seed_head=None if out is None else out["seed"].view(M, n))
            return dict(seed=seed.clone(), stats=st.clone(), verdict=ts.verdict.clone(), bad=ts.bad_index.clone())

        got = check_rows_beyond_the_batch(run, dict(seed=M * n))
        again = run()
        torch.cuda.synchronize()
        label = f"cat_trpo_surrogate M={M} n={n}"
        _bound_check(label + " seed", got["seed"], seed32, seed64)
        _bound_check(label + " surrogate", got["stats"][0], sur32, sur64)
        _bound_check(label + " kl", got["stats"][1], kl32, kl64)
        assert int(got["verdict"].item()) == int(want_verdict) and int(got["bad"].item()) == 0
        for k in got:
            assert torch.equal(got[k], again[k]), k
        assert (ts.buf.view(torch.int32)[4 + 2 * 2 * 64:] == 0).all()   # the ticket and the running count behind it
    # the same verdict for a surrogate of the other sign (the advantages negated), the KL well inside delta
    ts.set_delta(float(kl64) + 1e-3 + 0.1)
    ts.run(t["head_new"], t["head_old"], t["act"], -t["adv"], want_seed=False)
    assert int(ts.verdict.item()) == int(-float(sur64) > 0)
    # aliased logits (the evaluation at theta_old): the ratio is exactly 1 - the surrogate is mean(adv) in double, rounded once - and
    # the KL exactly 0; no seed is written when none is asked for
    untouched = torch.full((M * n,), S, device="cuda")
    _, st = ts.run(t["head_new"], t["head_new"], t["act"], t["adv"], seed_head=untouched.view(M, n), want_seed=False)
    torch.cuda.synchronize()
    mean_adv = host["adv"].double().mean().item()
    assert float(st[1]) == 0.0 and abs(float(st[0]) - mean_adv) <= EPS32 * abs(mean_adv)
    assert (untouched == S).all()


def test_cat_surrogate_leaves_out_rows_with_a_bad_index():
    """M = 257 with three bad rows - an index of -1, one equal to n and a NaN: `bad_index` counts them, their seed rows are exactly
    zero, the sums are the float64 sums over the other rows divided by M, and the sentinel behind the outputs is intact."""
    from gops_amd import hip_backend as hb
    M, n = 257, 5
    host = td.synthetic_logits(M, n)
    rows = torch.ones(M, dtype=torch.bool)
    for i, v in ((3, -1.0), (100, float(n)), (256, float("nan"))):
        host["act"][i], rows[i] = v, False
    safe = dict(host, act=torch.where(rows, host["act"], torch.zeros(())))
    sur64, kl64, seed64 = td.restate_surrogate(safe, rows=rows)
    sur32, kl32, seed32 = td.restate_surrogate(safe, dtype=torch.float32, device="cuda", rows=rows)
    t = {k: v.cuda() for k, v in host.items()}
    ts = hb.CatTrpoSurrogate(n, "cuda")
    ts.set_delta(1.0)

    def run(out=None):
        seed, st = ts.run(t["head_new"], t["head_old"], t["act"], t["adv"], seed_head=out["seed"].view(M, n))
        return dict(seed=seed.clone(), stats=st.clone())

    got = check_rows_beyond_the_batch(run, dict(seed=M * n))
    torch.cuda.synchronize()
    assert int(ts.bad_index.item()) == 3 and ts.flags()[1] == 3
    assert (got["seed"].view(M, n)[~rows.cuda()] == 0.0).all() and (got["seed"].view(M, n)[rows.cuda()] != 0.0).any()
    _bound_check("bad rows seed", got["seed"], seed32, seed64)
    _bound_check("bad rows surrogate", got["stats"][0], sur32, sur64)
    _bound_check("bad rows kl", got["stats"][1], kl32, kl64)
    t["act"][~rows.cuda()] = 0.0   # the count is the call's own: back to zero with a clean batch
    ts.run(t["head_new"], t["head_old"], t["act"], t["adv"], want_seed=False)
    assert int(ts.bad_index.item()) == 0


# ---- local_update ------------------------------------------------------------------------------------------------------------------
def _policy_flat(alg):
    return th.flat([p.detach() for p in alg.networks.policy.parameters()]).double().cpu()


@pytest.mark.parametrize("name", td.FIXTURES)
def test_local_update_against_float64(name, monkeypatch):
    """One local_update per fixture, eager: the accepted index is the fixture's and the CG iteration count the restatement's; g, x,
    step and the final policy within 4 x the fp32 REFERENCE's own error against the float64 restatement
    (tests/golden/trpo_dis_reference_error.json), measured against that restatement; value parameters rel-L2 1e-4 against the
    reference, tb values `close`; for the rejected fixture the policy comes back bit-identical."""
    monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
    alg, g, meta = td.load_trpo_dis(name, use_gpu=True)
    want = td.restate_trpo_update(alg, th.data_of(g))
    before = _policy_flat(alg)
    tb = alg.local_update(th.data_of(g), 0)
    cg = alg._cache["cg"]
    got = dict(g=cg.g.cpu(), x=cg.x.cpu(), step=cg.step_vec.cpu(), policy=_policy_flat(alg))
    bars = td.reference_error()[name]
    errs = {k: th.rel_max(got[k], th.flat(want[k]) if k == "policy" else want[k]) for k in th.QUANTITIES}
    print(f"{name}: kernels against float64 {errs}; fp32 reference against float64 {bars}")
    assert (-1 if alg.last_search_index is None else alg.last_search_index) == int(g["accepted"])
    assert alg.last_cg_iterations == want["cg_iterations"]
    for k, v in alg.networks.value.state_dict().items():
        assert rel_l2(v.cpu(), g["sd_after/value." + k]) < TOL, k
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), (k, float(tb[k[3:]]), float(g[k]))
    if int(g["accepted"]) == -1:
        assert torch.equal(_policy_flat(alg), before)
    for k in th.QUANTITIES:
        assert errs[k] <= 4 * bars[k], (k, errs[k], bars[k])


def test_graph_replay_matches_eager_launches(monkeypatch):
    """GOPS_HIP_GRAPH=1 against 0 over 5 local_updates with new data each: x and every parameter bit-equal; the CG loop and the value
    step are each captured once and replayed from then on."""
    def run(mode):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        alg, g, meta = td.load_trpo_dis("trpo_dis_cart_relu", use_gpu=True)
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


def test_local_update_with_an_action_out_of_range_raises():
    """An index equal to act_num in one row: ValueError (the reference raises inside `gather`), and the policy is left at theta_old."""
    alg, g, meta = td.load_trpo_dis("trpo_dis_o3n5_gelu", use_gpu=True)
    data = th.data_of(g)
    data["act"][7] = float(meta["cfg"]["act_num"])
    before = _policy_flat(alg)
    with pytest.raises(ValueError, match="1 rows of `act` hold an action index outside"):
        alg.local_update(data, 0)
    assert torch.equal(_policy_flat(alg), before)


def test_on_serial_trainer_runs_discrete_trpo(tmp_path):
    """Five iterations of OnSerialTrainer with TRPO on the on-policy device sampler and the cartpole model with the action table
    [[-1.], [1.]]: tb values and parameters stay finite, every stored `act` is 0.0 or 1.0 and its `logp` the policy's."""
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    torch.manual_seed(0)
    args = td.dis_kwargs(4, 2, [64, 64], "relu", use_gpu=True, env_id="gym_cartpoleconti", action_dim=1, max_iteration=8, sample_batch_size=128,
                         log_save_interval=1000, apprfunc_save_interval=1000, eval_interval=10 ** 9, save_folder=str(tmp_path),
                         ini_network_dir=None)
    alg = create_alg(**args)
    alg.networks.to("cuda")
    model = create_env_model(**args)
    smp = OnPolicyDeviceSampler(dict(env_id="gym_cartpoleconti"), model, n_envs=8, steps_per_sample=16, max_episode_steps=50, seed=3,
                                env_step="model", action_table=[[-1.0], [1.0]])
    smp.networks = alg.networks
    batch, _ = smp.sample()
    assert batch["act"].shape == (128, 1) and ((batch["act"] == 0.0) | (batch["act"] == 1.0)).all() and (batch["act"] == 1.0).any()
    logp = torch.log_softmax(alg.networks.policy(batch["obs"]), dim=-1).gather(1, batch["act"].long()).squeeze(1)
    assert torch.allclose(batch["logp"], logp, rtol=1e-5, atol=1e-6)
    trainer = create_trainer(alg, smp, None, None, **args)
    seen = []
    sample = smp.sample
    smp.sample = lambda: seen.append(sample()) or seen[-1]
    for _ in range(5):
        trainer.step()
        trainer.iteration += 1
        assert all(np.isfinite(float(v)) for v in alg.tb_info.values()), dict(alg.tb_info)
    assert all(torch.isfinite(p).all() for p in alg.networks.state_dict().values())
    assert len(seen) == 5 and all(((b["act"] == 0.0) | (b["act"] == 1.0)).all() for b, _ in seen)
