"""GPU: the optimizer tail element by element - `gops_adam_step` (adam_kernel), its restatement in the fused reduce
(`gops_rollout_backward_update` / `gops_value_backward_update`), `gops_polyak_update` and `gops_value_loss` / `gops_mean_loss` - against
the float64 reference, the bounds and the expected bits of tests/optim_helpers.py, at the sizes that sit on the kernels' loop edges."""
import numpy as np
import pytest
import torch

import optim_helpers as oh

from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

HYPER = [dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8), dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6)]
HYPER_IDS = ["default", "betas-0.8-0.99"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _grids(sizes, seed, betas, fresh=False):
    return [oh.adam_grid(n, seed + i, betas, fresh=fresh) for i, n in enumerate(sizes)]


def _check_step(case, worst, label, hyper, t, gs, inputs, carried=None):
    """Every tensor of `case` after ONE step from `inputs` [(p, m, v, g)] (float64 when carried from earlier steps): p, m, v within the
    bounds of `adam_ref64`, elements without a finite scaled gradient and the g = m0 = v0 = 0 elements bit-unchanged.  -> (the
    float64 state after the step, the bounds) per tensor."""
    out = []
    for i, (p, m, v, g) in enumerate(inputs):
        ref = oh.adam_ref64(p, m, v, g, t=t, grad_scale=gs, **hyper)
        bounds = oh.adam_bounds(m, v, g, ref, lr=hyper["lr"], betas=hyper["betas"], t=t, grad_scale=gs, carried=None if carried is None else carried[i])
        got = case.read(i)
        worst.check(f"{label} tensor {i} (n = {g.size})", got, ref, bounds)
        if carried is None:
            same = oh.adam_zero_case(m, v, g) | ~oh.stepped(g, gs)
            for a, b in zip(got, (p, m, v)):
                assert oh.bits_equal(a[same], b[same]), (label, i)
        out.append((ref[:3], bounds))
    return out


# ------------------------------------------------------------------------------------------
# gops_adam_step through HipAdam
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", HYPER, ids=HYPER_IDS)
@pytest.mark.parametrize("t", [1, 10001])
def test_adam_one_step_per_element(dev, hyper, t):
    """ONE table with a tensor of every Adam size (1 and 262147 elements in the same launch: most blocks of the short tensors have
    nothing to do), one step from a state the test has filled - t = 1: zero moments, step 0; t = 10001: a loaded state - at every
    grad_scale: every element of p, m, v within E_p, E_m, E_v of float64; the guard region behind every tensor, and the gradients,
    untouched; the g = m0 = v0 = 0 elements bit-unchanged."""
    worst = oh.Worst()
    for k, gs in enumerate(oh.GRAD_SCALES):
        inputs = _grids(oh.ADAM_SIZES, 100, hyper["betas"], fresh=(t == 1))
        case = oh.AdamCase(inputs, dev, step=t - 1, **hyper)
        case.opt.grad_scale = gs
        case.opt.step()
        torch.cuda.synchronize()
        _check_step(case, worst, f"t={t} gs={gs:.3g}", hyper, t, gs, inputs)
        assert case.guards_intact()
        for i, (_, _, _, g) in enumerate(inputs):
            assert oh.bits_equal(case.bufs[i]["g"][:g.size].cpu(), g)
        assert all(int(case.opt.state[p]["step"]) == t for p in case.params)
        assert case.opt.skipped_nonfinite() == 0
    worst.report(f"adam_kernel, one step, t = {t}, betas = {hyper['betas']}")


def test_adam_changed_lr_between_two_steps(dev):
    """param_groups[0]["lr"] edited between two steps (a scheduler): the second step uses the new value - both steps within the
    bounds, the second against float64 carried from the first with the bounds added."""
    hyper, sizes, worst = HYPER[0], (257, 65537), oh.Worst()
    inputs = _grids(sizes, 300, hyper["betas"])
    case = oh.AdamCase(inputs, dev, step=40, **hyper)
    case.opt.step()
    torch.cuda.synchronize()
    first = _check_step(case, worst, "lr 3e-4", hyper, 41, 1.0, inputs)
    case.opt.param_groups[0]["lr"] = 1e-4
    g2 = [oh.adam_grid(n, 310 + i)[3] for i, n in enumerate(sizes)]
    for i, g in enumerate(g2):
        case.set_grad(i, g)
    case.opt.step()
    torch.cuda.synchronize()
    second = [(*state, g) for (state, _), g in zip(first, g2)]
    _check_step(case, worst, "lr 1e-4", dict(hyper, lr=1e-4), 42, 1.0, second, carried=[b for _, b in first])
    # the bounds do tell the two learning rates apart: the old one misses them
    ref_old = oh.adam_ref64(*second[1], t=42, grad_scale=1.0, **hyper)
    b_old = oh.adam_bounds(second[1][1], second[1][2], g2[1], ref_old, lr=hyper["lr"], betas=hyper["betas"], t=42, grad_scale=1.0, carried=first[1][1])
    assert oh.ratios(case.read(1)[0], ref_old[0], b_old[2])[0] > 1.0
    assert case.guards_intact()
    worst.report("adam_kernel, lr changed between two steps")


@pytest.mark.parametrize("k", [1, 3, 7])
def test_adam_device_state_advances(dev, k):
    """After k steps from a loaded state at step k0 the device GopsAdamState holds step = k0 + k, beta^step as the same sequence of
    double multiplications gives it in Python - bit for bit -, and a zero ticket."""
    hyper, k0 = HYPER[1], 5
    case = oh.AdamCase(_grids((257, 1025), 400, hyper["betas"]), dev, step=k0, **hyper)
    for _ in range(k):
        case.opt.step()
    torch.cuda.synchronize()
    b1p, b2p = float(hyper["betas"][0]) ** k0, float(hyper["betas"][1]) ** k0
    for _ in range(k):
        b1p, b2p = b1p * hyper["betas"][0], b2p * hyper["betas"][1]
    (lr, step, d1, d2, ticket, skipped, gsc), = case.device_state()
    assert (lr, step, ticket, skipped, gsc) == (hyper["lr"], k0 + k, 0, 0, 1.0)
    assert d1 == b1p and d2 == b2p, (d1, b1p, d2, b2p)
    assert all(int(case.opt.state[p]["step"]) == k0 + k for p in case.params)
    assert case.guards_intact()


def test_adam_three_steps_from_a_loaded_state(dev):
    """Three steps with fresh gradients from a loaded state at step 40 against three steps of `adam_ref64` carried in float64 from
    the same state: per element within the bounds of every step, added up (`adam_bounds(carried=)`)."""
    hyper, sizes, gs, worst = HYPER[0], (257, 65537, 81921), 1.0 / 3.0, oh.Worst()
    inputs = _grids(sizes, 500, hyper["betas"])
    case = oh.AdamCase(inputs, dev, step=40, **hyper)
    case.opt.grad_scale = gs
    state, carried = [x[:3] for x in inputs], None
    for k in range(3):
        gk = [x[3] for x in inputs] if k == 0 else [oh.adam_grid(n, 510 + 10 * k + i)[3] for i, n in enumerate(sizes)]
        for i, g in enumerate(gk):
            case.set_grad(i, g)
        case.opt.step()
        torch.cuda.synchronize()
        res = _check_step(case, worst, f"step {k + 1}", hyper, 41 + k, gs, [(*s, g) for s, g in zip(state, gk)], carried=carried if k else None)
        state, carried = [r[0] for r in res], [r[1] for r in res]
    assert case.device_state()[0][1] == 43 and case.guards_intact()
    worst.report("adam_kernel, three carried steps")


SMALL = (1, 255, 256, 257, 1023, 1024, 1025)


@pytest.mark.parametrize("sizes", [tuple(SMALL[i % 7] for i in range(16)), tuple(SMALL[i % 7] for i in range(17)),
                                   tuple(SMALL[i % 7] for i in range(33)), (1023,), (1024,), (1025,)],
                         ids=["16-tensors", "17-tensors", "33-tensors", "alone-1023", "alone-1024", "alone-1025"])
def test_adam_tables_and_chunks(dev, sizes):
    """16, 17 and 33 parameter tensors in one group - one, two and three chunks of the 16-entry table, the last chunks of one tensor
    each -, and tables of one tensor at the sizes where gridDim.x goes from 1 to 2: every tensor of every chunk is stepped within
    the bounds, and every chunk's device state advances alike."""
    hyper, worst = HYPER[0], oh.Worst()
    inputs = _grids(sizes, 600, hyper["betas"])
    case = oh.AdamCase(inputs, dev, step=7, **hyper)
    case.opt.step()
    torch.cuda.synchronize()
    _check_step(case, worst, f"{len(sizes)} tensors", hyper, 8, 1.0, inputs)
    chunks = case.device_state()
    assert len(chunks) == (len(sizes) + 15) // 16
    assert all(c == chunks[0] for c in chunks) and chunks[0][1] == 8 and chunks[0][4] == 0
    assert chunks[0][2] == 0.9 ** 7 * 0.9 and chunks[0][3] == 0.999 ** 7 * 0.999
    assert case.guards_intact()
    worst.report(f"adam_kernel, {len(sizes)} tensors")


def test_adam_two_param_groups_with_their_own_lr(dev):
    hyper, sizes, worst = HYPER[0], (257, 1025, 1, 65537, 256), oh.Worst()
    inputs = _grids(sizes, 700, hyper["betas"])
    case = oh.AdamCase(inputs, dev, step=3, groups=[([0, 1, 2], 1e-3), ([3, 4], 1e-5)], **hyper)
    case.opt.step()
    torch.cuda.synchronize()
    for idx, lr in (([0, 1, 2], 1e-3), ([3, 4], 1e-5)):
        sub = oh.AdamCase.__new__(oh.AdamCase)   # (a view of the group's tensors for _check_step)
        sub.params, sub.bufs = [case.params[i] for i in idx], [case.bufs[i] for i in idx]
        _check_step(sub, worst, f"lr {lr:g}", dict(hyper, lr=lr), 4, 1.0, [inputs[i] for i in idx])
    assert [s[0][:2] for s in (case.device_state(0), case.device_state(1))] == [(1e-3, 4), (1e-5, 4)]
    assert case.guards_intact()
    worst.report("adam_kernel, two param groups")


def test_adam_skips_nonfinite_elements_among_finite_ones(dev):
    """NaN, +inf and -inf gradients at the first indices, the last indices and in the second outer trip of tensors of 257, 65537 and
    81921 elements, and +-3e38 - finite, but not after grad_scale = 2: exactly those elements keep p, m and v bit for bit, every other
    element is stepped within its bound, `skipped_nonfinite()` rises by exactly the number placed, and the step count advances."""
    hyper, sizes, gs, worst = HYPER[0], (257, 65537, 81921), 2.0, oh.Worst()
    inputs = _grids(sizes, 800, hyper["betas"])
    bad = [np.nan, np.inf, -np.inf]
    placed = 0
    for j, (p, m, v, g) in enumerate(inputs):
        n = g.size
        where = [0, 1, 2, n - 1, n - 2, n - 3] + ([65536] if n == 65537 else []) + ([65536, 70000, 81000] if n == 81921 else [])
        for r, i in enumerate(dict.fromkeys(where)):
            g[i] = bad[(r + j) % 3]   # (another of the three at index 0 and n - 1 of every tensor)
        mid = [n // 2, n // 2 + 1]
        g[mid] = [3e38, -3e38]
        placed += len(set(where)) + 2
        assert np.count_nonzero(~oh.stepped(g, gs)) == len(set(where)) + 2 and np.all(oh.stepped(g[mid], 1.0))
    case = oh.AdamCase(inputs, dev, step=40, **hyper)
    case.opt.grad_scale = gs
    assert case.opt.skipped_nonfinite() == 0
    case.opt.step()
    torch.cuda.synchronize()
    _check_step(case, worst, "non-finite among finite", hyper, 41, gs, inputs)   # (bit-equality of the skipped elements included)
    assert case.opt.skipped_nonfinite() == placed
    assert case.device_state()[0][1] == 41 and all(int(case.opt.state[p]["step"]) == 41 for p in case.params)
    assert case.guards_intact()
    case.opt.step()   # the counter is cumulative
    torch.cuda.synchronize()
    assert case.opt.skipped_nonfinite() == 2 * placed
    worst.report("adam_kernel, non-finite elements among finite ones")


# ------------------------------------------------------------------------------------------
# gops_polyak_update
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.005, 0.5, 1.0])
def test_polyak_bits(dev, tau):
    """PolyakUpdater over 18 tensors (two chunks of the table) of the Polyak sizes: the targets are `polyak_ref32` bit for bit, the
    guard regions and the online tensors untouched."""
    rng = np.random.default_rng(7)
    sizes = [oh.POLYAK_SIZES[i % len(oh.POLYAK_SIZES)] for i in range(18)]
    host = [(rng.standard_normal(n).astype(np.float32) * np.float32(10.0 ** rng.uniform(-3, 3)), rng.standard_normal(n).astype(np.float32)) for n in sizes]
    target, online = [oh.guarded(t, dev) for t, _ in host], [oh.guarded(o, dev) for _, o in host]
    pk = hb.PolyakUpdater([t for t, _ in target], [o for o, _ in online])
    assert len(pk.tables) == 2
    pk.step(tau)
    torch.cuda.synchronize()
    for i, ((t, o), (tv, tb), (ov, ob)) in enumerate(zip(host, target, online)):
        want = torch.from_numpy(oh.polyak_ref32(t, o, tau))
        assert torch.equal(tv.cpu(), want), (i, sizes[i], int((tv.cpu() != want).sum()))
        assert oh.guard_intact(tb) and oh.guard_intact(ob) and oh.bits_equal(ov.cpu(), o)
    if tau == 1.0:
        assert all(torch.equal(tv, ov) for (tv, _), (ov, _) in zip(target, online))


# ------------------------------------------------------------------------------------------
# gops_value_loss / gops_mean_loss
# ------------------------------------------------------------------------------------------
def _stat_bound(want, terms):
    """4u relative to the float64 value: u for the final rounding to fp32, and for sum((a - b)^2) 2u for the fp32 difference and u
    for its fp32 square (non-negative terms: the relative errors carry over to the sum); the double sums add at most n 2^-53 of
    mean|term|, which a cancelling mean needs."""
    terms = np.asarray(terms, dtype=np.float64)
    return 4.0 * oh.U * abs(want) + terms.size * 2.0 ** -53 * float(np.mean(np.abs(terms)))


def _check_loss_call(st, a, b, dev, label, dirty):
    """One value_loss (with gradient) + the same again without + one mean_loss on the LossStats `st`; -> whether the partial sums
    behind the results have been written since the buffer was made."""
    n = a.size
    many = n > oh.LOSS_ONE_BLOCK_MAX
    av, ab = oh.guarded(a, dev)
    bv, bb = oh.guarded(b, dev)
    gv, gb = oh.guarded(np.full(n, 123.0, np.float32), dev)
    before = st.buf.clone()
    out = st.value_loss(av, bv, gv).clone()
    torch.cuda.synchronize()
    assert torch.equal(gv.cpu(), torch.from_numpy(oh.value_grad_ref32(a, b))), label
    assert oh.guard_intact(gb) and oh.guard_intact(ab) and oh.guard_intact(bb)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = (float(np.mean((a64 - b64) ** 2)), float(np.mean(a64)))
    got = out.cpu().double().numpy()
    bounds = (_stat_bound(want[0], (a64 - b64) ** 2), _stat_bound(want[1], a64))
    ratio = [abs(got[k] - want[k]) / bounds[k] if bounds[k] > 0 else float(got[k] != want[k]) for k in range(2)]
    print(f"{label}: n = {n} ({'64 blocks' if many else 'one block'}) error / bound: sum of squares {ratio[0]:.3f}, mean {ratio[1]:.3f}")
    assert max(ratio) <= 1.0, (label, got, want, bounds)

    def scratch_rule(prev):
        # the header: everything zero before the first call, the ticket left zero by every call.  One block touches neither the
        # partial sums nor the ticket; 64 blocks leave their partial sums behind
        buf = st.buf.cpu()
        assert float(buf[oh.LOSS_TICKET:].abs().max()) == 0.0, label
        if not many:
            assert oh.bits_equal(buf[2:], prev.cpu()[2:]), label
        if not (dirty or many):
            assert float(buf[2:].abs().max()) == 0.0, label
    scratch_rule(before)
    again = st.value_loss(av, bv, None).clone()
    assert oh.bits_equal(again.cpu(), out.cpu()), label
    assert torch.equal(gv.cpu(), torch.from_numpy(oh.value_grad_ref32(a, b)))   # (no gradient asked for: none written)
    mean = st.mean_loss(av, -1.0).clone().cpu().double().numpy()
    mb = _stat_bound(want[1], a64)
    assert abs(mean[0] + want[1]) <= mb and abs(mean[1] - want[1]) <= mb, (label, mean, want[1], mb)
    assert oh.bits_equal(st.mean_loss(av, -1.0).cpu(), mean.astype(np.float32))
    scratch_rule(before if not many else st.buf)
    return dirty or many


def test_loss_scalars_at_every_loop_edge(dev):
    """Every loss-scalar size, the one-block and the 64-block form taking turns on ONE LossStats buffer: the gradient is
    `value_grad_ref32` bit for bit, both scalars within 4u relative of float64, a repeated call returns the same bits, and the
    scratch behind the results is zero wherever the header says it is left zero."""
    st = hb.LossStats(dev)
    one = [n for n in oh.LOSS_SIZES if n <= oh.LOSS_ONE_BLOCK_MAX]
    many = [n for n in oh.LOSS_SIZES if n > oh.LOSS_ONE_BLOCK_MAX]
    order = [n for pair in zip(one, many) for n in pair]
    assert sorted(order) == sorted(oh.LOSS_SIZES) and len(one) == len(many)
    rng = np.random.default_rng(11)
    dirty = False
    for n in order:
        a = (rng.standard_normal(n) * 3 - 1).astype(np.float32)
        b = rng.standard_normal(n).astype(np.float32)
        dirty = _check_loss_call(st, a, b, dev, "N(-1, 9) against N(0, 1)", dirty)


@pytest.mark.parametrize("n", [8192, 262145])
def test_loss_scalars_need_the_double_accumulation(dev, n):
    """Inputs a float accumulator misses the 4u bound on.  v, target = 1e4 + N(0, 1) (the mean of v is 1e4: the float64 mean is the
    reference; a float sum of 262145 such values has 2^-6 granularity at the end).  And a thread's own sum: v = 4096 at the first
    index every thread reads, 1 at its other 15 (64 blocks, n = 262145) or 31 (one block, n = 8192), target 0: the squares are
    2^24, 1, 1, ... - in float 2^24 + 1 = 2^24 every time, the sum of squares comes out (n - first) / (first 2^24) = 15u or 31u short."""
    rng = np.random.default_rng(13)
    st = hb.LossStats(dev)
    a = (1e4 + rng.standard_normal(n)).astype(np.float32)
    b = (1e4 + rng.standard_normal(n)).astype(np.float32)
    dirty = _check_loss_call(st, a, b, dev, "1e4 + N(0, 1)", False)
    first = 256 * (64 if n > oh.LOSS_ONE_BLOCK_MAX else 1)
    a = np.ones(n, np.float32)
    a[:first] = 4096.0
    _check_loss_call(st, a, np.zeros(n, np.float32), dev, "4096 then ones", dirty)


# ------------------------------------------------------------------------------------------
# the fused tails
# ------------------------------------------------------------------------------------------
def _make_alg(cfg, dev, seed, **more):
    from bench import alg_kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.utils.synthetic import make_batch
    torch.manual_seed(seed)
    alg = create_alg(**dict(alg_kwargs(cfg, seed), precision_check_interval=0, **more))
    if cfg["alg"] != "FHADP":
        alg.forward_step, alg.gamma = cfg["horizon"], cfg["gamma"]
    alg.networks.to(dev)
    return alg, {k: v.to(dev) for k, v in make_batch(cfg, seed).items()}


def _spy_fused(monkeypatch, opt):
    """Counts the fused steps `opt` hands out (`begin_fused` returning a table, then `end_fused`)."""
    calls = []
    begin, end = opt.begin_fused, opt.end_fused
    monkeypatch.setattr(opt, "begin_fused", lambda: (lambda fa: (calls.append("begin") if fa is not None else None, fa)[1])(begin()))
    monkeypatch.setattr(opt, "end_fused", lambda: (calls.append("end"), end())[1])
    return calls


def test_fused_tail_against_float64(dev, monkeypatch):
    """One `gops_rollout_backward_update` at the 64-wide FHADP shape of test_fused_update_tail_equals_separate_calls: the gradient the
    call leaves in .grad, fed with the pre-update p, m, v to `adam_ref64`, bounds the fused result - the fused restatement
    (common.h adam_element) tied to float64 directly, not through the stand-alone kernel."""
    monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
    cfg = dict(alg="FHADP", env_id="pyth_idpendulum", batch=96, horizon=8, hidden=(64, 64), act="gelu", gamma=0.99)
    alg, data = _make_alg(cfg, dev, 7)
    opt = alg.networks.policy_optimizer
    alg.local_update(data, 0)   # (allocates gradients and moments; step 1)
    calls = _spy_fused(monkeypatch, opt)
    params = list(alg.networks.policy.parameters())
    before = [(p.detach().cpu().numpy().copy(), opt.state[p]["exp_avg"].cpu().numpy().copy(), opt.state[p]["exp_avg_sq"].cpu().numpy().copy()) for p in params]
    assert all(int(opt.state[p]["step"]) == 1 for p in params)
    alg.local_update(data, 1)
    torch.cuda.synchronize()
    assert calls == ["begin", "end"]
    group, worst = opt.param_groups[0], oh.Worst()
    hyper = dict(lr=group["lr"], betas=group["betas"], eps=group["eps"])
    for (name, par), (p, m, v) in zip(alg.networks.policy.named_parameters(), before):
        g = par.grad.detach().cpu().numpy()
        assert np.all(np.isfinite(g)) and np.abs(g).max() > 0
        ref = oh.adam_ref64(p, m, v, g, t=2, grad_scale=1.0, **hyper)
        bounds = oh.adam_bounds(m, v, g, ref, lr=hyper["lr"], betas=hyper["betas"], t=2, grad_scale=1.0)
        got = (par.detach().cpu().numpy(), opt.state[par]["exp_avg"].cpu().numpy(), opt.state[par]["exp_avg_sq"].cpu().numpy())
        worst.check(f"fused tail {name}", got, ref, bounds)
        assert not oh.bits_equal(got[0], p)
    assert opt.skipped_nonfinite() == 0 and int(opt._dev[0]["state"][0][1].item()) == 2
    worst.report("fused tail (reduce_partials_kernel), FHADP 64-wide")


def _overflowing_infadp(dev):
    """The INFADP counterpart of test_trained256_gpu.py's overflow case: 256-wide ReLU nets on pyth_lq after one healthy PEV and one
    healthy PIM update (targets and online nets then differ, the moments are non-zero), then the policy's first layer blown up so
    that H_1 ~ 1e8 leaves the half range of the plane-split kernels: their answer is NaN."""
    cfg = dict(alg="INFADP", env_id="pyth_lq", lq_config="s4a2", batch=64, horizon=3, hidden=(256, 256), act="relu", gamma=0.99)
    alg, data = _make_alg(cfg, dev, 21)
    for it in range(2):
        alg.local_update(data, it)
    torch.cuda.synchronize()
    nets = alg.networks
    assert any(not torch.equal(a, b) for a, b in zip(nets.policy.parameters(), nets.policy_target.parameters()))
    assert any(not torch.equal(a, b) for a, b in zip(nets.v.parameters(), nets.v_target.parameters()))
    with torch.no_grad():
        l0, l1 = nets.policy.linear_layers()[:2]
        l0.weight.mul_(2.0e8)
        l0.bias.mul_(2.0e8)
        l1.weight.mul_(1.0e-8)
    return alg, data


def _snapshot(alg, net):
    nets = alg.networks
    opt = nets.optimizer_dict[net]
    ps = list(nets.net_dict[net].parameters())
    return ([p.detach().clone() for p in ps], [p.detach().clone() for p in nets.target_net_dict[net].parameters()],
            [opt.state[p]["exp_avg"].clone() for p in ps], [opt.state[p]["exp_avg_sq"].clone() for p in ps])


def _assert_untouched(alg, net, snap):
    for before, now in zip(snap, _snapshot(alg, net)):
        for i, (a, b) in enumerate(zip(before, now)):
            assert oh.bits_equal(a, b), (net, i)


def test_skipped_fused_step_leaves_the_polyak_target_untouched(dev, monkeypatch):
    """common.h: a gradient element that is not finite takes no optimizer step, and in the fused tail the Polyak target of that element
    stays as it is.  A fused PIM update (`gops_rollout_backward_update`) whose gradients leave as NaN: policy_target, policy, both
    moments bit-identical, every element counted, the step count still advanced."""
    monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
    alg, data = _overflowing_infadp(dev)
    opt = alg.networks.policy_optimizer
    calls = _spy_fused(monkeypatch, opt)
    snap = _snapshot(alg, "policy")
    assert opt.skipped_nonfinite() == 0
    alg.local_update(data, 1)   # PIM
    torch.cuda.synchronize()
    assert calls == ["begin", "end"]
    n_params = sum(p.numel() for p in snap[0])
    assert all(torch.isnan(p.grad).all() for p in alg.networks.policy.parameters())
    assert opt.skipped_nonfinite() == n_params
    _assert_untouched(alg, "policy", snap)
    assert int(opt._dev[0]["state"][0][1].item()) == 2 and all(int(opt.state[p]["step"]) == 2 for p in alg.networks.policy.parameters())


def test_skipped_fused_value_step_leaves_v_target_untouched(dev, monkeypatch):
    """The same through `gops_value_backward_update` (PEV): the blown-up policy makes the rollout's backup NaN, so every element of
    the value net's gradient is NaN - v, v_target and the moments stay bit-identical."""
    monkeypatch.setenv("GOPS_HIP_GRAPH", "0")
    alg, data = _overflowing_infadp(dev)
    opt = alg.networks.v_optimizer
    calls = _spy_fused(monkeypatch, opt)
    snap = _snapshot(alg, "v")
    alg.local_update(data, 0)   # PEV
    torch.cuda.synchronize()
    assert calls == ["begin", "end"]
    assert all(torch.isnan(p.grad).all() for p in alg.networks.v.parameters())
    assert opt.skipped_nonfinite() == sum(p.numel() for p in snap[0])
    _assert_untouched(alg, "v", snap)
