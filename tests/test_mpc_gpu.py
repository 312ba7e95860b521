"""Batched shooting MPC on the device: gops_mpc_step against its float64 restatement (mpc_helpers) step by step, every status
word, and BatchOptController against the reference's recorded optima (golden/mpc_batch.npz)."""
import json
import os

import numpy as np
import pytest
import torch

import mpc_helpers as mh
from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_batch.npz")
SENTINEL, PAD = -7.25, 64
EPS32 = float(np.finfo(np.float32).eps)
VEC, EXACT = ("x", "g", "x_prev", "g_prev", "d", "x_trial", "s", "y"), ("status", "iterations", "evaluations", "ls_count", "head", "count")
DBL = ("f", "f_prev", "alpha", "dphi", "gamma", "rho")


def _padded(solver):
    """Re-seat every output of `solver` in front of PAD sentinel elements; returns the padded buffers."""
    bufs = {}
    for name in ("x_trial", "x", "f_best", "status", "iterations"):
        t = getattr(solver, name)
        sent = SENTINEL if t.dtype == torch.float32 else -77
        buf = torch.full((t.numel() + PAD,), sent, dtype=t.dtype, device=t.device)
        setattr(solver, name, buf[:t.numel()].view(t.shape))
        bufs[name] = (buf, t.numel(), sent)
    return bufs


def _assert_padding(bufs):
    for name, (buf, n, sent) in bufs.items():
        assert bool((buf[n:] == sent).all()), f"{name}: wrote behind its end"


def _problems(B, n, first_seed=1000):
    return [mh.Quadratic(n, first_seed + 13 * n + r) for r in range(B)]


def _x0(B, n, first_row=0):
    return np.stack([np.random.RandomState(5000 + first_row + r).uniform(-1.5, 1.5, n) for r in range(B)]).astype(np.float32)


def _feed(solver, fun):
    """Cost and gradient in float64 on the host at the solver's trial point, handed over as fp32."""
    f, g = fun(solver.x_trial.cpu().numpy().astype(np.float64))
    solver.f.copy_(torch.from_numpy(f.astype(np.float32)))
    solver.g.copy_(torch.from_numpy(g.astype(np.float32)))
    return solver.f.cpu().numpy(), solver.g.cpu().numpy()


def _hyper_of(solver):
    h = solver.hyper.cpu().numpy().astype(np.float64)   # what the kernel reads: the fp32 values
    return dict(zip(("c1", "shrink", "max_ls", "pgtol", "ftol", "curv_eps"), h))


def _run(B, n, m, steps, problems, x0, compare=True):
    """`steps` calls of the kernel; before each, the restatement takes the kernel's own block and says what the call must leave.
    Returns (the raw block after every step, the largest error per section in units of the bound)."""
    dev = torch.device("cuda", 0)
    solver = hb.MpcSolver(B, n, -1.0, 1.0, dev, history=m)
    bufs = _padded(solver)
    solver.init(torch.from_numpy(x0).to(dev))
    fun, hyper = mh.batch_fun(problems), _hyper_of(solver)
    raws, worst = [], {}
    for _ in range(steps):
        f32, g32 = _feed(solver, fun)
        want = solver.state() if compare else None
        if compare:
            want_out = mh.step(want, f32, g32, hyper, store=np.float32)
        solver.step()
        raws.append(solver._state.cpu().numpy().tobytes())
        if not compare:
            continue
        got, got_out = solver.state(), solver.x_trial.cpu().numpy()
        for k in EXACT:
            assert (got[k] == want[k]).all(), (k, got[k], want[k])
        # every element is one rounding of a double expression of fp32 inputs, formed without fused multiply-adds on both sides;
        # the two sides differ only in the order of the sums that feed it: 4 fp32 ulp of the tensor's own largest magnitude, the
        # floor of the project's rule (the fp32 composition that could widen it is not consulted: no wider bound is taken)
        for k, a, b in [(k, got[k], want[k]) for k in VEC] + [("x_trial argument", got_out, want_out)]:
            bound = 4 * EPS32 * float(np.abs(b).max())
            err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
            worst[k] = max(worst.get(k, 0.0), err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, (k, err, bound)
        for k in DBL:   # doubles: sums of up to 256 products in another order
            err = np.abs(got[k] - want[k])
            assert (err <= 1e-12 * np.maximum(np.abs(want[k]), 1.0) + 1e-9 * np.abs(want[k])).all(), (k, err.max())
    x, f, status, iterations = (t.cpu().numpy() for t in solver.finish())   # (into the padded buffers)
    last = solver.state()
    assert np.array_equal(x, last["x"]) and np.array_equal(f, last["f"].astype(np.float32))
    assert np.array_equal(status, last["status"]) and np.array_equal(iterations, last["iterations"])
    _assert_padding(bufs)
    return raws, worst, solver


@pytest.mark.parametrize("m", [1, 8])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 128])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_step_against_restatement(B, n, m):
    """12 steps; after each one x_trial, the status words, the counters and the ring against the restatement started from the same
    block; a second run from the same inputs leaves the same bits after every step."""
    problems = _problems(B, n)
    raws, worst, _ = _run(B, n, m, 12, problems, _x0(B, n))
    print(f"B {B} n {n} m {m}: largest error / bound per section:", {k: round(v, 3) for k, v in worst.items()})
    raws2, _, _ = _run(B, n, m, 12, problems, _x0(B, n), compare=False)
    assert raws == raws2


@pytest.mark.parametrize("m", [1, 8])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 128])
def test_row_bits_do_not_depend_on_batch_or_row(n, m):
    """The problem that is row 37 of B = 70, solved alone at B = 1: the same bits in every section after every one of 12 steps."""
    problems, x0 = _problems(70, n), _x0(70, n)
    whole, _, _ = _run(70, n, m, 12, problems, x0, compare=False)
    alone, _, _ = _run(1, n, m, 12, problems[37:38], x0[37:38], compare=False)
    for k, (a, b) in enumerate(zip(whole, alone)):
        sa, sb = hb.mpc_decode_state(a, 70, n, m), hb.mpc_decode_state(b, 1, n, m)
        for name in DBL + EXACT + VEC:
            assert np.ascontiguousarray(sa[name][37]).tobytes() == np.ascontiguousarray(sb[name][0]).tobytes(), (k, name)


def test_relaunch_from_copied_block_is_bit_identical():
    B, n, m = 70, 65, 8
    problems = _problems(B, n)
    _, _, solver = _run(B, n, m, 5, problems, _x0(B, n), compare=False)
    _feed(solver, mh.batch_fun(problems))
    saved, saved_trial = solver._state.clone(), solver.x_trial.clone()
    solver.step()
    after, trial = solver._state.clone(), solver.x_trial.clone()
    solver._state.copy_(saved), solver.x_trial.copy_(saved_trial)
    solver.step()
    assert torch.equal(solver._state.view(torch.int64), after.view(torch.int64)) and torch.equal(solver.x_trial, trial)


def _solve(problems, x0, m=8, max_steps=400, shifted=False, **hyper):
    B, n = x0.shape
    solver = hb.MpcSolver(B, n, -1.0, 1.0, torch.device("cuda", 0), history=m)
    solver.set_hyper(**hyper)
    solver.init(torch.from_numpy(x0.astype(np.float32)).cuda())
    fun = mh.batch_fun(problems, shifted)
    for _ in range(max_steps):
        _feed(solver, fun)
        solver.step()
        if (solver.state()["status"] != hb.MPC_RUNNING).all():
            break
    return solver


def test_status_converged_inside_and_on_every_bound():
    inner, corner = mh.Quadratic(6, 7, n_active=0), mh.Quadratic(6, 8, n_active=6)
    # (the cost handed over is f - f_opt: fp32 resolves its decrease down to the optimum; ftol < 0 never stops a row)
    solver = _solve([inner, corner], np.zeros((2, 6)), shifted=True, ftol=-1.0)
    x, f, status, iterations = (t.cpu().numpy() for t in solver.finish())
    assert list(status) == [hb.MPC_CONVERGED_PG] * 2 and (np.abs(x[0]) < 1).all() and (np.abs(x[1]) == 1).all()
    np.testing.assert_allclose(x[0], inner.x_opt, atol=1e-4)
    assert (x[1] == corner.x_opt).all() and (iterations > 0).all()
    # a problem that is not running is left unchanged by further steps, whatever they are fed; its x_trial row is its x
    before = solver._state.clone()
    solver.f.fill_(float("nan")), solver.g.fill_(3.0), solver.x_trial.fill_(9.0)
    solver.step()
    assert torch.equal(solver._state.view(torch.int64), before.view(torch.int64)) and torch.equal(solver.x_trial.cpu(), torch.from_numpy(x))


def test_status_nonfinite_on_its_row_alone():
    B, n = 5, 7
    problems = _problems(B, n)
    x0 = _x0(B, n)
    clean = _solve(problems, x0, max_steps=3)
    solver = hb.MpcSolver(B, n, -1.0, 1.0, torch.device("cuda", 0))
    solver.init(torch.from_numpy(x0).cuda())
    fun = mh.batch_fun(problems)
    for k in range(3):
        _feed(solver, fun)
        if k == 1:
            solver.g[2, 4] = float("nan")
        solver.step()
    got, want = solver.state(), clean.state()
    assert list(got["status"]) == [0, 0, hb.MPC_NONFINITE, 0, 0] and got["evaluations"][2] == 2
    keep = np.array([0, 1, 3, 4])
    for k in DBL + EXACT + VEC:
        assert np.array_equal(got[k][keep], want[k][keep], equal_nan=True), k


def test_status_line_search_exhausted_at_the_count_limit():
    solver = hb.MpcSolver(1, 3, -1.0, 1.0, torch.device("cuda", 0), history=4)
    solver.set_hyper(max_ls=6)
    solver.init(torch.zeros(1, 3, device="cuda"))
    solver.g.fill_(1.0)
    calls = 0
    while solver.state()["status"][0] == hb.MPC_RUNNING and calls < 50:
        solver.f.fill_(float(calls > 0))   # the cost at every trial point lies above the accepted one
        solver.step()
        calls += 1
    st = solver.state()
    assert st["status"][0] == hb.MPC_LINE_SEARCH and st["ls_count"][0] == 6 and calls == 1 + 6 and st["evaluations"][0] == 7
    assert (st["x"][0] == 0).all() and np.isclose(st["alpha"][0], 0.5 ** 5 / np.sqrt(3.0), rtol=1e-14)   # five shrinks of min(1, 1 / |d|)


# ---- BatchOptController against the reference's record ---------------------------------------------------------------------------
def _cases():
    with np.load(GOLDEN) as z:
        meta = json.loads(str(z["meta"]))
        return [(c, {k: z[f"{c['name']}/{k}"] for k in ("x0", "plan", "cost", "status")}) for c in meta["cases"]]


def _model(c):
    from gops_amd.create_pkg.create_env_model import create_env_model
    return create_env_model(**{k: c[k] for k in ("env_id", "lq_config") if k in c}, use_gpu=True)


def _oracle_cost(c, x0, plan):
    """The cost of `plan` [B, control points, A] from x0 in float64: oracle/adp_oracle.py's open-loop rollout of the raw model
    (raw_shooting_cost) on double tensors."""
    from oracle import adp_oracle as orc
    env = orc.make_env(c["env_id"], lq_config=c.get("lq_config", "s4a2"))
    if env["kind"] == "lq":
        env = dict(env, lq={k: (v.double() if torch.is_tensor(v) else v) for k, v in env["lq"].items()})
    acts = torch.as_tensor(np.asarray(plan), dtype=torch.float64).repeat_interleave(c["ci"], dim=1)
    cost, _, _ = orc.raw_shooting_cost(env, torch.as_tensor(x0, dtype=torch.float64), {}, acts, 1.0)
    return cost.numpy()


@pytest.fixture(scope="module")
def record():
    """Per case: the record, its cost under the float64 oracle, and the excess and first-action deviation of the existing
    OptController (scipy on the same kernels) - the yardstick the batched solver gets twice of."""
    from gops_amd.sys_simulator import OptController
    out = []
    for c, rec in _cases():
        model = _model(c)
        ref_cost = _oracle_cost(c, rec["x0"], rec["plan"])
        plans = []
        for b in range(c["B"]):
            ctrl = OptController(model, num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0, mode="shooting")
            ctrl(rec["x0"][b])
            plans.append(ctrl.last_result.x.reshape(rec["plan"].shape[1:]))
        plans = np.stack(plans)
        out.append(dict(case=c, rec=rec, model=model, ref_cost=ref_cost, opt_excess=_oracle_cost(c, rec["x0"], plans) - ref_cost,
                        opt_action=np.abs(plans[:, 0] - rec["plan"][:, 0]).max(1)))
    return out


def test_controller_against_reference_record(record):
    """Every row of every case: the cost of the device plan, evaluated by the float64 oracle (oracle/adp_oracle.py:
    raw_shooting_cost on double tensors - not the kernel's own v_pi), exceeds the reference's recorded optimum by at most twice what
    the existing OptController exceeds it by on the same case (its largest row), and not less than 4 fp32 ulp of the cost: both
    solvers see the cost in fp32 and cannot tell plans apart below that.  pyth_lq (strictly convex): the first action against the
    record, with the margin formed the same way from OptController's deviation (floor: 4 fp32 ulp of the action bound)."""
    from gops_amd.sys_simulator import BatchOptController
    for r in record:
        c, rec = r["case"], r["rec"]
        ctrl = BatchOptController(r["model"], num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0)
        res = ctrl.solve(rec["x0"])
        plan = res["plan"].cpu().numpy()
        excess = _oracle_cost(c, rec["x0"], plan) - r["ref_cost"]
        floor = 4 * EPS32 * np.maximum(np.abs(r["ref_cost"]), 1.0)
        allow = np.maximum(2 * r["opt_excess"].max(), floor)
        status = np.bincount(res["status"].cpu().numpy(), minlength=5)
        print(f"{c['name']}: excess batched max {excess.max():.3e} (OptController max {r['opt_excess'].max():.3e}, allowed {allow.max():.3e}); "
              f"iterations {res['iterations'].cpu().numpy().tolist()}; status counts {status.tolist()}; evaluations {res['evaluations']}")
        assert (excess <= allow).all(), (c["name"], excess, allow)
        if c["env_id"] == "pyth_lq":
            dev = np.abs(plan[:, 0] - rec["plan"][:, 0]).max(1)
            hi = float(r["model"].unwrapped.action_upper_bound.abs().max())
            allow_a = max(2 * r["opt_action"].max(), 4 * EPS32 * hi)
            print(f"{c['name']}: first action deviation batched max {dev.max():.3e} (OptController max {r['opt_action'].max():.3e})")
            assert (dev <= allow_a).all(), (c["name"], dev, allow_a)


def test_controller_batch_independence(record):
    from gops_amd.sys_simulator import BatchOptController
    r = next(r for r in record if r["case"]["name"] == "lqs4a2_T10_ci2")
    c, x0 = r["case"], r["rec"]["x0"]
    mk = lambda: BatchOptController(r["model"], num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0)
    whole, alone = mk().solve(x0), mk().solve(x0[3:4])
    assert torch.equal(whole["plan"][3], alone["plan"][0]) and whole["iterations"][3] == alone["iterations"][0]


def test_controller_warm_start(record):
    """A second call on the states advanced by one step of the first plan's action, warm-started by the shifted plan, needs no more
    iterations in total than a cold solve of those states."""
    from gops_amd.sys_simulator import BatchOptController
    from oracle import adp_oracle as orc
    r = next(r for r in record if r["case"]["name"] == "lqs4a2_T10_ci1")
    c, x0 = r["case"], r["rec"]["x0"]
    ctrl = BatchOptController(r["model"], num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0)
    first = ctrl.solve(x0)
    env = orc.make_env(c["env_id"], lq_config=c["lq_config"])
    x1, _, _ = orc.lq_step(env["lq"], torch.from_numpy(x0), first["action"].cpu())
    warm = ctrl.solve(x1.numpy())["iterations"].sum().item()
    ctrl.reset()
    cold = ctrl.solve(x1.numpy())["iterations"].sum().item()
    print(f"warm start: {warm} iterations in total, cold {cold}")
    assert warm <= cold


def test_controller_with_terminal_cost(record):
    """`use_terminal_cost=True` (pyth_lq's x'Px, through backward_open_loop_adj).  The optimum of the total cost (stage costs +
    terminal cost) comes from the float64 solver of mpc_helpers on the float64 oracle; the existing OptController's largest excess
    over it is measured, and the batched solver is allowed twice that, and not less than 4 fp32 ulp of the cost (both see the cost
    in fp32) - the rule of test_controller_against_reference_record."""
    from gops_amd.sys_simulator import BatchOptController, OptController
    from oracle import adp_oracle as orc
    r = next(r for r in record if r["case"]["name"] == "lqs4a2_T6_ci2")
    c, x0, model = r["case"], r["rec"]["x0"], r["model"]
    B, n_cp, ci = c["B"], c["T"] // c["ci"], c["ci"]
    P = torch.as_tensor(model.unwrapped.dynamics.P, dtype=torch.float64)
    env = orc.make_env(c["env_id"], lq_config=c["lq_config"])
    env = dict(env, lq={k: (v.double() if torch.is_tensor(v) else v) for k, v in env["lq"].items()})

    def fun(x):   # total cost and its gradient with respect to the control points, float64
        acts = torch.as_tensor(x, dtype=torch.float64).reshape(B, n_cp, -1).repeat_interleave(ci, dim=1)
        cost, _, jac = orc.raw_shooting_cost(env, torch.as_tensor(x0, dtype=torch.float64), {}, acts, 1.0, terminal=lambda xT: xT @ P @ xT)
        return cost.numpy(), jac.reshape(B, n_cp, ci, -1).sum(2).reshape(B, -1).numpy()

    total = lambda plan: fun(np.asarray(plan, dtype=np.float64).reshape(B, -1))[0]
    base = model.unwrapped
    lo, hi = (np.tile(v.cpu().numpy().astype(np.float64), n_cp) for v in (base.action_lower_bound, base.action_upper_bound))
    best = mh.solve(fun, np.zeros((B, lo.size)), lo, hi)
    assert (best["status"] != mh.RUNNING).all()
    plans = []
    for b in range(B):
        ctrl = OptController(model, num_pred_step=c["T"], ctrl_interval=ci, gamma=1.0, mode="shooting", use_terminal_cost=True)
        ctrl(x0[b])
        plans.append(ctrl.last_result.x)
    opt_excess = total(np.stack(plans)) - best["f"]
    batched = BatchOptController(model, num_pred_step=c["T"], ctrl_interval=ci, gamma=1.0, use_terminal_cost=True)
    excess = total(batched.solve(x0)["plan"].cpu().numpy()) - best["f"]
    plain = total(BatchOptController(model, num_pred_step=c["T"], ctrl_interval=ci, gamma=1.0).solve(x0)["plan"].cpu().numpy()) - best["f"]
    allow = np.maximum(2 * opt_excess.max(), 4 * EPS32 * np.maximum(np.abs(best["f"]), 1.0))
    print(f"terminal cost: excess batched max {excess.max():.3e} (OptController max {opt_excess.max():.3e}, allowed {allow.max():.3e}); "
          f"plans found without the terminal cost exceed by up to {plain.max():.3e}; vmap used: {batched._terminal_vmap}")
    assert (excess <= allow).all(), (excess, allow)
    assert batched._terminal_vmap and plain.max() > allow.max()   # the terminal cost did change the plans
