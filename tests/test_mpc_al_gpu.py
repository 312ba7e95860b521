"""Path constraints of the batched MPC on the device: gops_mpc_al_eval / _update / _advance against their float64 restatements
(mpc_al_helpers), the whole augmented-Lagrangian loop on a problem with a closed-form KKT point, and BatchOptController with
path_constraints="augmented_lagrangian" against OptController's SLSQP on the constrained vehicle models."""
import numpy as np
import pytest
import torch

import mpc_al_helpers as ah
import mpc_helpers as mh
from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -7.25, 64
EPS32 = float(np.finfo(np.float32).eps)
H = 3


def _dev():
    return torch.device("cuda", 0)


def _padded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), SENTINEL if dtype == torch.float32 else -77, dtype=dtype, device=_dev())
    return buf[:n].view(shape), buf, n


def _inputs(B, nc, seed=0):
    """c [H, B, n_c], lambda [B, H, n_c], rho [B], f [B]: lambda + rho c on both sides of zero; row 0 term 0 exactly zero
    (1 + 2 (-0.5)); row 1 all inactive with zero multipliers; row 2 holds a NaN; row 3 (B > 3) a constraint at -inf."""
    rng = np.random.RandomState(100 * B + 10 * nc + seed)
    c = rng.uniform(-1.0, 1.0, (H, B, nc)).astype(np.float32)
    lam = (rng.uniform(0.0, 2.0, (B, H, nc)) * (rng.uniform(size=(B, H, nc)) < 0.7)).astype(np.float32)
    rho = rng.choice([0.5, 2.0, 10.0, 1000.0], B).astype(np.float32)
    f = rng.uniform(-3.0, 3.0, B).astype(np.float32)
    c[0, 0, 0], lam[0, 0, 0], rho[0] = -0.5, 1.0, 2.0
    c[:, 1], lam[1] = -np.abs(c[:, 1]) - 0.1, 0.0
    c[1, 2, nc - 1] = np.nan
    c[2, 3, 0] = -np.inf
    return c, lam, rho, f


def _ulp_apart(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("nc", [1, 2, 3])
@pytest.mark.parametrize("B", [5, 17])
def test_al_eval_against_the_restatement(B, nc):
    c, lam, rho, f = _inputs(B, nc)
    want_f, want_seed, want_viol = ah.al_eval(c, lam, rho, f)
    solver = hb.MpcSolver(B, 4, -1.0, 1.0, _dev(), constraints=(H, nc))
    (solver.f, fbuf, nf), (solver.seed, sbuf, ns), (solver.viol, vbuf, nv) = _padded((B,)), _padded((H, B, nc)), _padded((B,))
    solver.lam.copy_(torch.from_numpy(lam)), solver.rho.copy_(torch.from_numpy(rho)), solver.f_al_in.copy_(torch.from_numpy(f))
    solver.al_eval(torch.from_numpy(c).to(_dev()))
    got_f, got_seed, got_viol = solver.f.cpu().numpy(), solver.seed.cpu().numpy(), solver.viol.cpu().numpy()
    print("f_al", got_f, want_f, "viol", got_viol)
    assert np.isnan(want_f[2]) and np.isnan(want_f[3]) and np.isfinite(np.delete(want_f, [2, 3])).all() and want_viol[1] == 0
    assert want_seed[0, 0, 0] == 0 and (want_seed[:, 1] == 0).all() and (want_seed > 0).any()
    # f_al: the fp32 rounding of the float64 value (the restatement adds in the kernel's order, so the double is the same one)
    assert np.array_equal(got_f, want_f, equal_nan=True), (got_f, want_f)
    nan = np.isnan(want_seed)
    assert np.array_equal(np.isnan(got_seed), nan) and nan.sum() == 1
    assert (_ulp_apart(got_seed[~nan], want_seed[~nan]) <= 1).all()
    assert np.array_equal(got_viol, want_viol)
    assert bool((fbuf[nf:] == SENTINEL).all()) and bool((sbuf[ns:] == SENTINEL).all()) and bool((vbuf[nv:] == SENTINEL).all())


def _armed_solver(B, n, nc, statuses):
    """A solver six steps into its quadratics (pairs in the ring), its status words then set row by row to `statuses` (cycled)."""
    dev = _dev()
    solver = hb.MpcSolver(B, n, -1.0, 1.0, dev, history=4, constraints=(H, nc))
    fun = mh.batch_fun([mh.Quadratic(n, 300 + r) for r in range(B)])
    solver.init(torch.from_numpy(np.stack([np.random.RandomState(r).uniform(-1, 1, n) for r in range(B)]).astype(np.float32)).to(dev))
    for _ in range(6):
        f, g = fun(solver.x_trial.cpu().numpy().astype(np.float64))
        solver.f.copy_(torch.from_numpy(f.astype(np.float32))), solver.g.copy_(torch.from_numpy(g.astype(np.float32)))
        solver.step()
    words = torch.tensor([statuses[r % len(statuses)] for r in range(B)], dtype=torch.int32, device=dev)
    solver.status_words().copy_(words)
    return solver


ALL_STATUSES = [hb.MPC_RUNNING, hb.MPC_CONVERGED_PG, hb.MPC_LINE_SEARCH, hb.MPC_NONFINITE, hb.MPC_FROZEN, hb.MPC_CONVERGED_F]


def _al_arrays(solver):
    return dict(lam=solver.lam.cpu().numpy(), rho=solver.rho.cpu().numpy(), viol=solver.viol.cpu().numpy(),
                viol_prev=solver.viol_prev.cpu().numpy(), outer=solver.outer.cpu().numpy())


@pytest.mark.parametrize("nc", [1, 2, 3])
@pytest.mark.parametrize("B", [5, 17])
def test_al_update_against_the_restatement(B, nc):
    """Rows in every inner status; two updates with max_outer = 2 and rho_max = 25: the first re-arms or ends the rows whose inner
    solve has ended (rho 10 -> 25, capped, where the violation did not shrink), the second - the re-armed rows set to converged again -
    leaves by the max_outer exit.  After each: multipliers, rho, viol_prev, the outer words and the whole solver block."""
    n = 5
    solver = _armed_solver(B, n, nc, ALL_STATUSES)
    solver.set_al_hyper(rho_max=25.0, max_outer=2)
    hyper = dict(ah.hyper32(), rho_max=25.0, max_outer=2)
    rng = np.random.RandomState(B + nc)
    c = rng.uniform(-0.3, 0.5, (H, B, nc)).astype(np.float32)
    c[:, 1] = -0.2   # row 1: feasible, zero multipliers: converged at its first update
    c[0, 2, 0] = 0.4   # row 2 (line search): violated
    lam0 = rng.uniform(0.0, 1.0, (B, H, nc)).astype(np.float32)
    lam0[1] = 0.0
    solver.lam.copy_(torch.from_numpy(lam0))
    viol = np.maximum(0.0, c.max((0, 2))).astype(np.float32)
    solver.viol.copy_(torch.from_numpy(viol))
    solver.viol_prev.copy_(torch.from_numpy(np.where(np.arange(B) % 2 == 1, np.inf, 0.0).astype(np.float32)))   # even rows: viol did not shrink
    cd = torch.from_numpy(c).to(_dev())
    for round_ in range(2):
        st, al = solver.state(), _al_arrays(solver)
        before = {k: v.copy() for k, v in st.items()}
        touched = ah.al_update(st, c, al["lam"], al["rho"], al["viol"], al["viol_prev"], al["outer"], hyper)
        solver.al_update(cd)
        got, got_al = solver.state(), _al_arrays(solver)
        for k in ("lam", "rho", "viol_prev", "outer"):
            assert np.array_equal(got_al[k], al[k]), (round_, k, got_al[k], al[k])
        for k in st:
            assert np.array_equal(got[k], st[k], equal_nan=True), (round_, k)
        assert np.array_equal(got["x"], before["x"]) and np.array_equal(got["iterations"], before["iterations"])
        want_touched = [r for r in range(B) if before["status"][r] in (1, 2, 3) and (round_ == 0 or r != 1)]
        assert touched == want_touched, (touched, want_touched)
        untouched = np.setdiff1d(np.arange(B), touched)
        assert np.array_equal(got_al["lam"][untouched], (lam0 if round_ == 0 else lam1)[untouched])
        if round_ == 0:
            rearmed = [r for r in touched if r != 1]
            assert (got["status"][rearmed] == hb.MPC_RUNNING).all() and (got["count"][rearmed] == 0).all() and (before["count"][rearmed] > 0).any()
            assert (got["evaluations"][rearmed] == 0).all() and (got_al["outer"][rearmed, 2] == before["evaluations"][rearmed]).all() and (before["evaluations"][rearmed] > 0).all() and (got_al["outer"][rearmed, 0] == 0).all()
            assert got_al["outer"][1, 0] == hb.MPC_AL_CONVERGED and got["status"][1] == hb.MPC_CONVERGED_PG
            grown = [r for r in rearmed if r % 2 == 0 and viol[r] > 0]
            assert len(grown) > 0 and (got_al["rho"][grown] == 25.0).all() and (got_al["rho"][[r for r in rearmed if r % 2 == 1]] == 10.0).all()
            lam1 = got_al["lam"].copy()
            solver.status_words()[torch.tensor(rearmed, device=_dev())] = hb.MPC_CONVERGED_F
        else:
            violated = [r for r in touched if viol[r] > 0]   # (a feasible row whose multipliers the first update took to 0 converges)
            assert len(violated) > 0 and (got_al["outer"][violated, 0] == hb.MPC_AL_MAX_OUTER).all() and (got_al["outer"][touched, 1] == 2).all()
            assert (got_al["outer"][touched, 0] != hb.MPC_AL_RUNNING).all()
            assert (got["status"][touched] == hb.MPC_CONVERGED_F).all()


@pytest.mark.parametrize("nc,A,shift", [(1, 1, 1), (2, 1, 2), (3, 5, 3)])
@pytest.mark.parametrize("B", [5, 17])
def test_al_advance_against_the_restatement(B, nc, A, shift):
    """The block, the action, the record and x_trial as gops_mpc_advance leaves them (a second solver), the multipliers shifted by
    `shift` steps with zeros entering, rho back to rho0, outer words cleared and their evaluations added to the record; rows with
    r % 3 == 1 are frozen and keep all of it."""
    n = 5
    a, b = (_armed_solver(B, n, nc, ALL_STATUSES[:4]) for _ in range(2))
    rng = np.random.RandomState(7 * B + nc)
    lam = rng.uniform(0.1, 1.0, (B, H, nc)).astype(np.float32)
    b.lam.copy_(torch.from_numpy(lam))
    b.rho.fill_(1000.0), b.viol_prev.fill_(0.25)
    b.outer.copy_(torch.from_numpy(np.tile(np.array([1, 4, 9, 0], np.int32), (B, 1))))
    frozen = torch.from_numpy((np.arange(B) % 3 == 1).astype(np.float32)).to(_dev())
    al, hyper = _al_arrays(b), ah.hyper32()
    start = np.arange(4 * B, dtype=np.int32).reshape(B, 4)
    ra, rb = (torch.from_numpy(start.copy()).to(_dev()) for _ in range(2))
    act_a = torch.zeros(B, A, device=_dev())
    (act_b, abuf, na) = _padded((B, A))
    a.advance(frozen, act_a, ra)
    want_record = ra.cpu().numpy()
    want_lam = ah.al_advance(al["lam"], al["rho"], al["viol_prev"], al["outer"], want_record, frozen.cpu().numpy(), shift, hyper)
    b.al_advance(frozen, act_b, rb, shift=shift)
    assert torch.equal(b._state.view(torch.int64), a._state.view(torch.int64)) and torch.equal(b.x_trial, a.x_trial) and torch.equal(act_b, act_a)
    got = _al_arrays(b)
    assert np.array_equal(got["lam"], want_lam) and np.array_equal(rb.cpu().numpy(), want_record)
    for k in ("rho", "viol_prev", "outer"):
        assert np.array_equal(got[k], al[k]), k
    fz = np.arange(B) % 3 == 1
    assert np.array_equal(got["lam"][fz], lam[fz]) and (got["rho"][fz] == 1000.0).all() and (got["outer"][fz] == [1, 4, 9, 0]).all()
    assert (got["lam"][~fz][:, H - min(shift, H):] == 0).all() and (got["rho"][~fz] == 10.0).all() and np.isinf(got["viol_prev"][~fz]).all()
    if shift < H:
        assert np.array_equal(got["lam"][~fz][:, :H - shift], lam[~fz][:, shift:])
    assert bool((abuf[na:] == SENTINEL).all())


def test_whole_loop_on_a_problem_with_a_closed_form_kkt_point():
    """min sum_i (x_i - a_i)^2 subject to x_i - b_i <= 0, i < 3, four rows, cost and constraint formed by torch operations (float64,
    the cost handed over minus its optimal value so that fp32 resolves its decrease).  KKT: x_i = min(a_i, b_i), lambda_i =
    max(0, 2 (a_i - b_i)); every row has active and inactive constraints.  Tolerances from the solver's own: an active constraint
    ends with |c| <= cstr_tol (viol <= cstr_tol above zero, change / rho <= lambda_tol = cstr_tol below); the inner solve ends with
    |2 (x - a) + lambda| <= pgtol, so an inactive x_i is within pgtol / 2 and lambda_i within 2 cstr_tol + pgtol."""
    dev, B, n = _dev(), 4, 3
    rng = np.random.RandomState(3)
    b = rng.uniform(-1.0, 1.0, (B, n))
    a = b + np.where(rng.uniform(size=(B, n)) < 0.6, rng.uniform(0.3, 1.5, (B, n)), -rng.uniform(0.3, 1.5, (B, n)))
    a[:, 0], a[:, 1] = b[:, 0] + 0.7, b[:, 1] - 0.4   # one active and one inactive constraint on every row
    x_opt, lam_opt = np.minimum(a, b), np.maximum(0.0, 2 * (a - b))
    f_opt = torch.from_numpy(((x_opt - a) ** 2).sum(1)).to(dev)
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    pgtol = 1e-4
    solver = hb.MpcSolver(B, n, -5.0, 5.0, dev, constraints=(n, 1))
    solver.set_hyper(pgtol=pgtol, ftol=-1.0)
    tol = solver.al_hyper_host["cstr_tol"]
    assert solver.al_hyper_host["lambda_tol"] == tol
    solver.init(torch.zeros(B, n, device=dev))
    solver.al_reset()

    def evaluate(backward=True):
        x = solver.x_trial.double()
        solver.f_al_in.copy_((((x - ad) ** 2).sum(1) - f_opt).float())
        c = (x - bd).float().t().contiguous().view(n, B, 1)
        solver.al_eval(c)
        if backward:   # d f / d x + J' seed, J = I
            solver.g.copy_((2 * (x - ad) + solver.seed.view(n, B).t().double()).float())
        return c

    for _ in range(60):
        for _ in range(8):
            evaluate()
            solver.step()
        solver.al_update(evaluate(backward=False))
        x, _, status, iterations, viol, outer, outer_it = (t.cpu().numpy() for t in solver.finish())
        if (outer != hb.MPC_AL_RUNNING).all():
            break
    lam = solver.lam.cpu().numpy()[:, :, 0]
    print("outer", outer, outer_it, "inner", status, iterations, "viol", viol, "|x - x*|", np.abs(x - x_opt).max(), "|lam - lam*|", np.abs(lam - lam_opt).max())
    assert (outer == hb.MPC_AL_CONVERGED).all() and (status == hb.MPC_CONVERGED_PG).all() and (viol <= tol).all()
    active = lam_opt > 0
    assert (np.abs(x - x_opt)[active] <= tol + 4 * EPS32).all() and (np.abs(x - x_opt)[~active] <= pgtol / 2 + 4 * EPS32).all()
    assert (lam[~active] == 0).all() and (np.abs(lam - lam_opt)[active] <= 2 * tol + pgtol + 4 * EPS32 * lam_opt.max()).all()


# ---- BatchOptController -----------------------------------------------------------------------------------------------------------
def _surr_model():
    from gops_amd.create_pkg.create_env_model import create_env_model
    return create_env_model(**ah.SURR_CFG, use_gpu=True)


def _surr_controller(model, **kw):
    from gops_amd.sys_simulator import BatchOptController
    return BatchOptController(model, num_pred_step=ah.SURR_T, ctrl_interval=1, gamma=1.0, path_constraints="augmented_lagrangian", **kw)


def test_surrcstr_against_slsqp():
    """Per row: outer status CONVERGED, constraint_violation <= cstr_tol, and the cost between OptController's SLSQP optimum of the
    problem loosened to c <= +cstr_tol and that of the problem tightened to c <= -cstr_tol, up to eps = 4 fp32 ulp of max(|J|, 1) -
    the floor of the cost agreement tests/test_mpc_gpu.py accepts between BatchOptController and OptController (its line 259: `floor =
    4 * EPS32 * np.maximum(np.abs(r["ref_cost"]), 1.0)`; the measured part of that test's allowance belongs to its cases)."""
    from gops_amd.sys_simulator import OptController
    model = _surr_model()
    obs, info = ah.surr_states()
    ctrl = _surr_controller(model)
    res = ctrl.solve(obs, info)
    tol = hb.MPC_AL_HYPER_DEFAULTS["cstr_tol"]
    J = res["cost"].cpu().numpy().astype(np.float64)
    viol, outer = res["constraint_violation"].cpu().numpy(), res["outer_status"].cpu().numpy()
    print("J", J, "viol", viol, "outer", outer, res["outer_iterations"].cpu().numpy(), "inner", res["status"].cpu().numpy(), "evaluations", res["evaluations"])
    print("multipliers", res["multipliers"].cpu().numpy()[:, :, 0], "c0", res["initial_constraint"].cpu().numpy().ravel())
    assert (res["initial_constraint"].cpu().numpy() < 0).all()

    class Offset(OptController):
        offset = 0.0

        def _constraint_fcn(self, inputs, x, info):
            return super()._constraint_fcn(inputs, x, info) + self.offset   # -c + offset >= 0  <=>  c <= offset

    bounds = []
    for off in (+tol, -tol):
        costs = []
        for b in range(ah.SURR_B):
            oc = Offset(model, num_pred_step=ah.SURR_T, ctrl_interval=1, gamma=1.0, mode="shooting")
            oc.offset = off
            oc(obs[b], {k: v[b] for k, v in info.items()})
            print("SLSQP offset", off, "row", b, oc.last_result.message, "iterations", oc.last_result.nit, "cost", oc.last_result.fun)
            costs.append(float(oc.last_result.fun))
        bounds.append(np.array(costs))
    loose, tight = bounds
    eps = 4 * EPS32 * np.maximum(np.abs(J), 1.0)
    print("J_slsqp loosened", loose, "tightened", tight, "J - loose", J - loose, "tight - J", tight - J)
    assert (outer == hb.MPC_AL_CONVERGED).all() and (viol <= tol).all()
    assert (loose - eps <= J).all() and (J <= tight + eps).all()


def test_veh2dof_errcstr_with_inactive_constraints_is_the_unconstrained_solve():
    """pyth_veh2dofconti_errcstr from states on the path (|delta_y| stays far inside its tube): multipliers exactly 0, one outer
    iteration, and the plan of BatchOptController on pyth_veh2dofconti - the same model without the constraint - bit for bit: the
    padded step of the constraint rollout does not enter the cost."""
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.sys_simulator import BatchOptController
    from gops_amd.utils.synthetic import make_batch
    cfg, T, B = dict(env_id="pyth_veh2dofconti_errcstr", pre_horizon=10), 6, 3
    d = {k: v.numpy() for k, v in make_batch(dict(cfg, batch=B), 4).items()}
    ref = d["ref_points"]
    state = np.concatenate((ref[:, 0] + np.array([[0.03, 0.01], [-0.02, -0.01], [0.0, 0.02]], np.float32), np.zeros((B, 2), np.float32)), 1)
    obs = np.concatenate((state[:, :2] - ref[:, 0], state[:, 2:], state[:, :1] - ref[:, 1:, 0]), 1).astype(np.float32)
    info = dict(state=state, ref_points=ref, path_num=d["path_num"], u_num=d["u_num"], ref_time=d["ref_time"])
    con = BatchOptController(create_env_model(**cfg, use_gpu=True), num_pred_step=T, gamma=1.0, path_constraints="augmented_lagrangian")
    got = con.solve(obs, info)
    plain = BatchOptController(create_env_model("pyth_veh2dofconti", pre_horizon=10, use_gpu=True), num_pred_step=T, gamma=1.0)
    want = plain.solve(obs, info)
    print("viol", got["constraint_violation"].cpu().numpy(), "outer", got["outer_status"].cpu().numpy(), got["outer_iterations"].cpu().numpy(),
          "evaluations", got["evaluations"], want["evaluations"])
    assert (got["multipliers"] == 0).all() and (got["constraint_violation"] == 0).all() and (got["initial_constraint"] < 0).all()
    assert (got["outer_status"] == hb.MPC_AL_CONVERGED).all() and (got["outer_iterations"] == 1).all()
    assert torch.equal(got["plan"], want["plan"]) and torch.equal(got["status"], want["status"]) and torch.equal(got["iterations"], want["iterations"])
    assert torch.equal(got["cost"], want["cost"])


def test_run_episodes_hands_the_multipliers_over(monkeypatch):
    """3 control steps, B = 3 of the surrcstr rows: after each hand-over the multipliers are the restatement's shift of the ones
    before it, and max_constraint is the largest info["constraint"] of a replay of the returned actions through gops_env_step."""
    model = _surr_model()
    obs, info = ah.surr_states()
    obs, info = obs[:3], {k: v[:3] for k, v in info.items()}
    ctrl = _surr_controller(model)
    seen = []
    advance = hb.MpcSolver.al_advance

    def spy(self, frozen, action_out, record, shift=1):
        before = {k: v.copy() for k, v in _al_arrays(self).items()}
        advance(self, frozen, action_out, record, shift=shift)
        seen.append((before, self.lam.cpu().numpy(), frozen.cpu().numpy(), shift))

    monkeypatch.setattr(hb.MpcSolver, "al_advance", spy)
    got = ctrl.run_episodes(obs, 3, info)
    assert len(seen) == 3
    hyper = ah.hyper32()
    for before, after, frozen, shift in seen:
        rec = np.zeros((3, 4), np.int32)
        want = ah.al_advance(before["lam"], before["rho"], before["viol_prev"], before["outer"], rec, frozen, shift, hyper)
        assert shift == 1 and np.array_equal(after, want) and (after[:, -1] == 0).all()
    assert (seen[0][0]["lam"] > 0).any()   # the constraint was active: there was something to hand over
    dev = ctrl.device
    o = torch.from_numpy(obs).to(dev)
    step_info = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in info.items()}
    zeros, worst = torch.zeros(3, device=dev), torch.full((3,), float("-inf"), device=dev)
    for k in range(3):
        o, _, done, info2 = hb.env_step(ctrl._env, o, got["actions"][k], zeros, step_info)
        step_info.update({key: v for key, v in info2.items() if key in step_info})
        worst = torch.maximum(worst, info2["constraint"].max(1).values)
        assert not bool(done.any())
    print("max constraint per episode", got["max_constraint"].cpu().numpy(), "status", got["status"].cpu().numpy())
    assert torch.equal(got["max_constraint"], worst) and not got["done"].any()
    assert torch.equal(got["obs"][-1], o)
