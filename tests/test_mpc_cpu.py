"""Batched shooting MPC without a device: what gops_mpc_* refuse and with which code (every row is refused by an argument check,
before the library makes any HIP call), the ABI surface, the float64 restatement of the step (mpc_helpers) against scipy's
L-BFGS-B, and what BatchOptController refuses at construction."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.optimize as opt

import mpc_helpers as mh
from gops_amd import hip_backend as hb

BAD, UNS, WS = -1, -2, -3
P, ODD = 0x1000, 0x1004   # a pointer that is never followed (16-byte aligned) / one that is not 8-byte aligned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40             # a state block size no check finds too small


def _call(name, state=P, nbytes=BIG, B=4, n=6, m=8, null=None):
    ptrs = [P] * 4
    if null is not None:
        ptrs[null] = None
    tail = {"gops_mpc_init": ptrs, "gops_mpc_step": ptrs, "gops_mpc_finish": ptrs}[name]
    return getattr(hb.lib(), name)(state, nbytes, B, n, m, *tail, None)


ENTRY = ("gops_mpc_init", "gops_mpc_step", "gops_mpc_finish")
ROWS = [
    ("null state", dict(state=None), BAD), ("null arg 0", dict(null=0), BAD), ("null arg 1", dict(null=1), BAD),
    ("null arg 2", dict(null=2), BAD), ("null arg 3", dict(null=3), BAD),
    ("batch 0", dict(B=0), BAD), ("n 0", dict(n=0), BAD), ("n above the maximum", dict(n=hb.MPC_MAX_DIM + 1), UNS),
    ("m 0", dict(m=0), BAD), ("m 9", dict(m=9), BAD), ("misaligned state", dict(state=ODD), BAD),
    ("small state", dict(nbytes=hb.lib().gops_mpc_state_bytes(4, 6, 8) - 1 if os.path.exists(hb.LIB_PATH) else 0), WS),
    # two faults: BAD_ARG before UNSUPPORTED before WORKSPACE
    ("misaligned + n above", dict(state=ODD, n=hb.MPC_MAX_DIM + 1), BAD), ("m 9 + small", dict(m=9, nbytes=8), BAD),
    ("n above + small", dict(n=hb.MPC_MAX_DIM + 1, nbytes=8), UNS), ("null arg + small", dict(null=1, nbytes=8), BAD),
    ("batch 0 + n above", dict(B=0, n=hb.MPC_MAX_DIM + 1), BAD),
]


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("what,kw,code", ROWS, ids=[r[0] for r in ROWS])
def test_refusals(name, what, kw, code):
    assert _call(name, **kw) == code, (name, what)


def test_state_bytes():
    q = hb.lib().gops_mpc_state_bytes
    assert [q(0, 6, 8), q(4, 0, 8), q(4, hb.MPC_MAX_DIM + 1, 8), q(4, 6, 0), q(4, 6, 9), q(-1, 6, 8)] == [0] * 6
    B, n, m = 4, 5, 3   # doubles, counters, the bounds padded to even, the vectors
    assert q(B, n, m) == 8 * B * (hb.MPC_SCALARS + m) + 4 * B * hb.MPC_COUNTERS + 4 * 2 * 6 + 4 * B * (hb.MPC_VECTORS + 2 * m) * n
    assert q(1, hb.MPC_MAX_DIM, hb.MPC_MAX_HISTORY) > 0 and hb.MPC_MAX_DIM >= 128
    # the exact size is accepted as far as the argument checks go: the next check that fails is a later one
    assert _call("gops_mpc_step", nbytes=q(4, 6, 8), null=3) == BAD and _call("gops_mpc_step", nbytes=q(4, 6, 8) - 1) == WS


def test_abi_surface():
    names = ("gops_mpc_state_bytes", "gops_mpc_init", "gops_mpc_step", "gops_mpc_finish")
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    assert re.search(r"#define GOPS_HIP_ABI_VERSION 15\b", header) and hb.lib().gops_hip_version() == 15
    exported = subprocess.run(["nm", "-D", "--defined-only", hb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in hb.EXPORTED_SYMBOLS and re.search(r" T " + name + r"$", exported, re.M), name
    for macro, value in (("MAX_DIM", hb.MPC_MAX_DIM), ("MAX_HISTORY", hb.MPC_MAX_HISTORY), ("HYPER_FLOATS", hb.MPC_HYPER_FLOATS),
                         ("SCALARS", hb.MPC_SCALARS), ("COUNTERS", hb.MPC_COUNTERS), ("VECTORS", hb.MPC_VECTORS)):
        assert re.search(rf"#define GOPS_MPC_{macro} {value}\b", header), macro
    assert hb.MPC_MAX_HISTORY == 8 and hb.MPC_HYPER_DEFAULTS == mh.HYPER


@pytest.mark.parametrize("n", [1, 3, 64, 65, 128])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_against_scipy(n, seed):
    """The float64 restatement and scipy's L-BFGS-B, both at scipy's default ftol (factr epsmch = 2.2e-9) and pgtol (1e-5), on a
    strictly convex quadratic (smallest eigenvalue mu >= 1) whose optimum has ceil(n / 4) variables on a bound (none for n = 1) and
    the rest free.  Bound on the cost: a solver that stops on pgtol with the optimum's active set has f - f* <= n pgtol^2 / (2 mu); one
    that stops on ftol after a last decrease of at most ftol max(|f|, 1) is allowed one more such decrease (steps that at least
    halve the remaining gap leave no more than the last decrease).
    Both solvers get that allowance against the constructed optimum, so they differ by at most twice it.  Active set: the variables
    on a bound are the constructed ones (multipliers >= 0.5 against a projected gradient <= 1e-5)."""
    prob = mh.Quadratic(n, 100 * n + seed)
    x0 = np.random.RandomState(seed).uniform(-1, 1, (1, n))
    st = mh.solve(mh.batch_fun([prob]), x0, prob.lo, prob.hi)
    ref = opt.minimize(lambda x: prob(x), x0[0], jac=True, method="L-BFGS-B", bounds=opt.Bounds(prob.lo, prob.hi))
    allow = mh.HYPER["ftol"] * max(abs(prob.f_opt), 1.0) + n * mh.HYPER["pgtol"] ** 2 / 2
    assert st["status"][0] in (mh.CONVERGED_PG, mh.CONVERGED_F), st["status"]
    slack = 1e-12 * max(abs(prob.f_opt), 1.0)   # float64 rounding of the cost itself: no point of the box lies below the optimum
    assert -slack <= st["f"][0] - prob.f_opt <= allow and -slack <= ref.fun - prob.f_opt <= allow, (st["f"][0], ref.fun, prob.f_opt)
    assert abs(st["f"][0] - ref.fun) <= 2 * allow
    on_bound = lambda x: (x <= prob.lo) | (x >= prob.hi)
    assert (on_bound(st["x"][0]) == prob.active).all() and (on_bound(ref.x) == prob.active).all()
    assert (4 * prob.active.sum() >= n or n == 1) and (~prob.active).sum() >= 1


def test_restatement_statuses():
    """Every status word of the restatement: an interior optimum and an all-bounds optimum stop on pgtol, a NaN gradient is
    non-finite on its row alone, a cost that never decreases spends the line search at the count limit exactly."""
    inner, corner = mh.Quadratic(5, 7, n_active=0), mh.Quadratic(5, 8, n_active=5)
    st = mh.solve(mh.batch_fun([inner, corner]), np.zeros((2, 5)), inner.lo, inner.hi, hyper=dict(mh.HYPER, ftol=0.0))
    assert (st["status"] == mh.CONVERGED_PG).all() and (np.abs(st["x"][1]) == 1).all() and (np.abs(st["x"][0]) < 1).all()
    st = mh.init_state(np.zeros((2, 3)), -1, 1, 4)
    g = np.ones((2, 3))
    g[1, 2] = np.nan
    mh.step(st, np.zeros(2), g)
    assert list(st["status"]) == [mh.RUNNING, mh.NONFINITE]
    st = mh.init_state(np.zeros((1, 3)), -1, 1, 4)
    calls = 0
    while st["status"][0] == mh.RUNNING:
        mh.step(st, np.array([float(calls > 0)]), np.ones((1, 3)))
        calls += 1
    assert st["status"][0] == mh.LINE_SEARCH and st["ls_count"][0] == mh.HYPER["max_ls"] and calls == 1 + mh.HYPER["max_ls"]


def test_batch_opt_controller_refuses_constrained_model():
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.sys_simulator import BatchOptController, OptController   # noqa: F401  (exported side by side)
    model = create_env_model("pyth_veh3dofconti_errcstr", pre_horizon=10)
    with pytest.raises(NotImplementedError, match="path constraints"):
        BatchOptController(model, num_pred_step=4, device="cpu")
    with pytest.raises(AssertionError, match="ctrl_interval"):
        BatchOptController(create_env_model("pyth_lq", lq_config="s2a1"), num_pred_step=5, ctrl_interval=2, device="cpu")
