"""Shared by test_mpc_cpu.py / test_mpc_gpu.py: a numpy restatement of gops_mpc_init / gops_mpc_step (include/gops_hip.h has the
rule; csrc/mpc_lbfgs.hip the kernel) on a dict of arrays named as `hip_backend.mpc_decode_state` names the state block's sections,
and the box-constrained quadratics both files solve.

`store` is the type every stored vector element is rounded to: np.float64 for the pure float64 solver that test_mpc_cpu.py pins
against scipy's L-BFGS-B, np.float32 to state what the kernel must leave behind when it starts from the same block (all sums in
double, every stored value rounded once)."""
import numpy as np

RUNNING, CONVERGED_PG, CONVERGED_F, LINE_SEARCH, NONFINITE = range(5)
HYPER = dict(c1=1e-4, shrink=0.5, max_ls=20, pgtol=1e-5, ftol=2.220446049250313e-9, curv_eps=2.220446049250313e-16)
SCALARS = ("f", "f_prev", "alpha", "dphi", "gamma", "rho")
COUNTERS = ("status", "iterations", "evaluations", "ls_count", "head", "count")
VECTORS = ("x", "g", "x_prev", "g_prev", "d", "x_trial", "s", "y")


def init_state(x0, lo, hi, m, store=np.float64):
    """gops_mpc_init: x = x_trial = clamp(x0), the rest cleared, gamma = 1."""
    x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
    B, n = x0.shape
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=store), (n,)).copy() for v in (lo, hi))
    st = {k: np.zeros(B) for k in SCALARS[:5]}
    st["gamma"][:] = 1.0
    st["rho"] = np.zeros((B, m))
    st.update({k: np.zeros(B, dtype=np.int32) for k in COUNTERS})
    st.update({k: np.zeros((B, n), dtype=store) for k in VECTORS[:6]})
    st.update(s=np.zeros((B, m, n), dtype=store), y=np.zeros((B, m, n), dtype=store), lo=lo, hi=hi)
    st["x"][:] = st["x_trial"][:] = np.clip(x0, lo.astype(np.float64), hi.astype(np.float64)).astype(store)
    return st


def _free(x, g, lo, hi):
    return ~(((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0)))


def _steepest(st, b, store):
    x, g = st["x"][b].astype(np.float64), st["g"][b].astype(np.float64)
    st["d"][b] = np.where(_free(x, g, st["lo"], st["hi"]), -g, 0.0).astype(store)
    return np.sqrt(np.sum(st["d"][b].astype(np.float64) ** 2))


def _two_loop(st, b, store):
    m = st["rho"].shape[1]
    x, g = st["x"][b].astype(np.float64), st["g"][b].astype(np.float64)
    fr = _free(x, g, st["lo"], st["hi"])
    q = np.where(fr, g, 0.0)
    head, count = int(st["head"][b]), int(st["count"][b])
    slots = [(head + 2 * m - 1 - j) % m for j in range(count)]   # newest first
    a = []
    for k in slots:
        a.append(st["rho"][b, k] * np.dot(st["s"][b, k].astype(np.float64)[fr], q[fr]))
        q = q - np.where(fr, a[-1] * st["y"][b, k].astype(np.float64), 0.0)
    q = q * st["gamma"][b]
    for k, aj in reversed(list(zip(slots, a))):
        beta = st["rho"][b, k] * np.dot(st["y"][b, k].astype(np.float64)[fr], q[fr])
        q = q + np.where(fr, (aj - beta) * st["s"][b, k].astype(np.float64), 0.0)
    st["d"][b] = (-q).astype(store)


def _project(st, b, alpha, store):
    x = st["x"][b].astype(np.float64)
    xt = np.clip(x + alpha * st["d"][b].astype(np.float64), st["lo"].astype(np.float64), st["hi"].astype(np.float64)).astype(store)
    st["x_trial"][b] = xt
    return float(np.dot(st["g"][b].astype(np.float64), xt.astype(np.float64) - x))


def _trial(st, b, alpha, store):
    dphi = _project(st, b, alpha, store)
    if dphi >= 0.0 and st["count"][b] > 0:   # no descent along the projected step: drop the ring, projected steepest descent
        dn = _steepest(st, b, store)
        alpha = 1.0 / dn if dn > 1.0 else 1.0
        dphi = _project(st, b, alpha, store)
        st["count"][b] = 0
    st["alpha"][b], st["dphi"][b] = alpha, dphi


def step(st, f_in, g_in, hyper=HYPER, store=np.float64):
    """gops_mpc_step on every row of `st` in place; returns the x_trial argument the call leaves [B, n]."""
    B, n = st["x"].shape
    m = st["rho"].shape[1]
    out = np.empty((B, n), dtype=store)
    f_in, g_in = np.asarray(f_in).reshape(B), np.asarray(g_in).reshape(B, n)
    for b in range(B):
        if st["status"][b] != RUNNING:
            out[b] = st["x"][b]
            continue
        first = st["evaluations"][b] == 0
        st["evaluations"][b] += 1
        fin, gin = float(f_in[b]), g_in[b].astype(np.float64)
        if not (np.isfinite(fin) and np.isfinite(gin).all()):
            st["status"][b] = NONFINITE
            out[b] = st["x"][b]
            continue
        f_acc = st["f"][b]
        if not first and not fin <= f_acc + hyper["c1"] * st["dphi"][b]:
            st["ls_count"][b] += 1
            if st["ls_count"][b] >= int(hyper["max_ls"]):
                st["status"][b] = LINE_SEARCH
                out[b] = st["x"][b]
            else:
                _trial(st, b, st["alpha"][b] * hyper["shrink"], store)
                out[b] = st["x_trial"][b]
            continue
        if not first:
            s = (st["x_trial"][b].astype(np.float64) - st["x"][b].astype(np.float64)).astype(store)
            y = (gin - st["g"][b].astype(np.float64)).astype(store)
            sy, yy = np.dot(s.astype(np.float64), y.astype(np.float64)), np.dot(y.astype(np.float64), y.astype(np.float64))
            if sy > hyper["curv_eps"] * yy:
                head = int(st["head"][b])
                st["s"][b, head], st["y"][b, head] = s, y
                st["rho"][b, head], st["gamma"][b] = 1.0 / sy, sy / yy
                st["head"][b], st["count"][b] = (head + 1) % m, min(st["count"][b] + 1, m)
            st["iterations"][b] += 1
        st["x_prev"][b], st["g_prev"][b], st["f_prev"][b] = st["x"][b], st["g"][b], f_acc
        if not first:
            st["x"][b] = st["x_trial"][b]
        st["g"][b], st["f"][b], st["ls_count"][b] = gin.astype(store), fin, 0
        x, g = st["x"][b].astype(np.float64), st["g"][b].astype(np.float64)
        pg = np.max(np.abs(x - np.clip(x - g, st["lo"].astype(np.float64), st["hi"].astype(np.float64))))
        if pg <= hyper["pgtol"]:
            st["status"][b] = CONVERGED_PG
        elif not first and f_acc - fin <= hyper["ftol"] * max(abs(f_acc), abs(fin), 1.0):
            st["status"][b] = CONVERGED_F
        if st["status"][b] != RUNNING:
            out[b] = st["x"][b]
            continue
        alpha = 1.0
        if st["count"][b] > 0:
            _two_loop(st, b, store)
        else:
            dn = _steepest(st, b, store)
            alpha = 1.0 / dn if dn > 1.0 else 1.0
        _trial(st, b, alpha, store)
        out[b] = st["x_trial"][b]
    return out


def solve(fun, x0, lo, hi, m=8, hyper=HYPER, max_iter=500):
    """The float64 solver: `fun(x [B, n]) -> (f [B], g [B, n])`.  Returns the final state dict."""
    st = init_state(x0, lo, hi, m)
    xt = st["x_trial"].copy()
    for _ in range(max_iter * 4):
        f, g = fun(xt)
        xt = step(st, f, g, hyper)
        if (st["status"] != RUNNING).all() or st["iterations"].max() >= max_iter:
            break
    return st


class Quadratic:
    """f(x) = x'Ax / 2 - b'x on [-1, 1]^n, A symmetric with eigenvalues in [1, 20]; built from its optimum: `active` variables on a
    bound with a multiplier in [0.5, 1.5] (strict complementarity), the others strictly inside with a zero gradient.  The active set
    holds ceil(n / 4) variables for n > 1 - at least a quarter of them - and none for n = 1, where a quarter and a
    free variable cannot both be had; both counts are asserted."""

    def __init__(self, n, seed, n_active=None):
        rng = np.random.RandomState(seed)
        k = (-(-n // 4) if n > 1 else 0) if n_active is None else n_active
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        self.A = (Q * rng.uniform(1.0, 20.0, n)) @ Q.T
        self.A = 0.5 * (self.A + self.A.T)
        self.active = np.zeros(n, dtype=bool)
        self.active[rng.permutation(n)[:k]] = True
        side = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
        self.x_opt = np.where(self.active, side, rng.uniform(-0.7, 0.7, n))
        g_opt = np.where(self.active, -side * rng.uniform(0.5, 1.5, n), 0.0)   # on the lower bound the gradient is positive
        self.b = self.A @ self.x_opt - g_opt
        self.n, self.lo, self.hi = n, -np.ones(n), np.ones(n)
        self.f_opt = self(self.x_opt)[0]
        if n_active is None:   # (an explicit count is the status tests' interior and all-bounds optimum)
            assert (4 * self.active.sum() >= n or n == 1) and (~self.active).sum() >= 1

    def __call__(self, x):
        x = np.asarray(x, dtype=np.float64)
        g = x @ self.A - self.b
        return 0.5 * np.sum(x * (g - self.b), -1), g


def batch_fun(problems, shifted=False):
    """fun(x [B, n]) -> (f [B], g [B, n]) in float64 over one Quadratic per row; `shifted`: f - f_opt, whose decrease near the
    optimum an fp32 cost still resolves."""
    def fun(x):
        res = [p(x[i]) for i, p in enumerate(problems)]
        return np.array([r[0] - (p.f_opt if shifted else 0.0) for r, p in zip(res, problems)]), np.stack([r[1] for r in res])
    return fun
