"""Shared by test_mpc_al_cpu.py / test_mpc_al_gpu.py: float64 numpy restatements of gops_mpc_al_eval / _update / _advance
(include/gops_hip.h has the rules; csrc/mpc_constraint.hip and csrc/mpc_lbfgs.hip the kernels), the states of the GPU cases, and the
float64 oracle of the surrounding-vehicle model's shooting problem (oracle/adp_oracle.py's veh_surr_step).

Layouts as the kernels take them: c, seed [H, B, n_c]; lambda [B, H, n_c]; rho, viol, viol_prev, f [B]; outer [B, 4] int32."""
import numpy as np
import torch

from mpc_helpers import CONVERGED_F, CONVERGED_PG, LINE_SEARCH, RUNNING

AL_RUNNING, AL_CONVERGED, AL_MAX_OUTER = range(3)
AL_HYPER = dict(rho0=10.0, growth=10.0, rho_max=1e6, shrink_target=0.25, cstr_tol=1e-4, max_outer=30, lambda_tol=1e-4)
FROZEN = 5


def hyper32(h=AL_HYPER):
    """The hyper-parameters as the kernels read them: rounded to fp32."""
    return {k: float(np.float32(v)) for k, v in h.items()}


def _wave_sum(terms):
    """The kernel's order: lane l adds its terms l, l + 64, .. in index order, then the xor butterfly 32, .., 1."""
    v = np.zeros(64)
    for j, t in enumerate(terms):
        v[j % 64] = v[j % 64] + t
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def al_eval(c, lam, rho, f):
    """-> (f_al [B] float32, seed [H, B, n_c] float32, viol [B] float32)."""
    H, B, nc = c.shape
    c64, lam64, rho64 = c.astype(np.float64), lam.astype(np.float64), rho.astype(np.float64)
    f_al, viol = np.empty(B, np.float32), np.empty(B, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = lam64 + rho64[:, None, None] * c64.transpose(1, 0, 2)          # [B, H, n_c]
        p = np.maximum(0.0, u)                                              # (numpy's maximum keeps a NaN, as the kernel does)
        seed = p.transpose(1, 0, 2).astype(np.float32)
        terms = (p * p - lam64 * lam64).reshape(B, H * nc)
        for b in range(B):
            s = _wave_sum(terms[b])
            f_al[b] = np.float32(np.float64(f[b]) + s / (2.0 * rho64[b])) if np.isfinite(c64[:, b]).all() else np.nan
            viol[b] = np.float32(np.fmax(0.0, np.fmax.reduce(np.fmax(0.0, c64[:, b]).reshape(-1))))   # fmax passes over a NaN
    return f_al, np.ascontiguousarray(seed), viol


def al_update(st, c, lam, rho, viol, viol_prev, outer, hyper):
    """gops_mpc_al_update in place on the solver block `st` (mpc_helpers' dict: status, evaluations, ls_count, head, count, f_prev)
    and on lam, rho, viol_prev, outer; `hyper`: what the kernel reads (hyper32).  Returns the rows it touched."""
    H, B, nc = c.shape
    touched = []
    for b in range(B):
        if st["status"][b] not in (CONVERGED_PG, CONVERGED_F, LINE_SEARCH) or outer[b, 0] != AL_RUNNING:
            continue
        touched.append(b)
        rh, old = np.float64(rho[b]), lam[b].astype(np.float64)
        new = np.maximum(0.0, old + rh * c[:, b].astype(np.float64)).astype(np.float32)
        change = float(np.abs(new.astype(np.float64) - old).max())
        lam[b] = new
        if not np.float64(viol[b]) <= hyper["shrink_target"] * np.float64(viol_prev[b]):
            rho[b] = np.float32(min(rh * hyper["growth"], hyper["rho_max"]))
        viol_prev[b] = viol[b]
        outer[b, 1] += 1
        if np.float64(viol[b]) <= hyper["cstr_tol"] and change <= hyper["lambda_tol"] * rh:
            outer[b, 0] = AL_CONVERGED
        elif outer[b, 1] >= int(hyper["max_outer"]):
            outer[b, 0] = AL_MAX_OUTER
        else:
            outer[b, 2] += st["evaluations"][b]
            st["f_prev"][b] = 0.0
            st["status"][b], st["evaluations"][b], st["ls_count"][b], st["head"][b], st["count"][b] = RUNNING, 0, 0, 0, 0
    return touched


def al_advance(lam, rho, viol_prev, outer, record, frozen, shift, hyper):
    """The multiplier side of gops_mpc_al_advance -> the new lambda; rho, viol_prev, outer, record in place."""
    B, H, nc = lam.shape
    out = lam.copy()
    for b in range(B):
        if frozen[b] != 0:
            continue
        out[b] = 0.0
        if shift < H:
            out[b, :H - shift] = lam[b, shift:]
        record[b, 2] += outer[b, 2]
        outer[b] = 0
        rho[b], viol_prev[b] = np.float32(hyper["rho0"]), np.inf
    return out


# ---- the surrounding-vehicle case -----------------------------------------------------------------------------------------------
# pyth_veh3dofconti_surrcstr, pre_horizon = 5, T = 5, one surrounding vehicle, 4 rows.  The ego vehicle starts ON the reference path
# (make_batch(seed SURR_SEED) gives path, speed profile and time) at the reference speed; the other vehicle drives LON m ahead of it
# along the ego's heading, LAT m to its left, SLOWER by DU m/s, so that the ego closes in and passing on the right is the cheaper side.
# What test_mpc_al_cpu.py::test_surr_case_premises found for these rows with the float64 oracle and scipy (L-BFGS-B, the box only):
# see SURR_RECORD below - the initial state and the step-1 state (which no action moves) are feasible on every row, and the
# unconstrained optimum violates the constraint on every row by far more than 10 cstr_tol = 1e-3.
SURR_CFG = dict(env_id="pyth_veh3dofconti_surrcstr", pre_horizon=5, surr_veh_num=1)
SURR_T, SURR_B, SURR_SEED = 5, 4, 11
SURR_LON = (6.05, 6.0, 6.1, 6.0)
SURR_LAT = (0.3, 0.5, -0.4, 0.2)
SURR_DU = (1.5, 1.2, 1.6, 1.0)
# largest constraint value of the unconstrained optimum per row (m), float64 oracle, as test_surr_case_premises prints it; the
# constrained optimum (SLSQP on the oracle) costs 0.0256, 0.0115, 0.0252, 0.0094 against 0.0000, 0.0019, 0.0020, 0.0001 without
SURR_RECORD = (0.3105, 0.1859, 0.3048, 0.1207)


def surr_states():
    """-> (obs [B, O], info dict of [B, ..] float32 arrays: state, ref_points, path_num, u_num, ref_time, surr_state)."""
    from gops_amd.utils.synthetic import make_batch, veh_obs_f32
    d = {k: v.numpy() for k, v in make_batch(dict(SURR_CFG, batch=SURR_B), SURR_SEED).items()}
    ref = d["ref_points"]
    state = np.concatenate((ref[:, 0, :4], np.zeros((SURR_B, 2), np.float32)), 1).astype(np.float32)
    phi = state[:, 2].astype(np.float64)
    lon, lat, du = (np.asarray(v, dtype=np.float64) for v in (SURR_LON, SURR_LAT, SURR_DU))
    surr = np.stack((state[:, 0] + lon * np.cos(phi) - lat * np.sin(phi), state[:, 1] + lon * np.sin(phi) + lat * np.cos(phi), phi,
                     state[:, 3] - du, np.zeros(SURR_B)), 1).astype(np.float32)[:, None, :]
    obs = np.concatenate((veh_obs_f32(state, ref), (surr[..., :4] - state[:, None, :4]).reshape(SURR_B, -1)), 1).astype(np.float32)
    info = dict(state=state, ref_points=ref, path_num=d["path_num"], u_num=d["u_num"], ref_time=d["ref_time"], surr_state=surr)
    return obs, info


def surr_oracle(obs, info, plan, want_grad=False):
    """The raw model's shooting problem in float64 (oracle/adp_oracle.py: veh_surr_step over the actions plan [B, T, 2], gamma 1):
    -> (cost [B], c [B, T, n_c] of the states 1 .. T, c0 [B, n_c]) and, with `want_grad`, (d cost / d plan, a function
    w [B, T, n_c] -> d (sum w c) / d plan)."""
    from oracle import adp_oracle as orc
    env = orc.make_env(SURR_CFG["env_id"], pre_horizon=SURR_CFG["pre_horizon"], surr_veh_num=SURR_CFG["surr_veh_num"])
    acts = torch.as_tensor(np.asarray(plan), dtype=torch.float64).clone().requires_grad_(want_grad)
    o = torch.as_tensor(obs, dtype=torch.float64)
    inf = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in info.items()}
    with orc._active_ref(env):
        c0 = orc.surr_constraint(env, inf["state"], inf["surr_state"])
        cost, rows = torch.zeros(o.shape[0], dtype=torch.float64), []
        for t in range(acts.shape[1]):
            o, r, _, inf = orc.veh_surr_step(env, o, acts[:, t], inf)
            cost = cost - r
            rows.append(inf["constraint"])
        c = torch.stack(rows, 1)
        if not want_grad:
            return cost.numpy(), c.numpy(), c0.numpy()
        (gcost,) = torch.autograd.grad(cost.sum(), acts, retain_graph=True)

        def cgrad(w):
            (g,) = torch.autograd.grad((torch.as_tensor(w, dtype=torch.float64) * c).sum(), acts, retain_graph=True, allow_unused=True)
            return np.zeros(tuple(acts.shape)) if g is None else g.numpy()
    return cost.detach().numpy(), c.detach().numpy(), c0.numpy(), gcost.numpy(), cgrad
