"""Shared by test_mpc_episode_cpu.py / test_mpc_episode_gpu.py and golden/make_golden_mpc_episode.py: a numpy restatement of
gops_mpc_advance (include/gops_hip.h has the rule; csrc/mpc_lbfgs.hip the kernel) on the dict of arrays mpc_helpers works on, the
closed-loop cases, and the float64 oracle's replay of a closed loop (oracle/adp_oracle.py on double tensors)."""
import os

import numpy as np
import torch

import mpc_helpers as mh

FROZEN = 5
STEPS = 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_episode.npz")
EPS32 = float(np.finfo(np.float32).eps)
# the closed-loop cases of the GPU tests and of the reference's record
CASES = [dict(name="lqs2a1_T5_ci1", env_id="pyth_lq", lq_config="s2a1", T=5, ci=1),
         dict(name="lqs4a2_T6_ci2", env_id="pyth_lq", lq_config="s4a2", T=6, ci=2),
         dict(name="idpendulum_T10_ci1", env_id="pyth_idpendulum", T=10, ci=1)]


def advance(st, frozen, act_dim, record, store=np.float64):
    """gops_mpc_advance on every row of `st` in place; `record` [B, 4] int is updated; returns (action [B, act_dim], the x_trial
    argument the call leaves [B, n]).  Element i of the new start is element i + act_dim of the accepted point where that exists and
    element i itself from there on."""
    B, n = st["x"].shape
    A, fz = int(act_dim), np.asarray(frozen).reshape(B) != 0
    assert n % A == 0
    x = st["x"].copy()
    i = np.arange(n)
    x0 = x[:, np.where(i + A < n, i + A, i)].astype(np.float64)
    action = np.where(fz[:, None], 0, x[:, :A]).astype(store)
    record[:, 0] = np.where(fz, FROZEN, st["status"])
    record[:, 1] += np.where(fz, 0, st["iterations"])
    record[:, 2] += np.where(fz, 0, st["evaluations"])
    record[:, 3] += np.where(fz, 0, 1)
    for k in mh.SCALARS[:5] + mh.COUNTERS:
        st[k][:] = 0
    for k in mh.VECTORS + ("rho",):
        st[k][...] = 0
    st["gamma"][:] = 1.0
    st["status"][fz] = FROZEN
    st["x"][:] = st["x_trial"][:] = np.clip(x0, st["lo"].astype(np.float64), st["hi"].astype(np.float64)).astype(store)
    return action, st["x_trial"].copy()


def oracle_env(c):
    """The float64 oracle's description of a case's raw model."""
    from oracle import adp_oracle as orc
    env = orc.make_env(c["env_id"], lq_config=c.get("lq_config", "s4a2"))
    if env["kind"] == "lq":
        env = dict(env, lq={k: (v.double() if torch.is_tensor(v) else v) for k, v in env["lq"].items()})
    return env


def oracle_step(env, x, a):
    """One raw model step in float64: (next state [B, obs], reward [B], done [B])."""
    from oracle import adp_oracle as orc
    x, a = torch.as_tensor(np.asarray(x), dtype=torch.float64), torch.as_tensor(np.asarray(a), dtype=torch.float64)
    x2, r, d = orc.lq_step(env["lq"], x, a) if env["kind"] == "lq" else orc.idp_step(x, a)
    return x2.numpy(), r.numpy(), d.numpy()


def replay(c, x0, actions):
    """The closed loop of `actions` [steps, B, A] (each held over ctrl_interval model steps) from x0 under the float64 oracle, rows
    frozen once done as run_episodes freezes them: (return [B], done [B], states [steps + 1, B, obs])."""
    env = oracle_env(c)
    x = np.asarray(x0, dtype=np.float64)
    ret, live, states = np.zeros(x.shape[0]), np.ones(x.shape[0], dtype=bool), [x]
    for a in np.asarray(actions, dtype=np.float64):
        for _ in range(c["ci"]):
            x2, r, d = oracle_step(env, x, a)
            ret = ret + np.where(live, r, 0.0)
            x = np.where(live[:, None], x2, x)
            live = live & ~d
        states.append(x)
    return ret, ~live, np.stack(states)


def shooting_cost(c, env, x, plan):
    """(cost [B], d cost / d plan [B, n]) of the plans [B, n] from the states x in float64 (raw_shooting_cost, gamma 1)."""
    from oracle import adp_oracle as orc
    B, n_cp = plan.shape[0], c["T"] // c["ci"]
    acts = torch.as_tensor(plan, dtype=torch.float64).reshape(B, n_cp, -1).repeat_interleave(c["ci"], dim=1)
    cost, _, jac = orc.raw_shooting_cost(env, torch.as_tensor(x, dtype=torch.float64), {}, acts, 1.0)
    return cost.numpy(), jac.reshape(B, n_cp, c["ci"], -1).sum(2).reshape(B, -1).numpy()


def host_plans(c, states, guess, lo, hi):
    """The reference's solve restated on the host in float64: per state scipy's L-BFGS-B (defaults, as the golden maker's stand-in
    runs it) on the oracle's shooting cost from the start points `guess` [B, n].  -> plans [B, n]."""
    import scipy.optimize as opt
    env = oracle_env(c)
    x = np.asarray(states, dtype=np.float64)
    n_cp = c["T"] // c["ci"]
    bounds = opt.Bounds(np.tile(lo, n_cp), np.tile(hi, n_cp))
    plans = []
    for b in range(x.shape[0]):
        fun = lambda p, b=b: tuple(v[0] for v in shooting_cost(c, env, x[b:b + 1], p[None]))   # noqa: E731
        plans.append(opt.minimize(fun, guess[b], jac=True, bounds=bounds, method="L-BFGS-B").x)
    return np.stack(plans)


def idp_states(B=7):
    """Initial states of the pyth_idpendulum closed loop: near the upright position except the last two rows, which lean 0.55 rad
    with both links falling outward at 3 rad/s - the tip sinks below the model's done test (l1 cos th1 + l2 cos th2 <= 1) within
    the first control steps whatever the cart does (checked under the float64 oracle by the tests that use them)."""
    rng = np.random.RandomState(77)
    x = rng.uniform(-0.03, 0.03, (B, 6))
    for r, sign in zip((B - 2, B - 1), (1.0, -1.0)):
        x[r] = [0.0, sign * 0.55, sign * 0.55, 0.0, sign * 3.0, sign * 3.0]
    return x.astype(np.float32)


def lq_states(c, B=7):
    n = int(c["lq_config"][1])
    return np.random.RandomState(78 + n).uniform(-1.0, 1.0, (B, n)).astype(np.float32)


def case_states(c, B=7):
    return idp_states(B) if c["env_id"] == "pyth_idpendulum" else lq_states(c, B)
