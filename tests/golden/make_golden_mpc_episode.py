"""Generate mpc_episode.npz: closed-loop episodes of the UNMODIFIED reference's `gops.sys_simulator.opt_controller.OptController`,
driven through the reference's env model.

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_mpc_episode.py

As in make_golden_mpc.py, a stand-in module supplies `cyipopt.minimize_ipopt` (not installed here): it hands the reference's own
cost-and-Jacobian callback, start point and bounds to scipy's L-BFGS-B and keeps the result.  The loop is the one `sys_run` and the
evaluator drive: per control step one call of the controller on the current state (its warm start is its own shift of the last
plan), then `ctrl_interval` calls of the raw model's `forward` with the action held.  Everything evaluated - the model's forward,
the rollout, the cost, its autograd Jacobian, the warm-start rule - is the reference's code.

Cases (mpc_episode_helpers.CASES): pyth_lq s2a1 (T 5, ci 1), s4a2 (T 6, ci 2), pyth_idpendulum (T 10, ci 1); 6 control steps from 3
initial states each (the first 3 near-upright / interior rows of the states the GPU tests use).  Per case `<name>/states`
[7, 3, obs], `/actions` [6, 3, A], `/rewards` [6, 3] (summed over the control interval), `/done` [6, 3], `/plan` [6, 3, n] and
`/cost` [6, 3] (the plan and the cost of every solve), and `/cost_tol` [6, 3]: how far the cost of a float64 solve of the same
problem may lie from the cost of the recorded plan.  The reference forms its cost in fp32 as a running sum of T
rewards; the rounding of that sum alone is bounded by (T - 1) u sum |r_i| (u = eps32 / 2, the bound of recursive summation), and a
search that compares two such costs cannot tell plans apart below twice that: cost_tol = max(T, 4) eps32 max(|f|, 1), 4 eps32
being the floor of DESIGN.md 4.19's rule (|f| stands for sum |r_i|: the rewards of a case share their sign or the cost is below 1) -
no measured quantity enters it."""
import json
import os
import sys
import types

import numpy as np
import scipy.optimize as opt
import torch

import make_golden as mg  # noqa: F401  (installs the reference import hook)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpc_episode_helpers as eh  # noqa: E402

_LAST = []


def _minimize_ipopt(fun, x0, args=(), jac=None, bounds=None, constraints=(), options=None, **_):
    for c in constraints:
        v = np.asarray(c["fun"](np.asarray(x0), *c["args"]))   # (the reference's "no constraint" is the constant [0.0])
        assert v.shape == (1,) and v[0] == 0.0, "a case with constraints: not a box-constrained problem"
    res = opt.minimize(fun, x0, args=args, jac=jac, bounds=bounds, method="L-BFGS-B", options=options)
    _LAST.append(res)
    return res


sys.modules["cyipopt"] = types.ModuleType("cyipopt")
sys.modules["cyipopt"].minimize_ipopt = _minimize_ipopt

from gops.create_pkg.create_env_model import create_env_model  # noqa: E402
from gops.sys_simulator.opt_controller import OptController  # noqa: E402

ROWS = 3


def main():
    out = {}
    for c in eh.CASES:
        cfg = {key: c[key] for key in ("env_id", "lq_config") if key in c}
        model = create_env_model(**cfg)
        model = getattr(model, "unwrapped", model)
        x0 = eh.case_states(c)[:ROWS]
        states, actions, rewards, dones, costs, plans = [], [], [], [], [], []
        for b in range(ROWS):
            ctrl = OptController(model, num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0, mode="shooting")
            x = torch.tensor(x0[b:b + 1], dtype=torch.float32)
            xs, acts, rews, ds, fs, ps = [x[0].numpy().copy()], [], [], [], [], []
            for _ in range(eh.STEPS):
                a = np.asarray(ctrl(x[0].numpy()), dtype=np.float32)
                fs.append(float(_LAST[-1].fun)), ps.append(np.asarray(_LAST[-1].x, dtype=np.float64).copy())
                rew, done = 0.0, False
                for _ in range(c["ci"]):
                    x, r, d, _ = model.forward(x, torch.tensor(a[None]), torch.zeros(1, dtype=torch.bool), {})
                    rew, done = rew + float(r[0]), done or bool(d[0])
                xs.append(x[0].detach().numpy().copy()), acts.append(a), rews.append(rew), ds.append(done)
            states.append(np.stack(xs)), actions.append(np.stack(acts)), rewards.append(rews), dones.append(ds), costs.append(fs), plans.append(np.stack(ps))
        costs = np.array(costs).T
        rec = dict(states=np.stack(states, 1).astype(np.float32), actions=np.stack(actions, 1).astype(np.float32),
                   rewards=np.array(rewards).T, done=np.array(dones).T, cost=costs, plan=np.stack(plans, 1),
                   cost_tol=max(c["T"], 4) * eh.EPS32 * np.maximum(np.abs(costs), 1.0))
        assert not rec["done"].any(), "the recorded rows are meant to run all their steps"
        out.update({f"{c['name']}/{k}": v for k, v in rec.items()})
        print(c["name"], "return", rec["rewards"].sum(0), "largest cost_tol", rec["cost_tol"].max())
    out["meta"] = np.array(json.dumps(dict(cases=eh.CASES, steps=eh.STEPS, rows=ROWS, gamma=1.0, solver="scipy L-BFGS-B, defaults",
                                           torch=torch.__version__)))
    np.savez_compressed(eh.GOLDEN, **out)


if __name__ == "__main__":
    main()
