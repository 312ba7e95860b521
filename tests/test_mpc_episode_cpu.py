"""Closed-loop batched MPC without a device: the ABI surface and the refusals of gops_mpc_advance, its float64 restatement
(mpc_episode_helpers.advance) against the composition it replaces, what run_episodes refuses, and the host restatement of the closed
loop against the reference's record (golden/mpc_episode.npz)."""
import json

import numpy as np
import pytest

import mpc_episode_helpers as eh
import mpc_helpers as mh
from abi_helpers import check_abi
from gops_amd import hip_backend as hb

BAD, P, ODD = -1, 0x1000, 0x1004


def test_abi_surface(tmp_path):
    check_abi(tmp_path, [], ["gops_mpc_advance"], [("GOPS_MPC_FROZEN", hb.MPC_FROZEN)])
    assert hb.MPC_FROZEN == eh.FROZEN == len(hb.MPC_STATUS_NAMES) - 1 and hb.MPC_FROZEN > hb.MPC_NONFINITE


def _call(state=P, nbytes=None, B=4, n=6, m=8, A=2, null=None):
    ptrs = [P] * 4
    if null is not None:
        ptrs[null] = None
    nbytes = hb.lib().gops_mpc_state_bytes(4, 6, 8) if nbytes is None else nbytes
    return hb.lib().gops_mpc_advance(state, nbytes, B, n, m, A, *ptrs, None)


ROWS = [("null state", dict(state=None)), ("null frozen", dict(null=0)), ("null action", dict(null=1)), ("null record", dict(null=2)),
        ("null x_trial", dict(null=3)), ("batch 0", dict(B=0)), ("n 0", dict(n=0)), ("n above the maximum", dict(n=hb.MPC_MAX_DIM + 1)),
        ("act_dim 0", dict(A=0)), ("n no multiple of act_dim", dict(A=4)), ("state too small", dict(nbytes=-1)),
        ("state too large", dict(nbytes=+1)), ("misaligned state", dict(state=ODD)), ("m 9", dict(m=9))]


@pytest.mark.parametrize("what,kw", ROWS, ids=[r[0] for r in ROWS])
def test_refusals(what, kw):
    """Every row is refused by an argument check, before the library makes any HIP call."""
    if "nbytes" in kw:
        kw = dict(nbytes=hb.lib().gops_mpc_state_bytes(4, 6, 8) + kw["nbytes"])
    assert _call(**kw) == BAD, what


@pytest.mark.parametrize("n,A", [(1, 1), (3, 1), (6, 3), (64, 2), (65, 1), (128, 4)])
def test_restatement_against_composition(n, A):
    """Random blocks a few steps into a solve: advance() against finish values -> the cat shift -> mpc_helpers.init_state."""
    B, m = 6, 3
    rng = np.random.RandomState(n)
    problems = [mh.Quadratic(n, 40 + r) for r in range(B)]
    st = mh.init_state(rng.uniform(-1.5, 1.5, (B, n)), -1.0, 1.0, m)
    xt = st["x_trial"].copy()
    for k in range(4):
        f, g = mh.batch_fun(problems)(xt)
        if k == 1:
            g[2, 0] = np.nan   # a row that is not running at the hand-over
        xt = mh.step(st, f, g)
    frozen = (np.arange(B) % 3 == 1).astype(np.float32)
    x, status, it, ev = st["x"].copy(), st["status"].copy(), st["iterations"].copy(), st["evaluations"].copy()
    assert status[2] == mh.NONFINITE and (status == mh.RUNNING).any()
    record = rng.randint(0, 9, (B, 4)).astype(np.int32)
    want_record = record.copy()
    action, trial = eh.advance(st, frozen, A, record)
    want = mh.init_state(np.concatenate((x[:, A:], x[:, n - A:]), 1), -1.0, 1.0, m)
    want["status"][frozen != 0] = eh.FROZEN
    for k in want:
        assert np.array_equal(st[k], want[k]), k
    assert np.array_equal(trial, want["x_trial"])
    assert np.array_equal(action, np.where(frozen[:, None] != 0, 0.0, x[:, :A]))
    live = frozen == 0
    want_record[:, 0] = np.where(live, status, eh.FROZEN)
    want_record[:, 1:] += np.where(live[:, None], np.stack((it, ev, np.ones(B, dtype=np.int32)), 1), 0)
    assert np.array_equal(record, want_record)
    # the frozen rows are left alone by a further step, whatever it is fed
    before = {k: st[k].copy() for k in mh.VECTORS + mh.COUNTERS}
    out = mh.step(st, np.zeros(B), np.ones((B, n)))
    for k in before:
        assert np.array_equal(st[k][~live], before[k][~live]), k
    assert np.array_equal(out[~live], st["x"][~live])


def test_run_episodes_refuses_what_the_constructor_refuses():
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.sys_simulator import BatchOptController
    cstr = create_env_model("pyth_veh3dofconti_errcstr", pre_horizon=10)
    with pytest.raises(NotImplementedError, match="path constraints") as at_construction:
        BatchOptController(cstr, num_pred_step=4, device="cpu")
    ctrl = BatchOptController(create_env_model("pyth_lq", lq_config="s2a1"), num_pred_step=4, device="cpu")
    with pytest.raises(ValueError, match="env_step"):
        ctrl.run_episodes(np.zeros((2, 2), dtype=np.float32), 2, env_step="neither")
    other = BatchOptController.__new__(BatchOptController)   # the constrained model behind an object the constructor never finished
    other.__dict__.update(ctrl.__dict__)
    other.base = cstr.unwrapped
    other._env = hb.make_env(other.base.hip_kind, other.base.obs_dim, other.base.action_dim, act_low=other.base.action_lower_bound,
                             act_high=other.base.action_upper_bound, pre_horizon=10, **other.base.hip_constants())
    with pytest.raises(NotImplementedError) as at_run:
        other.run_episodes(np.zeros((2, other.base.obs_dim), dtype=np.float32), 2)
    assert str(at_run.value) == str(at_construction.value)
    ctrl.n = hb.MPC_MAX_DIM + 1
    with pytest.raises(NotImplementedError, match="decision variables per state"):
        ctrl.run_episodes(np.zeros((2, 2), dtype=np.float32), 2)


def test_idpendulum_states_end_and_do_not_end_inside_the_episode():
    """The states the GPU closed-loop test starts from, under the float64 oracle: the two leaning rows are done within the 6 control
    steps for the action held at either bound and at zero; the others are not."""
    c = eh.CASES[2]
    x0 = eh.idp_states()
    for a in (-1.0, 0.0, 1.0):
        _, done, _ = eh.replay(c, x0, np.full((eh.STEPS, x0.shape[0], 1), a))
        assert done.tolist() == [False] * 5 + [True] * 2, (a, done)


def test_host_closed_loop_reproduces_the_record():
    """Along the reference's recorded closed loop, every solve restated on the host (float64 oracle + scipy's L-BFGS-B, started
    from the shift of the recorded previous plan as the reference starts it): the cost of its plan and the cost of the recorded
    plan, both under the float64 oracle from the recorded state, differ by no more than the maker's `cost_tol` (its docstring has
    the rule); the recorded action is the recorded plan's first control point, and the recorded states chain."""
    from gops_amd.create_pkg.create_env_model import create_env_model
    with np.load(eh.GOLDEN) as z:
        meta = json.loads(str(z["meta"]))
        assert meta["cases"] == eh.CASES and meta["steps"] == eh.STEPS
        for c in eh.CASES:
            rec = {k: z[f"{c['name']}/{k}"] for k in ("states", "actions", "plan", "cost_tol", "done")}
            base = create_env_model(**{k: c[k] for k in ("env_id", "lq_config") if k in c}).unwrapped
            lo, hi = (v.cpu().numpy().astype(np.float64) for v in (base.action_lower_bound, base.action_upper_bound))
            A, env = lo.size, eh.oracle_env(c)
            assert np.array_equal(rec["states"][0], eh.case_states(c)[:meta["rows"]]) and not rec["done"].any()
            assert rec["states"].shape[0] == eh.STEPS + 1 and np.array_equal(rec["actions"], rec["plan"][:, :, :A].astype(np.float32))
            worst = 0.0
            for k in range(eh.STEPS):
                prev = rec["plan"][k - 1] if k else None
                guess = np.concatenate((prev[:, A:], prev[:, -A:]), 1) if k else np.zeros_like(rec["plan"][0])
                plans = eh.host_plans(c, rec["states"][k], guess, lo, hi)
                diff = np.abs(eh.shooting_cost(c, env, rec["states"][k], plans)[0] - eh.shooting_cost(c, env, rec["states"][k], rec["plan"][k])[0])
                worst = max(worst, float((diff / rec["cost_tol"][k]).max()))
                assert (diff <= rec["cost_tol"][k]).all(), (c["name"], k, diff, rec["cost_tol"][k])
            print(c["name"], "largest cost difference / cost_tol", worst)
