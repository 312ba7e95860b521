"""Closed-loop batched MPC on the device: gops_mpc_advance against the calls it replaces bit for bit, run_episodes against the
hand-written loop over solve(), against the reference's recorded closed loop (golden/mpc_episode.npz), and its host reads."""
import json

import numpy as np
import pytest
import torch

import mpc_episode_helpers as eh
import mpc_helpers as mh
from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -7.25, 64


def _padded(shape, dtype, dev):
    """A tensor of `shape` in front of PAD sentinel elements: (the tensor, the whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + PAD,), SENTINEL if dtype == torch.float32 else -77, dtype=dtype, device=dev)
    return buf[:n].view(shape), buf


def _feed(solvers, fun, nan_row=None):
    f, g = fun(solvers[0].x_trial.cpu().numpy().astype(np.float64))
    if nan_row is not None:
        g[nan_row, 0] = np.nan
    for s in solvers:
        s.f.copy_(torch.from_numpy(f.astype(np.float32))), s.g.copy_(torch.from_numpy(g.astype(np.float32)))


def _bits(solver):
    return solver._state.view(torch.int64)


@pytest.mark.parametrize("m", [1, 8])
@pytest.mark.parametrize("n,A", [(1, 1), (3, 1), (6, 3), (64, 2), (65, 1), (128, 4), (256, 4)])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_advance_against_finish_shift_init(B, n, A, m):
    """4 steps of a solve (row 2 is fed a NaN and stops, B > 2), then (a) finish + the cat shift + init on a second solver and
    (b) advance in place: the whole block, x_trial, the action and the record are the same bits - copies and a clamp, nothing to
    round.  Rows with r % 3 == 1 are frozen: zero action, status MPC_FROZEN, untouched by the step that follows; nothing is
    written behind the end of action, record or x_trial."""
    dev = torch.device("cuda", 0)
    problems = [mh.Quadratic(n, 1000 + 13 * n + r) for r in range(B)]
    fun = mh.batch_fun(problems)
    x0 = torch.from_numpy(np.stack([np.random.RandomState(5000 + r).uniform(-1.5, 1.5, n) for r in range(B)]).astype(np.float32)).to(dev)
    a, b = (hb.MpcSolver(B, n, -1.0, 1.0, dev, history=m) for _ in range(2))
    b.x_trial, trial_buf = _padded((B, n), torch.float32, dev)
    b.init(x0)
    for k in range(4):
        _feed([b], fun, nan_row=2 if (k == 1 and B > 2) else None)
        b.step()
    frozen = torch.from_numpy((np.arange(B) % 3 == 1).astype(np.float32)).to(dev)
    # (a) what the host did between two solves
    x, f, status, iterations = (t.clone() for t in b.finish())
    evaluations = torch.from_numpy(b.state()["evaluations"]).to(dev)
    a.init(torch.cat((x[:, A:], x[:, -A:]), 1).contiguous())
    a.status_words().masked_fill_(frozen != 0, hb.MPC_FROZEN)
    want_action = torch.where(frozen.unsqueeze(1) != 0, torch.zeros_like(x[:, :A]), x[:, :A])
    start = torch.arange(4 * B, dtype=torch.int32, device=dev).view(B, 4)
    live = (frozen == 0).to(torch.int32)
    want_record = start.clone()
    want_record[:, 0] = torch.where(frozen != 0, torch.full_like(status, hb.MPC_FROZEN), status)
    want_record[:, 1] += live * iterations
    want_record[:, 2] += live * evaluations
    want_record[:, 3] += live
    if B > 2:
        assert status[2] == hb.MPC_NONFINITE
    # (b) one launch
    action, action_buf = _padded((B, A), torch.float32, dev)
    record, record_buf = _padded((B, 4), torch.int32, dev)
    record.copy_(start)
    b.advance(frozen, action, record)
    assert torch.equal(_bits(b), _bits(a)) and torch.equal(b.x_trial, a.x_trial)
    assert torch.equal(action, want_action) and torch.equal(record, want_record)
    assert bool((action_buf[B * A:] == SENTINEL).all()) and bool((record_buf[4 * B:] == -77).all()) and bool((trial_buf[B * n:] == SENTINEL).all())
    st = b.state()
    assert (st["status"] == np.where(frozen.cpu().numpy() != 0, hb.MPC_FROZEN, hb.MPC_RUNNING)).all() and (st["gamma"] == 1.0).all()
    # the next evaluation starts from x_trial without another launch; a step moves the live rows alike on both and no frozen row
    before = _bits(b).clone()
    _feed([a, b], fun)
    a.step(), b.step()
    assert torch.equal(_bits(b), _bits(a)) and torch.equal(b.x_trial, a.x_trial)
    after, was = b.state(), hb.mpc_decode_state(before.cpu().numpy().tobytes(), B, n, m)
    fz = frozen.cpu().numpy() != 0
    for k in ("x", "g", "x_prev", "g_prev", "d", "x_trial", "s", "y", "status", "iterations", "evaluations"):
        assert np.array_equal(after[k][fz], was[k][fz]), k
    assert (after["evaluations"][~fz] == 1).all()
    assert bool((trial_buf[B * n:] == SENTINEL).all())


# ---- run_episodes -------------------------------------------------------------------------------------------------------------
def _model(c):
    from gops_amd.create_pkg.create_env_model import create_env_model
    return create_env_model(**{k: c[k] for k in ("env_id", "lq_config") if k in c}, use_gpu=True)


def _controller(c, model, **kw):
    from gops_amd.sys_simulator import BatchOptController
    return BatchOptController(model, num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0, **kw)


def _hand_loop(ctrl, c, x0, steps):
    """The loop a user writes around solve(): per control step a solve of the rows whose episode still runs (a row's bits depend on
    neither the batch nor its index), the warm start kept per row, the env model stepped with the action held, the books on the host."""
    dev, B, A = ctrl.device, x0.shape[0], ctrl.action_dim
    ctrl.reset()
    obs = torch.from_numpy(x0).to(dev)
    zeros = torch.zeros(B, device=dev)
    live = torch.ones(B, dtype=torch.bool, device=dev)
    guess, ret, length, evals = None, zeros.clone(), zeros.clone(), 0
    actions, observations, statuses = [], [obs], []
    for _ in range(steps):
        idx = live.nonzero(as_tuple=True)[0]
        ctrl._guess = None if guess is None else guess[idx].contiguous()
        res = ctrl.solve(obs[idx].contiguous())
        evals += res["evaluations"]
        guess = torch.zeros(B, ctrl.n, device=dev).index_copy(0, idx, ctrl._guess)
        act = torch.zeros(B, A, device=dev).index_copy(0, idx, res["action"])
        statuses.append(torch.full((B,), hb.MPC_FROZEN, dtype=torch.int32, device=dev).index_copy(0, idx, res["status"]))
        for _ in range(c["ci"]):
            obs2, rew, done, _ = hb.env_step(ctrl._env, obs, act, zeros, {})
            ret = ret + rew * live
            length = length + live
            obs = torch.where(live.unsqueeze(1), obs2, obs)
            live = live & (done == 0)
        actions.append(act), observations.append(obs)
    return {"return": ret, "length": length, "done": ~live, "actions": torch.stack(actions), "obs": torch.stack(observations),
            "status": torch.stack(statuses), "evaluations": evals}


@pytest.mark.parametrize("c", eh.CASES, ids=[c["name"] for c in eh.CASES])
def test_run_episodes_against_the_hand_written_loop(c):
    model, x0 = _model(c), eh.case_states(c)
    got = _controller(c, model).run_episodes(x0, eh.STEPS)
    want = _hand_loop(_controller(c, model), c, x0, eh.STEPS)
    for k in ("actions", "obs", "return", "length", "done", "status"):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert got["evaluations"] == want["evaluations"]
    done = got["done"].cpu().numpy()
    if c["env_id"] == "pyth_idpendulum":   # the two leaning rows end inside the episode, the others run all of it
        assert done.tolist() == [False] * 5 + [True] * 2
        length, status, actions = got["length"].cpu().numpy(), got["status"].cpu().numpy(), got["actions"].cpu().numpy()
        assert (length[:5] == eh.STEPS).all() and (length[5:] < eh.STEPS).all() and (length[5:] >= 1).all()
        for r in (5, 6):
            k = int(length[r])
            assert (status[k:, r] == hb.MPC_FROZEN).all() and (status[:k, r] != hb.MPC_FROZEN).all() and (actions[k:, r] == 0).all()
            assert torch.equal(got["obs"][k:, r], got["obs"][k, r].expand(eh.STEPS + 1 - k, -1))
        assert (got["record"][:, 3].cpu().numpy() == length).all()
    else:
        assert not done.any() and (got["length"] == eh.STEPS * c["ci"]).all()
    assert not (got["status"] == hb.MPC_NONFINITE).any()


def test_run_episodes_against_the_reference_record():
    """Every row of every case: the closed-loop return of run_episodes' actions, replayed by the float64 oracle, falls short of the
    return of the reference's recorded actions under the same replay by at most twice what this project's OptController falls
    short by in the same loop (its largest row), and not less than 4 fp32 ulp of the return (DESIGN.md 4.19's rule)."""
    from gops_amd.sys_simulator import OptController
    with np.load(eh.GOLDEN) as z:
        recs = {c["name"]: {k: z[f"{c['name']}/{k}"] for k in ("states", "actions")} for c in eh.CASES}
        assert json.loads(str(z["meta"]))["cases"] == eh.CASES
    for c in eh.CASES:
        rec, model = recs[c["name"]], _model(c)
        x0 = rec["states"][0]
        B = x0.shape[0]
        ref_ret, ref_done, _ = eh.replay(c, x0, rec["actions"])
        got = _controller(c, model).run_episodes(x0, eh.STEPS)
        assert not (got["status"] == hb.MPC_NONFINITE).any() and not got["done"].any() and not ref_done.any()
        ret, _, _ = eh.replay(c, x0, got["actions"].cpu().numpy())
        # this project's OptController in the same loop: one controller per row, the env model stepped with its action held
        dev, zeros = got["actions"].device, torch.zeros(1, device=got["actions"].device)
        env = _controller(c, model)._env
        opt_actions = np.zeros_like(rec["actions"])
        for b in range(B):
            ctrl = OptController(model, num_pred_step=c["T"], ctrl_interval=c["ci"], gamma=1.0, mode="shooting")
            obs = torch.from_numpy(x0[b:b + 1]).to(dev)
            for k in range(eh.STEPS):
                a = np.asarray(ctrl(obs[0].cpu().numpy()), dtype=np.float32).reshape(1, -1)
                opt_actions[k, b] = a[0]
                for _ in range(c["ci"]):
                    obs = hb.env_step(env, obs, torch.from_numpy(a).to(dev), zeros, {})[0]
        opt_ret, _, _ = eh.replay(c, x0, opt_actions)
        excess, opt_excess = ref_ret - ret, ref_ret - opt_ret
        allow = np.maximum(2 * opt_excess.max(), 4 * eh.EPS32 * np.maximum(np.abs(ref_ret), 1.0))
        print(f"{c['name']}: return shortfall batched max {excess.max():.3e} (OptController max {opt_excess.max():.3e}, allowed {allow.max():.3e}); "
              f"evaluations {got['evaluations']}; status counts {np.bincount(got['status'].cpu().numpy().ravel(), minlength=6).tolist()}")
        assert (excess <= allow).all(), (c["name"], excess, allow)


def test_run_episodes_reads_the_status_words_once_per_solve(monkeypatch):
    """check_every >= max_iter: one poll per solve and none for the hand-over - finish() is the only host read of the status words."""
    c = eh.CASES[1]
    ctrl = _controller(c, _model(c), max_iter=40, check_every=40)
    calls = []
    finish = hb.MpcSolver.finish
    monkeypatch.setattr(hb.MpcSolver, "finish", lambda self: (calls.append(1), finish(self))[1])
    got = ctrl.run_episodes(eh.case_states(c), eh.STEPS)
    assert len(calls) == eh.STEPS and got["evaluations"] == eh.STEPS * 40
    ctrl.reset()
    assert ctrl.last_episodes is None
