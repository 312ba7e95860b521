"""`gops_episode_rollout_dis` (csrc/rollout_episode.hip) and `Evaluator(action_table=...)` on the MI355X: whole evaluation episodes
of a discrete policy - a_t = action_table[argmax y(obs_t)] - in one launch.

Along the kernel's own trace (nothing accumulates): the index against the float64 arg-max (lowest index among equal maxima) with
the close-call rule of tests/test_sample_dis_gpu.py - d = the largest |y(fp32 torch) - y(float64)| over all traced rows of an env's
group; where the float64 top-two gap is below 8 d either of the two is accepted; at most 1 % of the rows may be such -, `hb.env_step`
on (trace_obs_t, table[index]) against trace_rew_t and trace_obs_{t+1} at the step tests' rtol 1e-5 / atol 2e-5, `ret` as the double
sum of the episode's trace_rew rounded once, `length` / `terminated` against the recomputed `done`, and rows beyond `length` against
`trace_fill`.  Every figure is printed before the assertions (run with -s)."""
import copy

import numpy as np
import pytest
import torch

import closed_loop_helpers as cl
from closed_loop_helpers import ATOL, RTOL

pytestmark = pytest.mark.gpu
ENVS = ("cartpole", "idp", "lq")
MAX_T, FILL = 12, -7.0
SHAPES = [(1, (16,), "tanh", 2), (17, (64, 64), "relu", 5), (40, (16,), "tanh", 5), (40, (64, 64), "relu", 2)]   # E, hidden, act, act_num


def make_evaluator(env, hidden, act, n, networks=None, **kw):
    from gops_amd.utils.synthetic import obs_dim_of
    if networks is None:   # a categorical policy, logits apart from each other: few close calls
        networks = cl.Nets(cl.dis_net("categorical", obs_dim_of(cl.CFGS[env]), n, hidden, act).to("cuda"))
    return cl.make_evaluator(env, networks, MAX_T, num_eval_episode=4, action_table=cl.table_of(env, n), **kw)


def initial_conditions(ev, env, E, seed):
    """Reset states of the data env; with E > 1 the last episode starts where its first step ends it."""
    return cl.initial_conditions(ev, env, E, seed, doomed=(E - 1,) if E > 1 else ())


def close_calls_of(net, obs, index):
    """(y32, y64, index) numpy rows -> judged later with the group's d."""
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        return net(obs).double().cpu().numpy(), net64(obs.double()).cpu().numpy(), index.cpu().numpy()


def judge(y64, index, d):
    order = np.argsort(-y64, axis=1, kind="stable")   # (stable: the lowest index among equal maxima first)
    top, second = order[:, 0], order[:, 1]
    gap = np.take_along_axis(y64, top[:, None], 1)[:, 0] - np.take_along_axis(y64, second[:, None], 1)[:, 0]
    close_call = gap < 8 * d
    return (index == top) | (close_call & (index == second)), close_call


def check_trace(ev, res, init):
    """One episode batch along its trace; -> (live mask [E, T], index [E, T])."""
    from gops_amd import hip_backend as hb
    env, table = ev._hip_env(), ev.action_table
    E, T = res["trace_rew"].shape
    length, term = res["length"].long(), res["terminated"]
    assert res["trace_act"].shape == (E, T, 1) and res["length"].dtype == torch.int32
    assert int(length.min()) >= 1 and int(length.max()) <= T
    steps = torch.arange(T, device=length.device)
    live = steps[None, :] < length[:, None]
    for k in ("trace_obs", "trace_act", "trace_rew"):   # rows beyond `length` are untouched
        dead = ~live.reshape(live.shape + (1,) * (res[k].dim() - 2)).expand_as(res[k])
        assert bool((res[k][dead] == FILL).all()), k
        assert bool(torch.isfinite(res[k][~dead]).all()) and not bool((res[k][~dead] == FILL).any()), k
    assert torch.equal(res["trace_obs"][:, 0], init["obs"])
    index = torch.where(live, res["trace_act"][..., 0], torch.zeros_like(res["trace_rew"])).long()
    assert torch.equal(torch.where(live, index.float(), torch.full_like(res["trace_rew"], FILL)), res["trace_act"][..., 0])
    assert int(index.min()) >= 0 and int(index.max()) < table.shape[0]
    zeros = torch.zeros(E, device=ev.device)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)   # noqa: E731
    for t in range(T):
        m = live[:, t]
        obs = torch.where(m[:, None], res["trace_obs"][:, t], init["obs"]).contiguous()   # (episodes that ended: any valid state)
        nobs, rew, done, _ = hb.env_step(env, obs, table[index[:, t]].contiguous(), zeros, {})
        close(res["trace_rew"][:, t][m], rew[m])
        last = m & (length == t + 1)
        assert torch.equal(done[last] != 0, term[last] != 0)   # the last step: `done` ended it, or the time limit did
        assert not bool((done[m & ~last] != 0).any())   # an episode goes on only while the env says so
        if t + 1 < T:
            nxt = live[:, t + 1]
            close(res["trace_obs"][:, t + 1][nxt], nobs[nxt])
    assert bool(((term != 0) | (length == T)).all())   # what was not terminated ran into the time limit
    want_ret = torch.where(live, res["trace_rew"], torch.zeros_like(res["trace_rew"])).double().sum(dim=1)
    # (a sequential double sum of at most 12 floats is exact up to far below half an fp32 ulp of the result: one rounding)
    assert torch.equal(res["ret"], want_ret.float())
    return live, index


@pytest.mark.parametrize("env", ENVS)
def test_trace_is_one_step_consistent(env):
    rows, episodes, ended = [], 0, 0
    for E, hidden, act, n in SHAPES:
        ev = make_evaluator(env, hidden, act, n)
        init = initial_conditions(ev, env, E, seed=10 * E + n)
        res = ev.run_episodes(init, trace=True, trace_fill=FILL)
        assert ev.path == "fused"
        live, index = check_trace(ev, res, init)
        rows.append(close_calls_of(ev.networks.policy, res["trace_obs"][live], index[live]))
        episodes, ended = episodes + E, ended + int((res["terminated"] != 0).sum())
    d = max(float(np.abs(y32 - y64).max()) for y32, y64, _ in rows)
    total = close_calls = wrong = 0
    for _, y64, index in rows:
        ok, cc = judge(y64, index, d)
        total, close_calls, wrong = total + len(ok), close_calls + int(cc.sum()), wrong + int((~ok).sum())
    print(f"\n{env}: d = {d:.3e}, traced rows {total}, close calls {close_calls}, rows with a wrong index {wrong}, "
          f"episodes {episodes}, terminated {ended}")
    assert close_calls <= 0.01 * total   # the condition of the comparison, not a measurement
    assert wrong == 0
    assert 1 <= ended < episodes   # both ways an episode ends


def _dqn_networks():
    from dqn_helpers import dqn_kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    torch.manual_seed(0)
    alg = create_alg(**dqn_kwargs(4, 2, [64, 64], "relu", use_gpu=True))
    return alg.networks.to("cuda")


@pytest.mark.parametrize("kind", ["dqn", "categorical"])
def test_evaluator_paths_agree_where_no_call_is_close(kind):
    E = 40
    networks = _dqn_networks() if kind == "dqn" else None
    ev = make_evaluator("cartpole", (64, 64), "relu", 2, networks=networks)
    init = initial_conditions(ev, "cartpole", E, seed=21)
    fused = {k: v.clone() for k, v in ev.run_episodes(init, trace=True, trace_fill=FILL).items()}
    assert ev.path == "fused"
    loop = ev.run_episodes(init, trace=True, trace_fill=FILL, fused=False)
    assert ev.path == "loop: fused=False"
    assert list(loop) and set(loop) == set(fused) and all(loop[k].shape == fused[k].shape and loop[k].dtype == fused[k].dtype for k in fused)
    live, index = check_trace(ev, fused, init)
    net = ev._policy_module()
    y32, y64, idx = close_calls_of(net, fused["trace_obs"][live], index[live])
    d = float(np.abs(y32 - y64).max())
    ok, cc = judge(y64, idx, d)
    per_row = torch.zeros_like(live)
    per_row[live] = torch.from_numpy(cc).to(live.device)
    clean = ~per_row.any(dim=1)   # episodes without a close call along the fused trace
    n_clean = int(clean.sum())
    length = fused["length"].float()
    tol = length * (ATOL + RTOL * torch.where(live, fused["trace_rew"].abs(), torch.zeros_like(fused["trace_rew"])).amax(dim=1))
    err = (fused["ret"] - loop["ret"]).abs()
    print(f"\n{kind}: d = {d:.3e}, {n_clean} of {E} episodes without a close call; terminated {int((fused['terminated'] != 0).sum())}; "
          f"largest |ret(fused) - ret(loop)| among them {float(err[clean].max()):.3e} (bar of that episode {float(tol[clean][err[clean].argmax()]):.3e})")
    assert bool(ok.all()) and 2 * n_clean >= E
    assert torch.equal(fused["length"][clean], loop["length"][clean]) and torch.equal(fused["terminated"][clean], loop["terminated"][clean])
    assert bool((err[clean] <= tol[clean]).all())
    assert torch.equal(fused["trace_act"][clean], loop["trace_act"][clean])
    # the reference's surface runs on the same path
    assert np.isfinite(ev.run_evaluation(0)) and ev.path == "fused"
