"""`gops_sample_rollout_dis` (csrc/rollout_sample.hip), `hb.SampleRollout(action_table=...)` and the samplers' fused path with an
action table on the MI355X.

One-step consistency along the kernel's own record, as tests/test_sample_gpu.py does it (nothing accumulates): for every recorded
(obs_t, u_t) the network's outputs y are recomputed in float64 and the index by `reset_pool.restate_discrete_head` from the
recorded uniforms; `hb.env_step` on the recorded (obs_t, env_act_t, info_t) gives rew, done, obs2 and the next info.

Close calls.  d = the largest |y(fp32 torch) - y(float64)| over ALL rows of an env / head group (a single row's distance can be zero
by chance).  A row is a close call when (EPS_GREEDY) it did not explore and its float64 top-two gap is below 8 d, or (CATEGORICAL)
u0 lies within 4 act_num d of a float64 CDF boundary; there either of the two adjacent candidates is accepted and logp is checked
against the candidate the kernel took.  Everywhere else the index is exact.  Condition: at most 1 % of a group's rows are close
calls (the output layers are scaled x4).  Checked on the CPU beforehand (`cpu_close_call_check` below, d from the same CPU run):
2048 reset-pool observations of each of the four envs, each head, each (hidden, act_num) of SHAPES - 32 groups, d between 1.8e-7
and 7.0e-7.  EPS_GREEDY: 0 close calls in all 16 groups.  CATEGORICAL: 0 in 13 groups, and 3 / 1 / 1 of 2048 in lq n = 16,
veh3dof n = 16 and mountaincar n = 5 - not zero, and no scale of the logits makes it so: a row is a close call when its UNIFORM u0
falls into one of n - 1 windows of width 8 n d, so 2048 rows at n = 16 expect 2048 x 15 x 8 x 16 x 7e-7 = 2.8 of them whatever
the network is.  That is 0.15 % of a group's rows at the worst, against the 1 % of the condition.

logp: exactly 0 for EPS_GREEDY; for CATEGORICAL 4 x the distance of fp32 torch `log_softmax` from float64, relative to the largest
|logp|, over all rows of the group (DESIGN.md 4.16's convention).  Books: bit for bit against `reset_pool.restate_sample_books`.
Every figure is printed before the assertions (run with -s)."""
import copy

import numpy as np
import pytest
import torch

import closed_loop_helpers as cl
from closed_loop_helpers import ATOL, INFO, RTOL, SAMPLE_ENVS as ENVS, check_sample_books as check_books, sample_inputs

pytestmark = pytest.mark.gpu
EPS = 0.25
HEADS = ("eps_greedy", "categorical")
SHAPES = [(1, (16,), "tanh", 2), (15, (64, 64), "relu", 3), (17, (16,), "tanh", 5), (70, (64, 64), "relu", 16)]   # N, hidden, act, act_num
GROUPS = [(env, head) for env in ("cartpole", "lq", "mountaincar") for head in HEADS] + [("veh3dof", "eps_greedy")]
T = 5


def shapes_of(env):
    return [(17, (64, 64), "relu", 3)] if env == "veh3dof" else SHAPES   # one veh3dof case: the info tensors carry through


def make_sampler(env, head, hidden, act, n, N, steps=T, cls=None, device="cuda", **kw):
    from gops_amd.utils.synthetic import obs_dim_of
    return cl.make_sampler(env, lambda smp: cl.dis_net(head, obs_dim_of(smp.cfg), n, hidden, act).to(device), N, steps, cls=cls,
                           action_table=cl.table_of(env, n), device=device, epsilon=EPS if head == "eps_greedy" else 0.0, **kw)


def make_rollout(smp, head, N, steps, state):
    from gops_amd import hip_backend as hb
    return cl.make_rollout(smp, hb.SAMPLE_EPS_GREEDY if head == "eps_greedy" else hb.SAMPLE_CATEGORICAL, N, steps, state,
                           action_table=smp.action_table, epsilon=smp.epsilon)


def judge(head, y64, y32, u, index, d):
    """Per row (numpy): `ok` - the index is the restated one, or on a close call one of the two adjacent candidates -, `close_call`,
    `explored`.  The explore decision and the uniform index are exact on every row: an explored row is never a close call."""
    from gops_amd.trainer.sampler.reset_pool import HEAD_CATEGORICAL, HEAD_EPS_GREEDY, restate_discrete_head
    n = y64.shape[1]
    if head == "eps_greedy":
        want, _ = restate_discrete_head(y64, u, HEAD_EPS_GREEDY, EPS)
        explored = u[:, 0].astype(np.float64) < EPS
        order = np.argsort(-y64, axis=1, kind="stable")
        top, second = order[:, 0], order[:, 1]
        gap = np.take_along_axis(y64, top[:, None], 1)[:, 0] - np.take_along_axis(y64, second[:, None], 1)[:, 0]
        close_call = ~explored & (gap < 8 * d)
        ok = (index == want) | (close_call & ((index == top) | (index == second)))
        return ok, close_call, explored
    want, _ = restate_discrete_head(y64, u, HEAD_CATEGORICAL)
    z = np.exp(y64 - y64.max(axis=1, keepdims=True))
    cdf = np.cumsum(z, axis=1)
    cdf = cdf[:, :-1] / cdf[:, -1:]                                   # the n - 1 inner boundaries
    dist = np.abs(cdf - u[:, :1].astype(np.float64))
    k = dist.argmin(axis=1)                                           # the nearest boundary separates k and k + 1
    close_call = dist.min(axis=1) < 4 * n * d
    ok = (index == want) | (close_call & ((index == k) | (index == k + 1)))
    return ok, close_call, np.zeros(len(index), bool)


def outputs_of(net, obs):
    """(y in fp32 torch, y in float64) [rows, n] as numpy float64 arrays."""
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        return net(obs).double().cpu().numpy(), net64(obs.double()).cpu().numpy()


def cpu_close_call_check(rows=2048):
    """The check the module docstring records: no GPU involved.  -> {(env, head, hidden, act_num): (d, close calls)}."""
    from gops_amd.trainer.sampler.reset_pool import draw_reset_pool
    res = {}
    for env, head in [(e, h) for e in ENVS if e in ("cartpole", "lq", "mountaincar", "veh3dof") for h in HEADS]:
        for _, hidden, act, n in SHAPES:
            smp = make_sampler(env, head, hidden, act, n, 4, device="cpu")
            obs = draw_reset_pool(smp.cfg, smp.env_model, 77, rows, "cpu", smp.data_env)["obs"]
            y32, y64 = outputs_of(smp.networks.policy, obs)
            d = float(np.abs(y32 - y64).max())
            u = np.random.RandomState(5).uniform(size=(rows, 2)).astype(np.float32)
            _, close_call, _ = judge(head, y64, y32, u, np.zeros(rows, np.int64), d)
            res[(env, head, hidden, n)] = (d, int(close_call.sum()))
    return res


def run_case(env, head, N, hidden, act, n, seed):
    smp = make_sampler(env, head, hidden, act, n, N)
    return (smp,) + cl.run_sample(smp, env, N, T, seed, "uniform", lambda state: make_rollout(smp, head, N, T, state))


def check_env_step(smp, out):
    """env_act is the table's row bit for bit, act the index; `hb.env_step` on the recorded row reproduces the transition."""
    from gops_amd import hip_backend as hb
    env = smp._hip_env()
    steps, N = out["rew"].shape
    zeros = torch.zeros(N, device=smp.device)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)   # noqa: E731
    n = smp.action_table.shape[0]
    assert out["act"].shape == (steps, N, 1) and out["act"].dtype == torch.float32
    index = out["act"][..., 0].long()
    assert torch.equal(index.float(), out["act"][..., 0]) and int(index.min()) >= 0 and int(index.max()) < n
    assert torch.equal(out["env_act"], smp.action_table[index])
    for t in range(steps):
        obs = out["obs"][t].contiguous()
        info = {k: out[k][t].contiguous() for k in INFO if k in out}
        nobs, rew, done, ninfo = hb.env_step(env, obs, out["env_act"][t].contiguous(), zeros, info)
        close(out["rew"][t], rew)
        assert torch.equal(out["done"][t], done)
        close(out["obs2"][t], nobs)
        for k in info:
            close(out["next_" + k][t], ninfo[k])


@pytest.mark.parametrize("env,head", GROUPS)
def test_record_is_one_step_consistent_and_the_books_are_exact(env, head):
    acc = dict(done_resets=0, limit_resets=0, continues=0, most_resets=0)
    rows = []   # per shape: (n, y64, y32, u, index, logp of the kernel, fp32 torch's and float64's log-softmax at the kernel's index)
    for N, hidden, act, n in shapes_of(env):
        smp, before, state, pool, noise, out = run_case(env, head, N, hidden, act, n, seed=100 * N + T)
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        check_env_step(smp, out)
        check_books(before, state, pool, out, acc)
        obs = out["obs"].flatten(0, 1)
        y32, y64 = outputs_of(smp.networks.policy, obs)
        index = out["act"].flatten().long()
        with torch.no_grad():
            lp32 = torch.log_softmax(smp.networks.policy(obs), dim=-1).gather(1, index[:, None])[:, 0].double().cpu().numpy()
        lp64 = torch.log_softmax(torch.from_numpy(y64), dim=-1).gather(1, index.cpu()[:, None])[:, 0].numpy()
        rows.append((n, y64, y32, noise.flatten(0, 1).cpu().numpy(), index.cpu().numpy(), out["logp"].flatten().double().cpu().numpy(), lp32, lp64))
    d = max(float(np.abs(y32 - y64).max()) for _, y64, y32, *_ in rows)
    total = close_calls = explored = wrong = 0
    for n, y64, y32, u, index, *_ in rows:
        ok, cc, ex = judge(head, y64, y32, u, index, d)
        total, close_calls, explored, wrong = total + len(ok), close_calls + int(cc.sum()), explored + int(ex.sum()), wrong + int((~ok).sum())
    print(f"\n{env} / {head}: d = {d:.3e}, rows {total}, close calls {close_calls}, explored {explored} ({explored / total:.3f}), "
          f"rows with a wrong index {wrong}; books {acc}")
    assert close_calls <= 0.01 * total   # the condition of the comparison, not a measurement
    assert wrong == 0
    assert acc["limit_resets"] >= 1 and acc["continues"] >= 1 and acc["done_resets"] >= 1 and acc["most_resets"] >= 3
    if head == "eps_greedy":
        assert 0 < explored < total
        assert all(not kernel.any() for *_, kernel, _, _ in rows)   # logp = 0 exactly
    else:
        scale = max(float(np.abs(lp64).max()) for *_, lp64 in rows)
        rel_kernel = max(float(np.abs(kernel - lp64).max()) for *_, kernel, _, lp64 in rows) / scale
        rel_host = max(float(np.abs(lp32 - lp64).max()) for *_, lp32, lp64 in rows) / scale
        print(f"{env} / {head}: logp against float64, relative to max |logp| = {scale:.3e}: kernel {rel_kernel:.3e}, "
              f"fp32 torch {rel_host:.3e}, bar {4 * rel_host:.3e}")
        assert rel_kernel <= 4 * rel_host


@pytest.mark.parametrize("env,head,n", [("lq", "categorical", 16), ("veh3dof", "eps_greedy", 3), ("cartpole", "eps_greedy", 5)])
def test_launches_repeat_and_rows_do_not_depend_on_the_tiling(env, head, n):
    N = 70
    smp = make_sampler(env, head, (64, 64), "relu", n, N)
    state, pool, noise = sample_inputs(smp, env, N, T, 9, "uniform")
    before = {k: v.clone() for k, v in state.items()}
    ro = make_rollout(smp, head, N, T, state)
    out = {k: v.clone() for k, v in ro.run(state, pool, noise).items()}
    after = {k: v.clone() for k, v in state.items()}
    for k, v in before.items():   # a second launch on restored inputs: a pure function of its inputs
        state[k].copy_(v)
    again = ro.run(state, pool, noise)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    for k in after:
        assert torch.equal(after[k], state[k]), k
    for lo, hi in ((0, 16), (16, 47), (47, 69), (69, 70)):   # column blocks, launched on their own: whole tiles, tiles cut across, one column
        st = {k: v[lo:hi].clone() for k, v in before.items()}
        part = make_rollout(smp, head, hi - lo, T, st).run(st, {k: v[:, lo:hi].contiguous() for k, v in pool.items()}, noise[:, lo:hi].contiguous())
        for k in out:
            assert torch.equal(out[k][:, lo:hi], part[k]), (k, lo)
        for k in after:
            assert torch.equal(after[k][lo:hi], st[k]), (k, lo)


# ---- the samplers -------------------------------------------------------------------------------------------------------------
def _count_host_reads(monkeypatch):
    """Every way a device tensor reaches the host, counted with the bytes it moves."""
    reads, depth = [], [0]
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__", "nonzero"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda and depth[0] == 0:   # (a counted call that goes through another one counts once)
                reads.append((_name, self.numel() * self.element_size()))
            depth[0] += 1
            try:
                return _orig(self, *a, **kw)
            finally:
                depth[0] -= 1
        monkeypatch.setattr(torch.Tensor, name, counted)
    return reads


def _dqn_sampler(fused, N=17, steps=16):
    from dqn_helpers import dqn_kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    torch.manual_seed(0)
    alg = create_alg(**dqn_kwargs(4, 2, [64, 64], "relu", use_gpu=True))
    alg.networks.to("cuda")
    cfg = dict(env_id="gym_cartpoleconti")
    smp = DeviceEnvSampler(cfg, create_env_model(**cfg), n_envs=N, steps_per_sample=steps, max_episode_steps=50, seed=3, fused=fused,
                           action_table=[[-1.0], [1.0]], epsilon=0.25)
    smp.networks = alg.networks
    return smp


def test_dqn_sampler_fused_returns_the_loops_columns_and_reads_four_bytes(monkeypatch):
    smp, loop = _dqn_sampler(True), _dqn_sampler(False)
    got, _ = smp.sample()
    ref, _ = loop.sample()
    assert smp.path == "fused" and loop.path == "loop: fused=False"
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    assert bool(((got["act"] == 0.0) | (got["act"] == 1.0)).all()) and not bool(got["logp"].any())
    reads = _count_host_reads(monkeypatch)
    smp.sample()
    monkeypatch.undo()
    assert reads == [("item", 4)], reads
    assert smp.get_total_sample_number() == 2 * 17 * 16

    def off_greedy():   # the share of rows whose stored index is not the arg-max of q at the stored observation
        batch, _ = smp.sample()
        greedy = smp.networks.q(batch["obs"]).argmax(dim=-1)
        return float((batch["act"][:, 0].long() != greedy).float().mean())

    smp.epsilon = 0.0
    share0 = off_greedy()
    assert smp._frollout.dis.epsilon == 0.0
    smp.epsilon = 1.0
    share1 = off_greedy()
    assert smp._frollout.dis.epsilon == 1.0
    print(f"\nrows off the arg-max: epsilon 0 -> {share0:.3f}, epsilon 1 -> {share1:.3f} (two actions: 0.5 +- 0.03 expected over 272 rows)")
    assert share0 <= 0.01 and 0.3 <= share1 <= 0.7   # 272 rows: sigma = 0.03


def test_on_policy_sampler_fused_with_a_categorical_policy(monkeypatch):
    from gops_amd.apprfunc.mlp import StateValue
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    N, steps = 17, 8
    pair = []
    for fused in (True, False):
        smp = make_sampler("mountaincar", "categorical", (64, 64), "relu", 2, N, steps=steps, cls=OnPolicyDeviceSampler, gamma=0.97,
                           gae_lambda=0.9, fused=fused)
        assert ENVS["mountaincar"][0] == "model" and smp.action_table.tolist() == [[-1.0], [1.0]]
        torch.manual_seed(1)
        smp.networks.value = StateValue(obs_dim=2, hidden_sizes=[64, 64], hidden_activation="relu", output_activation="linear",
                                        action_distribution_cls=None).to("cuda")
        pair.append((smp, smp.sample()[0]))
    (smp, got), (loop, ref) = pair
    assert smp.path == "fused" and loop.path == "loop: fused=False"
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    assert bool(torch.isfinite(got["ret"]).all()) and bool(torch.isfinite(got["adv"]).all())
    logp = torch.log_softmax(smp.networks.policy(got["obs"]), dim=-1).gather(1, got["act"].long())[:, 0]
    assert torch.allclose(got["logp"], logp, rtol=1e-5, atol=1e-6)
    reads = _count_host_reads(monkeypatch)
    smp.sample()
    monkeypatch.undo()
    assert reads == [("item", 4)], reads
    smp.epsilon = 0.1
    with pytest.raises(ValueError, match="epsilon > 0 with a StochaPolicyDis"):
        smp.sample()
