"""`gops_sample_rollout` (csrc/rollout_sample.hip), `hb.SampleRollout` and the samplers' `fused=True` path on the MI355X.

One-step consistency along the kernel's own record (nothing accumulates): for every recorded (obs_t, eps_t) the torch policy with
`get_act_dist(...).rsample(eps)` gives act / logp, and `hb.env_step` on the recorded (obs_t, act_t, info_t) gives rew, done, obs2
and the next info - compared at the step tests' rtol 1e-5 / atol 2e-5.  logp: 4 x the distance of the same evaluation in fp32
torch from float64, relative to the largest |logp| (DESIGN.md 4.16's convention), taken over ALL rows of an env / head group - a
single row's fp32 distance can be zero by chance, which would make the bar a coincidence of that row.
Carry-over, resets, the final state, `time_limited` and `end`: bit for bit against `reset_pool.restate_sample_books` of the `done`
column.  gym_pendulum's model never terminates: its group asserts a `done` column of zeros instead of a `done` reset.
Every figure is printed before the assertions (run with -s)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import closed_loop_helpers as cl
from closed_loop_helpers import ATOL, INFO, MAX_STEPS, R, RTOL, SAMPLE_ENVS as ENVS, Nets, check_sample_books as check_books, sample_inputs

pytestmark = pytest.mark.gpu
MIN_LS, MAX_LS = -2.0, 0.5
NOISE_STD = 0.1
HEADS = ("determ", "gauss", "tanh_gauss")
SHAPES = [(1, ((16,), "tanh")), (15, ((64, 64), "relu")), (17, ((16,), "tanh")), (70, ((64, 64), "relu"))]   # N = GOPS_TILE -+ 1, ...


def make_policy(head, O, A, hidden, act, seed=0):
    from gops_amd.apprfunc.mlp import DetermPolicy, StochaPolicy
    from gops_amd.utils.act_distribution import DiracDistribution, GaussDistribution, TanhGaussDistribution
    torch.manual_seed(seed)
    kw = dict(obs_dim=O, act_dim=A, hidden_sizes=list(hidden), hidden_activation=act, act_high_lim=np.full(A, 1.0, np.float32),
              act_low_lim=np.full(A, -0.8, np.float32))
    if head == "determ":
        pol = DetermPolicy(action_distribution_cls=DiracDistribution, **kw)
    else:
        pol = StochaPolicy(min_log_std=MIN_LS, max_log_std=MAX_LS,
                           action_distribution_cls=GaussDistribution if head == "gauss" else TanhGaussDistribution, **kw)
        with torch.no_grad():   # raw log stds on both sides of the clamp
            pol.linear_layers()[-1].weight[A:] *= 8.0
    return pol.to("cuda")


def make_sampler(env, head, hidden, act, N, T, cls=None, **kw):
    from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

    def policy_of(smp):
        A = act_dim_of(smp.cfg)
        pol = make_policy(head, obs_dim_of(smp.cfg), A, hidden, act)
        if head != "determ":   # the median raw log std of the env's reset states ON the upper clamp: rows on both sides of it
            from gops_amd.trainer.sampler.reset_pool import draw_reset_pool
            with torch.no_grad():
                raw = pol.policy(draw_reset_pool(smp.cfg, smp.env_model, 77, 64, smp.device, smp.data_env)["obs"])[:, A:]
                pol.linear_layers()[-1].bias[A:] += MAX_LS - raw.median(dim=0).values
        return pol

    return cl.make_sampler(env, policy_of, N, T, cls=cls, noise_std=NOISE_STD if head == "determ" else 0.0, **kw)


def make_rollout(smp, head, N, T, state):
    return cl.make_rollout(smp, HEADS.index(head), N, T, state, noise_std=NOISE_STD if head == "determ" else 0.0, min_log_std=MIN_LS,
                           max_log_std=MAX_LS)


def run(smp, env, head, N, T, seed):
    return cl.run_sample(smp, env, N, T, seed, "normal", lambda state: make_rollout(smp, head, N, T, state))


def head_of(policy, head, obs, eps):
    logits = policy(obs)
    if head == "determ":
        return logits + NOISE_STD * eps, torch.zeros(obs.shape[0], dtype=obs.dtype, device=obs.device)
    return policy.get_act_dist(logits).rsample(eps)


def check_one_step(smp, head, noise, out, acc):
    """Every recorded step against the torch policy and `hb.env_step`; logp distances from float64 accumulate in `acc`."""
    from gops_amd import hip_backend as hb
    env, pol = smp._hip_env(), smp.networks.policy
    pol64 = copy.deepcopy(pol).double()
    T, N = out["rew"].shape
    zeros = torch.zeros(N, device=smp.device)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)   # noqa: E731
    for t in range(T):
        obs, act = out["obs"][t].contiguous(), out["act"][t].contiguous()
        with torch.no_grad():
            want_act, logp32 = head_of(pol, head, obs, noise[t])
            _, logp64 = head_of(pol64, head, obs.double(), noise[t].double())
        close(act, want_act)
        info = {k: out[k][t].contiguous() for k in INFO if k in out}
        nobs, rew, done, ninfo = hb.env_step(env, obs, act, zeros, info)
        close(out["rew"][t], rew)
        assert torch.equal(out["done"][t], done)
        close(out["obs2"][t], nobs)
        for k in info:
            close(out["next_" + k][t], ninfo[k])
        if head == "determ":
            assert not bool(out["logp"][t].any())
        else:
            acc["scale"] = max(acc["scale"], float(logp64.abs().max()))
            acc["kernel"] = max(acc["kernel"], float((out["logp"][t].double() - logp64).abs().max()))
            acc["host"] = max(acc["host"], float((logp32.double() - logp64).abs().max()))
            ls = torch.chunk(pol.policy(obs), 2, dim=-1)[1]
            acc["clamped"] += int(((ls < MIN_LS) | (ls > MAX_LS)).sum())
            acc["inside"] += int(((ls >= MIN_LS) & (ls <= MAX_LS)).sum())


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("env", sorted(ENVS))
def test_record_is_one_step_consistent_and_the_books_are_exact(env, head):
    acc = dict(scale=0.0, kernel=0.0, host=0.0, clamped=0, inside=0, done_resets=0, limit_resets=0, continues=0, most_resets=0)
    for N, (hidden, act) in SHAPES:
        for T in (1, 5):
            smp = make_sampler(env, head, hidden, act, N, T)
            before, state, pool, noise, out = run(smp, env, head, N, T, seed=100 * N + T)
            assert all(bool(torch.isfinite(v).all()) for v in out.values())
            check_one_step(smp, head, noise, out, acc)
            check_books(before, state, pool, out, acc)
    print(f"\n{env} / {head}: {acc}")
    assert acc["limit_resets"] >= 1 and acc["continues"] >= 1
    if ENVS[env][1]:
        assert acc["done_resets"] >= 1 and acc["most_resets"] >= 3   # (three resets of one instance in one call: past the pool's end)
    else:
        assert acc["done_resets"] == 0   # the pendulum model has no termination rule
    if head != "determ":
        assert acc["clamped"] >= 1 and acc["inside"] >= 1
        rel_kernel, rel_host = acc["kernel"] / acc["scale"], acc["host"] / acc["scale"]
        print(f"{env} / {head}: logp against float64, relative to max |logp| = {acc['scale']:.3e}: kernel {rel_kernel:.3e}, "
              f"fp32 torch {rel_host:.3e}, bar {4 * rel_host:.3e}")
        assert rel_kernel <= 4 * rel_host


@pytest.mark.parametrize("env,head", [("lq", "gauss"), ("veh3dof", "tanh_gauss"), ("mountaincar", "determ")])
def test_rows_do_not_depend_on_the_tiling_and_launches_repeat(env, head):
    N, T = 70, 5
    smp = make_sampler(env, head, (64, 64), "relu", N, T)
    state, pool, noise = sample_inputs(smp, env, N, T, 9, "normal")
    before = {k: v.clone() for k, v in state.items()}
    ro = make_rollout(smp, head, N, T, state)
    out = {k: v.clone() for k, v in ro.run(state, pool, noise).items()}
    after = {k: v.clone() for k, v in state.items()}
    for k, v in before.items():   # a second launch on restored inputs
        state[k].copy_(v)
    again = ro.run(state, pool, noise)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    for k in after:
        assert torch.equal(after[k], state[k]), k
    one = make_rollout(smp, head, 1, T, {k: v[:1] for k, v in state.items()})
    for i in (0, 21, N - 1):   # first tile, inside the second, the last (partial) tile's doomed instance
        st = {k: v[i:i + 1].clone() for k, v in before.items()}
        alone = one.run(st, {k: v[:, i:i + 1].contiguous() for k, v in pool.items()}, noise[:, i:i + 1].contiguous())
        for k in out:
            assert torch.equal(out[k][:, i], alone[k][:, 0]), (k, i)
        for k in after:
            assert torch.equal(after[k][i:i + 1], st[k]), (k, i)


def _poly_policy(O, A):
    from gops_amd.apprfunc import poly
    from gops_amd.utils.act_distribution import DiracDistribution
    return poly.DetermPolicy(obs_dim=O, act_dim=A, degree=2, add_bias=True, act_high_lim=np.ones(A, np.float32),
                             act_low_lim=-np.ones(A, np.float32), action_distribution_cls=DiracDistribution).to("cuda")


def test_rejections_fall_back_to_the_loop():
    from gops_amd import hip_backend as hb
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    lib = hb.lib()

    def refused(smp):
        batch, _ = smp.sample()
        assert smp.path.startswith("loop: "), smp.path
        assert batch["obs"].shape[0] == smp.n * smp.steps
        return smp.path

    mlp16 = lambda O, A: make_policy("determ", O, A, (16,), "relu")   # noqa: E731
    # pyth_mobilerobot: obstacle noise drawn per step
    cfg = dict(env_id="pyth_mobilerobot")
    mob = DeviceEnvSampler(cfg, create_env_model(**cfg), n_envs=4, steps_per_sample=2, max_episode_steps=MAX_STEPS, fused=True)
    mob.networks = Nets(mlp16(13, 2))
    assert "mobilerobot" in refused(mob)
    assert lib.gops_sample_workspace_bytes(ctypes.byref(mob._hip_env()), ctypes.byref(mob.networks.policy.hip_mlp()), 4, 2) == 0
    # a constrained vehicle model
    cfg = dict(env_id="pyth_veh3dofconti_errcstr", pre_horizon=10)
    err = DeviceEnvSampler(cfg, create_env_model(**cfg), n_envs=4, steps_per_sample=2, max_episode_steps=MAX_STEPS, env_step="model", fused=True)
    err.networks = Nets(mlp16(46, 2))
    refused(err)
    assert lib.gops_sample_workspace_bytes(ctypes.byref(err._hip_env()), ctypes.byref(err.networks.policy.hip_mlp()), 4, 2) == 0
    # an action table: the policy output is read as action values.  The sampler refuses a table before it asks the kernel - the
    # entry point sees no table, and a TWO-action table's network has the width of a Gaussian head (2A); three values for one
    # action dimension are neither A nor 2A, which the entry point refuses too
    cfg = dict(env_id="gym_cartpoleconti")
    tab = DeviceEnvSampler(cfg, create_env_model(**cfg), n_envs=4, steps_per_sample=2, max_episode_steps=MAX_STEPS, fused=True,
                           action_table=[[-1.0], [0.0], [1.0]])
    tab.networks = Nets(mlp16(4, 3))
    assert "action table" in refused(tab)
    assert lib.gops_sample_workspace_bytes(ctypes.byref(tab._hip_env()), ctypes.byref(tab.networks.policy.hip_mlp()), 4, 2) == 0
    # a POLY policy
    ok = make_sampler("lq", "determ", (16,), "relu", 4, 2, fused=True)
    ok.sample()
    assert ok.path == "fused"
    poly = make_sampler("lq", "determ", (16,), "relu", 4, 2, fused=True)
    poly.networks = Nets(_poly_policy(4, 2))
    assert "POLY" in refused(poly)
    assert lib.gops_sample_workspace_bytes(ctypes.byref(poly._hip_env()), ctypes.byref(poly.networks.policy.hip_mlp()), 4, 2) == 0
    off = make_sampler("lq", "determ", (16,), "relu", 4, 2)
    off.sample()
    assert off.path == "loop: fused=False"


def test_bad_arguments_launch_nothing():
    from gops_amd import hip_backend as hb
    N, T = 4, 2
    smp = make_sampler("lq", "gauss", (16,), "relu", N, T)
    state, pool, noise = sample_inputs(smp, "lq", N, T, 1, "normal")
    ro = make_rollout(smp, "gauss", N, T, state)
    for v in ro.out.values():
        v.fill_(-7.0)
    st, pl = hb.GopsSampleState(), hb.GopsSamplePool()
    for k in ("obs", "t", "reset_count"):
        setattr(st, k, state[k].data_ptr())
    pl.obs = pool["obs"].data_ptr()

    def call(desc=ro.desc, n=N, steps=T, st=st, pl=pl, noise=noise.data_ptr(), out=ro._out, ws=ro.workspace.data_ptr(), nbytes=ro.workspace.numel()):
        ref = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
        return hb.lib().gops_sample_rollout(ctypes.byref(ro.env), ctypes.byref(ro.policy), ref(desc), n, steps, ref(st), ref(pl), noise,
                                            ref(out), ws, nbytes, None)

    no_pool = hb.GopsSampleDesc.from_buffer_copy(ro.desc)
    no_pool.pool_rows = 0
    determ = hb.GopsSampleDesc.from_buffer_copy(ro.desc)
    determ.head = hb.SAMPLE_DETERM   # 2A outputs under the deterministic head
    no_obs = hb.GopsSampleState.from_buffer_copy(st)
    no_obs.obs = None
    bad = [call(steps=0), call(n=0), call(desc=no_pool), call(desc=determ), call(desc=None), call(st=None), call(pl=None), call(noise=None),
           call(out=None), call(st=no_obs)]
    assert bad == [-1] * len(bad), bad
    assert call(ws=None) == -3 and call(nbytes=8) == -3
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in ro.out.values())
    odd = make_policy("determ", 4, 3, (16,), "relu")   # three outputs: neither A nor 2A of pyth_lq s4a2
    assert hb.lib().gops_sample_workspace_bytes(ctypes.byref(ro.env), ctypes.byref(odd.hip_mlp()), N, T) == 0
    assert call() == 0   # the description itself runs
    torch.cuda.synchronize()
    assert all(bool((v != -7.0).any()) for v in ro.out.values())


def test_on_policy_sampler_fused_returns_the_loops_columns():
    from gops_amd import hip_backend as hb
    from gops_amd.apprfunc.mlp import StateValue
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    from ppo_helpers import restate_gae
    N, T = 17, 5
    pair = []
    for fused in (True, False):
        smp = make_sampler("veh3dof", "gauss", (64, 64), "relu", N, T, cls=OnPolicyDeviceSampler, gamma=0.97, gae_lambda=0.9, fused=fused)
        torch.manual_seed(1)
        smp.networks.value = StateValue(obs_dim=46, hidden_sizes=[64, 64], hidden_activation="relu", output_activation="linear",
                                        action_distribution_cls=None).to("cuda")
        batch, _ = smp.sample()
        pair.append((smp, batch))
    (smp, got), (loop, ref) = pair
    assert smp.path == "fused" and loop.path == "loop: fused=False"
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
    val_net = hb.MlpNet(smp.networks.value.hip_mlp(), T * N)
    obs2 = smp._frollout.out["obs2"].flatten(0, 1)
    val, val_next = val_net.forward(got["obs"].contiguous()).view(T, N).clone(), val_net.forward(obs2.contiguous()).view(T, N).clone()
    done, tlim = got["done"].view(T, N), got["time_limited"].view(T, N)
    end = ((done != 0) | tlim).float()
    end[T - 1] = 1
    assert torch.equal(end, smp._frollout.out["end"]) and bool(tlim.any())
    want_ret, want_adv = hb.gae(got["rew"].view(T, N), val, val_next, done.contiguous(), end, 0.97, 0.9)
    assert torch.equal(got["ret"].view(T, N), want_ret) and torch.equal(got["adv"].view(T, N), want_adv)
    host_ret, host_adv = restate_gae(got["rew"].view(T, N).cpu(), val.cpu(), val_next.cpu(), done.cpu(), end.cpu(), 0.97, 0.9)
    assert np.array_equal(want_ret.cpu().numpy(), host_ret.astype(np.float32)) and np.array_equal(want_adv.cpu().numpy(), host_adv.astype(np.float32))
    assert smp.get_total_sample_number() == T * N
    # the pool is refreshed once an instance has used more than half of its rows, and the counts start over
    pools = smp._pools_made
    for _ in range(3):
        smp.sample()
    assert smp._pools_made > pools and int(smp._fstate["reset_count"].max()) <= R


def test_on_serial_trainer_runs_ppo_on_the_fused_sampler(tmp_path):
    import ppo_helpers   # noqa: F401  (registers PPO's constructor arguments with ac_helpers)
    import ac_helpers as ah
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    torch.manual_seed(0)
    args = ah._common_kwargs("PPO", "gym_pendulum", 3, 1, ([-2.0], [2.0]), [64, 64], "relu", 0, True)
    args.update(trainer="on_serial_trainer", max_iteration=8, num_repeat=2, num_mini_batch=2, mini_batch_size=64, sample_batch_size=128,
                policy_min_log_std=-3.0, policy_max_log_std=-0.5, log_save_interval=1000, apprfunc_save_interval=1000,
                eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    alg = create_alg(**args)
    alg.networks.to("cuda")
    smp = OnPolicyDeviceSampler(dict(env_id="gym_pendulum"), create_env_model(**args), n_envs=8, steps_per_sample=16, max_episode_steps=5,
                                seed=3, env_step="model", fused=True)
    smp.networks = alg.networks
    trainer = create_trainer(alg, smp, None, None, **args)
    trainer.step()
    assert smp.path == "fused"
    assert all(np.isfinite(float(v)) for v in alg.tb_info.values()), dict(alg.tb_info)
    assert all(bool(torch.isfinite(p).all()) for p in alg.networks.state_dict().values())
