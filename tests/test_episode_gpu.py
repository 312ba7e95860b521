"""`gops_episode_rollout` (csrc/rollout_episode.hip) and the device `Evaluator` on the MI355X.

One-step consistency along the kernel's own trace (no error accumulation, the step tests' rtol 1e-5 / atol 2e-5): every recorded
action is the torch policy on the recorded observation, and `gops_env_step(data_env = 1)` on (trace_obs[t], trace_act[t], info_t)
reproduces trace_obs[t + 1], trace_rew[t] and `done`; info_t is carried by the test from the initial condition through the same
calls.  Bookkeeping, tile independence, reproducibility, the fused path against the per-step loop, the refusals and the trainer.

Against the reference's record (tests/golden/eval_*.npz, written by tests/golden/make_golden_eval.py from the reference's own
`create_env` + `run_an_episode` steps; knife-edge episodes are filtered there): length and `terminated` equal the record for every
episode, on the fused path and on the per-step loop.  The bound on the return (against max(1, |return|)) and on the observations
of all recorded steps (against max(1, the record's largest |observation|)) is not chosen: the test first measures the per-step
loop's deviation from the record on the same fixture, and the fused kernel may deviate by 4 x that, floor 1e-5 - from the record,
and under the same bound from the loop.
Every figure is printed before the assertions (run with -s); none is quoted here because this file has not yet run on an MI355X."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import closed_loop_helpers as cl
from closed_loop_helpers import ATOL, EPISODE_ENVS as ENVS, INFO, POLICIES, RTOL, alg_kwargs, deviations, initial_conditions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def make_evaluator(env, policy, seed=0, T=40, **extra):
    from gops_amd.create_pkg.create_alg import create_alg
    torch.manual_seed(seed + 1)
    alg = create_alg(**alg_kwargs(env, policy, seed)[1])
    alg.networks.to("cuda")
    return cl.make_evaluator(env, alg.networks, T, env_model=alg.envmodel, num_eval_episode=5, seed=seed, **extra), alg


def check_trace(ev, init, res, T):
    """The one-step consistency of a traced run; returns the number of (episode, step) pairs checked."""
    from gops_amd import hip_backend as hb
    env, policy = ev._hip_env(), ev.networks.policy
    E = init["obs"].shape[0]
    length, term = res["length"].long(), res["terminated"]
    assert int(length.min()) >= 1 and int(length.max()) <= T
    info = {k: init[k] for k in INFO if k in init}
    zeros = torch.zeros(E, device=ev.device)
    assert torch.equal(res["trace_obs"][:, 0], init["obs"])
    checked = 0
    for t in range(int(length.max())):
        live = length > t
        obs, act = res["trace_obs"][:, t].clone(), res["trace_act"][:, t].clone()
        obs[~live], act[~live] = init["obs"][~live], 0.0   # (rows past their end hold the sentinel: any finite input will do)
        with torch.no_grad():
            want_act = policy(obs)
        torch.testing.assert_close(act[live], want_act[live], rtol=RTOL, atol=ATOL)
        nobs, rew, done, ninfo = hb.env_step(env, obs.contiguous(), act.contiguous(), zeros, info)
        torch.testing.assert_close(res["trace_rew"][:, t][live], rew[live], rtol=RTOL, atol=ATOL)
        ends = length == t + 1
        cont = length > t + 1
        torch.testing.assert_close(res["trace_obs"][:, t + 1][cont] if t + 1 < T else nobs[cont], nobs[cont], rtol=RTOL, atol=ATOL)
        assert not bool((done[cont] != 0).any()), "an episode went on after done"
        assert torch.equal((done[ends] != 0).float(), term[ends])
        info = {k: ninfo[k] for k in info}
        checked += int(live.sum())
    return checked


def check_books(res, T, fill):
    length, term = res["length"].long().cpu(), res["terminated"].cpu()
    rew = res["trace_rew"].double().cpu()
    steps = torch.arange(T)[None, :]
    inside = steps < length[:, None]
    want = torch.where(inside, rew, torch.zeros_like(rew)).sum(1)
    got = res["ret"].double().cpu()
    assert bool(((got - want).abs() <= 1e-6 * want.abs().clamp_min(1e-30) + 1e-30).all()), (got, want)
    assert bool((length[term == 0] == T).all()) and bool(((term == 0) | (term == 1)).all())
    for k in ("trace_obs", "trace_act", "trace_rew"):
        x = res[k].cpu().reshape(res[k].shape[0], T, -1)
        assert bool((x[~inside] == fill).all()), k + ": rows beyond length were written"
        assert bool(torch.isfinite(x[inside]).all())


@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("env", sorted(ENVS))
def test_trace_is_one_step_consistent(env, policy, dev):
    ev, _ = make_evaluator(env, policy)
    total = 0
    for T in (1, 40):
        ev.max_episode_steps = T
        for E in (1, 15, 16, 17, 33):
            init = initial_conditions(ev, env, E, seed=E, doomed=(E - 1,) if E > 1 else ())
            res = ev.run_episodes(init, trace=True, fused=True, trace_fill=-7.0)
            assert ev.kernel_refuses() is None
            total += check_trace(ev, init, res, T)
            check_books(res, T, -7.0)
            if E > 1:
                assert int(res["length"][E - 1]) == 1 and float(res["terminated"][E - 1]) == 1.0
                if env in ("lq", "veh3dof", "veh2dof"):   # the data env's terminal penalty
                    assert float(res["trace_rew"][E - 1, 0]) < -99.0
    assert total > 200


@pytest.mark.parametrize("env", ["lq", "idp", "veh3dof"])
def test_an_episode_that_ends_at_once_leaves_its_tile_alone_and_launches_repeat(env, dev):
    ev, _ = make_evaluator(env, "relu64")
    a = initial_conditions(ev, env, 16, seed=2)
    b = initial_conditions(ev, env, 16, seed=2, doomed=(5,))
    ra = ev.run_episodes(a, trace=True, trace_fill=0.0)
    rb = ev.run_episodes(b, trace=True, trace_fill=0.0)
    rb2 = ev.run_episodes(b, trace=True, trace_fill=0.0)
    others = [i for i in range(16) if i != 5]
    assert int(rb["length"][5]) == 1 and int(ra["length"][5]) > 1
    for k in ra:
        assert torch.equal(ra[k][others], rb[k][others]), k
        assert torch.equal(rb[k], rb2[k]), k


EVAL_CASES = ["eval_idp_fhadp_trained", "eval_lq_s4a2_infadp_trained", "eval_veh3dof_p10", "eval_veh2dof_p10", "eval_cartpole"]
_ENV_OF = {"pyth_idpendulum": "idp", "pyth_lq": "lq", "pyth_veh3dofconti": "veh3dof", "pyth_veh2dofconti": "veh2dof",
           "gym_cartpoleconti": "cartpole"}


def fixture_evaluator(g, T):
    """The evaluator of a recorded case: the fixture's policy (state_dict, action limits) on the fixture's env."""
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.trainer.evaluator import Evaluator
    meta = json.loads(str(g["meta/cfg"]))
    pol = meta["policy"]
    extra = dict(action_high_limit=np.array(pol["act_high"], np.float32), action_low_limit=np.array(pol["act_low"], np.float32))
    if pol["pre_horizon"]:
        extra["pre_horizon"] = pol["pre_horizon"]
    cfg, kw = alg_kwargs(_ENV_OF[meta["env"]["env_id"]], (pol["alg"], tuple(pol["hidden"]), pol["act"]), pol["seed"], **extra)
    alg = create_alg(**kw)
    alg.networks.policy.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")})
    alg.networks.to("cuda")
    return Evaluator(env_model=alg.envmodel, networks=alg.networks, cfg=cfg, num_eval_episode=1, eval_save=False, max_episode_steps=T)


def check_against_record(ev, init, obs, ret, length, terminated, label):
    """The issue's rule: the per-step loop's own deviation from the reference's record is measured first; the fused kernel may
    deviate by 4 x that (floor 1e-5 relative) from the record - and, under the same bound, from the loop."""
    loop = ev.run_episodes(init, trace=True, fused=False, trace_fill=0.0)
    fused = ev.run_episodes(init, trace=True, fused=True, trace_fill=0.0)
    assert ev.kernel_refuses() is None
    l_ret, l_obs = deviations(loop, obs, ret, length)
    f_ret, f_obs = deviations(fused, obs, ret, length)
    b_ret, b_obs = max(4.0 * l_ret, 1e-5), max(4.0 * l_obs, 1e-5)
    loop_np = {k: v.cpu().numpy() for k, v in loop.items()}
    x_ret, x_obs = deviations(fused, loop_np["trace_obs"], loop_np["ret"].astype(np.float64), loop_np["length"])
    print(f"{label}: loop vs record  ret {l_ret:.3e} obs {l_obs:.3e} | bounds ret {b_ret:.3e} obs {b_obs:.3e} | "
          f"fused vs record  ret {f_ret:.3e} obs {f_obs:.3e} | fused vs loop  ret {x_ret:.3e} obs {x_obs:.3e}")
    for name, res in (("loop", loop), ("fused", fused)):
        assert np.array_equal(res["length"].cpu().numpy(), length), name + ": episode lengths differ from the record"
        assert np.array_equal(res["terminated"].cpu().numpy(), terminated), name + ": terminations differ from the record"
    assert f_ret <= b_ret and f_obs <= b_obs
    assert x_ret <= b_ret and x_obs <= b_obs


@pytest.mark.parametrize("name", EVAL_CASES)
def test_episodes_against_the_reference_record_and_the_per_step_loop(name, dev):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    ev = fixture_evaluator(g, 40)
    vehicle = ev.cfg["env_id"].startswith("pyth_veh")
    init = {"obs": torch.from_numpy(g["init/obs"])}
    if vehicle:
        init.update({k: torch.from_numpy(np.asarray(g["init/" + k], np.float32)) for k in INFO})
    length = g["ep/length"]
    assert int((g["ep/terminated"] == 1).sum()) >= 4 and int((g["ep/terminated"] == 0).sum()) >= 4 and len(length) >= 30
    check_against_record(ev, init, g["ep/obs"], g["ep/ret"], length, g["ep/terminated"], name)
    if "full/obs" in g.files:   # one episode at the data env's registered limit
        from gops_amd.trainer.evaluator import registered_episode_steps
        T = registered_episode_steps(ev.cfg)
        assert T == int(g["full/length"]) == 500
        ev.max_episode_steps = T
        check_against_record(ev, {"obs": torch.from_numpy(g["full/obs0"][None])}, g["full/obs"][None], g["full/ret"][None],
                             np.array([T], np.int32), np.zeros(1, np.float32), name + " (full limit)")


def test_refusals_surface_as_runtime_errors(dev):
    from gops_amd import hip_backend as hb
    ev, alg = make_evaluator("lq", "relu64")
    env, mlp = ev._hip_env(), ev.networks.policy.hip_mlp()
    init = initial_conditions(ev, "lq", 4)
    hb.EpisodeRollout(env, mlp, episodes=4, max_steps=3).run(init)   # the accepted description runs
    model_env = hb.GopsEnv.from_buffer_copy(env)
    model_env.data_env = 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        hb.EpisodeRollout(model_env, mlp, episodes=4, max_steps=3)
    half = hb.make_mlp(*mlp._keep, "relu", dtype="fp16")
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        hb.EpisodeRollout(env, half, episodes=4, max_steps=3)
    w = torch.zeros(2, 4, device=dev)
    poly = hb.make_poly(w, None, hb.POLY_FULL[1])
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        hb.EpisodeRollout(env, poly, episodes=4, max_steps=3)
    mob = hb.GopsEnv.from_buffer_copy(env)
    mob.kind, mob.obs_dim, mob.act_dim = hb.ENV_MOBILEROBOT, 13, 2
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        hb.EpisodeRollout(mob, mlp, episodes=4, max_steps=3)
    small = hb.EpisodeRollout(env, mlp, episodes=4, max_steps=3, workspace_bytes=64)
    with pytest.raises(RuntimeError, match="GOPS_ERR_WORKSPACE"):
        small.run(init)


def test_mobilerobot_runs_through_the_per_step_loop(dev):
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.trainer.evaluator import Evaluator
    cfg = dict(env_id="pyth_mobilerobot")
    A = 2
    kw = dict(algorithm="INFADP", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_mobilerobot", obsv_dim=13,
              action_dim=A, action_type="continu", action_high_limit=np.ones(A, dtype=np.float32),
              action_low_limit=-np.ones(A, dtype=np.float32), policy_func_type="MLP", policy_func_name="DetermPolicy",
              policy_hidden_sizes=[64, 64], policy_hidden_activation="relu", policy_act_distribution="default",
              policy_learning_rate=1e-3, use_gpu=True, value_func_type="MLP", value_func_name="StateValue",
              value_hidden_sizes=[64, 64], value_hidden_activation="relu", value_learning_rate=1e-3)
    alg = create_alg(**kw)
    alg.networks.to("cuda")
    ev = Evaluator(env_model=alg.envmodel, networks=alg.networks, cfg=cfg, num_eval_episode=6, eval_save=False, max_episode_steps=12)
    assert ev.kernel_refuses() is not None
    assert np.isfinite(ev.run_evaluation(0))
    assert tuple(ev.last["length"].shape) == (6,) and int(ev.last["length"].max()) <= 12


def test_trainer_evaluates_on_the_device(tmp_path, dev):
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_buffer import create_buffer
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    torch.manual_seed(4)
    cfg, kw = alg_kwargs("idp", "finite_elu64", seed=4)
    kw.update(buffer_name="replay_buffer", buffer_max_size=4096, buffer_warm_size=256, replay_batch_size=64, sample_interval=1,
              additional_info={}, max_iteration=6, log_save_interval=1000, apprfunc_save_interval=1000, eval_interval=2,
              save_folder=str(tmp_path), ini_network_dir=None)
    alg = create_alg(**kw)
    alg.networks.to("cuda")
    smp = DeviceEnvSampler(cfg, alg.envmodel, n_envs=64, steps_per_sample=2, max_episode_steps=50, seed=4)
    ev = create_evaluator(evaluator_name="evaluator", env_model=alg.envmodel, networks=alg.networks, num_eval_episode=5, eval_save=True,
                          is_render=False, max_episode_steps=40, **kw)
    returns = []
    run = ev.run_evaluation
    ev.run_evaluation = lambda it: returns.append((it, run(it))) or returns[-1][1]
    ev.load_state_dict = lambda sd: pytest.fail("a device evaluator must not be handed a state_dict copy")
    trainer = create_trainer(alg, smp, create_buffer(**kw), ev, **kw)
    scalars = []

    class Writer:   # (records what the trainer logs, whether or not tensorboard is installed)
        def add_scalar(self, tag, value, step):
            scalars.append((tag, value, step))

        def flush(self):
            pass

    trainer.writer = Writer()
    ptrs = [p.data_ptr() for p in alg.networks.parameters()]
    trainer.train()
    assert [p.data_ptr() for p in alg.networks.parameters()] == ptrs and all(p.is_cuda for p in alg.networks.parameters())
    assert [it for it, _ in returns] == [1, 3, 5] or [it for it, _ in returns] == [2, 4], returns
    # the reference's rule: best-so-far return once iteration >= max_iteration / 5, one *_opt.pkl at the last improvement
    best, best_it = -float("inf"), None
    for it, r in returns:
        if r >= best and it >= 6 / 5:
            best, best_it = r, it
    opt = [os.path.basename(f) for f in glob.glob(os.path.join(str(tmp_path), "apprfunc", "*_opt.pkl"))]
    assert opt == [f"apprfunc_{best_it}_opt.pkl"], (opt, returns)
    from gops_amd.utils.tensorboard_setup import tb_tags
    for tag in ("TAR of RL iteration", "TAR of total time", "TAR of collected samples"):
        assert [v for t, v, _ in scalars if t == tb_tags[tag]] == [r for _, r in returns], tag
    saved = sorted(glob.glob(os.path.join(str(tmp_path), "evaluator", "iter*_ep*.npy")))
    assert len(saved) == 5 * len(returns)
    ep = np.load(saved[0], allow_pickle=True).item()
    assert set(ep) == {"reward_list", "action_list", "obs_list"} and len(ep["reward_list"]) == len(ep["obs_list"]) >= 1
