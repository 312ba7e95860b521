"""What the tests of the closed-loop kernels share - the device evaluator (tests/test_episode*_{cpu,gpu}.py) and the one-launch
sampler (tests/test_sample*_gpu.py): the env tables, the tolerances of the step tests, initial conditions with rows that end at their
first step, the sampler's inputs, and the builders of samplers, rollouts and evaluators.  Each of the two families adds what is its
own (the network factory, the head's keywords) and keeps its checks beside its tests."""
import numpy as np
import torch

from gops_amd import hip_backend as hb
from gops_amd.apprfunc.mlp import StochaPolicy
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.trainer.evaluator import Evaluator
from gops_amd.trainer.sampler.reset_pool import draw_reset_pool, restate_sample_books
from gops_amd.utils.act_distribution import GaussDistribution, TanhGaussDistribution
from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

RTOL, ATOL = 1e-5, 2e-5   # the step tests' bound on one env step
INFO = hb.SAMPLE_INFO_KEYS
MAX_STEPS, R = 3, 2       # the sampler tests' episode limit and pool factor

CFGS = {   # name: workload cfg
    "lq": dict(env_id="pyth_lq", lq_config="s4a2"),
    "idp": dict(env_id="pyth_idpendulum"),
    "cartpole": dict(env_id="gym_cartpoleconti"),
    "veh3dof": dict(env_id="pyth_veh3dofconti", pre_horizon=10),
    "veh2dof": dict(env_id="pyth_veh2dofconti", pre_horizon=10),
    "pendulum": dict(env_id="gym_pendulum"),
    "mountaincar": dict(env_id="gym_mountaincarconti"),
}
EPISODE_ENVS = ("lq", "idp", "cartpole", "veh3dof", "veh2dof")   # the data envs the evaluator tests run
SAMPLE_ENVS = {   # name: (the sampler's env_step, the model can terminate)
    "lq": ("data", True), "cartpole": ("data", True), "idp": ("data", True), "veh3dof": ("data", True), "pendulum": ("model", False),
    "mountaincar": ("model", True),
}
POLICIES = {   # name: (algorithm whose container holds the policy class, hidden sizes, activation)
    "relu64": ("INFADP", (64, 64), "relu"),
    "gelu256": ("INFADP", (256, 256), "gelu"),
    "tanh3": ("INFADP", (48, 32, 16), "tanh"),
    "finite_elu64": ("FHADP", (64, 64), "elu"),   # FiniteHorizonPolicy: virtual_t = 1 at every step
}
DISTS = {"gauss": GaussDistribution, "tanh_gauss": TanhGaussDistribution}
# asymmetric action limits per action dimension (so that half and mid of the tanh squash both matter)
LIMITS = {1: ([-0.8], [1.0]), 2: ([-0.8, -0.3], [1.0, 0.2])}


class Nets(torch.nn.Module):
    """What a sampler or an evaluator reads of an algorithm's container: `policy` and `parameters()`."""

    def __init__(self, policy):
        super().__init__()
        self.policy = policy


def alg_kwargs(env, policy, seed=0, **extra):
    cfg = dict(CFGS[env])
    alg, hidden, act = POLICIES[policy] if isinstance(policy, str) else policy
    A = act_dim_of(cfg)
    kw = dict(algorithm=alg, trainer="off_serial_trainer", seed=seed, cnn_shared=False, env_id=cfg["env_id"], obsv_dim=obs_dim_of(cfg),
              action_dim=A, action_type="continu", action_high_limit=np.ones(A, dtype=np.float32),
              action_low_limit=-np.ones(A, dtype=np.float32), policy_func_type="MLP",
              policy_func_name="FiniteHorizonPolicy" if alg == "FHADP" else "DetermPolicy", policy_hidden_sizes=list(hidden),
              policy_hidden_activation=act, policy_act_distribution="default", policy_learning_rate=1e-3, use_gpu=True)
    if alg == "INFADP":
        kw.update(value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=[64, 64], value_hidden_activation=act,
                  value_learning_rate=1e-3)
    if "pre_horizon" in cfg or alg == "FHADP":
        kw["pre_horizon"] = cfg.get("pre_horizon", 10)
    if "lq_config" in cfg:
        kw["lq_config"] = cfg["lq_config"]
    kw.update(extra)
    return cfg, kw


def table_of(env, n):
    """[n, A]: A = 1 a grid over [-1, 1]; A = 2 (lq s4a2, veh3dof) a second column that runs the other way at half the size."""
    col = torch.linspace(-1.0, 1.0, n)
    return col[:, None] if act_dim_of(CFGS[env]) == 1 else torch.stack((col, -0.5 * col), dim=1)


def dis_net(head, O, n, hidden, act, seed=0):
    """An ActionValueDis (head "eps_greedy") or a StochaPolicyDis with n outputs, the output layer scaled x4: values apart from each
    other, few close calls (tests/test_sample_dis_gpu.py's docstring)."""
    from gops_amd.apprfunc.mlp import ActionValueDis, StochaPolicyDis
    from gops_amd.utils.act_distribution import CategoricalDistribution, ValueDiracDistribution
    torch.manual_seed(seed)
    kw = dict(obs_dim=O, act_num=n, hidden_sizes=list(hidden), hidden_activation=act)
    net = ActionValueDis(action_distribution_cls=ValueDiracDistribution, **kw) if head == "eps_greedy" else \
        StochaPolicyDis(action_distribution_cls=CategoricalDistribution, **kw)
    with torch.no_grad():
        net.linear_layers()[-1].weight *= 4.0
        net.linear_layers()[-1].bias *= 4.0
    return net


# ---- initial conditions -------------------------------------------------------------------------------------------------------
def doom(env, flat, rows):
    """Move rows of a flat [rows, ...] set of initial conditions to where the first step ends the episode."""
    obs = flat["obs"]
    for r in rows:
        if env == "lq":
            obs[r] = torch.tensor([14.9, 9.0, 14.9, 9.0], device=obs.device)   # state bound 15, moving outwards
        elif env == "idp":
            obs[r, 1:3] = 1.4   # tip far below the threshold
        elif env == "cartpole":
            obs[r, 0], obs[r, 1] = 2.399, 3.0
        elif env == "veh3dof":   # 4 m beside the first reference point (bound 2 m); the observation follows the state
            flat["state"][r, 1] += 4.0
            obs[r, 1] -= 4.0 * torch.cos(flat["state"][r, 2])
        elif env == "veh2dof":
            flat["state"][r, 0] += 4.0
            obs[r, 0] += 4.0
        elif env == "mountaincar":
            obs[r, 0], obs[r, 1] = 0.44, 0.06   # 0.45 is the goal
    return flat


def initial_conditions(ev, env, E, seed=5, doomed=()):
    """E reset states of the evaluator's data env; rows of `doomed` start where their first step ends the episode."""
    init = {k: v.contiguous() for k, v in draw_reset_pool(ev.cfg, ev.env_model, seed, E, ev.device).items()}
    return doom(env, init, doomed)


def rows(init, idx):
    return {k: v[idx].contiguous() for k, v in init.items()}


def sample_inputs(smp, env, N, T, seed, noise):
    """(state, pool, noise): reset states of the env, instance N - 1 (N > 1) doomed in the state and in BOTH of its pool rows - it
    resets at every step, past the pool's end -, instances at different steps into their episodes.  `noise`: "normal" - [T, N, A]
    standard normals - or "uniform" - [T, N, 2] uniforms in [0, 1), what the discrete heads draw from."""
    dev = smp.device
    keep = lambda d: {k: v.contiguous() for k, v in d.items() if k == "obs" or k in INFO}   # noqa: E731
    state = keep(draw_reset_pool(smp.cfg, smp.env_model, seed, N, dev, smp.data_env))
    flat = keep(draw_reset_pool(smp.cfg, smp.env_model, seed + 1, R * N, dev, smp.data_env))
    if N > 1 and SAMPLE_ENVS[env][1]:
        doom(env, state, [N - 1])
        doom(env, flat, [r * N + N - 1 for r in range(R)])
    pool = {k: v.reshape((R, N) + tuple(v.shape[1:])).contiguous() for k, v in flat.items()}
    state["t"] = (torch.arange(N, device=dev) % MAX_STEPS).to(torch.int32)
    state["reset_count"] = ((torch.arange(N, device=dev) // 3) % 2).to(torch.int32)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed + 2)
    if noise == "normal":
        return state, pool, torch.randn((T, N, smp._hip_env().act_dim), generator=gen, device=dev)
    assert noise == "uniform"
    return state, pool, torch.rand((T, N, 2), generator=gen, device=dev)


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def make_sampler(env, net_of, N, T, cls=None, **kw):
    """The sampler of SAMPLE_ENVS[env] with the container of `net_of(sampler)`; `kw`: the head's sampler keywords and `device`."""
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    cfg = CFGS[env]
    smp = (cls or DeviceEnvSampler)(cfg, create_env_model(**cfg), n_envs=N, steps_per_sample=T, max_episode_steps=MAX_STEPS, seed=3,
                                    pool_factor=R, env_step=SAMPLE_ENVS[env][0], **kw)
    smp.networks = Nets(net_of(smp))
    return smp


def make_rollout(smp, head, N, T, state, **kw):
    """`hb.SampleRollout` over the sampler's env and policy; `head`: a GOPS_SAMPLE_* id, `kw`: that head's keywords."""
    return hb.SampleRollout(smp._hip_env(), smp.networks.policy.hip_mlp(), n_envs=N, steps=T, head=head, max_episode_steps=MAX_STEPS,
                            pool_rows=R, info_like={k: state[k] for k in INFO if k in state}, device=smp.device, **kw)


def run_sample(smp, env, N, T, seed, noise, rollout_of):
    """One launch of the rollout `rollout_of(state)` on `sample_inputs` -> (state before, state after, pool, noise, outputs)."""
    state, pool, noise = sample_inputs(smp, env, N, T, seed, noise)
    before = {k: v.clone() for k, v in state.items()}
    out = {k: v.clone() for k, v in rollout_of(state).run(state, pool, noise).items()}
    return before, state, pool, noise, out


def check_sample_books(before, state, pool, out, acc):
    """Carry-over, resets, the final state, time_limited and end, bit for bit against the host restatement of `done`."""
    T, N = out["rew"].shape
    done = out["done"].cpu().numpy()
    want = restate_sample_books(done, before["t"].cpu().numpy(), before["reset_count"].cpu().numpy(), MAX_STEPS, R)
    assert np.array_equal(out["time_limited"].cpu().numpy(), want["time_limited"])
    assert np.array_equal(out["end"].cpu().numpy(), want["end"])
    assert np.array_equal(state["t"].cpu().numpy(), want["t"]) and np.array_equal(state["reset_count"].cpu().numpy(), want["reset_count"])
    src = torch.from_numpy(want["src"]).to(out["obs"].device)
    cols = torch.arange(N, device=src.device)
    nxt = {"obs": "obs2", "state": "next_state", "ref_points": "next_ref_points", "ref_time": "next_ref_time", "path_num": "path_num",
           "u_num": "u_num"}
    for k in ["obs"] + [k for k in INFO if k in out]:
        assert torch.equal(out[k][0], before[k]), k
        for t in range(T):
            reset = src[t] >= 0
            fresh = pool[k][src[t].clamp_min(0), cols]
            mask = reset.reshape((N,) + (1,) * (fresh.dim() - 1))
            want_row = torch.where(mask, fresh, out[nxt[k]][t])
            got_row = out[k][t + 1] if t + 1 < T else state[k]
            assert torch.equal(got_row, want_row), (k, t)
        if k in ("path_num", "u_num"):
            assert torch.equal(out["next_" + k], out[k])
    over = want["src"] >= 0
    acc["done_resets"] += int((over & (done != 0)).sum())
    acc["limit_resets"] += int((over & (done == 0)).sum())
    acc["continues"] += int((~over).sum())
    acc["most_resets"] = max(acc["most_resets"], int(over.sum(axis=0).max()))


# ---- the evaluator ------------------------------------------------------------------------------------------------------------
def make_evaluator(env, networks, T, env_model=None, **kw):
    """The device evaluator of `networks` on the data env `env`; `kw`: what differs between the families - num_eval_episode, seed,
    device, action_table, stochastic_mode."""
    cfg = dict(CFGS[env])
    return Evaluator(env_model=env_model or create_env_model(**cfg), networks=networks, cfg=cfg, eval_save=False, max_episode_steps=T, **kw)


def stocha_evaluator(env, hidden, dist, *, seed=0, T=12, device="cuda", nets=None, dist_cls=None, **extra):
    """(evaluator, networks) of a StochaPolicy with the action distribution `dist` (a key of DISTS; or the class `dist_cls`) on the
    data env `env`; `nets`: the container of an earlier call instead of a new one."""
    if nets is None:
        cfg = CFGS[env]
        torch.manual_seed(seed)
        A = act_dim_of(cfg)
        low, high = LIMITS[A]
        nets = Nets(StochaPolicy(obs_dim=obs_dim_of(cfg), act_dim=A, hidden_sizes=list(hidden), hidden_activation="relu", min_log_std=-20,
                                 max_log_std=0.5, act_high_lim=np.array(high, np.float32), act_low_lim=np.array(low, np.float32),
                                 action_distribution_cls=dist_cls or DISTS[dist])).to(device)
    return make_evaluator(env, nets, T, num_eval_episode=5, seed=seed, device=device, **extra), nets


def deviations(res, obs, rew_ret, length):
    """Largest deviation of a run from a record: the return against max(1, |return|), the observations of every recorded step
    against max(1, the record's largest |observation|)."""
    E, T = obs.shape[:2]
    inside = (np.arange(T)[None, :] < length[:, None])[:, :, None]
    got = res["trace_obs"].cpu().numpy()
    d_obs = float((np.abs(got - obs) * inside).max() / max(1.0, float((np.abs(obs) * inside).max())))
    d_ret = float((np.abs(res["ret"].double().cpu().numpy() - rew_ret) / np.maximum(1.0, np.abs(rew_ret))).max())
    return d_ret, d_obs
