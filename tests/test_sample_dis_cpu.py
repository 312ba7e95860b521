"""The discrete heads of the one-launch sampler and evaluator without a GPU: the C ABI of `gops_sample_rollout_dis` and
`gops_episode_rollout_dis`, their refusal codes (every refusal is an argument check in the entry point, before any HIP call: the
pointers are never followed), the host restatement `reset_pool.restate_discrete_head`, and the path choice of the sampler and the
evaluator on `device="cpu"`."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_helpers import check_abi
from closed_loop_helpers import Nets as _Nets
from desc_helpers import BAD, UNS, WS, P, mlp_desc, ptr_struct

from gops_amd import hip_backend as hb
from gops_amd.trainer.sampler.reset_pool import HEAD_CATEGORICAL, HEAD_EPS_GREEDY, restate_discrete_head


def test_abi_of_the_discrete_entry_points(tmp_path):
    check_abi(tmp_path, [("GopsSampleDis", hb.GopsSampleDis), ("GopsSampleDesc", hb.GopsSampleDesc), ("GopsSampleOut", hb.GopsSampleOut),
                         ("GopsEpisodeOut", hb.GopsEpisodeOut)],
              ("gops_sample_dis_workspace_bytes", "gops_sample_rollout_dis", "gops_episode_dis_workspace_bytes", "gops_episode_rollout_dis"),
              [("GOPS_SAMPLE_EPS_GREEDY", hb.SAMPLE_EPS_GREEDY), ("GOPS_SAMPLE_CATEGORICAL", hb.SAMPLE_CATEGORICAL),
               ("GOPS_SAMPLE_TANH_GAUSS", hb.SAMPLE_TANH_GAUSS), ("GOPS_DQN_MAX_ACTIONS", hb.DQN_MAX_ACTIONS)])
    assert [f[0] for f in hb.GopsSampleDis._fields_] == ["action_table", "act_num", "head", "epsilon", "env_act"]
    assert hb.SAMPLE_EPS_GREEDY > hb.SAMPLE_TANH_GAUSS and hb.SAMPLE_CATEGORICAL > hb.SAMPLE_TANH_GAUSS   # gops_sample_rollout refuses both
    assert (HEAD_EPS_GREEDY, HEAD_CATEGORICAL) == (hb.SAMPLE_EPS_GREEDY, hb.SAMPLE_CATEGORICAL)
    assert hb.lib().gops_hip_version() == 15


# ---- refusal codes ------------------------------------------------------------------------------------------------------------
def _env(env_id="gym_cartpoleconti", data_env=True, **cfg):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.utils.synthetic import act_dim_of
    model = create_env_model(env_id=env_id, **cfg)
    A = act_dim_of(dict(env_id=env_id, **cfg))
    return hb.GopsEnv.from_buffer_copy(model.hip_env(-np.ones(A, np.float32), np.ones(A, np.float32), data_env=data_env))


def _mlp(sizes, **fields):
    return mlp_desc(sizes, act=hb.ACT_IDS["relu"], **fields)


def _sample_call(env=None, mlp=None, n=3, head=None, eps=0.25, table=P, env_act=P, N=4, T=2, pool_rows=2, max_steps=3, noise=P, out_act=P,
                 ws=P, ws_bytes=hb.SAMPLE_WORKSPACE_BYTES, dis=True):
    env = _env() if env is None else env
    mlp = _mlp([env.obs_dim, 16, n]) if mlp is None else mlp
    desc = hb.GopsSampleDesc(head=0, max_episode_steps=max_steps, pool_rows=pool_rows)
    d = hb.GopsSampleDis(action_table=table, act_num=n, head=hb.SAMPLE_EPS_GREEDY if head is None else head, epsilon=eps, env_act=env_act)
    st, pl, out = ptr_struct(hb.GopsSampleState), ptr_struct(hb.GopsSamplePool), ptr_struct(hb.GopsSampleOut, act=out_act)
    return hb.lib().gops_sample_rollout_dis(C.byref(env), C.byref(mlp), C.byref(desc), C.byref(d) if dis else None, N, T, C.byref(st),
                                            C.byref(pl), noise, C.byref(out), ws, ws_bytes, None)


def test_refusal_codes_of_the_sample_entry_point():
    cat = hb.SAMPLE_CATEGORICAL
    # GOPS_ERR_UNSUPPORTED: act_num out of range, and what sample_check refuses
    assert _sample_call(n=1) == UNS
    assert _sample_call(n=hb.DQN_MAX_ACTIONS + 1) == UNS
    assert _sample_call(mlp=_mlp([4, 24, 3])) == UNS                    # a hidden width that is no multiple of 16
    assert _sample_call(mlp=_mlp([4, 3])) == UNS                        # a POLY net (one layer)
    assert _sample_call(mlp=_mlp([5, 16, 3])) == UNS                    # a time-augmented policy
    assert _sample_call(env=_env(data_env=False)) == UNS                # cartpole has no env-model path in the sampler
    assert _sample_call(env=_env("pyth_mobilerobot"), mlp=_mlp([13, 16, 3])) == UNS
    # GOPS_ERR_BAD_ARG
    assert _sample_call(table=None) == BAD
    assert _sample_call(env_act=None) == BAD
    assert _sample_call(head=5) == BAD and _sample_call(head=hb.SAMPLE_TANH_GAUSS) == BAD and _sample_call(head=hb.SAMPLE_DETERM) == BAD
    assert _sample_call(mlp=_mlp([4, 16, 2]), n=3) == BAD               # output width other than act_num
    assert _sample_call(mlp=_mlp([4, 16, 6]), n=3) == BAD               # (also 2 x act_num)
    assert _sample_call(eps=-0.01) == BAD and _sample_call(eps=1.01) == BAD and _sample_call(eps=float("nan")) == BAD
    assert _sample_call(head=cat, eps=0.25) == BAD                      # epsilon with the categorical head
    # .. the existing cases
    assert _sample_call(dis=False) == BAD and _sample_call(N=0) == BAD and _sample_call(T=0) == BAD
    assert _sample_call(pool_rows=0) == BAD and _sample_call(max_steps=0) == BAD
    assert _sample_call(noise=None) == BAD and _sample_call(out_act=None) == BAD
    # the workspace is asked for last: everything before it passed for these descriptions
    for kw in (dict(), dict(eps=0.0), dict(eps=1.0), dict(head=cat, eps=0.0), dict(n=2), dict(n=hb.DQN_MAX_ACTIONS)):
        assert _sample_call(ws=None, **kw) == WS and _sample_call(ws_bytes=8, **kw) == WS, kw


def _episode_call(env=None, mlp=None, n=3, table=P, E=4, T=5, init_obs=P, ws=None, ws_bytes=0):
    env = _env() if env is None else env
    mlp = _mlp([env.obs_dim, 16, n]) if mlp is None else mlp
    io, out = hb.GopsStepIO(), hb.GopsEpisodeOut()
    io.obs = init_obs
    out.ret = out.length = out.terminated = P
    return hb.lib().gops_episode_rollout_dis(C.byref(env), C.byref(mlp), table, n, E, T, C.byref(io), C.byref(out), ws, ws_bytes, None)


def test_refusal_codes_of_the_episode_entry_point():
    assert _episode_call(n=1) == UNS and _episode_call(n=hb.DQN_MAX_ACTIONS + 1) == UNS
    assert _episode_call(mlp=_mlp([4, 24, 3])) == UNS and _episode_call(mlp=_mlp([4, 3])) == UNS
    assert _episode_call(env=_env("pyth_mobilerobot"), mlp=_mlp([13, 16, 3])) == UNS
    assert _episode_call(table=None) == BAD
    assert _episode_call(mlp=_mlp([4, 16, 2]), n=3) == BAD              # output width other than act_num
    assert _episode_call(env=_env(data_env=False)) == BAD              # evaluation steps the data env
    assert _episode_call(E=0) == BAD and _episode_call(T=0) == BAD and _episode_call(init_obs=None) == BAD
    for n in (2, 3, hb.DQN_MAX_ACTIONS):
        assert _episode_call(n=n) == WS and _episode_call(n=n, ws=P, ws_bytes=8) == WS


def test_workspace_queries():
    lib, env = hb.lib(), _env()
    for n in (2, 3, 5, 16):
        m = _mlp([4, 64, 64, n])
        assert lib.gops_sample_dis_workspace_bytes(C.byref(env), C.byref(m), n, 70, 5) == hb.SAMPLE_WORKSPACE_BYTES
        assert lib.gops_episode_dis_workspace_bytes(C.byref(env), C.byref(m), n, 40, 12) == \
            lib.gops_episode_workspace_bytes(C.byref(env), C.byref(_mlp([4, 64, 64, 1])), 40, 12) > 0
        assert lib.gops_sample_dis_workspace_bytes(C.byref(env), C.byref(m), n + 1, 70, 5) == 0
        assert lib.gops_episode_dis_workspace_bytes(C.byref(env), C.byref(m), n + 1, 40, 12) == 0
    # the existing queries still refuse a table-shaped policy: three values for one action dimension are neither A nor 2A
    m3 = _mlp([4, 16, 3])
    assert lib.gops_sample_workspace_bytes(C.byref(env), C.byref(m3), 4, 2) == 0
    assert lib.gops_episode_workspace_bytes(C.byref(env), C.byref(m3), 4, 2) == 0
    assert lib.gops_sample_dis_workspace_bytes(C.byref(env), C.byref(m3), 1, 4, 2) == 0
    assert lib.gops_sample_dis_workspace_bytes(C.byref(env), C.byref(m3), 17, 4, 2) == 0


# ---- the host restatement -----------------------------------------------------------------------------------------------------
def test_restated_epsilon_greedy():
    values = np.array([[0.0, 2.0, 2.0, -1.0], [3.0, 3.0, 3.0, 3.0], [-1.0, -2.0, -0.5, -0.5]])
    u = np.array([[0.9, 0.99], [0.0, 0.5], [0.3, 0.26]])
    idx, logp = restate_discrete_head(values, u, HEAD_EPS_GREEDY, 0.0)
    assert idx.tolist() == [1, 0, 2] and idx.dtype == np.int64 and not logp.any()   # first-index ties
    rng = np.random.RandomState(0)
    y, uu = rng.randn(4096, 5), rng.uniform(size=(4096, 2))
    idx, logp = restate_discrete_head(y, uu, HEAD_EPS_GREEDY, 1.0)
    assert np.array_equal(idx, np.floor(uu[:, 1] * 5).astype(np.int64)) and not logp.any()
    idx, _ = restate_discrete_head(y, uu, HEAD_EPS_GREEDY, 0.25)
    explore = uu[:, 0] < 0.25
    assert np.array_equal(idx[~explore], np.argmax(y, axis=1)[~explore]) and np.array_equal(idx[explore], np.floor(uu[explore, 1] * 5))
    top = np.array([[0.0, 1.0]]), np.array([[0.0, np.nextafter(1.0, 0.0)]])
    assert restate_discrete_head(*top, HEAD_EPS_GREEDY, 1.0)[0].tolist() == [1]   # floor(u1 n) never reaches n


def test_restated_categorical():
    rng = np.random.RandomState(1)
    logits = np.array([0.3, -1.2, 2.0, 0.0, 1.1])
    p = np.exp(logits) / np.exp(logits).sum()
    u = rng.uniform(size=(4096, 2))
    idx, logp = restate_discrete_head(np.tile(logits, (4096, 1)), u, HEAD_CATEGORICAL, 0.0)
    freq = np.bincount(idx, minlength=5) / 4096.0
    sigma = np.sqrt(p * (1 - p) / 4096.0)
    assert (np.abs(freq - p) <= 5 * sigma).all(), (freq, p)
    y = rng.randn(4096, 7) * 3.0
    idx, logp = restate_discrete_head(y, u, HEAD_CATEGORICAL)
    want = torch.log_softmax(torch.from_numpy(y), dim=-1).gather(1, torch.from_numpy(idx)[:, None])[:, 0].numpy()
    assert np.abs(logp - want).max() <= 1e-12
    # the index is the inverse CDF of u0: exact boundaries on hand-made weights (z = 1, 1/2, 1/4; S = 7/4)
    y3 = np.log(np.array([[1.0, 0.5, 0.25]]))
    pick = lambda u0: int(restate_discrete_head(y3, np.array([[u0, 0.0]]), HEAD_CATEGORICAL)[0][0])   # noqa: E731
    assert [pick(0.0), pick(0.5), pick(0.58), pick(0.85), pick(0.86)] == [0, 0, 1, 1, 2]
    assert pick(np.nextafter(1.0, 0.0)) == 2 and pick(1.0) == 2   # u0 -> 1 picks the last index
    with pytest.raises(ValueError, match="epsilon"):
        restate_discrete_head(y3, np.zeros((1, 2)), HEAD_CATEGORICAL, 0.1)
    with pytest.raises(ValueError, match="head"):
        restate_discrete_head(y3, np.zeros((1, 2)), 0)


# ---- path choice on the host --------------------------------------------------------------------------------------------------
def _cpu_sampler(**kw):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    return DeviceEnvSampler(dict(env_id="gym_cartpoleconti"), create_env_model(env_id="gym_cartpoleconti"), n_envs=8, device="cpu", seed=3,
                            steps_per_sample=2, **kw)


def test_a_table_behind_a_determ_policy_stays_on_the_loop():
    from gops_amd.apprfunc.mlp import DetermPolicy
    from gops_amd.utils.act_distribution import DiracDistribution
    smp = _cpu_sampler(action_table=[[-1.0], [0.0], [1.0]], fused=True)
    smp.networks = _Nets(DetermPolicy(obs_dim=4, act_dim=3, hidden_sizes=[16], hidden_activation="relu", act_high_lim=np.ones(3, np.float32),
                                      act_low_lim=-np.ones(3, np.float32), action_distribution_cls=DiracDistribution))
    assert smp._choose_path() is False
    assert smp.path.startswith("loop: ") and "action table" in smp.path
    off = _cpu_sampler(action_table=[[-1.0], [1.0]])
    off.networks = smp.networks
    assert off._choose_path() is False and off.path == "loop: fused=False"


def _dqn_networks():
    from dqn_helpers import dqn_kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    return create_alg(**dqn_kwargs(4, 2, [32], "relu")).networks


def test_the_sampler_reads_dqns_q_network_behind_the_policy_function():
    from gops_amd.apprfunc.mlp import ActionValueDis
    smp = _cpu_sampler(action_table=[[-1.0], [1.0]], epsilon=0.25, fused=True)
    smp.networks = _dqn_networks()
    assert not isinstance(smp.networks.policy, torch.nn.Module)
    assert smp._policy_module() is smp.networks.q and isinstance(smp._policy_module(), ActionValueDis)


def test_evaluator_takes_a_dqn_container_with_a_table_only():
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.evaluator import Evaluator
    nets = _dqn_networks()
    kw = dict(env_model=create_env_model(env_id="gym_cartpoleconti"), networks=nets, cfg=dict(env_id="gym_cartpoleconti"), num_eval_episode=2,
              eval_save=False)
    ev = Evaluator(action_table=[[-1.0], [1.0]], device="cpu", **kw)
    assert ev.action_table.shape == (2, 1) and ev._policy_module() is nets.q
    henv = ev._hip_env()
    assert henv.data_env == 1 and henv.act_dim == 1
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        Evaluator(**kw)
    with pytest.raises(ValueError, match="one output per table row"):
        Evaluator(action_table=[[-1.0], [0.0], [1.0]], device="cpu", **kw)
    with pytest.raises(ValueError, match="action_table"):
        Evaluator(action_table=[-1.0, 1.0], device="cpu", **kw)


def test_create_evaluator_hands_the_table_through(monkeypatch):
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    from gops_amd.trainer import evaluator as ev_mod
    seen = {}
    monkeypatch.setattr(ev_mod, "Evaluator", lambda **kw: seen.update(kw) or "built")
    got = create_evaluator(env_model=object(), networks=object(), cfg=dict(env_id="gym_cartpoleconti"), num_eval_episode=2, eval_save=False,
                           action_table=[[-1.0], [1.0]])
    assert got == "built" and seen["action_table"] == [[-1.0], [1.0]]
    seen.clear()
    create_evaluator(env_model=object(), networks=object(), cfg=dict(env_id="gym_cartpoleconti"), num_eval_episode=2, eval_save=False)
    assert seen["action_table"] is None
