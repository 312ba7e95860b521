"""The host side of gops_stack_sample_rollout / gops_stack_episode_rollout: ABI, every refusal code before any HIP call, the reset pool."""
import ctypes as C

import numpy as np
import pytest
import torch

import stack_helpers as sh
from abi_helpers import check_abi

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.trainer.sampler.reset_pool import draw_reset_pool

ENTRY_POINTS = ("gops_stack_sample_workspace_bytes", "gops_stack_sample_rollout", "gops_stack_episode_workspace_bytes",
                "gops_stack_episode_rollout")
BAD, UNSUPPORTED, WORKSPACE = -1, -2, -3
PTR = 0x1000   # non-null: a refusal reads no memory


def test_abi_of_the_stack_entry_points(tmp_path):
    """No new struct: the entry points reuse GopsRnn and the sample / episode structs."""
    check_abi(tmp_path, [("GopsRnn", hb.GopsRnn), ("GopsSampleDesc", hb.GopsSampleDesc), ("GopsSampleState", hb.GopsSampleState),
                         ("GopsSamplePool", hb.GopsSamplePool), ("GopsSampleOut", hb.GopsSampleOut), ("GopsEpisodeOut", hb.GopsEpisodeOut)],
              ENTRY_POINTS)
    assert hb.STACK_MAX_LEN == 8


def _description(L=5, heads=2, kind=hb.ENV_CARTPOLE, data_env=1):
    env = hb.make_env(kind, 4, 1, act_low=[-1.0], act_high=[1.0], data_env=bool(data_env))
    rnn = hb.GopsRnn(seq_len=L, obs_dim=4, hidden=16, n_heads=heads, weight_ih=PTR, weight_hh=PTR, bias_ih=PTR, bias_hh=PTR)
    for h in range(min(heads, hb.RNN_MAX_HEADS)):
        m = rnn.head[h]
        m.n_layers, m.hidden_act = 2, hb.ACT_IDS["tanh"]
        m.sizes[0], m.sizes[1], m.sizes[2] = 16, 16, 1
        for l in range(2):
            m.weight[l] = m.bias[l] = PTR
    return env, rnn


# (knobs of the description, what is left NULL, workspace bytes handed in) -> the code of both families
REFUSALS = [(dict(L=9), None, 256, UNSUPPORTED), (dict(kind=hb.ENV_LQ), None, 256, UNSUPPORTED), (dict(data_env=0), None, 256, BAD),
            (dict(heads=1), None, 256, BAD), (dict(heads=3), None, 256, BAD), (dict(), "env", 256, BAD), (dict(), "policy", 256, BAD),
            (dict(), "io", 256, BAD), (dict(), "out", 256, BAD), (dict(), None, 255, WORKSPACE)]


@pytest.mark.parametrize("knobs, null, ws_bytes, code", REFUSALS, ids=lambda v: str(v).replace(" ", ""))
def test_refusal_codes_before_any_hip_call(knobs, null, ws_bytes, code):
    env, rnn = _description(**knobs)
    desc = hb.GopsSampleDesc(head=hb.SAMPLE_GAUSS, max_episode_steps=200, pool_rows=2, min_log_std=-20.0, max_log_std=2.0)
    st, pool = hb.GopsSampleState(obs=PTR, t=PTR, reset_count=PTR), hb.GopsSamplePool(obs=PTR)
    sout = hb.GopsSampleOut(**{k: PTR for k in ("obs", "act", "rew", "done", "obs2", "logp", "time_limited", "end")})
    eout = hb.GopsEpisodeOut(ret=PTR, length=PTR, terminated=PTR)
    e, p = (None if null == "env" else C.byref(env)), (None if null == "policy" else C.byref(rnn))
    lib = hb.lib()
    assert lib.gops_stack_sample_rollout(e, p, C.byref(desc), 17, 3, None if null == "io" else C.byref(st), C.byref(pool), PTR,
                                         None if null == "out" else C.byref(sout), PTR, ws_bytes, None) == code
    assert lib.gops_stack_episode_rollout(e, p, 17, 3, None if null == "io" else PTR, None if null == "out" else C.byref(eout), PTR,
                                          ws_bytes, None) == code
    for query in (lib.gops_stack_sample_workspace_bytes, lib.gops_stack_episode_workspace_bytes):   # 0: the description is refused
        assert query(e, p, 17, 3) == (0 if knobs or null in ("env", "policy") else 256)


def test_reset_pool_and_description_of_the_stacked_env():
    """reset(): uniform in +-[2, 0.05, 0.2, 0.05], one state per instance; obsv_dim (5, 4) by default, the stack length up to 8; the env
    model's own step is refused (the reference has no model of this env)."""
    model = create_env_model("gym_cartpolecontiwithstack")
    pool = draw_reset_pool(dict(env_id="gym_cartpolecontiwithstack"), model, 3, 4096, "cpu")["obs"].numpy()
    assert pool.shape == (4096, 4) and (np.abs(pool) <= sh.RESET_HALF_RANGE).all() and (np.abs(pool).max(axis=0) > 0.99 * sh.RESET_HALF_RANGE).all()
    assert model.obsv_dim == (5, 4) and create_env_model("gym_cartpolecontiwithstack", stack_length=8).obsv_dim == (8, 4)
    with pytest.raises(RuntimeError, match="stack_length"):
        create_env_model("gym_cartpolecontiwithstack", stack_length=9)
    with pytest.raises(RuntimeError, match="no env model"):
        model.forward(torch.zeros(1, 4), torch.zeros(1, 1), torch.zeros(1), {})


def test_restated_step_against_gym_cartpoleconti_physics():
    """The float64 restatement the GPU tests use: force 30 a, Euler step of 20 ms, done on the next state - one hand-computed step."""
    xn, done = sh.step64(np.array([0.0, 0.0, 0.0, 0.0]), 1.0)
    temp = 30.0 / 1.1
    thacc = -temp / (0.5 * (4.0 / 3.0 - 0.1 / 1.1))
    assert np.allclose(xn, [0.0, 0.02 * (temp - 0.05 * thacc / 1.1), 0.0, 0.02 * thacc], rtol=1e-15, atol=0) and not done
    assert sh.step64(np.array([0.0, 0.0, 0.2, 0.5]), 0.0)[1] and sh.step64(np.array([2.39, 1.0, 0.0, 0.0]), 0.0)[1]
