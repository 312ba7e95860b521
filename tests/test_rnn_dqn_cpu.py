"""CPU-only checks of DQN on recurrent networks: the ABI of gops_rnn_dqn_step, the codes it refuses with before any HIP call, and
create_alg building DQN on rnn.ActionValueDis or saying why not."""
import ctypes as C

import pytest

from dqn_helpers import dqn_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x1000   # a non-null, 8-byte aligned pointer: every call below is refused before anything reads it
TENSORS = ("obs", "obs2", "act", "rew", "done", "weight", "q_all", "backup", "a_star", "seed", "abs_err", "stats")


def test_abi_of_the_rnn_dqn_entry_points(tmp_path):
    from abi_helpers import check_abi
    check_abi(tmp_path, [("GopsRnnDqn", hb.GopsRnnDqn)], ("gops_rnn_dqn_step_workspace_bytes", "gops_rnn_dqn_step"))


def _net(seq_len=5, obs_dim=4, hidden=16, n_heads=1, dtype=0, out=2):
    r = hb.GopsRnn()
    r.seq_len, r.obs_dim, r.hidden, r.n_heads = seq_len, obs_dim, hidden, n_heads
    for name in hb.RNN_PARAMS:
        setattr(r, name, FAKE)
    for h in range(hb.RNN_MAX_HEADS):
        m = r.head[h]
        m.n_layers, m.hidden_act, m.dtype = 2, hb.ACT_IDS["tanh"], dtype
        m.sizes[0], m.sizes[1], m.sizes[2] = hidden, 32, out
        for l in range(2):
            m.weight[l] = m.bias[l] = FAKE
    return r


@pytest.mark.parametrize("online, target, call, code", [
    (dict(), dict(), dict(obs=None), BAD_ARG), (dict(), dict(), dict(a_star=None), BAD_ARG), (dict(), dict(), dict(stats=None), BAD_ARG),
    (dict(), dict(), dict(target=None), BAD_ARG), (dict(), dict(), dict(desc=None), BAD_ARG), (dict(), dict(), dict(batch=0), BAD_ARG),
    (dict(n_heads=2), dict(), dict(), BAD_ARG), (dict(), dict(n_heads=2), dict(), BAD_ARG),
    (dict(), dict(seq_len=4), dict(), UNSUPPORTED), (dict(), dict(obs_dim=5), dict(), UNSUPPORTED), (dict(hidden=32), dict(), dict(), UNSUPPORTED),
    (dict(out=3), dict(), dict(), UNSUPPORTED), (dict(out=1), dict(out=1), dict(act_num=1), UNSUPPORTED),
    (dict(out=17), dict(out=17), dict(act_num=17), UNSUPPORTED), (dict(), dict(), dict(act_num=3), UNSUPPORTED),
    (dict(hidden=24), dict(hidden=24), dict(), UNSUPPORTED), (dict(seq_len=33), dict(seq_len=33), dict(), UNSUPPORTED),
    (dict(dtype=1), dict(dtype=1), dict(), UNSUPPORTED), (dict(), dict(), dict(rnn_ws=None), WORKSPACE),
    (dict(), dict(), dict(rnn_bytes=64), WORKSPACE), (dict(), dict(), dict(ws=None), WORKSPACE), (dict(), dict(), dict(nbytes=64), WORKSPACE)])
def test_refusals_come_before_any_hip_call(online, target, call, code):
    """No device: every code is returned from the host checks.  `weight` alone may be NULL; a refused pair has no workspace."""
    lib, q, t, d = hb.lib(), _net(**online), _net(**target), hb.GopsRnnDqn()
    d.act_num, d.reward_scale, d.gamma = call.get("act_num", 2), 1.0, 0.99
    a = dict(dict(online=C.byref(q), target=C.byref(t), desc=C.byref(d), batch=17, rnn_ws=FAKE, rnn_bytes=1 << 30, ws=FAKE, nbytes=1 << 20),
             **dict.fromkeys(TENSORS, FAKE))
    a.update(weight=None, **call)
    assert lib.gops_rnn_dqn_step(a["online"], a["target"], a["desc"], a["batch"], *(a[k] for k in TENSORS), a["rnn_ws"], a["rnn_bytes"],
                                 a["ws"], a["nbytes"], None) == code
    described = not online and not target and all(a[k] is not None for k in ("target", "desc")) and a["batch"] > 0 and "act_num" not in call
    assert (lib.gops_rnn_dqn_step_workspace_bytes(a["online"], a["target"], a["desc"], a["batch"]) > 0) == described


def rnn_dqn_kwargs(**over):
    return dqn_kwargs((5, 4), 2, [16, 32], "tanh", **dict(dict(value_func_type="RNN", env_id="gym_cartpolecontiwithstack"), **over))


def test_create_alg_builds_dqn_on_the_recurrent_action_values():
    from gops_amd.apprfunc import rnn
    nets = create_alg(**rnn_dqn_kwargs()).networks
    assert type(nets.q) is rnn.ActionValueDis and type(nets.q_target) is rnn.ActionValueDis and nets.q.act_num == 2
    assert len(list(nets.q.parameters())) == 8 and not any(p.requires_grad for p in nets.q_target.parameters())


@pytest.mark.parametrize("over, reason", [(dict(obsv_dim=4), r"pair \(L, O\)"), (dict(obsv_dim=(33, 4)), "L in 1 .. 32"),
                                          (dict(value_hidden_sizes=[24]), "multiple of 16 in 16 .. 128"),
                                          (dict(action_num=17), "2 .. 16 discrete actions")])
def test_create_alg_refusals_carry_the_reason(over, reason):
    with pytest.raises(NotImplementedError, match=reason):
        create_alg(**rnn_dqn_kwargs(**over))
