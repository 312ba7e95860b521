"""`gops_episode_rollout_mode` (csrc/rollout_episode.hip) and `Evaluator(stochastic_mode=True)` without a device: the ABI surface, the
refusal codes - every call below is refused by an argument check before the library makes any HIP call; a description that passes
every check carries a null workspace and is refused with GOPS_ERR_WORKSPACE -, the old entry points' codes for the same description
(read from tests/golden/closed_loop_refusals.json) and the host layer's keyword."""
import ctypes as C
import json
import os
import re

import pytest

from closed_loop_helpers import alg_kwargs, stocha_evaluator
from desc_helpers import BAD, UNS, WS, env_desc, mlp_desc, ptr_struct as _ptrs

from gops_amd import hip_backend as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS, TANH_GAUSS = hb.SAMPLE_GAUSS, hb.SAMPLE_TANH_GAUSS


def _mlp(sizes, dtype=0):
    return mlp_desc(sizes, dtype=dtype)


def _env(kind=hb.ENV_CARTPOLE, O=4, A=1, data_env=1):
    return env_desc(kind, O, A, data_env=data_env)


def _rollout(env=True, pol=True, head=TANH_GAUSS, E=4, init=True, out_w=2, dtype=0, env_desc=None, in_w=4):
    """gops_episode_rollout_mode on the base description (gym_cartpoleconti as a data env, a 4-16-2 stack, A = 1, a null
    workspace) with the knobs given; `env` / `pol` / `init` False: a null pointer."""
    e, m = env_desc or _env(), _mlp([in_w, 16, out_w], dtype)
    return hb.lib().gops_episode_rollout_mode(C.byref(e) if env else None, C.byref(m) if pol else None, head, E, 8,
                                              C.byref(_ptrs(hb.GopsStepIO)) if init else None, C.byref(_ptrs(hb.GopsEpisodeOut)), None, 0, None)


def _query(head=TANH_GAUSS, E=4, out_w=2, dtype=0, env_desc=None, in_w=4):
    e, m = env_desc or _env(), _mlp([in_w, 16, out_w], dtype)
    return hb.lib().gops_episode_mode_workspace_bytes(C.byref(e), C.byref(m), head, E, 8)


def test_entry_points_are_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    assert "#define GOPS_HIP_ABI_VERSION 15" in header
    assert re.search(r"size_t gops_episode_mode_workspace_bytes\(const GopsEnv\* env, const GopsMlp\* policy, int32_t head, "
                     r"int32_t episodes, int32_t max_steps\);", header)
    assert re.search(r"int gops_episode_rollout_mode\(const GopsEnv\* env, const GopsMlp\* policy, int32_t head, int32_t episodes, "
                     r"int32_t max_steps,\s+const GopsStepIO\* init, const GopsEpisodeOut\* out, void\* workspace, size_t workspace_bytes, "
                     r"void\* stream\);", header)
    assert {"gops_episode_mode_workspace_bytes", "gops_episode_rollout_mode"} <= set(hb.EXPORTED_SYMBOLS)
    lib = C.CDLL(hb.LIB_PATH)
    assert hasattr(lib, "gops_episode_mode_workspace_bytes") and hasattr(lib, "gops_episode_rollout_mode")
    assert hb.lib().gops_hip_version() == 15


@pytest.mark.parametrize("head", [GAUSS, TANH_GAUSS])
def test_the_base_description_passes_every_check_but_the_workspace(head):
    assert _rollout(head=head) == WS
    assert _query(head=head) > 0


REFUSED = {
    "width-A": (dict(out_w=1), BAD), "width-3": (dict(out_w=3), BAD),
    "head-determ": (dict(head=hb.SAMPLE_DETERM), BAD), "head-7": (dict(head=7), BAD), "head-negative": (dict(head=-1), BAD),
    "fp16": (dict(dtype=1), UNS),
    "env-model": (dict(env_desc=_env(data_env=0)), BAD),
    "mobilerobot": (dict(env_desc=_env(hb.ENV_MOBILEROBOT, 13, 2), in_w=13, out_w=4), UNS),
    "episodes0": (dict(E=0), BAD),
}


@pytest.mark.parametrize("fault", sorted(REFUSED))
def test_refusal_codes(fault):
    knobs, code = REFUSED[fault]
    assert _rollout(**knobs) == code
    assert _query(**knobs) == 0   # the query of a refused description: no such workspace


def test_the_refusals_of_gops_episode_rollout_hold_here():
    """ActionRepeat, a constrained model, a hidden width off the tile: the codes `gops_episode_rollout` has for them (recorded)."""
    with open(os.path.join(ROOT, "tests", "golden", "closed_loop_refusals.json")) as f:
        want = json.load(f)["gops_episode_rollout"]["single"]
    e = _env()
    e.repeat_num = 2
    assert _rollout(env_desc=e) == want["repeat2"] == UNS
    e = _env()
    e.cstr_err = 1
    assert _rollout(env_desc=e) == want["cstr_err"] == UNS
    m = _mlp([4, 24, 2])
    assert hb.lib().gops_episode_rollout_mode(C.byref(_env()), C.byref(m), GAUSS, 4, 8, C.byref(_ptrs(hb.GopsStepIO)),
                                              C.byref(_ptrs(hb.GopsEpisodeOut)), None, 0, None) == want["hidden-24"] == UNS


@pytest.mark.parametrize("what", ["env", "pol", "init"])
def test_null_pointers(what):
    assert _rollout(**{what: False}) == BAD


def test_a_null_workspace_is_the_last_check():
    """Wrong twice - a null init and a null workspace: the code of the first."""
    assert _rollout(init=False) == BAD and _rollout() == WS
    io = _ptrs(hb.GopsStepIO)
    io.obs = None
    e, m = _env(), _mlp([4, 16, 2])
    assert hb.lib().gops_episode_rollout_mode(C.byref(e), C.byref(m), GAUSS, 4, 8, C.byref(io), C.byref(_ptrs(hb.GopsEpisodeOut)), None, 0,
                                              None) == BAD


def test_the_old_entry_points_keep_refusing_the_stochastic_stack():
    """The 4-16-2 description through `gops_episode_rollout` and its query: the codes recorded for `output-double`."""
    with open(os.path.join(ROOT, "tests", "golden", "closed_loop_refusals.json")) as f:
        golden = json.load(f)
    e, m = _env(), _mlp([4, 16, 2])
    got = hb.lib().gops_episode_rollout(C.byref(e), C.byref(m), 4, 2, C.byref(_ptrs(hb.GopsStepIO)), C.byref(_ptrs(hb.GopsEpisodeOut)), None, 0, None)
    assert got == golden["gops_episode_rollout"]["single"]["output-double"] and got in (BAD, UNS)
    assert hb.lib().gops_episode_workspace_bytes(C.byref(e), C.byref(m), 4, 2) == golden["gops_episode_workspace_bytes"]["single"]["output-double"] == 0


def test_stochastic_mode_needs_a_stochastic_policy():
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    cfg, kw = alg_kwargs("cartpole", "relu64", use_gpu=False)
    kw.update(num_eval_episode=2, eval_save=False, save_folder=None, is_render=False)
    assert create_evaluator(**kw).stochastic_mode is False
    with pytest.raises(ValueError, match="stochastic_mode"):
        create_evaluator(**dict(kw, stochastic_mode=True))


def test_stochastic_mode_goes_with_no_action_table():
    import torch
    from gops_amd.apprfunc.mlp import StochaPolicyDis
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.evaluator import Evaluator
    from gops_amd.utils.act_distribution import CategoricalDistribution

    class DisNets(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.policy = StochaPolicyDis(obs_dim=4, act_num=2, hidden_sizes=[16], hidden_activation="relu",
                                          action_distribution_cls=CategoricalDistribution)

    cfg = dict(env_id="gym_cartpoleconti")
    make = lambda **kw: Evaluator(env_model=create_env_model(**cfg), networks=DisNets(), cfg=cfg, num_eval_episode=2, eval_save=False,  # noqa: E731
                                  action_table=[[-1.0], [1.0]], device="cpu", **kw)
    assert make().stochastic_mode is False
    with pytest.raises(ValueError, match="stochastic_mode"):
        make(stochastic_mode=True)
    ev, _ = stocha_evaluator("cartpole", (16,), "gauss", device="cpu")
    with pytest.raises(ValueError):   # (a table behind a StochaPolicy is refused for the table already)
        type(ev)(env_model=ev.env_model, networks=ev.networks, cfg=ev.cfg, num_eval_episode=2, eval_save=False, action_table=[[-1.0], [1.0]],
                 device="cpu", stochastic_mode=True)


def test_the_default_keyword_keeps_the_loop_and_its_reason():
    ev, _ = stocha_evaluator("cartpole", (16,), "tanh_gauss", device="cpu")
    assert ev.stochastic_mode is False and ev.kernel_refuses() == "stochastic policy"


@pytest.mark.parametrize("dist, head", [("gauss", GAUSS), ("tanh_gauss", TANH_GAUSS)])
def test_the_head_follows_the_action_distribution(dist, head):
    ev, _ = stocha_evaluator("cartpole", (16,), dist, device="cpu", stochastic_mode=True)
    assert ev._mode_head() == (head, None)   # (the description itself needs device tensors: tests/test_episode_mode_gpu.py)


def test_other_distributions_and_log_stds_stay_on_the_loop():
    from gops_amd.utils.act_distribution import TanhGaussDistribution

    class Other(TanhGaussDistribution):   # a subclass may state another mode: it is not taken for its parent
        pass

    ev, nets = stocha_evaluator("cartpole", (16,), None, device="cpu", stochastic_mode=True, dist_cls=Other)
    assert ev._mode_head()[0] is None and "Other" in ev.kernel_refuses()
    ev, nets = stocha_evaluator("cartpole", (16,), "gauss", device="cpu", stochastic_mode=True)
    nets.policy.std_type = "parameter"
    why = ev.kernel_refuses()
    assert "log std" in why and "parameter" in why
