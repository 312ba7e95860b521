"""The device evaluator on the host: `create_evaluator` and its refusals, the reset-pool helper `DeviceEnvSampler` and `Evaluator`
share (the sampler's draws for a seed must not move), `TrainerBase._evaluate` with and without an `on_device` evaluator, and the C
ABI surface of `gops_episode_rollout`."""
import os
import re

import pytest
import torch

from abi_helpers import layout_probe
from closed_loop_helpers import alg_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_evaluator_builds_the_class_from_reference_style_kwargs(tmp_path):
    from gops_amd.create_pkg.create_evaluator import create_evaluator, registry
    from gops_amd.trainer.evaluator import Evaluator
    cfg, kw = alg_kwargs("idp", "relu64", seed=7, use_gpu=False)
    kw.update(evaluator_name="evaluator", num_eval_episode=5, eval_save=False, save_folder=str(tmp_path), is_render=False)
    ev = create_evaluator(**kw)
    assert isinstance(ev, Evaluator) and ev.on_device is True and "evaluator" in registry
    assert ev.num_eval_episode == 5 and ev.eval_save is False and ev.seed == 7 + 400
    assert ev.max_episode_steps == 500   # the data env's registered limit (pyth_idpendulum.py:51)
    assert ev.networks.policy.pi[0].in_features == 6 and ev.env_model.unwrapped.hip_kind == 2
    for name in ("load_state_dict", "run_an_episode", "run_n_episodes", "run_evaluation", "run_episodes"):
        assert callable(getattr(ev, name))
    # the learner's own objects are taken as they are
    ev2 = create_evaluator(**dict(kw, env_model=ev.env_model, networks=ev.networks, max_episode_steps=40))
    assert ev2.networks is ev.networks and ev2.env_model is ev.env_model and ev2.max_episode_steps == 40
    # like the reference's evaluator the description carries neither reward shaping nor action repeat
    cfg, kw2 = alg_kwargs("lq", "relu64", use_gpu=False, reward_scale=0.1, repeat_num=2)
    ev3 = create_evaluator(**dict(kw2, num_eval_episode=2, eval_save=False, save_folder=None, is_render=False))
    henv = ev3._hip_env()
    assert henv.data_env == 1 and henv.shaping == 0 and henv.repeat_num == 0 and ev3.max_episode_steps == 200


def test_create_evaluator_refusals():
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    cfg, kw = alg_kwargs("idp", "relu64", use_gpu=False)
    kw.update(num_eval_episode=2, eval_save=False, save_folder=None)
    with pytest.raises(NotImplementedError, match="render"):
        create_evaluator(**dict(kw, is_render=True))
    with pytest.raises(KeyError, match="No registered evaluator"):
        create_evaluator(evaluator_name="ray_evaluator", **kw)
    # a data env that is not restated in the step kernel: the sampler's message
    for env_id, extra in (("gym_pendulum", dict(obsv_dim=3)), ("pyth_veh2dofconti_errcstr", dict(obsv_dim=14, pre_horizon=10))):
        with pytest.raises(RuntimeError, match="is not restated in the step kernel"):
            create_evaluator(**dict(kw, env_id=env_id, is_render=False, **extra))
    from gops_amd import overlay
    assert not any("evaluator" in str(k) for k in overlay.OVERLAY)   # reference scripts keep the reference evaluator


# first reset pool (pool_factor 2 x 4 envs) of DeviceEnvSampler as the parent commit drew it: {key: (sum in float64, element 1)}
PARENT_POOLS = {
    ("veh3dof", 3): dict(obs=(265.0918698888272, 1.2924308776855469), ref_points=(5154.547278624028, -14.953723907470703),
                         ref_time=(83.65492367744446, 14.162956237792969), state=(446.41050987131894, -14.836015701293945),
                         path_num=(11.0, 2.0), u_num=(2.0, 0.0)),
    ("veh3dof", 11): dict(obs=(305.5164782050997, 1.2935481071472168), ref_points=(3845.9383342843503, 1.1525229215621948),
                          ref_time=(55.87360954284668, 0.3895048201084137), state=(319.9005044642836, 0.385997474193573),
                          path_num=(5.0, 1.0), u_num=(5.0, 1.0)),
    ("cartpole", 3): dict(obs=(-0.09863249282352626, 0.02081478200852871)),     # the +-0.05 branch
    ("cartpole", 11): dict(obs=(-0.18813492986373603, -0.04805247485637665)),
    ("idp_scaled", 3): dict(obs=(-0.18456729734316468, 0.08325912803411484)),   # ScaleObservation: obs_scale [1, 2, 2, .5, .5, .25]
    ("idp_scaled", 11): dict(obs=(-10.547143057454377, -0.1922098994255066)),
}


@pytest.mark.parametrize("case,seed", sorted(PARENT_POOLS))
def test_reset_pool_helper_keeps_the_samplers_draws(case, seed):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    from gops_amd.trainer.sampler.reset_pool import draw_reset_pool
    cfg = {"veh3dof": dict(env_id="pyth_veh3dofconti", pre_horizon=10), "cartpole": dict(env_id="gym_cartpoleconti"),
           "idp_scaled": dict(env_id="pyth_idpendulum")}[case]
    model = create_env_model(**cfg, **(dict(obs_scale=[1, 2, 2, 0.5, 0.5, 0.25]) if case == "idp_scaled" else {}))
    smp = DeviceEnvSampler(cfg, model, n_envs=4, seed=seed, device="cpu", pool_factor=2)
    want = PARENT_POOLS[(case, seed)]
    assert sorted(smp._pool) == sorted(want)
    for k, (total, second) in want.items():
        assert float(smp._pool[k].double().sum()) == total and float(smp._pool[k].reshape(-1)[1]) == second, k
    direct = draw_reset_pool(cfg, model, seed, 8, "cpu")
    assert all(torch.equal(direct[k], smp._pool[k]) for k in want)
    assert torch.equal(smp.obs, smp._pool["obs"][:4])   # the first draw is the head of the pool


class _Tensor:
    def __init__(self, log):
        self.log = log

    def cpu(self):
        self.log.append("cpu")
        return self


class _Networks:
    def __init__(self, log):
        self.log = log

    def state_dict(self):
        self.log.append("state_dict")
        return {"policy.pi.0.weight": _Tensor(self.log)}


class _StubEvaluator:
    def __init__(self, log, on_device):
        self.log = log
        if on_device:
            self.on_device = True

    def load_state_dict(self, sd):
        self.log.append("load_state_dict")

    def run_evaluation(self, iteration):
        self.log.append(("run_evaluation", iteration))
        return -3.5


@pytest.mark.parametrize("on_device", [True, False])
def test_evaluate_skips_the_state_dict_copy_for_a_device_evaluator(on_device):
    from gops_amd.trainer._common import TrainerBase
    log = []
    tr = object.__new__(TrainerBase)
    tr.evaluator, tr.networks, tr.sampler, tr.writer = _StubEvaluator(log, on_device), _Networks(log), None, None
    tr.iteration, tr.max_iteration, tr.best_tar, tr.last_eval_iteration = 1, 100, -float("inf"), 0
    tr._evaluate()
    assert tr.last_eval_iteration == 1
    if on_device:
        assert log == [("run_evaluation", 1)]
    else:
        assert log == ["state_dict", "cpu", "load_state_dict", ("run_evaluation", 1)]


def test_episode_entry_points_are_additive_in_the_abi(tmp_path):
    from gops_amd import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    assert "#define GOPS_HIP_ABI_VERSION 15" in header
    assert re.search(r"size_t gops_episode_workspace_bytes\(const GopsEnv\* env, const GopsMlp\* policy, int32_t episodes, int32_t max_steps\);", header)
    assert re.search(r"int gops_episode_rollout\(const GopsEnv\* env, const GopsMlp\* policy, int32_t episodes, int32_t max_steps, "
                     r"const GopsStepIO\* init,\s+const GopsEpisodeOut\* out, void\* workspace, size_t workspace_bytes, void\* stream\);", header)
    assert {"gops_episode_workspace_bytes", "gops_episode_rollout"} <= set(hb.EXPORTED_SYMBOLS)
    assert [f[0] for f in hb.GopsEpisodeOut._fields_] == ["ret", "length", "terminated", "trace_obs", "trace_act", "trace_rew"]
    layout_probe(tmp_path, [("GopsEpisodeOut", hb.GopsEpisodeOut)])
    makefile = open(os.path.join(ROOT, "gops_amd", "csrc", "Makefile")).read()
    assert "rollout_episode.hip" in makefile
