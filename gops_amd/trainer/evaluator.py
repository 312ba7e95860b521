"""In-process evaluator on the MI355X: the surface of the reference's `Evaluator` (gops/trainer/evaluator.py:18-95 -
`load_state_dict`, `run_an_episode`, `run_n_episodes`, `run_evaluation`, `num_eval_episode`, `eval_save`) with every episode of an
evaluation in ONE launch (`gops_episode_rollout`, csrc/rollout_episode.hip): policy, data-env step, termination, time limit and
return over the whole horizon, no host round trip per step.

The evaluator shares the learner's `networks` container (`on_device = True`: `TrainerBase._evaluate` copies no state_dict); the
kernel reads the live parameter tensors in place.  Episodes start from the data envs' reset distributions
(`sampler/reset_pool.py`, seed offset +400 as evaluator.py:28) or from explicit initial conditions (`run_episodes`).  Rewards are
the data env's own: like the reference (evaluator.py:20-25: reward_scale = None, repeat_num = None) the env description is built
without ShapingReward and ActionRepeat.

What the kernel refuses (POLY policies, pyth_mobilerobot - its obstacle noise is drawn per step -, fp16) runs the same episodes
through the per-step device loop (so do `ScaleObservation` on the vehicle families and hidden widths the kernel's LDS plan does
not hold; `Evaluator.path` names the path the last call took and why): torch `policy(obs)` + `gops_env_step(data_env)` per step, a `finished` mask kept on the device
and read back once at the end.  Env models whose data env is not restated in the step kernel raise.

Discrete action sets: with `action_table` [act_num, action_dim] the evaluated network is an ActionValueDis (DQN's `networks.q`) or a
StochaPolicyDis (discrete TRPO's `networks.policy`); every step acts with `action_table[argmax(outputs)]` - the `mode()` of both
ValueDiracDistribution and CategoricalDistribution, the lowest index among equal maxima - through `gops_episode_rollout_dis`, or the
same arg-max + table gather in the per-step loop; `trace_act` is the index, [E, T, 1].

Stochastic policies (`StochaPolicy`: SAC, DSAC, DSAC-T, PPO, TRPO) are evaluated with the `mode()` of their action distribution.  By
default they run the per-step loop (`path` = "loop: stochastic policy"); `stochastic_mode=True` takes them into the kernel through
`gops_episode_rollout_mode`: the 2A-wide stack's mean half, clamped to the policy's limits (GaussDistribution) or tanh-squashed into
them (TanhGaussDistribution).  Any other distribution class, or a log std outside the shared stack, stays on the loop.
"""
import ctypes
import os

import numpy as np
import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm.base import is_poly
from gops_amd.apprfunc.mlp import ActionValueDis, StochaPolicy, StochaPolicyDis
from gops_amd.trainer.closed_loop import ClosedLoopDriver
from gops_amd.trainer.sampler.reset_pool import INFO_KEYS, NOT_RESTATED, draw_reset_pool
from gops_amd.utils.act_distribution import GaussDistribution, TanhGaussDistribution

# TimeLimit of the data envs where create_env registers one (gops/create_pkg/create_env.py:142-148 takes the env's own
# `max_episode_steps` attribute): pyth_idpendulum.py:51, pyth_veh3dofconti.py:114, pyth_veh2dofconti.py:105,
# pyth_mobilerobot.py:30; pyth_lq: resources/lq_base.py:161 (the config's max_step).  gym_cartpoleconti registers none.
_REGISTERED_STEPS = {"pyth_idpendulum": 500, "pyth_veh3dofconti": 200, "pyth_veh2dofconti": 200, "pyth_mobilerobot": 200}


def registered_episode_steps(cfg: dict, default: int = 200) -> int:
    env_id = cfg.get("env_id", "")
    if env_id == "pyth_lq":
        from gops_amd.env.env_ocp.resources import lq_configs
        lqc = cfg.get("lq_config") or "s3a1"
        return int((lqc if isinstance(lqc, dict) else getattr(lq_configs, "config_" + lqc))["max_step"])
    return _REGISTERED_STEPS.get(env_id, default)


class Evaluator(ClosedLoopDriver):
    on_device = True   # trainers: the evaluator shares the learner's networks, no state_dict copy

    def __init__(self, index=0, *, env_model, networks, cfg: dict, num_eval_episode: int, eval_save: bool = True,
                 save_folder=None, seed: int = 0, max_episode_steps: int = None, device="cuda", fused: bool = True, action_table=None,
                 stochastic_mode: bool = False, **kwargs):
        """cfg: workload dict (env_id, pre_horizon, lq_config) as `DeviceEnvSampler` takes it; env_model: the wrapped model of
        `create_env_model`; networks: the learner's container (its `policy` is evaluated in place).  `max_episode_steps`: None =
        the data env's registered limit, else 200.  `fused=False` forces the per-step loop.  `action_table` [act_num, action_dim]:
        evaluate a discrete policy (see the module docstring); without one an ActionValueDis is refused.  `stochastic_mode=True`: a
        StochaPolicy acts by its distribution's mode inside the kernel instead of on the per-step loop."""
        self.cfg, self.env_model, self.networks = dict(cfg), env_model, networks
        self.device = torch.device(device)
        self._take_action_table(action_table)
        if self.action_table is not None:
            if not isinstance(self._policy_module(), ActionValueDis) or self._policy_module().act_num != self.action_table.shape[0]:
                raise ValueError("Evaluator: an action table needs an ActionValueDis `q` or a StochaPolicyDis `policy` with one output per "
                                 "table row")
        elif isinstance(getattr(networks, "q", None), ActionValueDis):
            raise NotImplementedError("Evaluator runs closed loops with continuous actions only: an ActionValueDis policy (DQN) emits "
                                      "action values over a discrete action set, and no action table is part of the evaluator")
        self.stochastic_mode = bool(stochastic_mode)
        if self.stochastic_mode and (self.action_table is not None or not isinstance(self._policy_module(), StochaPolicy)):
            raise ValueError("Evaluator: stochastic_mode=True evaluates a StochaPolicy by the mode of its action distribution; it goes "
                             "with neither an action table nor a deterministic policy")
        base = getattr(env_model, "unwrapped", env_model)
        if getattr(base, "ref_c", None) is not None:
            raise RuntimeError("Evaluator draws its initial states from the DEFAULT reference trajectories "
                               "(gops_amd.utils.synthetic); a model with custom path_para / u_para needs explicit initial conditions")
        if getattr(base, "hip_kind", None) not in hb.DATA_ENV_KINDS or self.cfg.get("env_id", "").endswith("errcstr"):
            raise RuntimeError(NOT_RESTATED.format(env_id=self.cfg.get("env_id")))
        self.num_eval_episode, self.eval_save, self.save_folder = int(num_eval_episode), bool(eval_save), save_folder
        self.seed = int(seed) + int(index) + 400   # evaluator.py:28
        self.max_episode_steps = int(registered_episode_steps(self.cfg) if max_episode_steps is None else max_episode_steps)
        if torch.cuda.is_available() and not next(networks.parameters()).is_cuda:   # (built from kwargs: not the learner's container)
            networks.to(self.device)
        self.fused = bool(fused)
        self.render = False
        self.print_time, self.print_iteration = 0, -1
        self._evals = 0
        self._henv, self._rollouts = None, {}
        self.last = None   # device results of the last run_episodes call

    def load_state_dict(self, state_dict):
        """The reference's surface; a trainer that knows `on_device` never calls it (the networks are shared)."""
        self.networks.load_state_dict(state_dict)

    # ---- descriptions ---------------------------------------------------------------------------
    def _hip_env(self):
        if self._henv is None:
            env = self.env_model.hip_env(*self._squash_limits(), data_env=True)
            env = hb.GopsEnv.from_buffer_copy(env)   # (the model caches its description: this one is the evaluator's own)
            env.shaping, env.reward_scale, env.reward_shift = 0, 1.0, 0.0
            env.repeat_num, env.repeat_last_reward = 0, 0
            self._henv = env
        return self._henv

    def _mode_head(self):
        """(head code of `gops_episode_rollout_mode`, None) for this evaluator's StochaPolicy, or (None, why it has none)."""
        pol = self._policy_module()
        if getattr(pol, "std_type", "mlp_shared") != "mlp_shared":
            return None, f"stochastic policy whose log std (std_type {pol.std_type!r}) is not the second half of the shared stack"
        cls = pol.action_distribution_cls   # (`is`: a subclass may state another mode)
        if cls is TanhGaussDistribution:
            return hb.SAMPLE_TANH_GAUSS, None
        if cls is GaussDistribution:
            return hb.SAMPLE_GAUSS, None
        return None, f"stochastic policy with a {getattr(cls, '__name__', cls)} (the mode heads: GaussDistribution, TanhGaussDistribution)"

    def kernel_refuses(self):
        """None when `gops_episode_rollout` (`_dis` with an action table, `_mode` with `stochastic_mode`) takes this evaluator's env
        and policy, else the reason."""
        pol = self._policy_module()
        if is_poly(pol):
            return "POLY policy"
        if getattr(pol, "is_lipsnet", False):
            return "LipsNet policy"
        head = None
        if isinstance(pol, StochaPolicy):   # (its stack emits (mean, log std): the mode heads read the mean half, on request)
            if not self.stochastic_mode:
                return "stochastic policy"
            head, why = self._mode_head()
            if why is not None:
                return why
        env = self._hip_env()
        if env.kind == hb.ENV_MOBILEROBOT:
            return "pyth_mobilerobot draws its obstacle noise per step"
        if self.action_table is not None:
            if hb.lib().gops_episode_dis_workspace_bytes(ctypes.byref(env), ctypes.byref(pol.hip_mlp()), int(self.action_table.shape[0]), 1, 1) == 0:
                return "env / policy description outside the episode kernel (more than GOPS_DQN_MAX_ACTIONS actions, hidden widths)"
            return None
        nbytes = hb.lib().gops_episode_workspace_bytes(ctypes.byref(env), ctypes.byref(pol.hip_mlp()), 1, 1) if head is None else \
            hb.lib().gops_episode_mode_workspace_bytes(ctypes.byref(env), ctypes.byref(pol.hip_mlp()), head, 1, 1)
        if nbytes == 0:
            # gops_hip.h lists them: ScaleObservation on the vehicle families or beyond 8 observations, ActionRepeat, hidden widths
            # that are no multiple of 16 or beyond the LDS plan (~1100)
            return "env / policy description outside the episode kernel (scaled vehicle observations, hidden widths)"
        return None

    def draw_initial_conditions(self, n: int) -> dict:
        """n initial conditions from the data env's reset distribution; a new draw per evaluation, reproducible for a seed."""
        pool = draw_reset_pool(self.cfg, self.env_model, self.seed + 7919 * self._evals, n, self.device, True)
        self._evals += 1
        return pool

    # ---- episodes -------------------------------------------------------------------------------
    @torch.no_grad()
    def run_episodes(self, init: dict, *, trace: bool = False, fused: bool = None, trace_fill: float = None) -> dict:
        """All episodes of `init` (obs [E, obs_dim] + info tensors, on the device): ret [E], length [E] int32, terminated [E] and
        - with `trace` - trace_obs / trace_act / trace_rew.  Device tensors; nothing is read back here."""
        init = {k: v.to(self.device, torch.float32).contiguous() for k, v in init.items() if k == "obs" or k in INFO_KEYS}
        fused = self.fused if fused is None else fused
        if self._set_path(self.kernel_refuses() if fused else "fused=False"):
            E = init["obs"].shape[0]
            mlp = self._policy_module().hip_mlp()
            head = self._mode_head()[0] if self.stochastic_mode else None   # (part of the key: a rollout is built for one head)
            key = (E, self.max_episode_steps, head)
            ro = self._rollouts.get(key)
            if ro is None:
                ro = self._rollouts[key] = hb.EpisodeRollout(self._hip_env(), mlp, episodes=E, max_steps=self.max_episode_steps,
                                                             device=self.device, action_table=self.action_table, mode_head=head)
            ro.set_policy(mlp)
            self.last = ro.run(init, trace=trace, trace_fill=trace_fill)
        else:
            self.last = self.step_loop(init, trace=trace, trace_fill=trace_fill)
        return self.last

    @torch.no_grad()
    def step_loop(self, init: dict, *, trace: bool = False, trace_fill: float = None, sync_every_step: bool = False) -> dict:
        """The same episodes through the per-step device loop (torch policy + one `gops_env_step` launch per step).  The
        `finished` mask stays on the device; `sync_every_step` adds the host read per step the sampler's bookkeeping has."""
        env, policy, T = self._hip_env(), self._policy_module(), self.max_episode_steps
        table = self.action_table
        obs, info = init["obs"], {k: init[k] for k in INFO_KEYS if k in init}
        E, dev = obs.shape[0], obs.device
        zeros = torch.zeros(E, device=dev)
        ret = torch.zeros(E, dtype=torch.float64, device=dev)
        length = torch.zeros(E, dtype=torch.int32, device=dev)
        terminated = torch.zeros(E, device=dev)
        finished = torch.zeros(E, dtype=torch.bool, device=dev)
        res = {}
        if trace:
            mk = (lambda *sh: torch.empty(*sh, device=dev)) if trace_fill is None else (lambda *sh: torch.full(sh, float(trace_fill), device=dev))
            res.update(trace_obs=mk(E, T, env.obs_dim), trace_act=mk(E, T, env.act_dim if table is None else 1), trace_rew=mk(E, T))
        for t in range(T):
            act = policy(obs)
            if table is not None:   # the mode of ValueDirac / Categorical: the arg-max (lowest index among equal maxima), then the table
                index = torch.argmax(act, dim=-1)
                act, stored = table[index], index.to(torch.float32).unsqueeze(-1)
            elif isinstance(policy, StochaPolicy):   # evaluation acts with the distribution's mode
                act = policy.get_act_dist(act).mode()
            act = act.contiguous()
            if table is None:
                stored = act
            obs2, rew, done, info2 = hb.env_step(env, obs, act, zeros, info)
            live = ~finished
            if trace:
                res["trace_obs"][:, t] = torch.where(live[:, None], obs, res["trace_obs"][:, t])
                res["trace_act"][:, t] = torch.where(live[:, None], stored, res["trace_act"][:, t])
                res["trace_rew"][:, t] = torch.where(live, rew, res["trace_rew"][:, t])
            ret += torch.where(live, rew.double(), torch.zeros_like(ret))
            length += live.to(torch.int32)
            terminated = torch.where(live & (done != 0), torch.ones_like(terminated), terminated)
            finished = finished | (done != 0)
            obs, info = obs2, {k: info2[k] for k in info}
            if sync_every_step and bool(finished.all().item()):
                break
        res.update(ret=ret.float(), length=length, terminated=terminated)
        return res

    # ---- the reference's surface ----------------------------------------------------------------
    def _save(self, res, iteration, first_index):
        folder = os.path.join(self.save_folder, "evaluator")
        os.makedirs(folder, exist_ok=True)
        host = {k: v.cpu().numpy() for k, v in res.items()}
        for e in range(host["ret"].shape[0]):
            n = int(host["length"][e])
            np.save(os.path.join(folder, "iter{}_ep{}".format(iteration, first_index + e)),
                    {"reward_list": list(host["trace_rew"][e, :n]), "action_list": list(host["trace_act"][e, :n]),
                     "obs_list": list(host["trace_obs"][e, :n])})

    def run_n_episodes(self, n, iteration):
        if self.print_iteration != iteration:
            self.print_iteration, self.print_time = iteration, 0
        save = self.eval_save and self.save_folder is not None
        res = self.run_episodes(self.draw_initial_conditions(int(n)), trace=save)
        mean = float(res["ret"].double().mean().item())   # the one sync of an evaluation (best_tar needs a Python float)
        if save:
            self._save(res, iteration, self.print_time)
        self.print_time += int(n)
        return mean

    def run_an_episode(self, iteration, render=False):
        if render:
            raise NotImplementedError("gops_amd's Evaluator does not render")
        return self.run_n_episodes(1, iteration)

    def run_evaluation(self, iteration):
        return self.run_n_episodes(self.num_eval_episode, iteration)
