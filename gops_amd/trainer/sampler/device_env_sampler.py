"""Closed-loop batched sampling on the GPU.

The reference's samplers step numpy data environments one env and one step at a time on the CPU
(gops/trainer/sampler/base.py:101-187) - the bottleneck once the learner runs on the MI355X (SURVEY
section 8(f) rank 3).  The data environments of this path share their dynamics and stage reward with the env
models but NOT their termination rules or terminal reward (pyth_veh3dofconti.py:224-226,263-271: -100 at done,
world-frame |dx| > 5, |dy| > 2 against the model's ego-frame 10 / 10; lq_base.py:224-239: done when the state leaves
its bounds, -100, no clipping; pyth_idpendulum.py:71-87 is identical to its model; gym_cartpoleconti.py:102-137: reward 1
also for the step that ends an episode; pyth_veh2dofconti.py:179-219: the model's step, -100 at done; pyth_mobilerobot.py:108-152:
the model's step with both headings clipped to +-pi, obstacle noise drawn on the device per step).  `env_step="data"` (default)
selects those data-env semantics in the step kernel (`GopsEnv.data_env`, checked against transitions recorded from the
reference's numpy envs: tests/golden/dataenv_*.npz); `env_step="model"` steps the env model instead.  N environment
instances are advanced together by `gops_env_step`:

    act = policy(obs)            # N x obs_dim through the policy MLP (library GEMMs), on the device
    obs2, rew, done, info2 = gops_env_step(obs, act, done=0, info)
    finished or timed-out instances are re-seeded from a device pool of reset states

`sample()` returns replay-format DEVICE tensors (`obs, act, rew, done, obs2, logp` + info / next_info
keys) for `ReplayBuffer.add_tensors`; nothing crosses PCIe in steady state.  Reset states come from the
data envs' reset distributions (`gops_amd.utils.synthetic.make_batch`), generated on the host in pools of
`pool_factor x n_envs` and uploaded once per pool.
"""
import ctypes
import time
import warnings

import torch

from gops_amd.apprfunc.mlp import ActionValueDis, DetermPolicy, StochaPolicy, StochaPolicyDis
from gops_amd import hip_backend as hb
from gops_amd.trainer.closed_loop import ClosedLoopDriver
from gops_amd.trainer.sampler.reset_pool import INFO_KEYS as _INFO, NOT_RESTATED, draw_reset_pool, pool_needs_refresh
from gops_amd.utils.act_distribution import GaussDistribution, TanhGaussDistribution
from gops_amd.utils.tensorboard_setup import tb_tags


class DeviceEnvSampler(ClosedLoopDriver):
    on_device = True   # trainers: do not move the networks to the CPU around sample()

    def __init__(self, cfg: dict, env_model, *, n_envs: int, steps_per_sample: int = 1, max_episode_steps: int = 200,
                 seed: int = 0, device="cuda", pool_factor: int = 8, noise_std: float = 0.0, env_step: str = "data",
                 action_table=None, epsilon: float = 0.0, fused: bool = False):
        """cfg: workload dict as in `gops_amd.utils.synthetic.CONFIGS` (env_id, pre_horizon, lq_config);
        env_model: the wrapped model from `create_env_model` (its constants drive the step kernel);
        action_table [act_num, action_dim] (None: continuous actions, the policy output is the action): the policy output is read as
        action values - the action index is their arg-max, replaced with probability `epsilon` by a uniform index from this sampler's
        device generator -, the env is stepped with `action_table[index]` and the stored `act` column is the index as a float, [N, 1]
        (DQN; `gym_cartpoleconti` with the table [[-1.], [1.]] is the two-action cartpole).  With a StochaPolicyDis (discrete TRPO) the
        policy output is read as logits instead: the index is drawn from softmax(logits) with the same generator, `logp` is the
        log-softmax at it, and `epsilon` must be 0 (`sample()` raises ValueError otherwise).
        `fused=True`: a whole `sample()` in ONE launch (`gops_sample_rollout`, csrc/rollout_sample.hip) - one `torch.randn` of
        [steps, n_envs, action_dim], the launch, one 4-byte read (the largest reset count, for the pool refresh) - wherever the kernel
        takes the env and the policy; `path` names the path the last call took and, for the loop, why.  The returned tensors are then
        views of buffers the next `sample()` overwrites.  Finished instances restart from their OWN column of the pool
        (`reset_pool.pool_row`), and the noise stream is the fused path's own: a seeded fused run does not reproduce a seeded loop run.
        With an action table the fused path is `gops_sample_rollout_dis`: head EPS_GREEDY for an ActionValueDis (DQN: the `q` network
        behind `networks.policy`), with `self.epsilon` read at every call, head CATEGORICAL for a StochaPolicyDis; one `torch.rand` of
        [steps, n_envs, 2] replaces the loop's argmax / multinomial / rand / randint / where / gather chain, and the index and logp
        are `reset_pool.restate_discrete_head` of the network's outputs and those uniforms - again a noise stream of its own, so a
        seeded fused run does not reproduce a seeded loop run.  A table behind any other policy class stays on the loop."""
        self.cfg, self.env_model = dict(cfg), env_model
        if getattr(getattr(env_model, "unwrapped", env_model), "ref_c", None) is not None:
            raise RuntimeError("DeviceEnvSampler draws its reset states from the DEFAULT reference trajectories "
                               "(gops_amd.utils.synthetic); a model with custom path_para / u_para needs its own reset pool")
        self.n, self.steps, self.max_steps = n_envs, steps_per_sample, max_episode_steps
        self.device = torch.device(device)
        self.seed, self.pool_factor, self.noise_std = seed, pool_factor, noise_std
        self._warned_noise = False
        self._take_action_table(action_table)
        self.epsilon = float(epsilon)
        if env_step not in ("data", "model"):
            raise ValueError("env_step must be 'data' (the data environment's step) or 'model' (the env model's)")
        self.data_env = env_step == "data"
        kind = getattr(getattr(env_model, "unwrapped", env_model), "hip_kind", None)
        if self.data_env and (kind not in hb.DATA_ENV_KINDS or self.cfg.get("env_id", "").endswith("errcstr")):
            raise RuntimeError(NOT_RESTATED.format(env_id=self.cfg.get("env_id")))
        self.networks = None
        self.total = 0
        self._pool, self._pool_pos, self._pools_made = None, 0, 0
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)
        self._henv = None
        first = self._draw(self.n)
        self.obs = first["obs"]
        self.info = {k: first[k] for k in _INFO if k in first}
        self.t = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.fused = bool(fused)
        self._fstate, self._fpool, self._frollout = None, None, None

    # ---- reset pool ---------------------------------------------------------------------------
    def _draw(self, k: int):
        """k fresh initial conditions (device tensors) from the pool; refills the pool when it runs dry."""
        size = self.pool_factor * self.n
        if self._pool is None or self._pool_pos + k > size:
            self._pool = draw_reset_pool(self.cfg, self.env_model, self.seed + 7919 * self._pools_made, size, self.device, self.data_env)
            self._pool_pos, self._pools_made = 0, self._pools_made + 1
        sl = slice(self._pool_pos, self._pool_pos + k)
        self._pool_pos += k
        return {key: v[sl].clone() for key, v in self._pool.items()}

    def _hip_env(self):
        if self._henv is None:
            self._henv = self.env_model.hip_env(*self._squash_limits(), data_env=self.data_env)
        return self._henv

    # ---- sampling -----------------------------------------------------------------------------
    def _step_once(self, policy, zeros):
        """Advance all N environments one step; -> (the step's row of replay-format columns, the mask of the instances whose episode
        this step ended - terminated or timed out - and that restart from a fresh reset state)."""
        obs, info = self.obs, self.info
        act, logp = policy(obs), zeros
        stored = None
        if self.action_table is not None:
            if isinstance(policy, StochaPolicyDis):   # the categorical policy explores by itself; its log-probability is stored
                self._check_categorical()
                stored, logp = self.sample_index(act)
            else:
                stored = self.select_index(act)
            act = self.action_table[stored]
            stored = stored.to(torch.float32).unsqueeze(-1)
        elif isinstance(policy, StochaPolicy):   # the policy's own distribution explores; its log-probability is stored
            act, logp = policy.get_act_dist(act).sample(generator=self._gen)
            if self.noise_std > 0.0 and not self._warned_noise:
                self._warned_noise = True
                warnings.warn("DeviceEnvSampler: noise_std is ignored with a stochastic policy (it samples its own distribution)")
        elif self.noise_std > 0.0:
            act = act + self.noise_std * torch.randn(act.shape, generator=self._gen, device=self.device)
        obs2, rew, done, info2 = hb.env_step(self._hip_env(), obs, act.contiguous(), zeros, info)
        row = dict(obs=obs, act=act if stored is None else stored, rew=rew, done=done, obs2=obs2, logp=logp)
        for k in info:
            row[k], row["next_" + k] = info[k], info2[k]
        # episode bookkeeping: terminated or timed-out instances restart from a fresh reset state
        self.t += 1
        over = (done != 0) | (self.t >= self.max_steps)
        n_over = int(over.sum().item())
        # (pyth_mobilerobot's info["constraint"] is a zero-size replay slot in the reference, pyth_mobilerobot.py:86-92:
        # the step's constraint output is not a stored column)
        self.obs, self.info = obs2, {k: info2[k] for k in info}
        if n_over:
            fresh = self._draw(n_over)
            idx = over.nonzero(as_tuple=True)[0]
            self.obs = self.obs.index_copy(0, idx, fresh["obs"])
            for k in self.info:
                self.info[k] = self.info[k].index_copy(0, idx, fresh[k])
            self.t.index_fill_(0, idx, 0)
        return row, over

    def select_index(self, values: torch.Tensor) -> torch.Tensor:
        """Epsilon-greedy over action values [N, act_num] -> indices [N] (int64): the arg-max, replaced with probability `epsilon` by
        a uniform index; both draws come from the sampler's generator."""
        index = torch.argmax(values, dim=-1)
        if self.epsilon > 0.0:
            explore = torch.rand(index.shape, generator=self._gen, device=values.device) < self.epsilon
            uniform = torch.randint(values.shape[-1], index.shape, generator=self._gen, device=values.device)
            index = torch.where(explore, uniform, index)
        return index

    def sample_index(self, logits: torch.Tensor):
        """A categorical policy's logits [N, act_num] -> (indices [N] (int64) drawn from softmax(logits) with the sampler's generator,
        their log-probabilities [N]: the log-softmax at the index)."""
        logp_all = torch.log_softmax(logits, dim=-1)
        index = torch.multinomial(logp_all.exp(), 1, generator=self._gen)
        return index.squeeze(-1), logp_all.gather(-1, index).squeeze(-1)

    def _check_categorical(self):
        if self.epsilon > 0.0:
            raise ValueError("DeviceEnvSampler: epsilon > 0 with a StochaPolicyDis - the policy samples its own categorical "
                             "distribution, and the stored logp would not be that of an epsilon-greedy index")

    # ---- the fused path ------------------------------------------------------------------------
    def kernel_refuses(self):
        """None when `gops_sample_rollout` takes this sampler's env and policy, else the reason."""
        policy = self._policy_module()
        if self.action_table is not None:
            if not isinstance(policy, ActionValueDis):   # (StochaPolicyDis is one)
                return "action table (discrete actions) behind a policy that is neither an ActionValueDis nor a StochaPolicyDis"
        else:
            if isinstance(policy, StochaPolicyDis):
                return "categorical policy"
            for flag, name in (("is_poly", "POLY"), ("is_rbf", "GAUSS (RBF)"), ("is_lipsnet", "LipsNet")):
                if getattr(policy, flag, False):
                    return name + " policy"
            if getattr(policy, "_time_input", False):
                return "time-augmented policy"
            if not isinstance(policy, (DetermPolicy, StochaPolicy)):
                return "policy class outside the sample kernel's heads"
            if isinstance(policy, StochaPolicy) and not issubclass(policy.action_distribution_cls, GaussDistribution):
                return "action distribution outside the sample kernel's heads"
        env = self._hip_env()
        if env.kind == hb.ENV_MOBILEROBOT:
            return "pyth_mobilerobot draws its obstacle noise per step"
        if self.action_table is not None:
            if hb.lib().gops_sample_dis_workspace_bytes(ctypes.byref(env), ctypes.byref(policy.hip_mlp()), int(self.action_table.shape[0]),
                                                        self.n, self.steps) == 0:
                # gops_hip.h lists them; gym_cartpoleconti with env_step="model" is one: the kernel steps it as a data env only
                return ("action table: env / policy description outside the sample kernel (an env the kernel steps under the other "
                        "env_step only, constrained model, ActionRepeat, hidden widths, more than GOPS_DQN_MAX_ACTIONS actions)")
        elif hb.lib().gops_sample_workspace_bytes(ctypes.byref(env), ctypes.byref(policy.hip_mlp()), self.n, self.steps) == 0:
            # gops_hip.h lists them: the constrained vehicle models, ActionRepeat, scaled vehicle observations, hidden widths that are
            # no multiple of 16 or beyond the LDS plan, more than GOPS_MAX_ACT actions
            return "env / policy description outside the sample kernel (constrained model, ActionRepeat, hidden widths)"
        return None

    def _draw_fused_pool(self):
        """`pool_factor` reset states per instance, [R, N, ...]: the same draw as the loop's pool, reshaped; the counts start over."""
        R, N = self.pool_factor, self.n
        pool = draw_reset_pool(self.cfg, self.env_model, self.seed + 7919 * self._pools_made, R * N, self.device, self.data_env)
        self._pools_made += 1
        self._fpool = {k: v.reshape((R, N) + tuple(v.shape[1:])).contiguous() for k, v in pool.items() if k == "obs" or k in self.info}
        self._fstate["reset_count"].zero_()

    def _fused_head(self, policy):
        """What the fused path takes from the policy's class: (the kernel's head, the draw of a call's noise - standard normals
        [T, N, action_dim], or [T, N, 2] uniforms for the discrete heads -, `SampleRollout`'s further keywords)."""
        if self.action_table is not None:
            categorical = isinstance(policy, StochaPolicyDis)
            if categorical:
                self._check_categorical()
            return hb.SAMPLE_CATEGORICAL if categorical else hb.SAMPLE_EPS_GREEDY, torch.rand, dict(action_table=self.action_table)
        stochastic = isinstance(policy, StochaPolicy)
        if stochastic and self.noise_std > 0.0 and not self._warned_noise:
            self._warned_noise = True
            warnings.warn("DeviceEnvSampler: noise_std is ignored with a stochastic policy (it samples its own distribution)")
        head = hb.SAMPLE_DETERM if not stochastic else \
            hb.SAMPLE_TANH_GAUSS if issubclass(policy.action_distribution_cls, TanhGaussDistribution) else hb.SAMPLE_GAUSS
        return head, torch.randn, dict(noise_std=0.0 if stochastic else self.noise_std, min_log_std=getattr(policy, "min_log_std", 0.0),
                                       max_log_std=getattr(policy, "max_log_std", 0.0))

    def _sample_fused(self):
        """One noise draw, one launch for all `steps` steps, the 4-byte read; -> the kernel's time-major output buffers ([T, N, ...] each)."""
        policy = self._policy_module()
        T, N, R = self.steps, self.n, self.pool_factor
        st = self._fstate
        if st is None or st["obs"] is not self.obs:   # the first fused call (or the loop ran since): the kernel advances its state in
            # place, and the loop hands out its state tensors as batch columns - the fused path owns copies
            st = self._fstate = dict(obs=self.obs.clone().contiguous(), t=self.t.clone(),
                                     reset_count=torch.zeros(N, dtype=torch.int32, device=self.device),
                                     **{k: v.clone().contiguous() for k, v in self.info.items()})
            self.obs, self.info, self.t = st["obs"], {k: st[k] for k in self.info}, st["t"]
            self._fpool = None
        if self._fpool is None:
            self._draw_fused_pool()
        head, draw, keywords = self._fused_head(policy)
        if self._frollout is None or (self._frollout.n_envs, self._frollout.steps) != (N, T):
            self._frollout = hb.SampleRollout(self._hip_env(), policy.hip_mlp(), n_envs=N, steps=T, head=head, max_episode_steps=self.max_steps,
                                              pool_rows=R, info_like=self.info, device=self.device, **keywords)
        ro = self._frollout
        ro.set_policy(policy.hip_mlp())
        ro.desc.max_episode_steps = int(self.max_steps)
        if ro.dis is not None:   # (read at every call, as max_episode_steps is: DQN anneals it)
            ro.dis.epsilon = float(self.epsilon)
        noise = draw((T, N, ro.noise_width), generator=self._gen, device=self.device)
        out = ro.run(st, self._fpool, noise)
        if pool_needs_refresh(int(st["reset_count"].max().item()), R):   # the one host read of a fused sample()
            self._draw_fused_pool()
        return out

    def _fused_batch(self, out):
        """The kernel's buffers as the loop's columns: views flattened time-major."""
        keys = ["obs", "act", "rew", "done", "obs2", "logp"] + [p + k for k in self.info for p in ("", "next_")]
        return {k: out[k].flatten(0, 1) for k in keys}

    def _choose_path(self) -> bool:
        return self._set_path(self.kernel_refuses() if self.fused else "fused=False")

    @torch.no_grad()
    def sample(self):
        """Advance all N environments `steps_per_sample` steps; returns (dict of [N*steps, ...] device
        tensors in replay format, tb dict)."""
        t0 = time.time()
        policy = self.networks.policy
        if self._choose_path():
            batch = self._fused_batch(self._sample_fused())
            self.total += self.n * self.steps
            return batch, {tb_tags["sampler_time"]: (time.time() - t0) * 1000}
        zeros = torch.zeros(self.n, device=self.device)
        chunks = [self._step_once(policy, zeros)[0] for _ in range(self.steps)]
        batch = {k: torch.cat([c[k] for c in chunks]) for k in chunks[0]} if len(chunks) > 1 else chunks[0]
        self.total += self.n * self.steps
        return batch, {tb_tags["sampler_time"]: (time.time() - t0) * 1000}

    def sample_with_replay_format(self):
        return self.sample()

    def get_total_sample_number(self):
        return self.total

    def load_state_dict(self, state_dict):
        pass
