"""Shared host part of the continuous-time zero-sum game models RPI evaluates (pyth_oscillatorconti, pyth_aircraftconti,
pyth_suspensionconti; specification: the reference's gops/env/env_ocp/env_model/pyth_{oscillator,aircraft,suspension}conti_model.py).

All three are input-affine, dx/dt = f(x) + g(x) u + k(x) w with one action u and one adversary w, the running cost is
x'Qx + R u^2 - gamma_atte^2 w^2 with diagonal Q, and a step is one explicit Euler step of `dt`.  A concrete model supplies
`f_x / g_x / k_x`, the reset distribution and its constants.  These models serve RPI only: `hip_kind` stays GOPS_ENV_NONE, so no
rollout entry point accepts them; RPI's device path reads `rpi_kind` (csrc/rollout_rpi.hip).  Unlike the other models here they have
a host (torch) `forward`: RPI's eager path and its samplers / evaluators use it.
"""
from typing import Dict, Tuple, Union

import numpy as np
import torch

from gops_amd.env.env_ocp.env_model.pyth_base_model import PythBaseModel


class ContiGameModel(PythBaseModel):
    hip_kind = 0
    rpi_kind = 0          # GOPS_RPI_ENV_* of include/gops_hip.h
    state_dim = 0
    action_dim = 1
    adversary_dim = 1
    dt = 0.0
    min_action = [-1.0]
    max_action = [1.0]
    adv_bound = 1.0       # the adversary's range is +- adv_bound / gamma_atte

    def __init__(self, device: Union[torch.device, str, None] = None, **kwargs):
        self.is_adversary = kwargs["is_adversary"]
        self.sample_batch_size = kwargs["reset_batch_size"]
        self.gamma = 1
        self.gamma_atte = kwargs["gamma_atte"]
        self.Q, self.R = self._weights(kwargs)
        self.fixed_initial_state = kwargs["fixed_initial_state"]
        self.initial_state_range = kwargs["initial_state_range"]
        self.state_threshold = [float(t) for t in kwargs["state_threshold"]]
        assert len(self.initial_state_range) == self.state_dim and len(self.state_threshold) == self.state_dim
        self.min_adv_action = [-self.adv_bound / self.gamma_atte]
        self.max_adv_action = [self.adv_bound / self.gamma_atte]
        self.lb_state = torch.tensor([-t for t in self.state_threshold], dtype=torch.float32)
        self.hb_state = torch.tensor(self.state_threshold, dtype=torch.float32)
        low = self.min_action + (self.min_adv_action if self.is_adversary else [])
        high = self.max_action + (self.max_adv_action if self.is_adversary else [])
        self.lb_action = torch.tensor(low, dtype=torch.float32)
        self.hb_action = torch.tensor(high, dtype=torch.float32)
        self.ones_ = torch.ones(self.sample_batch_size)
        self.zeros_ = torch.zeros(self.sample_batch_size)
        # parallel sampling state; the time limit per lane is drawn once, here, before anything else touches np.random
        self.parallel_state = None
        self.lower_step = kwargs["lower_step"]
        self.upper_step = kwargs["upper_step"]
        self.max_step_per_episode = self.max_step()
        self.step_per_episode = self.initial_step()
        super().__init__(obs_dim=self.state_dim, action_dim=self.action_dim, dt=self.dt, obs_lower_bound=self.lb_state.tolist(),
                         obs_upper_bound=self.hb_state.tolist(), action_lower_bound=low, action_upper_bound=high,
                         device="cpu")   # a host model: its bounds stay next to its other tensors whatever `use_gpu` asks for

    # ---- what a concrete model defines ------------------------------------------------------------------------------------------
    def _weights(self, kwargs):
        return torch.eye(self.state_dim), torch.eye(self.action_dim)

    def _reset_column(self, scale):
        return np.random.uniform(-scale, scale, [self.sample_batch_size, 1])

    def _reset_block(self, n, scale):
        """`n` consecutive resets in one draw, [n, state_dim, B] float64; `scale` [1, state_dim, 1].  np.random fills an array in
        order, so this is the stream of n calls of `reset()`: low + (high - low) u per value, as `_reset_column` computes it."""
        return -scale + (scale - -scale) * np.random.uniform(size=[n, self.state_dim, self.sample_batch_size])

    def _derivative(self, state, act, adv):
        """dx/dt [B, state_dim] at `state` under action `act` [B] and adversary `adv` [B]."""
        raise NotImplementedError

    def _g(self, state):
        """g(x) [B, state_dim] (one action column)."""
        raise NotImplementedError

    def _k(self, state):
        """k(x) [B, state_dim] (one adversary column)."""
        raise NotImplementedError

    # ---- the reference's surface ----------------------------------------------------------------------------------------------
    def max_step(self):
        return torch.from_numpy(np.floor(np.random.uniform(self.lower_step, self.upper_step, [self.sample_batch_size])))

    def initial_step(self):
        return torch.zeros(self.sample_batch_size)

    def reset(self):
        """One [B, 1] draw per state column, column by column: the same np.random stream as the reference's reset."""
        cols = [self._reset_column(scale) for scale in self.initial_state_range]
        return torch.from_numpy(np.concatenate(cols, axis=1)).float()

    def reset_many(self, n: int) -> torch.Tensor:
        """The next `n` resets as [n, state_dim, B] (column-major per reset: the layout gops_rpi_evaluate reads), value for value
        what `n` calls of `reset()` return and the same np.random state afterwards, in one draw instead of n * state_dim."""
        scale = np.asarray(self.initial_state_range, dtype=np.float64).reshape(1, self.state_dim, 1)
        return torch.from_numpy(self._reset_block(int(n), scale).astype(np.float32))

    def _cost(self, state, act, adv):
        cost = self.Q[0][0] * state[:, 0] ** 2
        for i in range(1, self.state_dim):
            cost = cost + self.Q[i][i] * state[:, i] ** 2
        return cost + self.R[0][0] * act ** 2 - self.gamma_atte ** 2 * adv ** 2

    def step(self, action: torch.Tensor):
        """Advances `parallel_state` by one Euler step under the RAW action [B, 2] (no wrapper sees it); returns the COST as
        the reward (no sign flip, as in the reference), `done` from the thresholds on the new state and the time-limit flag."""
        state = self.parallel_state
        act, adv = action[:, 0], action[:, 1]
        delta_state = self._derivative(state, act, adv)
        self.parallel_state = state + delta_state * self.dt
        reward = self._cost(state, act, adv)
        done = torch.abs(self.parallel_state[:, 0]) > self.state_threshold[0]
        for i in range(1, self.state_dim):
            done = done | (torch.abs(self.parallel_state[:, i]) > self.state_threshold[i])
        self.step_per_episode += 1
        info = {"TimeLimit.truncated": self.step_per_episode > self.max_step_per_episode}
        return self.parallel_state, reward, done, info

    def forward(self, obs: torch.Tensor, action: torch.Tensor, done: torch.Tensor, info: Dict
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Dict]:
        act = action[:, 0]
        adv = action[:, 1] if self.is_adversary else torch.zeros_like(act)
        delta_state = self._derivative(obs, act, adv)
        next_obs = obs + delta_state * self.dt
        reward = -self._cost(obs, act, adv)
        isdone = obs.new_zeros(obs.shape[0], dtype=torch.bool)
        return next_obs, reward, isdone, {"delta_state": delta_state}

    def f_x(self, state, batch_size=None):
        zero = torch.zeros(state.shape[0])
        fx = self._derivative(state, zero, zero)
        return fx if state.shape[0] > 1 else fx.t()

    def g_x(self, state, batch_size=None):
        gx = self._g(state)
        return gx.unsqueeze(-1) if state.shape[0] > 1 else gx.t()

    def k_x(self, state, batch_size=None):
        kx = self._k(state)
        return kx.unsqueeze(-1) if state.shape[0] > 1 else kx.t()

    def best_act(self, state, delta_value):
        """-1/2 R^-1 g(x)' dV/dx, [B, 1]."""
        return (-0.5 * (1.0 / self.R[0][0]) * (self._g(state) * delta_value).sum(1, keepdim=True)).detach()

    def worst_adv(self, state, delta_value):
        """1/2 gamma_atte^-2 k(x)' dV/dx, [B, 1]."""
        return (0.5 / (self.gamma_atte ** 2) * (self._k(state) * delta_value).sum(1, keepdim=True)).detach()

    def rpi_constants(self):
        """The model's part of the `const float*` table of gops_rpi_evaluate (include/gops_hip.h, GOPS_RPI_C_*)."""
        from gops_amd import hip_backend as hb
        c = np.zeros(hb.RPI_CONST_COUNT, dtype=np.float32)
        c[hb.RPI_C_GAMMA_ATTE], c[hb.RPI_C_DT], c[hb.RPI_C_R] = self.gamma_atte, self.dt, float(self.R[0][0])
        for i in range(self.state_dim):
            c[hb.RPI_C_Q + i] = float(self.Q[i][i])
            c[hb.RPI_C_THRESHOLD + i] = self.state_threshold[i]
        c[hb.RPI_C_ACT_LOW], c[hb.RPI_C_ACT_HIGH] = self.min_action[0], self.max_action[0]
        c[hb.RPI_C_ADV_LOW], c[hb.RPI_C_ADV_HIGH] = self.min_adv_action[0], self.max_adv_action[0]
        return c
