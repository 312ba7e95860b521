"""gym_mountaincarconti model: state = observation = (pos, vel), one action in [-1, 1], no dt.  A step pushes the speed by
0.0015 a - 0.0025 cos(3 pos) and saturates it at +-0.07, moves the position by the new speed and saturates it at [-1.2, 0.6],
then stops the car at the left wall (speed 0 where the position sits on -1.2 with a negative speed); done when the NEXT state has
pos >= 0.45 and vel >= 0; reward = 100 done - 0.1 a^2 (reference: gops/env/env_gym/env_model/gym_mountaincarconti_model.py:21-99).
Arithmetic on the device: csrc/env_models.h (mcar_forward / mcar_backward).

`forward` below is the same step on the host in torch, at the dtype of `obs` and under autograd: the yardstick the kernels are
tested against (in float64), not a path any algorithm takes."""
from typing import Dict, Tuple, Union

import torch

from gops_amd import hip_backend as hb
from gops_amd.env.env_ocp.env_model.pyth_base_model import PythBaseModel


class GymMountaincarcontiModel(PythBaseModel):
    hip_kind = hb.ENV_MOUNTAINCAR

    def __init__(self, device: Union[torch.device, str, None] = None, **kwargs):
        self.min_position, self.max_position, self.max_speed = -1.2, 0.6, 0.07
        self.goal_position, self.goal_velocity, self.power = 0.45, 0, 0.0015
        super().__init__(obs_dim=2, action_dim=1, dt=None, obs_lower_bound=[self.min_position, -self.max_speed],
                         obs_upper_bound=[self.max_position, self.max_speed], action_lower_bound=[-1.0],
                         action_upper_bound=[1.0], device=device)

    def forward(self, obs: torch.Tensor, action: torch.Tensor, done: torch.Tensor, info: Dict
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Dict]:
        """One step of the BARE model (`done` and `info` are not read, as in the reference).  The bounds and the goal are the fp32
        values the device compares against, widened to the dtype of `obs`; every product and sum is its own torch op, in the
        reference's order, so that fp32 inputs give the reference's bits."""
        low, high = self.obs_lower_bound.to(obs), self.obs_upper_bound.to(obs)
        goal = torch.tensor(self.goal_position, dtype=torch.float32).to(obs)
        a = action.reshape(obs.shape[0])
        vel = torch.clamp(obs[:, 1] + self.power * a - 0.0025 * torch.cos(3 * obs[:, 0]), low[1], high[1])
        pos = torch.clamp(obs[:, 0] + vel, low[0], high[0])
        wall = (pos == low[0]) & (vel < 0)
        vel = torch.where(wall, torch.zeros_like(vel), vel)   # behind the position update: pos keeps its path to the unzeroed speed
        isdone = (pos >= goal) & (vel >= self.goal_velocity)
        reward = 100.0 * isdone.to(obs.dtype) - 0.1 * a ** 2
        return torch.stack((pos, vel), dim=-1), reward, isdone, {}


def env_model_creator(**kwargs):
    """make env model `gym_mountaincarconti`"""
    return GymMountaincarcontiModel(kwargs.get("device", None))
