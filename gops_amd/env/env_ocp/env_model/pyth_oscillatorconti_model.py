"""pyth_oscillatorconti model: a memristor-controlled nonlinear oscillator as a zero-sum game, two states (battery a, battery b),
dt = 1/200, Q = R = I, action range +-5, adversary range +-1/gamma_atte (reference:
gops/env/env_ocp/env_model/pyth_oscillatorconti_model.py:24-313).  RPI only; shared parts: _contigame.py, device arithmetic:
csrc/rollout_rpi.hip."""
import torch

from gops_amd import hip_backend as hb
from gops_amd.env.env_ocp.env_model._contigame import ContiGameModel


class PythOscillatorcontiModel(ContiGameModel):
    rpi_kind = hb.RPI_ENV_OSCILLATOR
    state_dim = 2
    dt = 1 / 200
    min_action = [-5.0]
    max_action = [5.0]
    adv_bound = 1.0

    def _derivative(self, state, act, adv):
        a, b = state[:, 0], state[:, 1]
        d_a = -0.25 * a
        d_b = 0.5 * torch.mul(a ** 2, b) - 1 / (2 * self.gamma_atte ** 2) * b ** 3 - 0.5 * b + torch.mul(a, act) + torch.mul(b, adv)
        return torch.stack([d_a, d_b], dim=-1)

    def _g(self, state):
        return torch.stack([torch.zeros_like(state[:, 0]), state[:, 0]], dim=-1)

    def _k(self, state):
        return torch.stack([torch.zeros_like(state[:, 1]), state[:, 1]], dim=-1)
