"""pyth_suspensionconti model: a quarter-car active suspension as a zero-sum game, four states (body position and velocity, wheel
position and velocity), action = actuator force in kN (range +-1.2), adversary = road displacement (range +-2/gamma_atte),
dt = 1/500, Q = diag(state_weight), R = control_weight (reference:
gops/env/env_ocp/env_model/pyth_suspensionconti_model.py:24-450).  The tyre stiffness K_t / M_us = 3167 1/s^2 multiplies a wheel
position of a few centimetres, so the wheel acceleration is a difference of large terms in fp32.  RPI only; shared parts:
_contigame.py, device arithmetic: csrc/rollout_rpi.hip."""
import torch

from gops_amd import hip_backend as hb
from gops_amd.env.env_ocp.env_model._contigame import ContiGameModel


class PythSuspensioncontiModel(ContiGameModel):
    rpi_kind = hb.RPI_ENV_SUSPENSION
    state_dim = 4
    dt = 1 / 500
    min_action = [-1.2]
    max_action = [1.2]
    adv_bound = 2.0
    M_b, M_us = 300, 60                  # body and wheel mass [kg]
    K_t, K_a, C_a = 190000, 16000, 1000  # tyre stiffness, linear suspension stiffness [N/m], damping rate [N s/m]
    K_n = K_a / 10                       # cubic suspension stiffness
    control_gain = 1e3

    def _weights(self, kwargs):
        self.state_weight, self.control_weight = kwargs["state_weight"], kwargs["control_weight"]
        Q = torch.zeros((4, 4))
        for i in range(4):
            Q[i][i] = self.state_weight[i]
        R = torch.zeros((1, 1))
        R[0][0] = self.control_weight[0]
        return Q, R

    def _derivative(self, state, act, adv):
        pos_body, vel_body, pos_wheel, vel_wheel = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
        spring = (self.K_a * (pos_body - pos_wheel) + self.K_n * torch.pow(pos_body - pos_wheel, 3)
                  + self.C_a * (vel_body - vel_wheel))
        acc_body = -(spring - self.control_gain * act) / self.M_b
        acc_wheel = (spring - self.K_t * (pos_wheel - adv) - self.control_gain * act) / self.M_us
        return torch.stack([vel_body, acc_body, vel_wheel, acc_wheel], dim=-1)

    def _g(self, state):
        g = torch.tensor([0.0, self.control_gain / self.M_b, 0.0, -self.control_gain / self.M_us])
        return g.expand(state.shape[0], 4)

    def _k(self, state):
        k = torch.tensor([0.0, 0.0, 0.0, self.K_t / self.M_us])
        return k.expand(state.shape[0], 4)
