"""Shared by test_stack_cpu.py and test_stack_gpu.py: gym_cartpolecontiwithstack and the recurrent policy's heads restated in float64
from the reference's formulas (env_gym/gym_cartpolecontiwithstack.py stepPhysics / step / reset), and the description the kernels take."""
import copy
import math

import numpy as np
import torch

from rnn_helpers import apprfunc_kwargs

from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.create_pkg.create_env_model import create_env_model

X_TH, THETA_TH = 2.4, 12 * 2 * math.pi / 360
RESET_HALF_RANGE = np.array([2.0, 0.05, 0.2, 0.05])
MIN_LOG_STD, MAX_LOG_STD = -20.0, 2.0   # rnn_helpers.apprfunc_kwargs


def step64(x, act):
    """One env step in float64: x [..., 4] the newest state, act [...] the policy's action (clipped to the action space [-1, 1], as
    the description's ClipAction does) -> (next state, done).  The reward is 1 on every step."""
    x = np.asarray(x, np.float64)
    force = 30.0 * np.clip(np.asarray(act, np.float64), -1.0, 1.0)
    pos, vel, th, thd = (x[..., i] for i in range(4))
    c, s = np.cos(th), np.sin(th)
    temp = (force + 0.05 * thd * thd * s) / 1.1
    thacc = (9.8 * s - c * temp) / (0.5 * (4.0 / 3.0 - 0.1 * c * c / 1.1))
    xacc = temp - 0.05 * thacc * c / 1.1
    xn = np.stack((pos + 0.02 * vel, vel + 0.02 * xacc, th + 0.02 * thd, thd + 0.02 * thacc), axis=-1)
    return xn, (np.abs(xn[..., 0]) > X_TH) | (np.abs(xn[..., 2]) > THETA_TH)


def threshold_margin(xn):
    """The smallest distance of any next state to a threshold: above 1e-4, fp32 and float64 agree on `done`."""
    return float(np.minimum(np.abs(np.abs(xn[..., 0]) - X_TH), np.abs(np.abs(xn[..., 2]) - THETA_TH)).min())


def make_policy(H, head, seed):
    """A recurrent StochaPolicy over rows of 4 with one action, recurrent weights doubled as in test_rnn_gpu (a recurrence that
    matters, away from saturation), and its float64 copy."""
    torch.manual_seed(seed)
    net = create_apprfunc(**apprfunc_kwargs("StochaPolicy", (H,) + tuple(head), "tanh", O=4, out=1))
    with torch.no_grad():
        net.rnn.weight_hh_l0.mul_(2.0)
        net.rnn.weight_ih_l0.mul_(2.0)
    return net, copy.deepcopy(net).double()


def head64(ref, windows):
    """(mean, raw log std) [rows] of the float64 module on windows [rows, L, 4]."""
    with torch.no_grad():
        y = ref.policy(torch.as_tensor(np.asarray(windows), dtype=torch.float64)).numpy()
    return y[:, 0], y[:, 1]


def hip_env(net, L):
    """The C-ABI description of one row of the window, as the sampler and the evaluator build it."""
    model = create_env_model("gym_cartpolecontiwithstack", stack_length=L)
    return model.hip_env(net.act_low_lim.cpu().numpy(), net.act_high_lim.cpu().numpy(), data_env=True)


def episode64(ref, x0, L, max_steps, lo, hi):
    """One evaluation episode in float64 from the state x0: (length, terminated, the smallest threshold margin on the way)."""
    window, margin = np.repeat(np.asarray(x0, np.float64)[None], L, axis=0), np.inf
    for t in range(max_steps):
        mean, _ = head64(ref, window[None])
        xn, done = step64(window[-1], np.clip(mean[0], lo, hi))
        margin = min(margin, threshold_margin(xn))
        window = np.concatenate((window[1:], xn[None]))
        if done:
            return t + 1, 1.0, margin
    return max_steps, 0.0, margin
