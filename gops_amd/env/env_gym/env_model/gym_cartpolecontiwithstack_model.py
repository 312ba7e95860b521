"""gym_cartpolecontiwithstack: the cart-pole whose observation is the window of its last `stack_length` states [L, 4], oldest first
(reference: gops/env/env_gym/gym_cartpolecontiwithstack.py - a DATA environment; the reference has no env model of it).  A reset
fills every row with the initial state, uniform in +-[2, 0.05, 0.2, 0.05]; a step drops the oldest row and appends the new state; the
time limit is 200.  Physics, thresholds, reward and done rule are gym_cartpoleconti's with force 30 a instead of 10 a.

This object is the DESCRIPTION the closed-loop kernels of csrc/rollout_stack.hip take: one row of the window (obs_dim 4) as
ENV_CARTPOLE, stepped as a data env by `gops_stack_sample_rollout` / `gops_stack_episode_rollout` only (the fused
`OnPolicyDeviceSampler` and the `Evaluator` under a recurrent policy).  `forward` - the env MODEL's step - is refused: `gops_env_step`
would step the flat cart-pole's force."""
from gops_amd import hip_backend as hb
from gops_amd.env.env_gym.env_model.gym_cartpoleconti_model import GymCartpolecontiModel


class GymCartpolecontiwithstackModel(GymCartpolecontiModel):
    is_stack = True

    def __init__(self, device=None, stack_length: int = 5, **kwargs):
        super().__init__(device)
        if not 1 <= int(stack_length) <= hb.STACK_MAX_LEN:
            raise RuntimeError(f"gym_cartpolecontiwithstack: stack_length must be 1..{hb.STACK_MAX_LEN} for the HIP closed loops")
        self.stack_length = int(stack_length)
        self.obsv_dim = (self.stack_length, self.obs_dim)   # what a recurrent approximator takes as `obs_dim`


def env_model_creator(**kwargs):
    """make the description of `gym_cartpolecontiwithstack`"""
    return GymCartpolecontiwithstackModel(kwargs.get("device", None), stack_length=kwargs.get("stack_length", 5))
