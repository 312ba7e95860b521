"""TD3 - twin delayed deep deterministic policy gradient - on the HIP kernels.

Same class surface as the reference's gops/algorithm/td3.py (ApproxContainer :30-64, TD3 :67-283): twin action-value functions
regressed onto the clipped double-Q backup of the smoothed target action, a deterministic policy ascended along q1(o, pi(o)) every
`delay_update` iterations, Polyak-averaged targets.  The arithmetic and its kernels: algorithm/_actor_critic.py.

The reference's oddities are restated, not fixed: `Train/Critic avg value` logs the mean of the scalar critic loss (td3.py:153),
the hyper-parameters gamma / tau / delay_update / reward_scale are attributes set after construction, and with a prioritized
buffer the new priorities are |q1 - backup| only.

The target-policy noise is an INPUT of the update: `data["target_noise"]` holds the unit-normal draws [B, act_dim] (the reference's
`torch.randn_like(pi_targ)`, td3.py:170); when the batch has none they are drawn on the device from a generator this object owns
(seed + index), before the update's graph - the kernel forms clamp(xi * target_noise, -noise_clip, noise_clip).
"""
__all__ = ["ApproxContainer", "TD3"]

from copy import deepcopy

from gops_amd.algorithm._actor_critic import ActorCriticBase
from gops_amd.algorithm.base import ApprBase
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam


class ApproxContainer(ApprBase):
    """q1, q2, policy and their frozen targets; construction order (and with it the RNG draws) follows td3.py:33-60."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q1 = create_apprfunc(**q_args)
        self.q2 = create_apprfunc(**q_args)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.policy = create_apprfunc(**policy_args)
        self.q1_target = deepcopy(self.q1)
        self.q2_target = deepcopy(self.q2)
        self.policy_target = deepcopy(self.policy)
        for net in (self.q1_target, self.q2_target, self.policy_target):
            for p in net.parameters():
                p.requires_grad = False
        self.q1_optimizer = make_adam(self.q1.parameters(), lr=kwargs["value_learning_rate"])
        self.q2_optimizer = make_adam(self.q2.parameters(), lr=kwargs["value_learning_rate"])
        self.policy_optimizer = make_adam(self.policy.parameters(), lr=kwargs["policy_learning_rate"])

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class TD3(ActorCriticBase):
    """target_noise: std of the target policy's smoothing noise; noise_clip: its range; buffer_name: "prioritized_replay_buffer"
    makes `local_update` return (tb_info, idx, |q1 - backup|); fused_target: the Bellman backup as one `gops_ac_backup` launch
    for networks up to 64 wide, where it is the faster form ("force": wherever the kernel holds the shape; False: always composed from
    `gops_mlp_forward` calls and torch elementwise ops)."""

    _q_names = ("q1", "q2")
    _smooth = True

    def __init__(self, target_noise=0.2, noise_clip=0.5, buffer_name="replay_buffer", index=0, fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.target_noise = target_noise
        self.noise_clip = noise_clip
        self.gamma = 0.99
        self.tau = 0.005
        self.delay_update = 2
        self.reward_scale = 1
        self._init_common(index, buffer_name, fused_target, kwargs)

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "delay_update", "reward_scale")

    def _logged_value(self, stats):   # td3.py:153: torch.mean(loss_q) - the mean of a scalar
        return stats[3]
