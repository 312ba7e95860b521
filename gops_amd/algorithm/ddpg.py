"""DDPG - deep deterministic policy gradient - on the HIP kernels.

Same class surface as the reference's gops/algorithm/ddpg.py (ApproxContainer :30-63, DDPG :66-223): an action-value function
regressed onto `r + gamma (1 - d) q_target(o2, policy_target(o2))`, a deterministic policy ascended along q(o, pi(o)) every
`delay_update` iterations, Polyak-averaged targets.  The arithmetic and its kernels: algorithm/_actor_critic.py.

As in the reference, gamma / tau / delay_update are attributes set after construction, `Train/Critic avg value` logs mean(q), and
the policy optimizer is built before the critic's (ddpg.py:56-59).
"""
__all__ = ["ApproxContainer", "DDPG"]

from copy import deepcopy

from gops_amd.algorithm._actor_critic import ActorCriticBase
from gops_amd.algorithm.base import ApprBase
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam


class ApproxContainer(ApprBase):
    """q, policy and their frozen targets; construction order (and with it the RNG draws) follows ddpg.py:37-59."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q = create_apprfunc(**q_args)
        policy_args = get_apprfunc_dict("policy", **kwargs)
        self.policy = create_apprfunc(**policy_args)
        self.q_target = deepcopy(self.q)
        self.policy_target = deepcopy(self.policy)
        for net in (self.q_target, self.policy_target):
            for p in net.parameters():
                p.requires_grad = False
        self.policy_optimizer = make_adam(self.policy.parameters(), lr=kwargs["policy_learning_rate"])
        self.q_optimizer = make_adam(self.q.parameters(), lr=kwargs["value_learning_rate"])

    def create_action_distributions(self, logits):
        return self.policy.get_act_dist(logits)


class DDPG(ActorCriticBase):
    """buffer_name: "prioritized_replay_buffer" makes `local_update` return (tb_info, idx, |q - backup|); fused_target: the Bellman
    backup as one `gops_ac_backup` launch for networks up to 64 wide, where it is the faster form ("force": wherever the kernel holds the shape; False: always composed from
    `gops_mlp_forward` calls and torch elementwise ops)."""

    _q_names = ("q",)
    _smooth = False

    def __init__(self, index=0, buffer_name="replay_buffer", fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.networks = ApproxContainer(**kwargs)
        self.gamma = 0.99
        self.tau = 0.005
        self.delay_update = 1
        self._init_common(index, buffer_name, fused_target, kwargs)

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau", "delay_update")

    def _logged_value(self, stats):   # ddpg.py:136,155: torch.mean(q)
        return stats[2]
