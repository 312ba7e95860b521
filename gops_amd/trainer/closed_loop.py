"""What the drivers of the closed-loop kernels - `Evaluator` (trainer/evaluator.py, `gops_episode_rollout`) and `DeviceEnvSampler`
(trainer/sampler/device_env_sampler.py, `gops_sample_rollout`) - decide the same way: which network the loop reads, the action
table of a discrete action set, the squash limits of the env description, and the name of the path a call took.  Which descriptions
a kernel takes is its driver's own `kernel_refuses`: they answer for different kernels."""
import torch


class ClosedLoopDriver:
    """Mixin over `self.networks` and `self.device`; keeps `self.action_table` and `self.path`."""
    path = None   # how the last call ran: "fused", or "loop: <why the kernel was not used>"

    def _take_action_table(self, action_table):
        self.action_table = None if action_table is None else torch.as_tensor(action_table, dtype=torch.float32).to(self.device).contiguous()
        if self.action_table is not None and self.action_table.dim() != 2:
            raise ValueError("action_table must be [act_num, action_dim]")

    def _policy_module(self):
        """The network the loop reads: `networks.policy`, or - DQN, whose `policy` is a plain function over it - `networks.q`."""
        policy = self.networks.policy
        return policy if isinstance(policy, torch.nn.Module) else getattr(self.networks, "q", policy)

    def _squash_limits(self):
        """(low, high) of `hip_env`, numpy: with a table nothing is squashed and no policy module is there to ask - the limits are the
        table's column extremes; else the policy's."""
        if self.action_table is not None:
            low, high = self.action_table.min(dim=0).values, self.action_table.max(dim=0).values
        else:
            low, high = self.networks.policy.act_low_lim, self.networks.policy.act_high_lim
        return low.cpu().numpy(), high.cpu().numpy()

    def _set_path(self, why) -> bool:
        """`why`: None when the kernel runs, else the reason it does not.  -> whether it runs."""
        self.path = "fused" if why is None else "loop: " + why
        return why is None
