"""Action distributions.

The ADP algorithms, DDPG and TD3 only ever use the Dirac distribution (the policy output IS the
action; reference gops/utils/act_distribution_type.py:141-150 and the mixin
gops/utils/act_distribution_cls.py:13-27 that samplers/evaluators call through
`networks.create_action_distributions(logits)`).  DSAC-T's StochaPolicy emits `cat(mean, std)`: the diagonal Gaussian and its
tanh-squashed form (act_distribution_type.py:18-113).  Their `sample` / `rsample` take the unit-normal draws as an optional
argument: wherever a result has to be reproducible the draws are an input of the computation.  Discrete action spaces (DQN's
ActionValueDis) have the arg-max over action values, ValueDiracDistribution, and the categorical distribution (:116-160).
"""
import math

import torch

EPS = 1e-6   # inside the log of the tanh correction (act_distribution_type.py:15)


class GaussDistribution:
    """Independent normal per action dimension; logits = cat(mean, std)."""

    def __init__(self, logits: torch.Tensor):
        self.logits = logits
        self.mean, self.std = torch.chunk(logits, chunks=2, dim=-1)
        self.act_high_lim = torch.tensor([1.0])
        self.act_low_lim = torch.tensor([-1.0])

    def _draw(self, eps, generator=None):
        if eps is None:
            eps = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * eps

    def _gauss_log_prob(self, u):
        return (-((u - self.mean) ** 2) / (2 * self.std ** 2) - torch.log(self.std) - 0.5 * math.log(2 * math.pi)).sum(-1)

    def rsample(self, eps=None, generator=None):
        u = self._draw(eps, generator)
        return u, self._gauss_log_prob(u)

    def sample(self, eps=None, generator=None):
        with torch.no_grad():
            return self.rsample(eps, generator)

    def log_prob(self, action):
        return self._gauss_log_prob(action)

    def entropy(self):
        return (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(self.std)).sum(-1)

    def kl_divergence(self, other: "GaussDistribution") -> torch.Tensor:
        """KL(self || other) of the two diagonal Gaussians, summed over the action dimensions (act_distribution_type.py:110-113)."""
        ratio2 = (self.std / other.std) ** 2
        return (0.5 * (ratio2 + ((self.mean - other.mean) / other.std) ** 2 - 1 - torch.log(ratio2))).sum(-1)

    def mode(self):
        return torch.clamp(self.mean, self.act_low_lim, self.act_high_lim)


class TanhGaussDistribution(GaussDistribution):
    """The Gaussian draw u squashed into the action limits: a = half * tanh(u) + mid, with the change-of-variables term in the
    log-probability (EPS keeps the log finite where tanh saturates)."""

    def _half_mid(self):
        return (self.act_high_lim - self.act_low_lim) / 2, (self.act_high_lim + self.act_low_lim) / 2

    def _squashed(self, u):
        half, mid = self._half_mid()
        th = torch.tanh(u)
        logp = self._gauss_log_prob(u) - torch.log(1 + EPS - th ** 2).sum(-1) - torch.log(half).sum(-1)
        return half * th + mid, logp

    def rsample(self, eps=None, generator=None):
        return self._squashed(self._draw(eps, generator))

    def log_prob(self, action_limited):
        half, mid = self._half_mid()
        u = torch.atanh((1 - EPS) * (action_limited - mid) / half)
        return self._gauss_log_prob(u) - torch.log(half * (1 + EPS - torch.tanh(u) ** 2)).sum(-1)

    def mode(self):
        half, mid = self._half_mid()
        return half * torch.tanh(self.mean) + mid


class DiracDistribution:
    def __init__(self, logits: torch.Tensor):
        self.logits = logits

    def sample(self):
        return self.logits, torch.tensor([0.0])

    def mode(self):
        return self.logits


class CategoricalDistribution:
    """Discrete actions with probabilities softmax(logits) (act_distribution_type.py:116-138)."""

    def __init__(self, logits: torch.Tensor):
        self.logits = logits
        self.cat = torch.distributions.Categorical(logits=logits)

    def sample(self):
        action = self.cat.sample()
        return action, self.log_prob(action)

    def log_prob(self, action: torch.Tensor) -> torch.Tensor:
        if action.dim() > 1:
            action = action.squeeze(1)
        return self.cat.log_prob(action)

    def entropy(self):
        return self.cat.entropy()

    def mode(self):
        return torch.argmax(self.logits, dim=-1)

    def kl_divergence(self, other: "CategoricalDistribution"):
        return torch.distributions.kl.kl_divergence(self.cat, other.cat)


class ValueDiracDistribution:
    """The logits are action values: the action is their arg-max (act_distribution_type.py:152-160)."""

    def __init__(self, logits: torch.Tensor):
        self.logits = logits

    def sample(self):
        return torch.argmax(self.logits, dim=-1), torch.tensor([0.0])

    def mode(self):
        return torch.argmax(self.logits, dim=-1)


class Action_Distribution:
    """Mixin: builds `self.action_distribution_cls(logits)` and attaches the action limits."""

    def get_act_dist(self, logits):
        dist = getattr(self, "action_distribution_cls")(logits)
        if hasattr(self, "act_high_lim"):
            dist.act_high_lim = getattr(self, "act_high_lim")
            dist.act_low_lim = getattr(self, "act_low_lim")
        return dist
