"""The diagonal-Gaussian head on a policy's RAW output (mean, raw log std), restated once in torch at any dtype for ppo_helpers.py and
trpo_helpers.py: the clamp's default bounds, clamp and exp, log-probability, KL, and raw log stds on both sides of the clamp."""
import torch

MIN_LS, MAX_LS = -3.0, -0.5


def gauss(head, min_ls=MIN_LS, max_ls=MAX_LS):
    """(mean, std) of a raw head [.., 2A]."""
    mean, raw = torch.chunk(head, 2, dim=-1)
    return mean, torch.clamp(raw, min_ls, max_ls).exp()


def logits_of(head, min_ls=MIN_LS, max_ls=MAX_LS):
    """cat(mean, std) [.., 2A]: what the policy hands to its action distribution."""
    return torch.cat(gauss(head, min_ls, max_ls), dim=-1)


def log_prob(head, act, min_ls=MIN_LS, max_ls=MAX_LS):
    mean, std = gauss(head, min_ls, max_ls)
    return torch.distributions.Normal(mean, std).log_prob(act).sum(-1)


def kl_new_old(head, head_old, min_ls=MIN_LS, max_ls=MAX_LS):
    """mean_i KL(pi(head_i) || pi(head_old_i)): `pi.kl_divergence(pi_old).mean()` of trpo.py:148 with torch's kl_normal_normal."""
    new, old = (torch.distributions.Normal(*gauss(h, min_ls, max_ls)) for h in (head, head_old))
    return torch.distributions.kl_divergence(new, old).sum(-1).mean()


def raw_log_std(M, A, generator):
    """Raw log stds [M, A] in float64 on both sides of the clamp and at least 0.01 away from its bounds."""
    raw = -1.75 + 1.6 * torch.randn(M, A, generator=generator, dtype=torch.float64)
    for b in (MIN_LS, MAX_LS):
        raw = torch.where((raw - b).abs() < 0.01, raw + 0.03, raw)
    return raw
