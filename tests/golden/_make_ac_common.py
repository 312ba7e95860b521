"""What make_golden_td3.py, make_golden_sac.py and make_golden_dsact.py share: the cases' shapes, building the reference's algorithm
from a `cfg` (behind the import hook of make_golden.py), recording the draws the reference makes inside an update, and writing the
`in/`, `meta/cfg`, `sd/`, gradient and `tb/` entries of a fixture.  Build container only (needs the reference tree)."""
import json

import numpy as np
import torch

import make_golden as mg  # (installs the reference import hook)

from gops_amd.utils.synthetic import act_dim_of, make_batch

SHAPE_A = dict(env_id="gym_pendulum", batch=70, hidden=(32, 16), act="relu")               # obs 3 / act 1
SHAPE_B = dict(env_id="pyth_lq", lq_config="s4a2", batch=33, hidden=(64,), act="gelu")      # obs 4 / act 2
LIM_A = ([-2.0], [2.0])
LIM_B = ([-1.0, -0.5], [2.0, 0.5])
MIN_LOG_STD, MAX_LOG_STD = -3.0, -0.5
STOCHA = dict(policy_func_name="StochaPolicy", policy_act_distribution="TanhGaussDistribution", policy_min_log_std=MIN_LOG_STD,
              policy_max_log_std=MAX_LOG_STD, alpha_learning_rate=3e-4, buffer_name="replay_buffer")   # the soft families' policy


class DrawTap:
    """Records what `_standard_normal` (rsample), `torch.normal` (Normal.sample) and `torch.randn_like` (TD3's target noise,
    td3.py:170) return while the reference runs."""

    def __enter__(self):
        import torch.distributions.normal as tdn
        self.rsamples, self.samples, self.noise, self._tdn = [], [], [], tdn
        self._orig = tdn._standard_normal, torch.normal, torch.randn_like

        def tapped(fn, into):
            def call(*a, **k):
                x = fn(*a, **k)
                into.append(x.detach().clone())
                return x
            return call

        tdn._standard_normal, torch.normal, torch.randn_like = (tapped(f, l) for f, l in zip(self._orig, (self.rsamples, self.samples, self.noise)))
        return self

    def __exit__(self, *exc):
        self._tdn._standard_normal, torch.normal, torch.randn_like = self._orig


def last_linear(seq):
    return [m for m in seq if isinstance(m, torch.nn.Linear)][-1]


def close(a, b, tol=1e-6):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def build_reference(cls, cfg, lim, seed, **kw):
    """(alg, generator): the reference's `cls` on the networks of `cfg` with action limits `lim`, its targets - which start as
    copies - moved apart (the target policy by less: its head is shaped by the maker's `balance`)."""
    torch.manual_seed(seed)
    base = mg.alg_kwargs(dict(cfg, alg="INFADP", horizon=1), seed, action_low_limit=np.array(lim[0], dtype=np.float32),
                         action_high_limit=np.array(lim[1], dtype=np.float32))
    base.update(algorithm=cls.__name__, value_output_activation="linear", **kw)
    alg = cls(**base)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for n, p in alg.networks.named_parameters():
            if "_target." in n:
                p.add_((0.1 if n.startswith("policy") else 0.6) * (torch.rand(p.shape, generator=g) - 0.5))
    return alg, g


def batch_of(cfg, seed, g):
    B, A = cfg["batch"], act_dim_of(cfg)
    obs = make_batch(dict(cfg, alg="INFADP", horizon=1), seed)["obs"]
    return dict(obs=obs, act=torch.rand(B, A, generator=g) * 2 - 1, rew=torch.randn(B, generator=g),
                obs2=obs + 0.05 * torch.randn(obs.shape, generator=g), done=(torch.rand(B, generator=g) < 0.15).float())


def tanh_gauss_rsample(policy, logits, eps):
    """(action, log-probability, pre-squash u) of the reference's TanhGaussDistribution.rsample with the draw `eps` handed in."""
    lo, hi = policy.act_low_lim, policy.act_high_lim
    half, mid = (hi - lo) / 2, (hi + lo) / 2
    mean, std = torch.chunk(logits, 2, dim=-1)
    u = mean + std * eps
    logp = (torch.distributions.Normal(mean, std).log_prob(u).sum(-1) - torch.log(1 + 1e-6 - torch.tanh(u) ** 2).sum(-1)
            - torch.log(half).sum(-1))
    return half * torch.tanh(u) + mid, logp, u


def arrays(tensors, prefix):
    return {prefix + k: v.numpy().copy() for k, v in tensors.items()}


def state(alg, prefix="sd/"):
    return {k: v.copy() for k, v in mg.sd_to_np(alg.networks.state_dict(), prefix).items()}


def meta_entry(**meta):
    return {"meta/cfg": json.dumps(meta)}


def update_entries(info, tb, log_alpha):
    """Every network's gradients, log_alpha's where it is learnt (`log_alpha`), and the tb values but the timings."""
    out = {}
    for key, grads in info.items():
        if key.endswith("_grad") and key != "log_alpha_grad":
            for i, gr in enumerate(grads):
                out[f"{key}/{i}"] = gr.detach().numpy().copy()
    if log_alpha:
        out["log_alpha_grad"] = info["log_alpha_grad"].detach().numpy().copy()
    for k, v in tb.items():
        if not k.startswith("Time/"):
            out["tb/" + k] = np.float64(v)
    return out


def five_batches(alg, cfg, seed, g, balance, lr=1e-2):
    """The start of a five-update fixture: every learning rate raised to `lr` (each step well above fp32 rounding), five batches,
    `balance` on all five at once.  -> (batches, the `sd0/` entries)."""
    for opt in [v for k, v in vars(alg.networks).items() if k.endswith("_optimizer")]:
        for group in opt.param_groups:
            group["lr"] = lr
    batches = [batch_of(cfg, seed + k, g) for k in range(5)]
    balance({key: torch.cat([b[key] for b in batches]) for key in batches[0]})
    return batches, state(alg, "sd0/")
