"""LipsNet approximate functions of the ADP path: DetermPolicy (reference gops/apprfunc/lipsnet.py:46-233).

    y = K(x) * f(x) / (||df/dx||_F + eps),   action = y  or  the tanh squash of y (`squash_action`)

with f an MLP, K(x) = softplus(scalar) (global) or softplus(small tanh MLP) (local).  Module structure and parameter names
(`pi.mlp.0.weight` ..., `pi.K.K` or `pi.K.K.0.weight` ...), registered buffers and initialisation follow the reference, so its
`apprfunc_*.pkl` checkpoints load unchanged.

`forward` is the eager definition for samplers, evaluators and tests.  Where the reference calls `vmap(jacrev(mlp))`, it
propagates the n tangent columns T_0 = I_n next to the primal row through every layer (z = W h + b, U = W T, h' = act(z),
T' = act'(z) * U; J = W_L T): plain torch ops, differentiable by autograd (act'' comes from differentiating act'), no functorch,
any floating dtype - `.double()` of it is the float64 oracle of the GPU tests.  Inside INFADP's updates the same parameters are
read in place by the HIP tangent-propagation kernels (csrc/rollout_lips.hip, `hip_backend.LipsPolicy`), which never call `forward`.

The regular loss of `lips_auto_adjust` (reference :125-127 and the backward pre-hook :146-149: lambda * mean_b K(x_b)^2 added to
whatever is back-propagated through the module in training mode) enters here as its gradient, 2 lambda K_b / B on K's adjoint;
it is absent in eval mode and where no gradient is recorded, exactly as there.
"""
__all__ = ["DetermPolicy", "StochaPolicy"]

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from gops_amd.utils.act_distribution import Action_Distribution
from gops_amd.utils.common_utils import get_activation_func

_SELU_SCALE, _SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def act_derivative(name: str, z: torch.Tensor) -> torch.Tensor:
    """act'(z) of the project's activation set, as torch's own backward formulas give it (relu'(0) = 0; gelu in erf form)."""
    if name == "relu":
        return (z > 0).to(z.dtype)
    if name == "elu":
        return torch.where(z > 0, torch.ones_like(z), torch.exp(torch.clamp(z, max=0.0)))
    if name == "selu":
        return _SELU_SCALE * torch.where(z > 0, torch.ones_like(z), _SELU_ALPHA * torch.exp(torch.clamp(z, max=0.0)))
    if name == "gelu":
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if name == "sigmoid":
        s = torch.sigmoid(z)
        return s * (1.0 - s)
    if name == "tanh":
        t = torch.tanh(z)
        return 1.0 - t * t
    raise RuntimeError(f"LipsNet: unknown hidden activation {name!r}")


class _RegularLossGrad(torch.autograd.Function):
    """Identity on K whose backward adds d(lambda mean K^2)/dK = 2 lambda K / B to the incoming adjoint."""

    @staticmethod
    def forward(ctx, k, lam):
        ctx.save_for_backward(k)
        ctx.lam = lam
        return k.view_as(k)

    @staticmethod
    def backward(ctx, g):
        (k,) = ctx.saved_tensors
        return g + (2.0 * ctx.lam / k.shape[0]) * k, None


def _init_linear_stack(seq):
    for i, m in enumerate(seq):   # reference :59-66, :97-104
        if isinstance(m, nn.Linear):
            if isinstance(seq[i + 1], nn.ReLU):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            else:
                nn.init.xavier_normal_(m.weight)


class Lips_K(nn.Module):
    """K(x): softplus of one trainable scalar (global) or of a tanh MLP obs -> 1 (local); reference :46-75."""

    def __init__(self, local, lips_start, sizes):
        super().__init__()
        self.local = bool(local)
        if self.local:
            layers = []
            for j in range(len(sizes) - 2):
                layers += [nn.Linear(sizes[j], sizes[j + 1]), nn.Tanh()]
            layers += [nn.Linear(sizes[-2], sizes[-1], bias=True), nn.Softplus()]
            self.K = nn.Sequential(*layers)
            _init_linear_stack(self.K)
            self.K[-2].bias.data += torch.tensor(lips_start, dtype=torch.float).data
        else:
            self.K = nn.Parameter(torch.tensor(lips_start, dtype=torch.float), requires_grad=True)

    def linear_layers(self):
        return [m for m in self.K if isinstance(m, nn.Linear)] if self.local else []

    def forward(self, x):
        if self.local:
            return self.K(x)
        return F.softplus(self.K).repeat(x.shape[0]).unsqueeze(1)


class LipsNet(nn.Module):
    """The multi-dimensional gradient normalisation of an MLP (reference :79-144)."""

    def __init__(self, sizes, hidden_activation, lips_init_value, eps, lips_auto_adjust, loss_lambda, local_lips, lips_hidden_sizes):
        super().__init__()
        act = get_activation_func(hidden_activation)
        layers = []
        for j in range(len(sizes) - 2):
            layers += [nn.Linear(sizes[j], sizes[j + 1]), act()]
        layers += [nn.Linear(sizes[-2], sizes[-1]), nn.Identity()]
        self.mlp = nn.Sequential(*layers)
        _init_linear_stack(self.mlp)
        self._hidden_activation = hidden_activation
        self.local = bool(local_lips)
        self.K = Lips_K(local_lips, lips_init_value, lips_hidden_sizes)
        self.loss_lambda = float(loss_lambda)
        self.eps = float(eps)
        self.lips_auto_adjust = bool(lips_auto_adjust)

    def linear_layers(self):
        return [m for m in self.mlp if isinstance(m, nn.Linear)]

    def value_and_jacobian(self, x):
        """(f [B, m], J [B, m, n]) by propagating the n tangent columns next to the primal row."""
        B, n = x.shape
        layers = self.linear_layers()
        h = x
        T = torch.eye(n, dtype=x.dtype, device=x.device).expand(B, n, n)   # [B, column, feature]
        for lin in layers[:-1]:
            z = F.linear(h, lin.weight, lin.bias)
            U = T @ lin.weight.t()
            h = get_activation_func(self._hidden_activation)()(z)
            T = act_derivative(self._hidden_activation, z).unsqueeze(1) * U
        f = F.linear(h, layers[-1].weight, layers[-1].bias)
        J = (T @ layers[-1].weight.t()).transpose(1, 2)
        return f, J

    def parts(self, x):
        """(y, K [B, 1], N [B, 1]): the normalised output, K(x) and the Frobenius norm of the Jacobian."""
        k = self.K(x)
        if self.lips_auto_adjust and self.training and k.requires_grad:
            k = _RegularLossGrad.apply(k, self.loss_lambda)
        if k.requires_grad:
            f, J = self.value_and_jacobian(x)
        else:   # (reference :132-136: without a gradient on K the Jacobian is formed outside the graph)
            f = self.mlp(x)
            with torch.no_grad():
                J = self.value_and_jacobian(x)[1]
        norm = torch.norm(J, 2, dim=(1, 2)).unsqueeze(1)
        return k * f / (norm + self.eps), k, norm

    def forward(self, x):
        return self.parts(x)[0]


class DetermPolicy(nn.Module, Action_Distribution):
    """Deterministic LipsNet policy: obs -> action (tanh-squashed into the action limits with `squash_action`)."""

    is_lipsnet = True
    _time_input = False

    def __init__(self, **kwargs):
        super().__init__()
        obs_dim, act_dim = kwargs["obs_dim"], kwargs["act_dim"]
        for key in ("lips_init_value", "lips_auto_adjust", "local_lips", "lambda", "squash_action", "learning_rate", "lips_learning_rate"):
            assert kwargs.get(key) is not None, f"LipsNet DetermPolicy: `{key}` is required"
        if kwargs.get("output_activation", "linear") != "linear":
            raise NotImplementedError(f"LipsNet DetermPolicy: output activation {kwargs['output_activation']!r} - the normalisation "
                                      "and the HIP kernels are defined for a linear output layer only")
        if str(kwargs.get("mlp_dtype", "fp32") or "fp32").lower() in ("fp16", "f16", "float16", "half"):
            raise NotImplementedError("LipsNet DetermPolicy: fp16 - the tangent-propagation kernels are fp32 only")
        local = bool(kwargs["local_lips"])
        lips_hidden = kwargs.get("lips_hidden_sizes")
        if local:
            assert lips_hidden is not None, "LipsNet DetermPolicy: local_lips needs lips_hidden_sizes"
            lips_hidden = [obs_dim] + list(lips_hidden) + [1]
        self.squash_action = bool(kwargs["squash_action"])
        self.learning_rate = kwargs["learning_rate"]
        self.lips_learning_rate = kwargs["lips_learning_rate"]
        self._hidden_activation = kwargs["hidden_activation"]
        self._output_activation = "linear"
        self.pi = LipsNet([obs_dim] + list(kwargs["hidden_sizes"]) + [act_dim], self._hidden_activation, kwargs["lips_init_value"],
                          kwargs.get("eps", 1e-4), kwargs["lips_auto_adjust"], kwargs["lambda"], local, lips_hidden)
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))
        self.action_distribution_cls = kwargs["action_distribution_cls"]
        self.eval()

    # `parameters()` stays nn.Module's (mlp tensors, then K's: the reference's order); the reference's override, a list of
    # {"params", "lr"} entries, is `param_groups()` here
    def mlp_parameters(self):
        return list(self.pi.mlp.parameters())

    def lips_parameters(self):
        return list(self.pi.K.parameters())

    def param_groups(self):
        return [dict(params=self.mlp_parameters(), lr=self.learning_rate), dict(params=self.lips_parameters(), lr=self.lips_learning_rate)]

    def linear_layers(self):
        return self.pi.linear_layers()

    def _squash(self, y):
        if not self.squash_action:
            return y
        return (self.act_high_lim - self.act_low_lim) / 2 * torch.tanh(y) + (self.act_high_lim + self.act_low_lim) / 2

    def forward(self, obs):
        return self._squash(self.pi(obs))

    def forward_parts(self, obs):
        """(action, K [B], N [B]) - what `hip_backend.LipsPolicy.forward` returns."""
        y, k, norm = self.pi.parts(obs)
        return self._squash(y), k.squeeze(1), norm.squeeze(1)


class StochaPolicy(nn.Module):
    """The reference's stochastic LipsNet policy serves the model-free algorithms, which are outside this package."""

    def __init__(self, **kwargs):
        raise NotImplementedError("LipsNet StochaPolicy is outside the MI355X ADP path (model-based algorithms take a DetermPolicy)")
