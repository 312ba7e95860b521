"""CNN approximate functions: DetermPolicy, StochaPolicy, StateValue, ActionValueDis, StochaPolicyDis over an image [B, C, H, W] - a stack
of Conv2d + ReLU layers without padding whose flattened output feeds MLP heads.

Parameter names and shapes follow the reference (gops/apprfunc/cnn.py: `conv.{0,2,..}.weight / bias` of its `CNN(...)`, then `mlp.*` - or
`mean.*`, `log_std.*` for a StochaPolicy - of `MLP([F] + hidden + [out])`) so that its checkpoints load unchanged; the two geometries are
its `conv_type` tables (CONV_TYPES; the ReLU of the convolutions is fixed there, `hidden_activation` belongs to the heads).  `forward` is
the eager definition; PPO reads the same parameters in place through `gops_conv_forward / _backward` and `gops_mlp_*` (`hip_cnn()`),
which never calls `forward`.
"""
__all__ = ["DetermPolicy", "FiniteHorizonPolicy", "StochaPolicy", "ActionValue", "ActionValueDis", "ActionValueDistri", "StochaPolicyDis",
           "StateValue"]

import torch
import torch.nn as nn

from gops_amd.apprfunc.mlp import _HIP_CACHE, mlp
from gops_amd.utils.act_distribution import Action_Distribution
from gops_amd.utils.common_utils import get_activation_func

# conv_type -> kernels, channels, strides, the heads' hidden widths (`short`: those of StateValue and ActionValueDis)
CONV_TYPES = {
    "type_1": dict(kernels=(8, 4, 3), channels=(32, 64, 64), strides=(4, 2, 1), hidden=(512, 256), short=(512,)),
    "type_2": dict(kernels=(4, 3, 3, 3, 3, 3), channels=(8, 16, 32, 64, 128, 256), strides=(2, 2, 2, 2, 1, 1), hidden=(256, 256, 256),
                   short=(256, 256, 256)),
}


def feature_shape(conv_type: str, obs_dim):
    """(C, H, W) of the last convolution's output for an input of `obs_dim` = (C, H, W); an extent of 0: the image is too small."""
    from gops_amd.hip_backend import conv_out_shape
    t = CONV_TYPES[conv_type]
    return conv_out_shape(obs_dim, t["channels"], t["kernels"], t["strides"])


class _CnnBase(nn.Module, Action_Distribution):
    """The convolutions and the heads named in `_heads` (attribute names, each `mlp([F] + hidden + [out])`), and their C-ABI view."""

    is_cnn = True
    _heads = ("mlp",)
    _short_head = False

    def _build(self, out_dim: int, kwargs: dict):
        if kwargs["conv_type"] not in CONV_TYPES:
            raise NotImplementedError(f"conv_type {kwargs['conv_type']!r} ({', '.join(CONV_TYPES)} only)")
        t = CONV_TYPES[kwargs["conv_type"]]
        self.obs_dim = tuple(int(v) for v in kwargs["obs_dim"])
        self.strides = t["strides"]
        self._hidden_activation = kwargs["hidden_activation"]
        self._output_activation = kwargs.get("output_activation", "linear")
        C, H, W = feature_shape(kwargs["conv_type"], self.obs_dim)
        if H < 1 or W < 1:
            raise ValueError(f"an image of {self.obs_dim} is too small for the convolutions of {kwargs['conv_type']}")
        layers, c_in = [], self.obs_dim[0]
        for n, k, s in zip(t["channels"], t["kernels"], t["strides"]):
            layers += [nn.Conv2d(c_in, n, k, s), nn.ReLU()]
            c_in = n
        self.conv = nn.Sequential(*layers)
        sizes = [C * H * W] + list(t["short" if self._short_head else "hidden"]) + [out_dim]
        for name in self._heads:
            setattr(self, name, mlp(sizes, get_activation_func(self._hidden_activation), get_activation_func(self._output_activation)))
        self.action_distribution_cls = kwargs["action_distribution_cls"]

    def features(self, obs):
        img = self.conv(obs)
        return img.view(img.size(0), -1)

    def conv_layers(self):
        return [m for m in self.conv if isinstance(m, nn.Conv2d)]

    def head_layers(self):
        return [[m for m in getattr(self, name) if isinstance(m, nn.Linear)] for name in self._heads]

    def hip_cnn(self):
        """(`GopsConv`, [`GopsMlp` per head]) over the live parameter storage, cached outside the module (ctypes structs cannot be
        deep-copied) and rebuilt when the storage moved."""
        from gops_amd import hip_backend as hb
        if self._output_activation != "linear":
            raise RuntimeError("the HIP convolution path supports a linear output activation only")
        key = tuple(p.data_ptr() for p in self.parameters())
        cached = _HIP_CACHE.get(self)
        if cached is None or cached[0] != key:
            convs = self.conv_layers()
            desc = (hb.make_conv([c.weight.data for c in convs], [c.bias.data for c in convs], self.strides, self.obs_dim[1:]),
                    [hb.make_mlp([l.weight.data for l in layers], [l.bias.data for l in layers], self._hidden_activation)
                     for layers in self.head_layers()])
            cached = _HIP_CACHE[self] = (key, desc)
        return cached[1]

    def hip_cnn_grad(self):
        """`CnnNet.backward`'s gradient set over the parameters' `.grad` tensors (allocated by the caller: algorithm/base.py
        `_flat_grads`)."""
        from gops_amd import hip_backend as hb
        convs = self.conv_layers()
        return (hb.make_conv_grad([c.weight.grad for c in convs], [c.bias.grad for c in convs]),
                [([l.weight.grad for l in layers], [l.bias.grad for l in layers]) for layers in self.head_layers()])


class DetermPolicy(_CnnBase):
    """Deterministic policy: image -> tanh-squashed action."""

    def __init__(self, **kwargs):
        super().__init__()
        self._build(kwargs["act_dim"], kwargs)
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))

    def forward(self, obs):
        y = self.mlp(self.features(obs))
        return (self.act_high_lim - self.act_low_lim) / 2 * torch.tanh(y) + (self.act_high_lim + self.act_low_lim) / 2


class FiniteHorizonPolicy(nn.Module, Action_Distribution):
    """Not defined for the convolutional family (the reference's raises too)."""

    def __init__(self, **kwargs):
        raise NotImplementedError


class StochaPolicy(_CnnBase):
    """Stochastic policy: image -> (mean, std) from two heads over the features.  `hip_cnn()` exports both heads raw; the clamp of
    log std and the exp belong to the loss kernel (`gops_ppo_loss`) and to `forward`."""

    _heads = ("mean", "log_std")

    def __init__(self, **kwargs):
        super().__init__()
        self.act_dim = kwargs["act_dim"]
        self.min_log_std = kwargs["min_log_std"]
        self.max_log_std = kwargs["max_log_std"]
        self._build(self.act_dim, kwargs)
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))

    def policy(self, obs):
        """The raw head mean || log std [B, 2 act_dim]: what the kernels emit, under the attribute name of the MLP StochaPolicy's stack."""
        f = self.features(obs)
        return torch.cat((self.mean(f), self.log_std(f)), dim=-1)

    def forward(self, obs):
        mean, log_std = torch.chunk(self.policy(obs), chunks=2, dim=-1)
        return torch.cat((mean, torch.clamp(log_std, self.min_log_std, self.max_log_std).exp()), dim=-1)


def _joins_the_action(name):
    def __init__(self, **kwargs):
        raise NotImplementedError(f"CNN {name}: its head reads features || act, an input the convolution path does not form (the heads take "
                                  "the features alone); StateValue and ActionValueDis are the convolutional value functions here")
    return type(name, (nn.Module, Action_Distribution), dict(__init__=__init__, __doc__="Not on this path: the action joins the features."))


ActionValue = _joins_the_action("ActionValue")
ActionValueDistri = _joins_the_action("ActionValueDistri")


class ActionValueDis(_CnnBase):
    """Action-value function of a discrete action space: image -> the values of all actions."""

    _short_head = True

    def __init__(self, **kwargs):
        super().__init__()
        self.act_num = kwargs["act_num"]
        self._build(self.act_num, kwargs)

    def forward(self, obs):
        return torch.squeeze(self.mlp(self.features(obs)), -1)


class StochaPolicyDis(ActionValueDis):
    """Stochastic policy of a discrete action space: image -> the logits of all actions (the reference's is its ActionValueDis)."""


class StateValue(_CnnBase):
    """State-value function: image -> scalar."""

    _short_head = True

    def __init__(self, **kwargs):
        super().__init__()
        self._build(1, kwargs)

    def forward(self, obs):
        return torch.squeeze(self.mlp(self.features(obs)), -1)
