"""RNN approximate functions: DetermPolicy, StochaPolicy, StateValue, ActionValueDis over a STACK of observations [B, L, O] - an Elman
recurrence h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh) from h_0 = 0 whose last hidden state feeds MLP heads.

Parameter names and shapes follow the reference (gops/apprfunc/rnn.py: `rnn.weight_ih_l0` ... of an `nn.RNN(O, hidden_sizes[0])`, then
`pi.*` / `mean.*`, `log_std.*` / `v.*` / `q.*` of `mlp(hidden_sizes + [out])`) so that its checkpoints load unchanged.  `obs_dim` is
the pair (L, O): only O shapes the parameters, L is read from the input at the call.  `forward` is the eager definition; PPO reads the
same parameters in place through `gops_rnn_forward / _backward` (`hip_rnn()`), which never calls `forward`.
"""
__all__ = ["DetermPolicy", "FiniteHorizonPolicy", "StochaPolicy", "ActionValue", "ActionValueDis", "StateValue"]

import torch
import torch.nn as nn

from gops_amd.apprfunc.mlp import _HIP_CACHE, mlp
from gops_amd.utils.act_distribution import Action_Distribution
from gops_amd.utils.common_utils import get_activation_func


class _RnnBase(nn.Module, Action_Distribution):
    """The recurrence and the heads named in `_heads` (attribute names, each `mlp(hidden_sizes + [out])`), and their C-ABI view."""

    is_rnn = True
    _heads = ()

    def _build(self, out_dim: int, kwargs: dict):
        hidden = list(kwargs["hidden_sizes"])
        self._hidden_activation = kwargs["hidden_activation"]
        self._output_activation = kwargs.get("output_activation", "linear")
        self.rnn = nn.RNN(kwargs["obs_dim"][1], hidden[0], 1, batch_first=True)
        for name in self._heads:
            setattr(self, name, mlp(hidden + [out_dim], get_activation_func(self._hidden_activation),
                                    get_activation_func(self._output_activation)))
        self.action_distribution_cls = kwargs["action_distribution_cls"]

    def last_hidden(self, obs):
        return self.rnn(obs)[1].squeeze(0)

    def recurrent_parameters(self):
        r = self.rnn
        return [r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0]

    def head_layers(self):
        return [[m for m in getattr(self, name) if isinstance(m, nn.Linear)] for name in self._heads]

    def hip_rnn(self, seq_len: int):
        """The C-ABI `GopsRnn` over the live parameter storage for inputs [B, seq_len, O], cached outside the module (ctypes structs
        cannot be deep-copied) and rebuilt when the storage moved."""
        from gops_amd import hip_backend as hb
        if self._output_activation != "linear":
            raise RuntimeError("the HIP recurrent kernels support a linear output activation only")
        tensors = [p.data for p in self.parameters()]
        key = tuple(t.data_ptr() for t in tensors) + (int(seq_len),)
        cached = _HIP_CACHE.get(self)
        if cached is None or cached[0] != key:
            heads = [([l.weight.data for l in layers], [l.bias.data for l in layers]) for layers in self.head_layers()]
            cached = _HIP_CACHE[self] = (key, hb.make_rnn([p.data for p in self.recurrent_parameters()], heads, self._hidden_activation, seq_len))
        return cached[1]

    def hip_rnn_grad(self):
        """The `GopsRnnGrad` over the parameters' `.grad` tensors (allocated by the caller: algorithm/base.py `_flat_grads`)."""
        from gops_amd import hip_backend as hb
        return hb.make_rnn_grad([p.grad for p in self.recurrent_parameters()],
                                [([l.weight.grad for l in layers], [l.bias.grad for l in layers]) for layers in self.head_layers()])


class DetermPolicy(_RnnBase):
    """Deterministic policy: stacked obs -> tanh-squashed action."""

    _heads = ("pi",)

    def __init__(self, **kwargs):
        super().__init__()
        self._build(kwargs["act_dim"], kwargs)
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))

    def forward(self, obs):
        y = self.pi(self.last_hidden(obs))
        return (self.act_high_lim - self.act_low_lim) / 2 * torch.tanh(y) + (self.act_high_lim + self.act_low_lim) / 2


class FiniteHorizonPolicy(nn.Module, Action_Distribution):
    """Not defined for the recurrent family (the reference's raises too)."""

    def __init__(self, **kwargs):
        raise NotImplementedError


class StochaPolicy(_RnnBase):
    """Stochastic policy: stacked obs -> (mean, std) from two heads over the last hidden state.  `hip_rnn()` exports both heads raw;
    the clamp of log std and the exp belong to the loss kernel (`gops_ppo_loss`) and to `forward`."""

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
        h = self.last_hidden(obs)
        return torch.cat((self.mean(h), self.log_std(h)), dim=-1)

    def forward(self, obs):
        mean, log_std = torch.chunk(self.policy(obs), chunks=2, dim=-1)
        return torch.cat((mean, torch.clamp(log_std, self.min_log_std, self.max_log_std).exp()), dim=-1)


class ActionValue(nn.Module, Action_Distribution):
    """Not on this path: its head takes the last hidden state joined with the action, an input the recurrent kernels do not form."""

    def __init__(self, **kwargs):
        raise NotImplementedError("RNN ActionValue: its head reads h_L || act, which gops_rnn_forward / _backward do not form (the heads "
                                  "they run take h_L alone); StateValue and ActionValueDis are the recurrent value functions here")


class ActionValueDis(_RnnBase):
    """Action-value function of a discrete action space: stacked obs -> the values of all actions."""

    _heads = ("q",)

    def __init__(self, **kwargs):
        super().__init__()
        self.act_num = kwargs["act_num"] if "act_num" in kwargs else kwargs["act_dim"]   # (the reference's reads act_dim)
        self._build(self.act_num, kwargs)

    def forward(self, obs):
        return self.q(self.last_hidden(obs))


class StateValue(_RnnBase):
    """State-value function: stacked obs -> scalar."""

    _heads = ("v",)

    def __init__(self, **kwargs):
        super().__init__()
        self._build(1, kwargs)

    def forward(self, obs):
        return torch.squeeze(self.v(self.last_hidden(obs)), -1)
