"""POLY approximate functions of the ADP path: DetermPolicy, FiniteHorizonPolicy, StateValue.

Parameter names (`pi.weight` / `pi.bias`, `v.weight` / `v.bias`), registered buffers (`act_high_lim` / `act_low_lim`) and
`forward` arithmetic follow the reference (gops/apprfunc/poly.py:30-83,89-155,239-262) so that its `apprfunc_*.pkl` checkpoints
load unchanged.  `forward` is the eager definition used by samplers and evaluators; inside `compute_gradient` the same parameters
are read in place by the HIP POLY rollout (`hip_mlp()`: a one-layer `GopsMlp` with a feature-map code, ABI v15), which never calls
`forward`.  Unlike the reference, the features are built on the input's device.
"""
__all__ = ["DetermPolicy", "FiniteHorizonPolicy", "StateValue"]

import weakref
from math import factorial

import numpy as np
import torch
import torch.nn as nn

from gops_amd.utils.act_distribution import Action_Distribution


def make_features(x, degree):
    """Degree k block = the k-fold outer product of x in n_matmul order (reference poly.py:30-49)."""
    def matmul_crossing(a, b):
        batchsize = a.size(0)
        return torch.matmul(torch.transpose(a.unsqueeze(1), -1, -2), b.unsqueeze(1)).reshape(batchsize, -1)

    def n_matmul(x, n):
        a = x
        if n == 0:
            return torch.ones_like(a)
        for _ in range(n - 1):
            a = matmul_crossing(a, x)
        return a

    return torch.cat([n_matmul(x, i) for i in range(1, degree + 1)], 1)


def get_features_dim(input_dim, degree):
    return sum(input_dim ** k for k in range(1, degree + 1))


def combination(m, n):
    return int(factorial(m) / (factorial(n) * factorial(m - n)))


def create_features(x, degree=2):
    """x_i x_j for i <= j, i-major (reference poly.py:61-83), on x's device."""
    if degree != 2:
        raise ValueError("Not set degree properly")
    batch, obs_dim = x.shape[0], x.shape[1]
    features = torch.zeros((batch, combination(degree + obs_dim - 1, degree)), device=x.device)
    k = 0
    for i in range(0, obs_dim):
        for j in range(i, obs_dim):
            features[:, k:k + 1] = torch.mul(x[:, i:i + 1], x[:, j:j + 1])
            k = k + 1
    return features


def count_features_dim(input_dim, degree):
    if degree != 2:
        raise ValueError("Not set degree properly")
    return combination(degree + input_dim - 1, degree)


# ctypes structs cannot be pickled / deep-copied: the C-ABI views live outside the modules, keyed weakly by module
_HIP_CACHE = weakref.WeakKeyDictionary()


class _HipPolyMixin:
    """Exports the one Linear layer as a C-ABI POLY `GopsMlp` over the live parameter storage."""

    is_poly = True

    def linear_layers(self):
        return [getattr(self, self._net_attr)]

    def _feature_code(self):
        from gops_amd import hip_backend as hb
        if self.degree not in hb.POLY_FULL:
            raise RuntimeError(f"POLY degree {self.degree} is outside the HIP path (1, 2, 3)")
        return hb.POLY_FULL[self.degree]

    def _norm_device(self, device):
        return None

    def hip_mlp(self, dtype=None, variant_flags=None):
        """The POLY net as `GopsMlp` (n_layers = 1); `dtype` must be fp32 and `variant_flags` empty (no kernel variants)."""
        from gops_amd import hip_backend as hb
        if hb.dtype_id(dtype) != 0:
            raise RuntimeError("POLY approximators run in fp32 only (mlp_dtype fp16 is an MLP setting)")
        lin = getattr(self, self._net_attr)
        norm = self._norm_device(lin.weight.device)
        key = (lin.weight.data_ptr(), 0 if lin.bias is None else lin.bias.data_ptr(), 0 if norm is None else norm.data_ptr())
        cached = _HIP_CACHE.get(self)
        if cached is None or cached[0] != key:
            mlp = hb.make_poly(lin.weight.data, None if lin.bias is None else lin.bias.data, self._feature_code(), norm)
            _HIP_CACHE[self] = (key, mlp)
            return mlp
        return cached[1]


class DetermPolicy(nn.Module, Action_Distribution, _HipPolyMixin):
    """Deterministic policy: a = pi(features(obs)), no squash (the wrapper chain bounds the action)."""

    _net_attr = "pi"
    _time_input = False

    def __init__(self, **kwargs):
        super().__init__()
        obs_dim, act_dim = kwargs["obs_dim"], kwargs["act_dim"]
        self.degree = kwargs["degree"]
        self.add_bias = kwargs["add_bias"]
        self.pi = nn.Linear(get_features_dim(obs_dim, self.degree) + (1 if self._time_input else 0), act_dim, bias=self.add_bias)
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))
        self.action_distribution_cls = kwargs["action_distribution_cls"]

    def forward(self, obs):
        return self.pi(make_features(obs, self.degree))


class FiniteHorizonPolicy(DetermPolicy):
    """Finite-horizon policy: the virtual time step is one more column AFTER the features (not raised to any power)."""

    _time_input = True

    def forward(self, obs, virtual_t=1):
        obs = make_features(obs, self.degree)
        virtual_t = virtual_t * torch.ones(size=[obs.shape[0], 1], dtype=torch.float32, device=obs.device)
        return self.pi(torch.cat((obs, virtual_t), 1))


class StateValue(nn.Module, Action_Distribution, _HipPolyMixin):
    """State value: v(create_features(obs * norm_matrix, 2)); norm_matrix is a plain attribute, not a buffer (as in the reference)."""

    _net_attr = "v"

    def __init__(self, **kwargs):
        super().__init__()
        obs_dim = kwargs["obs_dim"]
        self.add_bias = kwargs["add_bias"]
        norm = kwargs.get("norm_matrix")
        self.norm_matrix = torch.from_numpy(np.array([1.0] * obs_dim if norm is None else norm, dtype=np.float32))
        self.degree = kwargs["degree"]
        self.v = nn.Linear(count_features_dim(obs_dim, self.degree), 1, bias=self.add_bias)
        self.action_distribution_cls = kwargs["action_distribution_cls"]

    def forward(self, obs):
        obs = create_features(torch.mul(obs, self.norm_matrix.to(obs.device)), self.degree)
        return self.v(obs).squeeze(-1)

    def _feature_code(self):
        from gops_amd import hip_backend as hb
        if self.degree != 2:
            raise RuntimeError(f"POLY StateValue degree {self.degree}: only 2 exists (reference create_features)")
        return hb.POLY_SYM_2

    def _norm_device(self, device):
        # (a device copy per host tensor version: no host sync, so the caller may be inside a graph capture)
        key = (id(self.norm_matrix), self.norm_matrix._version, str(device))
        cached = getattr(self, "_norm_dev", None)
        if cached is None or cached[0] != key:
            cached = self._norm_dev = (key, self.norm_matrix.to(device).contiguous())
        return cached[1]
