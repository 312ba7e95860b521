"""GAUSS approximate functions of the ADP path: DetermPolicy and FiniteHorizonPolicy over radial basis functions.

Parameter names (`pi.C`, `pi.sigma_square`, `pi.w`, `pi.b`), their shapes and draw order, the registered buffers (`act_high_lim` /
`act_low_lim`) and `forward` arithmetic follow the reference (gops/apprfunc/gauss.py:28-93), so that its `apprfunc_*.pkl`
checkpoints load unchanged and a seed gives the same initial parameters.  `forward` is the eager definition used by samplers and
evaluators; inside `compute_gradient` the same parameters are read in place by the HIP RBF rollout (`hip_mlp()`: a one-layer
`GopsMlp` with a GOPS_RBF_* head code, csrc/rollout_rbf.hip), which never calls `forward`.  The reference's StochaPolicy,
ActionValue, ActionValueDis and StateValue of this family are not on this path.
"""
__all__ = ["DetermPolicy", "FiniteHorizonPolicy"]

import weakref

import torch
import torch.nn as nn

from gops_amd.utils.act_distribution import Action_Distribution


class RBF(nn.Module):
    """y = w phi(x) + b over K Gaussian kernels, phi_k = exp(-|x - C_k|^2 / (2 |sigma_square_k|)).  Names, shapes (with their leading
    1) and the order of the four draws are the reference's (gauss.py:28-36): checkpoints and seeds carry over."""

    def __init__(self, n_in, n_out, n_kernel):
        super().__init__()
        self.C = nn.Parameter(torch.randn(1, n_kernel, n_in))
        self.sigma_square = nn.Parameter(torch.randn(1, n_kernel).abs() + 0.1)
        self.w = nn.Parameter(torch.randn(1, n_out, n_kernel))
        self.b = nn.Parameter(torch.randn(1, n_out, 1))

    def forward(self, x):
        centres, width = self.C[0], 2.0 * self.sigma_square[0].abs()           # [K, n], [K]
        dist2 = (x[:, None, :] - centres[None]).square().sum(dim=2)            # [B, K]
        phi = torch.exp(-dist2 / width)
        return phi @ self.w[0].T + self.b[0, :, 0]                             # [B, out]


# ctypes structs cannot be pickled / deep-copied: the C-ABI views live outside the modules, keyed weakly by module
_HIP_CACHE = weakref.WeakKeyDictionary()


class DetermPolicy(nn.Module, Action_Distribution):
    """Deterministic policy: a = half pi(obs) + mid, affine in the action limits (no tanh)."""

    is_rbf = True
    _time_input = False

    def __init__(self, **kwargs):
        super().__init__()
        obs_dim, act_dim = kwargs["obs_dim"], kwargs["act_dim"]
        self.pi = RBF(obs_dim + (1 if self._time_input else 0), act_dim, kwargs["num_kernel"])
        self.register_buffer("act_high_lim", torch.from_numpy(kwargs["act_high_lim"]))
        self.register_buffer("act_low_lim", torch.from_numpy(kwargs["act_low_lim"]))
        self.action_distribution_cls = kwargs["action_distribution_cls"]

    def forward(self, obs):
        half, mid = (self.act_high_lim - self.act_low_lim) / 2, (self.act_high_lim + self.act_low_lim) / 2
        return half * self.pi(obs) + mid

    def linear_layers(self):
        return []   # (no Linear layer: nothing for the plane-split precision guard to look at)

    def _head_code(self):
        from gops_amd import hip_backend as hb
        return hb.RBF_TANH if self._time_input else hb.RBF_AFFINE

    def hip_mlp(self, dtype=None, variant_flags=None):
        """The RBF net as `GopsMlp` (n_layers = 1) over the live parameter storage; `dtype` must be fp32 (no kernel variants)."""
        from gops_amd import hip_backend as hb
        if hb.dtype_id(dtype) != 0:
            raise RuntimeError("GAUSS approximators run in fp32 only (mlp_dtype fp16 is an MLP setting)")
        pi = self.pi
        key = tuple(p.data_ptr() for p in (pi.w, pi.b, pi.C, pi.sigma_square))
        cached = _HIP_CACHE.get(self)
        if cached is None or cached[0] != key:
            mlp = hb.make_rbf(pi.w.data, pi.b.data, pi.C.data, pi.sigma_square.data, self._head_code())
            _HIP_CACHE[self] = (key, mlp)
            return mlp
        return cached[1]


class FiniteHorizonPolicy(DetermPolicy):
    """Finite-horizon policy: the virtual time step is one more RBF input AFTER the observation; a = half tanh(pi) + mid."""

    _time_input = True

    def forward(self, obs, virtual_t=1):
        t = torch.full((obs.shape[0], 1), float(virtual_t), dtype=torch.float32, device=obs.device)
        half, mid = (self.act_high_lim - self.act_low_lim) / 2, (self.act_high_lim + self.act_low_lim) / 2
        return half * torch.tanh(self.pi(torch.cat((obs, t), dim=1))) + mid
