"""Per-element tests of the activation approximations in gops_amd/csrc/common.h (gelu_pair, gelu_pair_h, fast_tanh, the ELU / SELU
forms, act_bwd_t): float64 definitions, fp32 restatements of the kernel formulas, networks that make a network's output the
activation itself, the grids and the comparison rule.  tests/test_activations_cpu.py checks everything here without a GPU;
tests/test_activations_gpu.py runs the kernels.

Routing.  The kernels compute z = x W^T + b by matrix instructions whose operands may be split into planes (three bf16 planes, two
IEEE-half planes hi + lo / 2^11, or one half for GOPS_DTYPE_F16).  A routing net makes every product a product with 0 or 1 and every
sum a sum with ONE non-zero term, so z is the input bit for bit as long as the input itself survives the operand split:

* `route_mlp` (MlpNet, every fp32 family): layer 0 is one-hot with 1.0 entries - hidden unit j reads input j mod 16 -, further hidden
  layers and the output layer are identities, all biases 0.  Then y[b, j] = act(x[b, j mod 16]) (act(act(.)) with two hidden layers:
  the streamed plane-split family only takes nets with two 256-wide hidden layers) and, with grad_y = 1 on one unit per input,
  backward_x gives gx[b, i] = act'(x[b, i]) (times act'(act(x)) with two hidden layers).  Exact for the exact-fp32 families with ANY
  fp32 x (products with 1.0, sums with zeros); for the plane-split family with every x whose half planes are exact (the 8-bit
  grid: 8 significant bits, |x| 2^-4 inside the normal half range) - the second layer's input act(x) has 24 bits, of which the
  planes keep 22: `restate` rounds it the way split2h does.
* `route_value` (ValueNet, the only route to GOPS_DTYPE_F16): inputs x[b, b mod 64] = grid_b (one non-zero per row), an all-ones
  layer 0 and bias 0: every unit sees z = grid_b.  GOPS_DTYPE_F16: the head is all ones - the K stored activations are one half
  value h (11 bits), every partial sum m h (m <= 256) has at most 19 bits and is exact in the fp32 accumulator in any order:
  v_b = K half(act(grid_b)).  fp32: a sum of K equal 24-bit values is NOT exact in general, so the head is one-hot (unit `hot`):
  v_b = act(grid_b).  With grad_v = 1 on one block of 64 consecutive rows and 0 elsewhere, dW0[j, i] = delta[64 k + i, j] grid_{64 k + i}
  has one non-zero term; GOPS_VF_DW_F32 / GOPS_VF_DW_EXACT form it without adding an error of their own (at most the rounding of the
  product to fp32).  The 8-bit grid is exact as a half input.  Scaling is by powers of two only.
* `route_squash` (Rollout, pyth_lq, horizon 1): a ReLU policy with y = relu(x0) - relu(-x0) = x0 on both of two actions, policy limits
  (-2, 2) and (2, -2): abar = (2 tanh(x0), -2 tanh(x0)), of = 0, scale a power of two (so sc th is exact).  The env's action range is
  [0, 4] on both sides of ScaleAction: the wrapper is the identity on abar >= 0 (a1 - 0 exact, 4 (a1 / 4) exact) and clamps abar < 0 to 0.
  LQ matrices inv(I - A dt) = diag(0, 1, 1), B = [[0, 0], [1, 0], [0, 1]], dt = 1, Q = R = 0 (oracle lq_step: x' = inv_IA (x + dt B u))
  and x = (x0, 0, 0) give final_obs = (0, u0, u1): sc tanh(x0) = u0 - u1 with one of the two zero.  backward_adj with
  grad_final_obs = (0, 1, -1) and grad_v = 0 returns d(u0 - u1)/dx0 = 2 (1 - th^2) (relu'(x0) + relu'(-x0)) - zero at x0 = +-0,
  where the ROUTING has no slope (relu'(0) = 0); the float64 reference is that of the routed net.
"""
import ctypes
import math

import torch

ACTS = ("relu", "elu", "gelu", "selu", "sigmoid", "tanh")
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
F32 = torch.float32
EPS32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------
# float64 definitions
# ------------------------------------------------------------------------------------------
def _phi64(z):
    """Phi(z) = erfc(-z / sqrt 2) / 2: no cancellation on the negative side."""
    return 0.5 * torch.erfc(-z * math.sqrt(0.5))


def _sech2(z):
    t = torch.exp(-2.0 * z.abs())
    return 4.0 * t / (1.0 + t) ** 2


def act64(name, z):
    """(act(z), act'(z)) in float64; relu'(0) = 0 as in the kernels and in torch."""
    z = z.double()
    pos = z > 0
    if name == "relu":
        return torch.where(pos, z, torch.zeros_like(z)), pos.double()
    if name in ("elu", "selu"):
        zn = torch.where(pos, torch.zeros_like(z), z)
        a, d = torch.where(pos, z, torch.expm1(zn)), torch.where(pos, torch.ones_like(z), torch.exp(zn))
        if name == "elu":
            return a, d
        return SELU_SCALE * torch.where(pos, z, SELU_ALPHA * a), SELU_SCALE * torch.where(pos, d, SELU_ALPHA * d)
    if name == "gelu":
        cdf = _phi64(z)
        return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if name == "sigmoid":
        e = torch.exp(-z.abs())
        lo, hi = e / (1.0 + e), 1.0 / (1.0 + e)   # sigmoid(-|z|), sigmoid(|z|)
        return torch.where(pos, hi, lo), lo * hi
    if name == "tanh":
        return torch.tanh(z), _sech2(z)
    raise KeyError(name)


def squash64(y, sc, of):
    y = y.double()
    return sc * torch.tanh(y) + of, sc * _sech2(y)


# ------------------------------------------------------------------------------------------
# fp32 restatements of the kernel formulas (csrc/common.h), operation for operation
# ------------------------------------------------------------------------------------------
def f(x):
    return torch.as_tensor(x, dtype=F32)


def fma(a, b, c):
    """fmaf: the product is exact in float64 (48 bits), one rounding of the sum there and one to fp32."""
    return (f(a).double() * f(b).double() + f(c).double()).to(F32)


def to_half(x):
    return f(x).half().to(F32)


def hw_exp2(x):
    """v_exp_f32 up to its 1 ulp: 2^x rounded to fp32, results below the normal range flushed to zero (the instruction has no denormals)."""
    r = torch.exp2(f(x).double()).to(F32)
    return torch.where(r.abs() < 2.0 ** -126, torch.zeros_like(r), r)


def hw_exp(x):
    """__expf: v_exp_f32(x * log2 e), the argument rounded to fp32."""
    return hw_exp2(f(x) * f(1.4426950408889634))


def rcp(x):
    """v_rcp_f32 up to its 1 ulp: the IEEE quotient."""
    return f(1.0) / f(x)


def _gelu_tail(z, q, e):
    cdf = torch.where(z < 0, q, f(1.0) - q)
    return z * cdf, fma(z * f(0.39894228040143267794), e, cdf)


def gelu_pair(z):
    z = f(z)
    x = z.abs() * f(0.70710678118654752440)
    t = rcp(fma(f(0.3275911), x, f(1.0)))
    e = hw_exp(f(-0.5) * z * z)
    poly = fma(t, f(1.061405429), f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = fma(poly, t, f(c))
    return _gelu_tail(z, (f(0.5) * t) * poly * e, e)


GELU_H_COEF = (-1.45366924e-04, 2.07320246e-03, -1.29176200e-02, 4.79239046e-02, -1.23755032e-01, 2.46921233e-01, -3.98505880e-01,
               4.99984820e-01)


def gelu_pair_h(z):
    z = f(z)
    x = torch.clamp(z.abs(), max=6.0)
    e = hw_exp2(z * z * f(-0.72134752044448170368))
    p = fma(x, f(GELU_H_COEF[0]), f(GELU_H_COEF[1]))
    for c in GELU_H_COEF[2:]:
        p = fma(p, x, f(c))
    return _gelu_tail(z, p * e, e)


def fast_tanh_series(x):
    x = f(x)
    x2 = x * x
    poly = fma(x2, f(-17.0 / 315.0), f(2.0 / 15.0))
    poly = fma(poly, x2, f(-1.0 / 3.0))
    poly = fma(poly, x2, f(1.0))
    return x * poly


def fast_tanh_big(x):
    x = f(x)
    t = hw_exp(f(-2.0) * x.abs())
    return torch.copysign((f(1.0) - t) * rcp(f(1.0) + t), x)


def fast_tanh(x):
    x = f(x)
    return torch.where(x.abs() < 0.125, fast_tanh_series(x), fast_tanh_big(x))


def act_fwd(name, z, half_kernels=False):
    """act_fwd_t (and gelu_pair / gelu_pair_h) -> (h, stash): `stash` is what act_bwd reads - gelu'(z) for GELU, else h."""
    z = f(z)
    zero = torch.zeros_like(z)
    if name == "relu":
        h = torch.maximum(z, zero)
    elif name == "elu":
        h = torch.maximum(z, zero) + (hw_exp(torch.minimum(z, zero)) - f(1.0))
    elif name == "selu":
        # hipcc contracts a * b + c into an fma: SELU_ALPHA * (e - 1) joins the sum with max(z, 0)
        h = f(SELU_SCALE) * fma(f(SELU_ALPHA), hw_exp(torch.minimum(z, zero)) - f(1.0), torch.maximum(z, zero))
    elif name == "gelu":
        return gelu_pair_h(z) if half_kernels else gelu_pair(z)
    elif name == "sigmoid":
        h = f(1.0) / (f(1.0) + torch.exp(-z))
    elif name == "tanh":
        h = torch.tanh(z)
    else:
        raise KeyError(name)
    return h, h


def act_bwd(name, stash):
    """act_bwd_t from the stashed value."""
    h = f(stash)
    one = torch.ones_like(h)
    if name == "relu":
        return torch.where(h > 0, one, torch.zeros_like(h))
    if name == "elu":
        return torch.where(h > 0, one, h + f(1.0))
    if name == "gelu":
        return h
    if name == "selu":
        return torch.where(h > 0, f(SELU_SCALE) * one, h + f(SELU_SCALE) * f(SELU_ALPHA))
    if name == "sigmoid":
        return h * (f(1.0) - h)
    if name == "tanh":
        return fma(-h, h, f(1.0))   # 1 - h * h, contracted
    raise KeyError(name)


def split22(a, s=0.0625):
    """split2h: the two IEEE-half planes of a * s, put together again: what the next layer of a plane-split kernel multiplies."""
    x = f(a) * f(s)
    hi = to_half(x)
    lo = to_half((x - hi) * f(2048.0))
    return (hi.double() + lo.double() / 2048.0) / s   # (22 bits: exact in float64; the kernel never forms it in fp32)


def restate(name, z, layers=1, split=False, f16=False):
    """The routed net's (output, input gradient) as the kernels form them: `layers` hidden layers of act, the later ones fed through
    the half planes for a plane-split forward (`split`); `f16`: the GOPS_DTYPE_F16 kernels - gelu_pair_h, activation and gelu'
    stash rounded to half.  float64 tensors holding fp32 (or 22-bit) values."""
    cur, grad = f(z), None
    for j in range(layers):
        if j > 0 and split:
            cur = split22(cur).to(F32)   # (act_fwd's first operation on z rounds a 22-bit value to itself)
        h, st = act_fwd(name, cur, half_kernels=f16)
        if f16:
            h, st = to_half(h), to_half(st)
        d = act_bwd(name, st)
        grad = d if grad is None else grad * d
        cur = h
    return cur.double(), grad.double()


def reference(name, z, layers=1):
    """float64 (act o .. o act)(z) and its derivative."""
    cur, grad = f(z).double(), None
    for _ in range(layers):
        a, d = act64(name, cur)
        grad = d if grad is None else grad * d
        cur = a
    return cur, grad


# ------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------
def grid8():
    """Every value with 8 significant bits and 2^-14 <= |z| < 2^7, both signs (5376 points), +-0 and 14 values with 10 / 11
    significant bits beside the switch points (0.125 and its double for fast_tanh, 6.0 for gelu_pair_h, 1.0): exact as three bf16
    planes, as hi / lo half planes at scale 2^-4 and as one half.  [337, 16]: 21 tiles of 16 rows and one live row in the 22nd."""
    m = torch.arange(128, 256, dtype=torch.float64)
    mag = torch.cat([m * 2.0 ** (e - 7) for e in range(-14, 7)])
    special = [0.125 * (1 - 2.0 ** -10), 0.125 * (1 + 2.0 ** -10), 6.0 * (1 - 2.0 ** -9), 6.0 * (1 + 2.0 ** -9), 0.25 * (1 - 2.0 ** -10),
               0.25 * (1 + 2.0 ** -10), 1.0 + 2.0 ** -10]
    pts = torch.cat([mag, -mag, torch.tensor(special, dtype=torch.float64), -torch.tensor(special, dtype=torch.float64), torch.tensor([0.0, -0.0], dtype=torch.float64)])
    assert pts.numel() == 337 * 16 and torch.equal(pts.float().double(), pts) and torch.equal(pts.half().double(), pts)
    g = torch.Generator().manual_seed(11)
    return pts[torch.randperm(pts.numel(), generator=g)].float().reshape(337, 16)   # (shuffled: a tile holds every magnitude)


def grid_dense():
    """fp32 values of any bit pattern for the exact-fp32 family (z = x holds for every fp32 x there): uniform in [-12, 12],
    N(0, 1e-3) and a fine ramp over [-0.2, 0.2].  [4112, 16]: 257 tiles, the last input row alone in its tile... ragged batch."""
    g = torch.Generator().manual_seed(12)
    n = 4112 * 16
    a = (torch.rand(n // 2, generator=g, dtype=torch.float64) * 24 - 12).float()
    b = (torch.randn(n // 4, generator=g) * 1e-3).float()
    c = torch.linspace(-0.2, 0.2, n - a.numel() - b.numel(), dtype=torch.float64).float()
    pts = torch.cat([a, b, c])
    return pts[torch.randperm(n, generator=g)].reshape(4112, 16)


# ------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------
def ulp32(v):
    """Spacing of fp32 at |v| (float64 tensor; the denormal spacing below the normal range)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def binade_max(z, err):
    """For every point the largest `err` among the points of its binade (same sign and exponent of z; +0 / -0: their own)."""
    zf = f(z).reshape(-1)
    key = (zf.view(torch.int32) >> 23).long()   # sign and exponent
    err = err.reshape(-1)
    uniq, inv = torch.unique(key, return_inverse=True)
    top = torch.zeros(uniq.numel(), dtype=err.dtype).scatter_reduce(0, inv, err, reduce="amax", include_self=True)
    return top[inv].reshape(z.shape)


def bound_of(z, restated, want):
    """The rule of ac_helpers.check_backup per element: twice the restatement's error (its largest in the point's binade of z - a
    point the restatement happens to hit exactly sets no zero bound), and not less than 4 fp32 ulp of the wanted value.  The factor
    2: v_exp_f32 and v_rcp_f32 are within 1 ulp each of the libm exp / IEEE quotient of the restatement."""
    err_r = (restated.double() - want).abs()
    return torch.maximum(2.0 * binade_max(z, err_r), 4.0 * ulp32(want)), err_r


def check_elements(label, z, got, restated, want, stats=None):
    """Every element of `got` within `bound_of`; the message of a failure names the worst point.  -> (kernel max error, restated
    max error, largest bound) and a printed line."""
    assert torch.isfinite(want).all(), label
    got = got.detach().double().cpu().reshape(want.shape)
    zz = f(z).reshape(want.shape) if f(z).numel() == want.numel() else f(z).expand_as(want)
    bound, err_r = bound_of(zz, restated.reshape(want.shape), want)
    err_k = (got - want).abs()
    err_k = torch.where(torch.isnan(err_k), torch.full_like(err_k, float("inf")), err_k)
    line = (err_k.max().item(), err_r.max().item(), bound.max().item())
    print(f"{label}: kernel {line[0]:.3e} restated {line[1]:.3e} bound {line[2]:.3e}")
    if stats is not None:
        stats[label] = line
    bad = err_k > bound
    if bad.any():
        i = int(torch.argmax(torch.where(bad, err_k / bound.clamp_min(1e-300), torch.zeros_like(err_k))))
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} points outside the bound; worst at z = {zz.reshape(-1)[i].item()!r}: "
                             f"got {got.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}, error {err_k.reshape(-1)[i].item():.3e}, "
                             f"bound {bound.reshape(-1)[i].item():.3e} (restated {restated.reshape(-1)[i].item()!r})")
    return line


# ------------------------------------------------------------------------------------------
# routing nets
# ------------------------------------------------------------------------------------------
def route_mlp(width, layers=1, n_in=16):
    """(weights, biases) of the MlpNet routing net: n_in -> width (x layers) -> width."""
    w0 = torch.zeros(width, n_in)
    w0[torch.arange(width), torch.arange(width) % n_in] = 1.0
    ws = [w0] + [torch.eye(width) for _ in range(layers)]
    return ws, [torch.zeros(width) for _ in ws]


def route_mlp_units(width, n_in=16):
    """The hidden unit that carries grad_y = 1 for input i: one of the width / n_in units reading it, a different n-tile per input."""
    i = torch.arange(n_in)
    return i + n_in * ((5 * i + 3) % (width // n_in))


def route_mlp_grad_y(batch, width, n_in=16):
    gy = torch.zeros(batch, width)
    gy[:, route_mlp_units(width, n_in)] = 1.0
    return gy


VALUE_IN = 64   # input width of the value routing net: the widest the 64-row half kernels take


def route_value(width, f16, hot=0, layers=1):
    """(weights, biases) of the ValueNet routing net: all-ones layer 0; head of ones (f16) or one-hot at unit `hot` (fp32)."""
    head = torch.ones(1, width) if f16 else torch.zeros(1, width)
    if not f16:
        head[0, hot] = 1.0
    ws = [torch.ones(width, VALUE_IN)] + [torch.eye(width) for _ in range(layers - 1)] + [head]
    return ws, [torch.zeros(w.shape[0]) for w in ws]


def value_inputs(points):
    """[N] grid points -> [N, 64] with x[b, b mod 64] = points[b]."""
    n = points.numel()
    x = torch.zeros(n, VALUE_IN)
    x[torch.arange(n), torch.arange(n) % VALUE_IN] = points.reshape(-1).float()
    return x


SQUASH_SC = 2.0
SQUASH_LQ = dict(inv_IA=[[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], B=[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], Q=[0.0, 0.0, 0.0],
                 R=[0.0, 0.0], dt=1.0, reward_scale=1.0, reward_shift=0.0)
SQUASH_LIMITS = dict(policy_low=[-2.0, 2.0], policy_high=[2.0, -2.0], min_action=0.0, max_action=4.0, act_low=0.0, act_high=4.0)


def route_squash(width, layers=2):
    """(weights, biases) of the ReLU policy 3 -> width (x layers) -> 2 with y0 = y1 = relu(x0) - relu(-x0)."""
    w0 = torch.zeros(width, 3)
    w0[0, 0], w0[1, 0] = 1.0, -1.0
    wo = torch.zeros(2, width)
    wo[:, 0], wo[:, 1] = 1.0, -1.0
    ws = [w0] + [torch.eye(width) for _ in range(layers - 1)] + [wo]
    return ws, [torch.zeros(w.shape[0]) for w in ws]


def squash_restated(x0, fast):
    """(u0 - u1, d(u0 - u1)/dx0) of the squash routing in fp32: th = fast_tanh or tanhf, abar = +-2 th (exact), 2 (1 - th^2)."""
    x0 = f(x0)
    th = fast_tanh(x0) if fast else torch.tanh(x0)
    slope = (x0 != 0).to(F32)   # the ReLU routing: no slope at +-0
    return (f(SQUASH_SC) * th).double(), (f(SQUASH_SC) * (f(1.0) - th * th) * slope).double()


def squash_reference(x0):
    v, d = squash64(f(x0), SQUASH_SC, 0.0)
    return v, d * (f(x0) != 0).double()


# ------------------------------------------------------------------------------------------
# which kernels a call runs
# ------------------------------------------------------------------------------------------
def batch_variant(mlp, batch):
    """gops_rollout_variant of the description a gops_value_* / gops_mlp_* call plans with (api.hip value_desc: GOPS_ENV_NONE, one
    step, the net's hidden stack with a 1-wide head): 4 = streamed plane-split, 8 = 64-row half kernels, 0 = the streamed fp32-MFMA
    kernels (or the 16-row half kernels for GOPS_DTYPE_F16).  Host only."""
    from gops_amd import hip_backend as hb
    d = hb.GopsRolloutDesc()
    d.batch, d.horizon, d.need_grad, d.gamma = batch, 1, 1, 1.0
    d.env.kind, d.env.obs_dim, d.env.act_dim = hb.ENV_NONE, int(mlp.sizes[0]), 1
    m = hb.GopsMlp.from_buffer_copy(mlp)
    m.sizes[m.n_layers] = 1
    d.policy, d.dtype, d.variant_flags = m, mlp.dtype, mlp.variant_flags
    return hb.lib().gops_rollout_variant(ctypes.byref(d))


def claims():
    """Largest error of the restatements over both grids against float64: what common.h's comments and DESIGN.md state."""
    z = torch.cat([grid8().reshape(-1), grid_dense().reshape(-1)])
    z64 = z.double()
    out = {}
    phi = _phi64(z64)
    for tag, fn in (("gelu_pair", gelu_pair), ("gelu_pair_h", gelu_pair_h)):
        h, dh = fn(z)
        a, d = act64("gelu", z)
        cdf = torch.where(z != 0, h.double() / z64, phi)   # (h = z cdf: the quotient recovers cdf to 1 ulp)
        out[tag] = dict(phi=(cdf - phi).abs().max().item(), gelu=(h.double() - a).abs().max().item(), dgelu=(dh.double() - d).abs().max().item())
    nz = z != 0
    th = fast_tanh(z).double()
    rel = ((th - torch.tanh(z64)).abs() / torch.tanh(z64).abs().clamp_min(1e-300))[nz]
    out["fast_tanh"] = dict(rel=rel.max().item(), at=z[nz][int(rel.argmax())].item())
    for name in ("elu", "selu"):   # the negative branch (for z > 0 the result is z, or one rounding of SCALE z)
        zn = z[z <= 0]
        out[name] = dict(abs=(act_fwd(name, zn)[0].double() - act64(name, zn)[0]).abs().max().item())
    return out
