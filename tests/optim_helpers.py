"""Per-element tests of the optimizer tail (csrc/optim.hip: adam_kernel, polyak_kernel, batch_loss_kernel; csrc/common.h:
adam_element / polyak_element, called from dw_gemm.hip's fused reduce): the float64 Adam reference with its rounding-count bounds,
the fp32 restatements that give the expected BITS of the Polyak average and the value-loss gradient, an fp32 emulation of the
kernel's operation order (what tests/test_optim_cpu.py holds against the bounds without a GPU), the input grids and the size lists.
tests/test_optim_gpu.py runs the kernels.

The bounds (u = 2^-24, the unit round-off of fp32; s = lr / (1 - b1^t); G = g * grad_scale in double; first order in u, the slack
named below pays for the second order).  The kernel's element, as written in adam_kernel / adam_element, fp32 throughout:

    gi = g * gsc                      gsc = fp32(grad_scale)
    m  = m0 + (gi - m0) * omb1        omb1 = fp32(1 - b1)
    v  = v0 * b2 + omb2 * gi * gi     b2 = fp32(b2), omb2 = fp32(1 - b2)
    p  = p0 - step * (m / (sqrtf(v) / bc2 + eps))   step = fp32(s), bc2 = fp32(sqrt(1 - b2^t)), eps = fp32(eps)

* gi: the rounding of gsc and of the product: |gi - G| <= 2u |G|.
* E_m: 2u omb1 |G| (gi) + u omb1 |gi - m0| (the difference) + 2u omb1 |gi - m0| (omb1's own rounding, the product's) +
  u |M| (the sum; one rounding less when hipcc contracts product and sum into an fma), and |gi - m0| <= |G| + |m0|, |M| <=
  |m0| + |G|:  u (1 + 5 omb1) (|m0| + |G|)  <=  4u (|m0| + |G|)  for 1 - b1 <= 0.6 (asserted; the default is 0.1).  Absolute in
  |m0| + |G|, not relative to M: b1 m0 and (1 - b1) G may cancel.
* E_v: the term v0 b2 carries the rounding of b2, of the product and of the final sum: 3u; the term omb2 gi gi carries omb2's
  rounding (1), gi twice (2 x 2), two products (2) and the sum (1): 8u (7u with the second product contracted into the sum).  Both
  terms are non-negative, so  E_v = u (3 b2 v0 + 8 (1 - b2) G^2)  <=  8u V.  (A flat 5u V does not follow from the count: with
  v0 = 0 and a grad_scale that is no power of two the seven roundings of the second term are all there.)
* E_p: the final difference u |P|; m's error through the quotient s E_m / D; and the relative error of dP = s M / D: sqrtf
  E_v / (2V) + 1 <= 5, bc2 1, the quotient 1, eps and the sum 1, the quotient m / D 1, step 1, the product 1 (0 when contracted):
  <= 11u.  E_p = 2u |P| + s E_m / D + 12u |dP|: the second u |P| and the twelfth u |dP| are the slack for the second-order terms
  (the largest is 11u times the 4u-relative error of the quotient's operands).

fp32 division and sqrtf are correctly rounded in the build (hipcc's default); no operand of the grids is subnormal (|g| >= 1e-12
with grad_scale >= 0.125: omb2 gi^2 >= 1e-30), so no flush-to-zero question arises.  |g| <= 1e8: a finite gradient whose square
overflows steps to v = inf exactly as torch's fp32 Adam does, which is not this suite's subject.

Several steps carried in float64 (`adam_bounds(..., carried=)`): an error e_m in m0 reaches M as b1 e_m, an error e_v in v0 reaches
V as b2 e_v, an error in p0 reaches P unchanged; through dP they add s b1 e_m / D and |dP| b2 e_v / (2V).
"""
import numpy as np
import torch

U = 2.0 ** -24

# adam_kernel: blockDim 256, gridDim.x = min(64, ceil(largest numel of the table / 1024)), 4 elements per thread and outer trip:
# with a 64-block grid a trip covers 4 * 64 * 256 = 65536 elements, the groups of four sit 16384 apart
ADAM_SIZES = (
    1,        # one live thread in the whole grid
    255,      # one short of a block
    256,      # exactly one block
    257,      # one element in the second block
    1023,     # alone in a table: one short of the 1024 elements that one block takes in a trip
    1024,     # alone: exactly one block's trip (gridDim.x = 1)
    1025,     # alone: gridDim.x = 2
    65535,    # one short of the 64-block grid's first outer trip
    65536,    # exactly one outer trip: i0 += 4 * stride is never taken
    65537,    # one element in the second outer trip
    81921,    # second trip: first of the four full (16384), the second holds ONE element, the other two are empty
    262147,   # fifth outer trip, three elements in it
)
# polyak_kernel: gridDim.x = min(64, ceil(largest numel / 256)), one element per thread and trip: the grid-stride loop repeats from 16385
POLYAK_SIZES = (
    1,        # one live thread
    257,      # one element in the second block
    16384,    # the 64-block grid exactly once
    16385,    # the first element of the second trip
    65537,    # fifth trip, one element
)
# batch_loss_kernel: ONE block up to 8192 elements (LOSS_ONE_BLOCK_MAX), 64 beyond; 8 elements per thread and outer trip
LOSS_SIZES = (
    1,        # one live thread
    2047,     # one block: one short of its first outer trip (8 * 256)
    2048,     # one block: exactly one trip
    2049,     # one block: one element in the second trip
    8192,     # the largest one-block launch: four full trips
    8193,     # the smallest 64-block launch
    131071,   # 64 blocks: one short of the first outer trip (8 * 64 * 256)
    131072,   # 64 blocks: exactly one trip
    131073,   # 64 blocks: one element in the second trip
    262145,   # 64 blocks: one element in the third trip
)
LOSS_ONE_BLOCK_MAX = 8192        # csrc/block_reduce.h
LOSS_TICKET = 2 + 4 * 64         # float index of the ticket in a LossStats buffer: behind 64 blocks' two double partial sums
GUARD = 64                       # elements behind every tensor under test
GUARD_VALUE = -7.25e11           # (no result of any grid)

GRAD_SCALES = (1.0, 1.0 / 3.0, 0.125)


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def scaled_grad32(g, grad_scale):
    """fp32(g * fp32(grad_scale)): the value whose finiteness decides whether an element is stepped (common.h grad_is_finite)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _np(g).astype(np.float32) * np.float32(grad_scale)


def stepped(g, grad_scale):
    return np.isfinite(scaled_grad32(g, grad_scale))


def adam_ref64(p, m, v, g, *, lr, betas, eps, t, grad_scale):
    """One Adam step (torch.optim.Adam without weight decay / amsgrad) in float64 with the true double hyper-parameters; `t` is the
    1-based step.  -> float64 P, M, V, dP, D with D = sqrt(V) / sqrt(1 - b2^t) + eps and dP = lr / (1 - b1^t) * M / D = p - P.
    Elements whose scaled gradient fp32(g * fp32(grad_scale)) is not finite return their inputs (dP = 0)."""
    b1, b2 = float(betas[0]), float(betas[1])
    p, m, v = (_np(x).astype(np.float64) for x in (p, m, v))
    ok = stepped(g, grad_scale)
    G = np.where(ok, _np(g).astype(np.float64), 0.0) * float(grad_scale)
    M = m + (G - m) * (1.0 - b1)
    V = v * b2 + (1.0 - b2) * G * G
    D = np.sqrt(V) / np.sqrt(1.0 - b2 ** t) + float(eps)
    dP = float(lr) / (1.0 - b1 ** t) * M / D
    return np.where(ok, p - dP, p), np.where(ok, M, m), np.where(ok, V, v), np.where(ok, dP, 0.0), D


def adam_bounds(m, v, g, ref, *, lr, betas, t, grad_scale, carried=None):
    """(E_m, E_v, E_p) of the module docstring for the step whose inputs were m, v, g and whose `adam_ref64` result is `ref`;
    `carried` = the bounds the inputs themselves came with (several steps carried in float64).  Zero where no step is taken."""
    b1, b2 = float(betas[0]), float(betas[1])
    assert 1.0 - b1 <= 0.6, "E_m = 4u (|m0| + |G|) is derived for 1 - b1 <= 0.6"
    P, M, V, dP, D = ref
    m0, v0 = np.abs(_np(m).astype(np.float64)), _np(v).astype(np.float64)
    ok = stepped(g, grad_scale)
    G = np.abs(np.where(ok, _np(g).astype(np.float64), 0.0) * float(grad_scale))
    cm, cv, cp = carried if carried is not None else (0.0, 0.0, 0.0)
    s = float(lr) / (1.0 - b1 ** t)
    e_m = 4.0 * U * (m0 + G) + b1 * cm
    e_v = U * (3.0 * b2 * v0 + 8.0 * (1.0 - b2) * G * G)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_v_in = np.where(V > 0, b2 * cv / (2.0 * V), 0.0)   # (V = 0: v0 = 0 and G = 0, the kernel's v is an exact zero)
    e_p = cp + 2.0 * U * np.abs(P) + s * e_m / D + (12.0 * U + rel_v_in) * np.abs(dP)
    return np.where(ok, e_m, cm), np.where(ok, e_v + b2 * cv, cv), np.where(ok, e_p, cp)


# ------------------------------------------------------------------------------------------
# fp32 emulation of the kernel's operation order (numpy: one rounding per fp32 operation)
# ------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf through float64: the product of two fp32 values is exact there; the sum rounds once to float64 and once to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_emulate32(p, m, v, g, *, lr, betas, eps, t, grad_scale, form):
    """adam_kernel's element in fp32, scalar factors as adam_kernel forms them (beta^t = beta^(t-1) * beta in double).  `form`:
    "plain" - every product and sum rounded; "fma" - the contractions hipcc may make of m0 + d * omb1, (omb2 gi) gi + v0 b2 and
    p0 - step * q; "fma_alt" - the other contraction of v: v0 * b2 + (omb2 gi gi).  Every element is stepped."""
    f = np.float32
    b1, b2 = float(betas[0]), float(betas[1])
    b1p, b2p = b1 ** (t - 1) * b1, b2 ** (t - 1) * b2
    step, bc2 = f(float(lr) / (1.0 - b1p)), f(np.sqrt(1.0 - b2p))
    omb1, omb2, fb2, feps = f(1.0 - b1), f(1.0 - b2), f(b2), f(eps)
    p, m, v, g = (_np(x).astype(f) for x in (p, m, v, g))
    gi = g * f(grad_scale)
    if form == "plain":
        mi = m + (gi - m) * omb1
        vi = v * fb2 + omb2 * gi * gi
    elif form == "fma":
        mi = _fma(gi - m, np.full_like(m, omb1), m)
        vi = _fma(omb2 * gi, gi, v * fb2)
    elif form == "fma_alt":
        mi = _fma(gi - m, np.full_like(m, omb1), m)
        vi = _fma(v, np.full_like(v, fb2), omb2 * gi * gi)
    else:
        raise KeyError(form)
    q = mi / (np.sqrt(vi) / bc2 + feps)
    pi = p - step * q if form == "plain" else _fma(np.full_like(q, -step), q, p)
    return pi, mi, vi


def polyak_ref32(t, p, tau):
    """common.h polyak_element, the expected bits: fp32(fp32(t * omt) + fp32(tau * p)), omt = fp32(1 - tau), tau = fp32(tau)."""
    f = np.float32
    t, p = _np(t).astype(f), _np(p).astype(f)
    return (t * f(1.0 - float(tau))).astype(f) + (f(tau) * p).astype(f)


def value_grad_ref32(a, b):
    """gops_value_loss's gradient, the expected bits: fp32(fp32(2 / n) * fp32(a - b))."""
    f = np.float32
    a, b = _np(a).astype(f), _np(b).astype(f)
    return f(2.0 / a.size) * (a - b).astype(f)


# ------------------------------------------------------------------------------------------
# input grids
# ------------------------------------------------------------------------------------------
def _decades(rng, n, lo, hi):
    return 10.0 ** rng.uniform(lo, hi, n)


def adam_grid(n, seed, betas=(0.9, 0.999), fresh=False):
    """fp32 p, m0, v0, g of n elements.  |g| log-uniform over [1e-12, 1e8] with random sign, one in eight an exact zero; m0 of
    either sign over the same decades, or -g, or -g (1 - b1) / b1 (then b1 m0 + (1 - b1) g cancels), or 0; v0 log-uniform over
    [1e-24, 1e16], or g^2, or 0; one in sixteen elements has g = m0 = v0 = 0 (the step must leave p, m, v as they are, bit for bit -
    `adam_zero_case`).  The first and the last element are of the generic kind (an element the loop leaves out is then seen).
    `fresh`: m0 = v0 = 0 everywhere (step 1 of a new optimizer)."""
    rng = np.random.default_rng(seed)
    b1 = float(betas[0])
    sign = lambda: rng.choice([-1.0, 1.0], n)   # noqa: E731
    g = sign() * _decades(rng, n, -12, 8)
    kind_g, kind_m, kind_v = rng.integers(0, 8, n), rng.integers(0, 8, n), rng.integers(0, 8, n)
    zero = rng.integers(0, 16, n) == 0
    for k in (kind_g, kind_m, kind_v):
        k[[0, -1]] = 7
    zero[[0, -1]] = False
    g = np.where(kind_g == 0, 0.0, g)
    m = sign() * _decades(rng, n, -12, 8)
    m = np.where(kind_m == 0, -g, m)
    m = np.where(kind_m == 1, -g * (1.0 - b1) / b1, m)
    m = np.where(kind_m == 2, 0.0, m)
    v = _decades(rng, n, -24, 16)
    v = np.where(kind_v == 0, g * g, v)
    v = np.where((kind_v == 1) | ((kind_v == 0) & (np.abs(g) < 1e-12)), 0.0, v)   # (no g^2 below the decades above: nothing subnormal)
    g, m, v = (np.where(zero, 0.0, x) for x in (g, m, v))
    if fresh:
        m, v = np.zeros(n), np.zeros(n)
    p = rng.standard_normal(n) * _decades(rng, n, -4, 1)
    return tuple((x + 0.0).astype(np.float32) for x in (p, m, v, g))   # (+ 0.0: no negative zero - m0 = -0 leaves as +0, rightly)


def adam_zero_case(m, v, g):
    """Elements with g = m0 = v0 = 0: m0 + (0 - m0) omb1, v0 b2 + omb2 0 0 and p0 - step (0 / eps) are p0, m0, v0 themselves."""
    return (_np(g) == 0) & (_np(m) == 0) & (_np(v) == 0)


def ratios(got, ref, bound):
    """Largest |got - ref| / bound (0 / 0 counts as 0: an exact result under a zero bound) and its index."""
    err = np.abs(_np(got).astype(np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


class Worst:
    """The worst observed-to-bound ratio per quantity over the checks of one test, with where it was seen."""

    def __init__(self):
        self.r = {}

    def check(self, label, got, ref, bounds):
        """got, ref[:3]: (p, m, v); bounds: (E_m, E_v, E_p) as `adam_bounds` returns them; every element within its bound."""
        for name, a, b, e in zip("pmv", got, ref[:3], (bounds[2], bounds[0], bounds[1])):
            r, i = ratios(a, b, e)
            if r > self.r.get(name, (0.0, ""))[0]:
                self.r[name] = (r, f"{label}[{i}]")
            assert r <= 1.0, (f"{label}: {name}[{i}] = {float(_np(a).reshape(-1)[i])!r}, float64 {float(b.reshape(-1)[i])!r}, "
                              f"error / bound = {r:.3f} (bound {float(np.broadcast_to(e, b.shape).reshape(-1)[i]):.3e})")

    def report(self, title):
        print(title + ": worst error / bound " + ", ".join(f"{k} {v[0]:.3f} at {v[1]}" for k, v in sorted(self.r.items())))


# ------------------------------------------------------------------------------------------
# device tensors with a guard region
# ------------------------------------------------------------------------------------------
def guarded(values, device):
    """-> (view of the first n elements, whole buffer): the GUARD elements behind the view hold GUARD_VALUE."""
    x = torch.as_tensor(_np(values).astype(np.float32)).reshape(-1)
    buf = torch.full((x.numel() + GUARD,), GUARD_VALUE, dtype=torch.float32)
    buf[:x.numel()] = x
    buf = buf.to(device)
    return buf[:x.numel()], buf


def guard_intact(buf):
    tail = buf[-GUARD:]
    return bool(torch.equal(tail, torch.full_like(tail, GUARD_VALUE)))


def bits_equal(a, b):
    """Same bit patterns (NaN and the sign of zero included)."""
    a, b = _np(a).astype(np.float32).reshape(-1), _np(b).astype(np.float32).reshape(-1)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


class AdamCase:
    """Guarded device copies of one table of tensors with a HipAdam over them whose state the test has filled: exp_avg, exp_avg_sq,
    step (t - 1).  `tensors`: list of (p, m, v, g) fp32 arrays; `groups`: list of (indices, lr) - one param group by default."""

    def __init__(self, tensors, device, *, lr, betas, eps, step, groups=None):
        from gops_amd.hip_backend import HipAdam
        self.host = [tuple(np.array(x, dtype=np.float32) for x in t) for t in tensors]
        self.bufs, self.params = [], []
        for p, m, v, g in self.host:
            views, bufs = zip(*(guarded(x, device) for x in (p, m, v, g)))
            par = torch.nn.Parameter(views[0], requires_grad=False)
            par.grad = views[3]
            self.params.append(par)
            self.bufs.append(dict(zip("pmvg", bufs), m_view=views[1], v_view=views[2]))
        if groups is None:
            self.opt = HipAdam(self.params, lr=lr, betas=betas, eps=eps)
        else:
            self.opt = HipAdam([dict(params=[self.params[i] for i in idx], lr=glr) for idx, glr in groups], lr=lr, betas=betas, eps=eps)
        for par, b in zip(self.params, self.bufs):
            self.opt.state[par] = dict(step=int(step), exp_avg=b["m_view"], exp_avg_sq=b["v_view"])

    def set_grad(self, i, g):
        n = self.params[i].numel()
        self.bufs[i]["g"][:n] = torch.as_tensor(_np(g).astype(np.float32)).to(self.bufs[i]["g"].device)

    def read(self, i):
        """(p, m, v) of tensor i as fp32 arrays."""
        n = self.params[i].numel()
        return tuple(self.bufs[i][k][:n].cpu().numpy() for k in "pmv")

    def guards_intact(self):
        return all(guard_intact(b[k]) for b in self.bufs for k in "pmvg")

    def device_state(self, gi=0):
        """[(lr, step, beta1_pow, beta2_pow, ticket, skipped_nonfinite, grad_scale)] of the group's chunks (GopsAdamState)."""
        out = []
        for t in self.opt._dev[gi]["state"]:
            raw = t.cpu()
            f64, i32 = raw.view(torch.float64), raw.view(torch.int32)
            out.append((float(f64[0]), int(raw[1]), float(f64[2]), float(f64[3]), int(i32[8]), int(i32[9]) & 0xFFFFFFFF, float(f64[5])))
        return out
