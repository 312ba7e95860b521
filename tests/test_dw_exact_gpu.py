"""GPU: the weight-gradient stage (csrc/dw_gemm.hip: the GEMM kernels, plan_dw / choose_dw_gemm, reduce_partials_kernel) per
ELEMENT and without a tolerance.  Integer networks (dw_helpers.py: why the float64 result is then the only correct bit
pattern) through gops_mlp_backward - whose output layer is a plan_dw(pad16(W), K, K, S) GEMM over the caller's own grad_y -
and gops_value_backward, whose hidden layers are scaled launches (two-half-plane kernels).  Every case asserts through
gops_dw_plan_query that its layer runs on the kernel the case is named after; a mismatch names row, column and tile.

GOPS_DTYPE_F16 storage (DwKernel::F16, OutH) has its own cases: integers up to 1024 are halves.
Not here: InSweep slabs and dw_out_fm_kernel on rollouts (the rollouts' per-trajectory tests).

A real-valued tier at the end covers what integers leave empty (bf16 plane 3, the lo half plane)."""

import pytest
import torch

import dw_helpers as dh
from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name, c):
    """Inputs and float64 reference of a case (computed once, shared, never modified); premises asserted before any launch."""
    if name not in _cache:
        ws, bs, x, g = dh.int_net(c["sizes"], c["B"], dh.case_seed(name), dense_head=c["api"] == "value", boost=c.get("boost"))
        ref = dh.ref64(ws, bs, x, g)
        dh.check_premises(ref, c.get("boost"))
        _cache[name] = (ws, bs, x, g, ref)
    return _cache[name]


def _assert_plan(name, c):
    plan = dh.layer_plan(c["api"], c["sizes"], c["B"], c["layer"], c["flags"])
    got = (hb.DW_KERNEL_NAMES[plan["kernel"]], plan["splits"], plan["chunks_per_split"])
    assert got == (c["kernel"], c["splits"], c["chunks"]), f"{name}: layer {c['layer']} is planned as {got}"


@pytest.mark.parametrize("name", list(dh.CASES))
def test_dw_integer_exact(name):
    """Forward output, every weight and every bias gradient of the case equal float64 bit for bit (torch.equal)."""
    c = dh.CASES[name]
    _assert_plan(name, c)
    ws, bs, x, g, ref = _case(name, c)
    got = dh.run_gpu(c["api"], ws, bs, x, g, c["B"], c["flags"])
    dh.assert_exact(name, c["api"], c["sizes"], c["B"], c["flags"], got, ref)


@pytest.mark.parametrize("width", [256, 128, 384])
@pytest.mark.parametrize("B", [48, 272])
def test_dw_scaled_exact_and_f32_give_the_same_bits(width, B):
    """One integer value net on the two-half-plane kernel, with GOPS_VF_DW_EXACT and with GOPS_VF_DW_F32: the same bits."""
    kern = "Spec" if width == 256 else "RingH2"
    name = f"val_{kern}_{width}_b{B}"
    c = dh.CASES[name]
    ws, bs, x, g, ref = _case(name, c)
    runs = [dh.run_gpu("value", ws, bs, x, g, B, f) for f in (0, hb.VF_DW_EXACT, hb.VF_DW_F32)]
    for r in runs[1:]:
        for a, b in zip([runs[0][0]] + runs[0][1] + runs[0][2], [r[0]] + r[1] + r[2]):
            assert torch.equal(a, b)
    dh.assert_exact(name, "value", c["sizes"], B, 0, runs[0], ref)


@pytest.mark.parametrize("name", list(dh.F16_CASES))
def test_dw_f16_storage_integer_exact(name):
    """GOPS_DTYPE_F16 storage through gops_value_backward: hidden layers on dw_gemm_f16_kernel, the head on dw_out_h_kernel.
    Weights, activations and deltas are stored as halves - integers up to 2048 are halves - and the sweep's deltas carry
    f16_grad_scale(max|grad_v|) = 2^-3, which the reduce takes out again: |d| <= 1024 is an 11-bit multiple of 2^-3, still a
    half; products accumulate in fp32.  So the same bits as float64 are due here too."""
    c = dh.F16_CASES[name]
    plan = dh.layer_plan(c["api"], c["sizes"], c["B"], c["layer"], c["flags"], True)
    assert (hb.DW_KERNEL_NAMES[plan["kernel"]], plan["splits"], plan["chunks_per_split"]) == (c["kernel"], c["splits"], c["chunks"]), (name, plan)
    ws, bs, x, g, ref = _case(name, c)
    for fill in (0, 0xFF):   # (48 padding rows of the 64-row stash at B = 272 must not reach a result)
        got = dh.run_gpu(c["api"], ws, bs, x, g, c["B"], c["flags"], fill=fill, dtype="fp16")
        dh.assert_exact(name, c["api"], c["sizes"], c["B"], c["flags"], got, ref, f16=True)


def test_dw_saturated_half_planes_are_redone_exactly():
    """H_1 of six units is 2^11 times its integer (layer 0's rows times 2^11, layer 1's columns times 2^-11: the same function),
    so it exceeds 65504 wherever the integer is 32 or more.  split2h saturates there; the workgroups of dw_gemm_spec_kernel
    that convert those columns raise the flag and repeat their tiles with the three-plane split, which holds the same 11 bits
    whatever the exponent.  Own premise (dh.check_premises with boost): the integers behind the scaled values obey the
    usual bounds, so every partial sum is 2^11 times an exact integer.  B = 48 as in the other scaled cases."""
    c = dh.SATURATED
    _assert_plan("saturated", c)
    ws, bs, x, g, ref = _case("saturated", c)
    units = c["boost"][0]
    over = (ref["hs"][1][:, units] > 65504).sum().item()
    assert over >= 3, over
    got = dh.run_gpu("value", ws, bs, x, g, c["B"], 0)
    dh.assert_exact("saturated", "value", c["sizes"], c["B"], 0, got, ref)


@pytest.mark.parametrize("name", ["out_Fm2Bf3_130x64_b17", "out_Skinny_300x16_b48", "hid_RingExact_256x128_b272", "val_Spec_256_b272",
                                  "out_RingExact_4096x256_b640_7x3"])
def test_dw_does_not_read_stale_workspace(name):
    """The workspace filled with 0xFF bytes (every float a NaN) BEFORE the forward gives the bits of a zero-filled one: padded
    rows of the stash and of the padded grad_y, and the slabs of workgroups that return early, do not reach a result.  (The
    library asks for no zeroed workspace: hip_backend allocates it with torch.empty.)"""
    c = dh.CASES[name]
    ws, bs, x, g, ref = _case(name, c)
    zero = dh.run_gpu(c["api"], ws, bs, x, g, c["B"], c["flags"], fill=0)
    nan = dh.run_gpu(c["api"], ws, bs, x, g, c["B"], c["flags"], fill=0xFF)
    for a, b in zip([zero[0]] + zero[1] + zero[2], [nan[0]] + nan[1] + nan[2]):
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements depend on what the workspace held"
    dh.assert_exact(name, c["api"], c["sizes"], c["B"], c["flags"], nan, ref)


# ---- real-valued tier -------------------------------------------------------------------------------------------------
def _real_case(api, sizes, B, seed, drop_near_kink=False):
    """drop_near_kink: the output gradient of every sample with a hidden pre-activation within fp32 rounding of 0 is zeroed, so
    the sample leaves numerator and denominator of e alike.  There the ReLU mask of a fp32 forward can differ from float64's,
    which swaps a whole delta - forward noise that has nothing to do with the GEMM and would sit above its plane allowance.
    Within rounding: |z| < 2 (K_0 + K_1 + .. + 4) 2^-24 (sum |w| |h| + |b|), the a-priori bound of a fp32 dot product on inputs
    that carry the previous layers' bound themselves."""
    torch.manual_seed(seed)
    lin = [torch.nn.Linear(a, b) for a, b in zip(sizes[:-1], sizes[1:])]
    ws, bs = [l.weight.detach().clone() for l in lin], [l.bias.detach().clone() for l in lin]
    x, g = torch.randn(B, sizes[0]), torch.randn(B, sizes[-1])
    if drop_near_kink:
        # ... and both operands of the GEMM are made exactly computable, so that e measures the GEMM and not the forward (a fp32
        # forward's ABSOLUTE error on a barely active unit is a large RELATIVE error of that column's sum |d| |x|: e32 = 9.4e-6
        # without this).  x on a 2^-6 grid, layer 0 on a 2^-8 grid: z_1 has at most 20 bits in any order, H_1 is exact - and
        # fills hi and lo planes.  grad_v on a 2^-8 grid, the head on a 2^-14 grid: delta_2 = grad_v w is an exact 21-bit product.
        q = lambda t, bits: (t * 2.0 ** bits).round() * 2.0 ** -bits
        x, g = q(x, 6), q(g, 8)
        ws[0], bs[0], ws[-1] = q(ws[0], 8), q(bs[0], 8), q(ws[-1], 14)
        h, c = x.double(), 2.0 * (sum(sizes[:-2]) + 4) * 2.0 ** -24
        near = torch.zeros(B, dtype=torch.bool)
        for w, b in zip(ws[:-1], bs[:-1]):
            z = h @ w.double().T + b.double()
            near |= (z.abs() < c * (h.abs() @ w.double().abs().T + b.double().abs())).any(1)
            h = torch.relu(z)
        assert near.sum().item() < B // 4, near.sum().item()
        g[near] = 0.0
    ref = dh.ref64([w.double() for w in ws], [b.double() for b in bs], x.double(), g.double())
    wr, br = [w.clone().requires_grad_(True) for w in ws], [b.clone().requires_grad_(True) for b in bs]
    h = x
    for j, (w, b) in enumerate(zip(wr, br)):   # the fp32 reference: torch fp32 autograd on the CPU
        h = torch.nn.functional.linear(h, w, b)
        if j < len(wr) - 1:
            h = torch.relu(h)
    grads = torch.autograd.grad(h, wr + br, grad_outputs=g)
    return ws, bs, x, g, ref, grads[:len(wr)], grads[len(wr):]


def _e(got, ref, j):
    """max over the elements of dW_j of |got - ref64| / sum over the samples of |d| |x|"""
    den = ref["ds"][j].abs().T @ ref["hs"][j].abs()
    return ((got.double() - ref["gw"][j]).abs() / den)[den > 0].max().item()


def _real_setup(kernel):
    if kernel == "Spec":
        return "value", [12, 256, 256, 1], 1, hb.VF_NO_STREAMED_SPLIT_VALUE
    return "mlp", [24, 256, 272 if kernel == "Fm4Bf3" else 256], 1, 0


@pytest.mark.parametrize("kernel", ["Fm4Bf3", "RingExact", "Spec"])
def test_dw_real_valued_error_per_element(kernel):
    """N(0, 1) inputs, torch.nn.Linear default initialisation, ReLU, B = 272: e = max |got - ref64| / sum_s |d| |x| of the layer
    under test against float64.  Fm4Bf3: 272 x 256 (a 256 x 256 layer is the ring kernels' by choose_dw_gemm), RingExact:
    256 x 256 output layer, Spec: dW_1 of a 12-256-256-1 value net with GOPS_VF_NO_STREAMED_SPLIT_VALUE (fp32 forward and
    sweep: the GEMM alone carries half planes), on inputs whose H_1 and delta_2 are exact in fp32 and without the samples
    that sit on a ReLU kink (_real_case: otherwise forward noise, e32 = 9.4e-6, hides the lo plane).
    Bounds (none from the kernel's output): e32 is the same measure of torch fp32 autograd on the CPU.
      exact kernels: 4 e32 - six bf16 plane products drop terms below 2^-25 |d x|, the rest is fp32 sums in another order.
      Spec / RingH2: e32 + 2^-19.  split2h / split2h_mix keep hi + lo of v = x s to 2^-21 |v| each (two 11-bit halves; round
        toward zero, the wider of the two forms): two operands 2 x 2^-21 = 2^-20; the dropped lo x lo is below
        2^-10 |d| 2^-10 |x| = 2^-20 |d x|; together 2^-19 of sum |d| |x|, added to the fp32 figure.  (Nothing is allowed for a
        lo that is a subnormal half - |v| < 2^-4, spacing 2^-24.)
    Observed (MI355X): DESIGN.md 2.2d."""
    B = 272
    api, sizes, j, flags = _real_setup(kernel)
    plan = dh.layer_plan(api, sizes, B, j, flags)
    assert hb.DW_KERNEL_NAMES[plan["kernel"]] == kernel, plan
    ws, bs, x, g, ref, gw32, _ = _real_case(api, sizes, B, 11, drop_near_kink=kernel == "Spec")
    e32 = _e(gw32[j], ref, j)
    bound = e32 + 2.0 ** -19 if kernel == "Spec" else 4 * e32
    y, gw, gb = dh.run_gpu(api, [w.double() for w in ws], [b.double() for b in bs], x.double(), g.double(), B, flags)
    e = _e(gw[j], ref, j)
    print(f"dw real-valued tier: {kernel} e = {e:.3e}  fp32 reference e32 = {e32:.3e}  bound = {bound:.3e}")
    assert e <= bound, (kernel, e, e32, bound)
