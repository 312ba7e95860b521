"""Integer-exact inputs, float64 references and the case table of the weight-gradient stage's per-element tests
(test_dw_exact_gpu.py; the table's plans are pinned on the CPU in test_host_cpu.py).

Why no tolerance: with integer weights, inputs and output gradients and ReLU hidden layers every activation and every delta is
an integer.  csrc/common.h split3 carries an fp32 value as three bf16 planes (3 x 8 significant bits) and the exact kernels
take the six plane products a1b1, a1b2, a2b1, a1b3, a2b2, a3b1: an integer |v| <= 1024 (11 bits) sits in planes 1 and 2, and
all four products of those are among the six.  csrc/dw_gemm.hip split2h forms hi = f16(v s), lo = f16(v s - hi) with s a
power of two: an 11-bit integer is hi, lo = 0.  The fp32-MFMA kernels multiply fp32 values.  Every accumulator is fp32, so
while sum |d| |x| over the samples stays below 2^22 every partial sum is an exactly representable integer whatever the order:
the result equals the float64 one bit for bit, and a dropped, doubled or misplaced sample, tile, split or column is an
integer difference at a known (row, column)."""
import math

import torch

from gops_amd import hip_backend as hb

LIMIT_V, LIMIT_SUM = 1024, 2 ** 22


def pad16(n):
    return (n + 15) // 16 * 16


def int_net(sizes, B, seed, *, dense_head=False, boost=None):
    """Integer ReLU net and batch in float64: weights in [-2, 2] with at most 8 non-zeros per row, biases in [-4, 4], |x| <= 8,
    |g| <= 8 (g: gradient of the output, [B, sizes[-1]]; max|g| = 8 and one entry 1 are planted).  (In the output-layer cases the
    delta operand is g itself: it fills bf16 plane 1 only, so the a2 b1 / a2 b2 products of the exact kernels see a non-zero a2 in
    the hidden-layer cases - deltas and activations of several hundred - and in the real-valued tier, not there.)  dense_head: a one-row
    output layer (value nets) has no zero - with 8 non-zeros 248 of the last hidden layer's delta rows would be zero and the
    GEMM under test would form a mostly empty matrix.  boost = (units, p): rows `units` of layer 0 (and their biases) times
    2^p, the matching columns of layer 1 times 2^-p - the same function with H_1 of those units beyond the half range."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    ws, bs = [], []
    for j, (k, n) in enumerate(zip(sizes[:-1], sizes[1:])):
        w = torch.zeros(n, k, dtype=torch.float64)
        vals = ri(1, 2, (n, k)) * (2 * ri(0, 1, (n, k)) - 1)
        if dense_head and n == 1 and j == len(sizes) - 2:
            w = vals
        else:
            keep = torch.rand(n, k, generator=gen).argsort(1)[:, :min(8, k)]
            w.scatter_(1, keep, vals.gather(1, keep))
        ws.append(w)
        bs.append(ri(-4, 4, (n,)))
    if boost is not None:
        units, p = boost
        ws[0][units] *= 2.0 ** p
        bs[0][units] *= 2.0 ** p
        ws[1][:, units] *= 2.0 ** -p
    x = ri(-8, 8, (B, sizes[0]))
    g = ri(-8, 8, (B, sizes[-1]))
    g.view(-1)[0] = 8.0
    g.view(-1)[-1] = 1.0
    return ws, bs, x, g


def ref64(ws, bs, x, g):
    """Forward and backward in float64: y, layer inputs hs[j], deltas ds[j] (gradient of layer j's pre-activation), gw, gb."""
    n = len(ws)
    hs, z = [x], None
    for j in range(n):
        z = hs[j] @ ws[j].T + bs[j]
        if j < n - 1:
            hs.append(torch.relu(z))
    ds, gw, gb, d = [None] * n, [None] * n, [None] * n, g
    for j in reversed(range(n)):
        ds[j], gw[j], gb[j] = d, d.T @ hs[j], d.sum(0)
        if j > 0:
            d = (d @ ws[j]) * (hs[j] > 0)
    return dict(y=z, hs=hs, ds=ds, gw=gw, gb=gb)


def check_premises(ref, boost=None):
    """The exactness premises, asserted before anything runs on the GPU (a failure is a test error, not a skip): every hidden
    activation and delta an integer of at most 1024, every sum |d| |x| (bias: |d|) over the samples below 2^22, 20 - 80 % of the
    hidden units active.  boost = (units, p): H_1 of `units` is 2^p times such an integer and delta_0 (whose rows are those
    units) 2^-p times one - the premises hold on the values with the power of two taken out (it moves exponents only)."""
    n = len(ref["gw"])
    for j in range(n):
        x, d = ref["hs"][j].clone(), ref["ds"][j].clone()
        if boost is not None:
            units, p = boost
            if j == 1:
                x[:, units] *= 2.0 ** -p
            if j == 0:
                d[:, units] *= 2.0 ** p
        assert torch.equal(x, x.round()) and torch.equal(d, d.round()), f"layer {j}: operands are not integers"
        if j > 0:
            assert x.abs().max() <= LIMIT_V, f"layer {j}: |activation| up to {x.abs().max().item()}"
            active = (x > 0).double().mean().item()
            assert 0.2 <= active <= 0.8, f"layer {j}: {100 * active:.0f} % of the units active"
        assert d.abs().max() <= LIMIT_V, f"layer {j}: |delta| up to {d.abs().max().item()}"
        assert (d.abs().T @ x.abs()).max() < LIMIT_SUM and d.abs().sum(0).max() < LIMIT_SUM, f"layer {j}: partial sums beyond 2^22"


def run_gpu(api, ws, bs, x, g, B, flags=0, fill=None, dtype=None):
    """One forward + backward of hb.MlpNet ("mlp") / hb.ValueNet ("value") on fp32 copies; `fill`: byte written over the whole
    workspace BEFORE the forward (0xFF: every float a NaN); dtype "fp16": GOPS_DTYPE_F16 storage.  Returns y, gw, gb on the CPU."""
    dev = torch.device("cuda", 0)
    wd = [w.float().to(dev).contiguous() for w in ws]
    bd = [b.float().to(dev).contiguous() for b in bs]
    xd, gd = x.float().to(dev).contiguous(), g.float().to(dev).contiguous()
    mlp = hb.make_mlp(wd, bd, "relu", dtype=dtype, variant_flags=flags)
    net = hb.MlpNet(mlp, B) if api == "mlp" else hb.ValueNet(mlp, B)
    if fill is not None:
        net.workspace.fill_(fill)
    gw, gb = [torch.full_like(w, float("nan")) for w in wd], [torch.full_like(b, float("nan")) for b in bd]
    if api == "mlp":
        y = net.forward(xd)
        net.backward(xd, gd, gw, gb)
    else:
        y = net.forward(xd).reshape(B, 1)
        net.backward(xd, gd.reshape(B).contiguous(), gw, gb)
    torch.cuda.synchronize()
    return y.cpu(), [t.cpu() for t in gw], [t.cpu() for t in gb]


def layer_plan(api, sizes, B, layer, flags=0, f16=False):
    """gops_dw_plan_query for layer `layer` of the call: the output layer of gops_mlp_backward is an unscaled N = pad16(W) GEMM,
    its hidden layers are unscaled too (ext_delta), gops_value_backward's hidden layers are scaled (grad_v is the one source).
    GOPS_DTYPE_F16: inputs padded to 32, and the stash of an all-256-wide net with at most 64 padded inputs is in 64-row tiles
    (rollout_h64.hip h64_shape_ok; api.hip build_plan: S counts whole tiles)."""
    out_layer = layer == len(sizes) - 2
    assert api == "mlp" or not out_layer, "a value net's 1-wide head is not a GEMM of this stage"
    N = pad16(sizes[layer + 1]) if out_layer else sizes[layer + 1]
    K, rows = sizes[layer], 16
    if f16 and all(w == 256 for w in sizes[1:-1]) and (sizes[0] + 31) // 32 * 32 <= 64:
        rows = 64
    S = (B + rows - 1) // rows * rows
    return hb.dw_plan_query(N, K, S, Kp=(K + 31) // 32 * 32 if f16 else None, f16=f16, scaled=api == "value", vflags=flags)


# rows x columns of outputs one workgroup forms, by kernel (dw_gemm.hip): what `tile (i, j)` of a report counts in
WG_TILE = {hb.DW_SPEC: (256, 128), hb.DW_RING_H2: (128, 128), hb.DW_RING_EXACT: (128, 128), hb.DW_SKINNY: (256, 16),
           hb.DW_FM4_BF3: (128, 128), hb.DW_FM4_F32: (128, 128), hb.DW_FM2_BF3: (64, 64), hb.DW_FM2_F32: (64, 64), hb.DW_F16: (128, 128),
           hb.DW_NONE: (16, 16)}


def mismatch_report(name, layer, plan, got, want, tile):
    """Where two gradient matrices differ: count, the first few (n, k, got, want) and their tile coordinates."""
    bad = (got != want).nonzero()
    if want.dim() == 1:
        bad = torch.cat([bad, torch.zeros_like(bad)], 1)
    lines = [f"{name}: layer {layer} on {hb.DW_KERNEL_NAMES[plan['kernel']]} (splits {plan['splits']}, chunks/split "
             f"{plan['chunks_per_split']}): {len(bad)} of {want.numel()} elements of {'dW' if want.dim() == 2 else 'db'} differ"]
    for n, k in bad[:8].tolist():
        gv, wv = (got[n, k], want[n, k]) if want.dim() == 2 else (got[n], want[n])
        lines.append(f"  (n {n}, k {k}) got {gv.item()} want {wv.item()}   tile ({n // tile[0]}, {k // tile[1]}) n%16 {n % 16} k%16 {k % 16}")
    return "\n".join(lines)


def assert_exact(name, api, sizes, B, flags, got, ref, f16=False):
    """y first (a forward fault is not a GEMM fault), then every weight and bias gradient against float64 cast to fp32."""
    y, gw, gb = got
    assert torch.equal(y, ref["y"].float()), f"{name}: forward output differs in {(y != ref['y'].float()).sum().item()} elements"
    for j in range(len(gw)):
        out_layer = j == len(gw) - 1
        if api == "value" and out_layer:
            plan = dict(kernel=hb.DW_NONE, splits=0, chunks_per_split=0)   # (dw_out_fm_kernel / dw_out_h_kernel / in-sweep slabs)
        else:
            plan = layer_plan(api, sizes, B, j, flags, f16)
        tile = WG_TILE[plan["kernel"]]
        for g_, w_ in ((gw[j], ref["gw"][j].float()), (gb[j], ref["gb"][j].float())):
            assert torch.equal(g_, w_), mismatch_report(name, j, plan, g_, w_, tile)


# ---- the case table: name -> api, sizes, batch, variant flags, layer under test, and its pinned plan (kernel, splits,
# chunks per split).  test_host_cpu.py::test_dw_exact_case_table_plans asserts the pins against gops_dw_plan_query.
_OUT = [  # (kernel, W, K): output layer of gops_mlp_backward, sizes [in, K, W]
    ("Fm2Bf3", 7, 32, 0), ("Fm2Bf3", 130, 64, 0), ("Fm2Bf3", 20, 96, 0), ("Skinny", 40, 16, 0), ("Skinny", 300, 16, 0),
    ("Fm4Bf3", 130, 192, 0), ("RingExact", 128, 128, 0), ("RingExact", 256, 144, 0), ("RingExact", 384, 272, 0),
    ("Fm2F32", 130, 64, hb.VF_DW_F32), ("Fm2F32", 40, 16, hb.VF_DW_F32), ("Fm4F32", 130, 192, hb.VF_DW_F32),
]
# chunks = pad16(B) / 32 rounded up; (splits, chunks per split) by batch for every row above: one chunk per split up to 9 chunks
_BATCH_PLAN = {1: (1, 1), 17: (1, 1), 48: (2, 1), 272: (9, 1)}
CASES = {}
for _k, _w, _kk, _f in _OUT:
    for _b, (_s, _c) in _BATCH_PLAN.items():
        CASES[f"out_{_k}_{_w}x{_kk}_b{_b}"] = dict(api="mlp", sizes=[9, _kk, _w], B=_b, flags=_f, layer=1, kernel=_k, splits=_s, chunks=_c)
# 20 chunks on 64 counted tiles: 7 splits of 3 chunks (the last of 2), a grid of 8 per tile - every eighth workgroup returns at once
CASES["out_RingExact_4096x256_b640_7x3"] = dict(api="mlp", sizes=[9, 256, 4096], B=640, flags=0, layer=1, kernel="RingExact", splits=7, chunks=3)
for _b, (_s, _c) in ((48, (2, 1)), (272, (9, 1))):
    CASES[f"hid_RingExact_256x128_b{_b}"] = dict(api="mlp", sizes=[30, 128, 256, 5], B=_b, flags=0, layer=1, kernel="RingExact", splits=_s, chunks=_c)
    CASES[f"hid_Fm2Bf3_128x30_b{_b}"] = dict(api="mlp", sizes=[30, 128, 256, 5], B=_b, flags=0, layer=0, kernel="Fm2Bf3", splits=_s, chunks=_c)
    CASES[f"hid_Skinny_256x16_b{_b}"] = dict(api="mlp", sizes=[16, 256, 256, 3], B=_b, flags=0, layer=0, kernel="Skinny", splits=_s, chunks=_c)
    for _wd, _kern in ((256, "Spec"), (128, "RingH2"), (384, "RingH2")):
        for _tag, _f, _kn in (("", 0, _kern), ("_exact", hb.VF_DW_EXACT, "RingExact"), ("_f32", hb.VF_DW_F32, "Fm4F32")):
            CASES[f"val_{_kern}_{_wd}{_tag}_b{_b}"] = dict(api="value", sizes=[12, _wd, _wd, 1], B=_b, flags=_f, layer=1, kernel=_kn, splits=_s, chunks=_c)
# H_1 of 6 units times 2^11 (beyond 65504 where the integer is 32 or more): the workgroups that read them redo their tiles exactly
SATURATED = dict(api="value", sizes=[12, 256, 256, 1], B=48, flags=0, layer=1, kernel="Spec", splits=2, chunks=1,
                 boost=([3, 70, 129, 130, 200, 255], 11))


# GOPS_DTYPE_F16 storage through gops_value_backward: every hidden layer on dw_gemm_f16_kernel (choose_dw_gemm's first branch), the
# head on dw_out_h_kernel.  64-sample chunks; 256-wide nets stash 64-row tiles (B = 48 -> S = 64, 272 -> 320: 48 padding rows).
F16_CASES = {}
for _b, (_s, _c) in ((48, (1, 1)), (272, (5, 1))):
    for _wd in (256, 128):
        F16_CASES[f"val_F16_{_wd}_b{_b}"] = dict(api="value", sizes=[12, _wd, _wd, 1], B=_b, flags=0, layer=1, kernel="F16", splits=_s, chunks=_c, f16=True)


def case_seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


def yardstick_scale(max_abs_grad_v):
    """The power of two csrc/dw_gemm.hip multiplies the deltas of a scaled launch with: f16_grad_scale(m) * 16 (common.h)."""
    return 16.0 * 2.0 ** (1 - math.frexp(max_abs_grad_v)[1])
