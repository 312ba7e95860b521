"""GPU: every activation of csrc/common.h and its derivative, element by element against float64, in every kernel family that
evaluates it (act_helpers.py: routing nets, fp32 restatements, grids and the rule; DESIGN.md section 2.2e holds the figures these
tests print).  Every case first asks the library which kernels the call runs."""
import ctypes

import pytest
import torch

import act_helpers as ah
from ac_helpers import check_rows_beyond_the_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def grids():
    return ah.grid8(), ah.grid_dense()


def _odd(x, y):
    """y(-x) == -y(x) over a symmetric set of points."""
    order = torch.argsort(x.reshape(-1).double(), stable=True)
    g = y.reshape(-1)[order]
    xs = x.reshape(-1)[order]
    assert torch.equal(xs, -xs.flip(0))
    return torch.equal(g, -g.flip(0))


# ---- fp32 MLP batches (MlpNet) ----------------------------------------------------------------------------------
def _mlp_cases():
    from gops_amd import hip_backend as hb
    return {
        # name: hidden width, hidden layers, variant flags, gops_rollout_variant of the hidden stack, plane-split forward, exact fp32
        "plain_64": (64, 1, 0, 0, False, True),                                  # streamed fp32 kernels, LDS-resident weights
        "plain_64x64": (64, 2, 0, 0, False, False),                              # ... the obs-64-64 kernels written out
        "streamed_split_256": (256, 2, 0, 4, True, False),                       # default for 256-wide nets: two half planes
        "fp32_mfma_256": (256, 2, hb.VF_NO_STREAMED_SPLIT_VALUE, 0, False, False),
        "streamed_fp32_256": (256, 2, hb.VF_STREAMED_FP32 | hb.VF_NO_STREAMED_SPLIT_VALUE, 0, False, True),
    }


MLP_CASE_NAMES = ("plain_64", "plain_64x64", "streamed_split_256", "fp32_mfma_256", "streamed_fp32_256")


@pytest.mark.parametrize("name", ah.ACTS)
@pytest.mark.parametrize("case", MLP_CASE_NAMES)
def test_mlp_batch_activation_and_derivative_per_element(case, name, grids):
    """MlpNet.forward / backward_x on the routing net: y[b, j] = act(x[b, j mod 16]) in EVERY hidden unit column, gx = act'(x)
    (composed twice with two hidden layers).  The 8-bit grid everywhere, the dense grid on the exact-fp32 families.  The family is
    the one gops_rollout_variant reports for the call's hidden stack (api.hip value_desc); the library has no query that tells the
    streamed fp32 kernels with LDS-resident weights from those without, both report 0."""
    from gops_amd import hip_backend as hb
    width, layers, flags, variant, split, dense = _mlp_cases()[case]
    ws, bs = ah.route_mlp(width, layers)
    ws, bs = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    mlp = hb.make_mlp(ws, bs, name, variant_flags=flags)
    cols = torch.arange(width) % 16
    for gname, x in (("grid8", grids[0]),) + ((("dense", grids[1]),) if dense else ()):
        B = x.shape[0]
        assert ah.batch_variant(mlp, B) == variant, "the call would not run the kernels this case is named after"
        net = hb.MlpNet(mlp, B)
        xd = x.to(DEV)
        got = check_rows_beyond_the_batch(lambda out: net.forward(xd, out=out["y"]).clone(), dict(y=B * width)).reshape(B, width)
        assert torch.equal(got, net.forward(xd)), "a second launch differs"
        r_val, r_grad = ah.restate(name, x, layers, split=split)
        want, dwant = ah.reference(name, x, layers)
        label = f"{name} {case} {gname}"
        ah.check_elements(label + " act", x[:, cols], got, r_val[:, cols], want[:, cols])
        gy = ah.route_mlp_grad_y(B, width).to(DEV)
        gx = net.backward_x(xd, gy)
        torch.cuda.synchronize()
        assert torch.equal(gx, net.backward_x(xd, gy)), "a second launch differs"
        ah.check_elements(label + " act'", x, gx, r_grad, dwant)
        if name == "tanh" and gname == "grid8":
            assert _odd(x, got[:, :16].cpu()), "tanh is not odd"
        if name == "gelu":
            assert got.min().item() >= -0.17
            if layers == 1:
                assert 0.0 <= gx.min().item() + 0.13 and gx.max().item() + 0.13 <= 1.26


# ---- value batches (ValueNet): GOPS_DTYPE_F16 on both half families, fp32 through the weight-gradient GEMM ------------------
def _value_cases():
    from gops_amd import hip_backend as hb
    return {
        # name: width, dtype, flags, variant, hot unit of an fp32 head
        "half16_64": (64, "fp16", 0, 0, None),                 # rollout_f16.h, 16-row tiles
        "half64_256": (256, "fp16", 0, 8, None),               # rollout_h64.hip, 64-row tiles, first-layer gradient inside the sweep
        "fp32_64_dw_f32": (64, "fp32", hb.VF_DW_F32, 0, 37),
        "fp32_64_dw_exact": (64, "fp32", hb.VF_DW_EXACT, 0, 5),
    }


VALUE_CASE_NAMES = ("half16_64", "half64_256", "fp32_64_dw_f32", "fp32_64_dw_exact")


@pytest.mark.parametrize("name", ah.ACTS)
@pytest.mark.parametrize("case", VALUE_CASE_NAMES)
def test_value_batch_activation_and_derivative_per_element(case, name, grids):
    """ValueNet.forward on the value routing net: v_b = K half(act(grid_b)) (GOPS_DTYPE_F16, head of ones) or act(grid_b) (fp32,
    one-hot head); act' through the first layer's weight gradient, one block of 64 rows per backward call:
    dW0[j, i] = grid_i act'(grid_i).  gops_rollout_variant tells the 64-row half kernels (bit 3) from the 16-row ones (0)."""
    from gops_amd import hip_backend as hb
    width, dtype, flags, variant, hot = _value_cases()[case]
    f16 = dtype == "fp16"
    pts = grids[0].reshape(-1)
    N = pts.numel()
    ws, bs = ah.route_value(width, f16, hot=hot or 0)
    ws, bs = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    mlp = hb.make_mlp(ws, bs, name, dtype=dtype, variant_flags=flags)
    assert ah.batch_variant(mlp, N) == variant, "the call would not run the kernels this case is named after"
    vn = hb.ValueNet(mlp, N)
    x = ah.value_inputs(pts).to(DEV)
    v = vn.forward(x).clone()
    assert torch.equal(v, vn.forward(x)), "a second launch differs"
    r_val, r_grad = ah.restate(name, pts, f16=f16)
    want, dwant = ah.reference(name, pts)
    K = width if f16 else 1
    label = f"{name} {case}"
    ah.check_elements(label + " act", pts, v / K, r_val, want)   # (K a power of two: the division is exact)
    gw, gb = [torch.empty_like(w) for w in ws], [torch.empty_like(b) for b in bs]
    rows = []
    for k in range((N + ah.VALUE_IN - 1) // ah.VALUE_IN):
        gv = torch.zeros(N, device=DEV)
        gv[k * ah.VALUE_IN:(k + 1) * ah.VALUE_IN] = 1.0
        vn.backward(x, gv, gw, gb)
        rows.append(gw[0].t().clone())   # [64 inputs, width]
    torch.cuda.synchronize()
    got = torch.cat(rows)[:N].cpu()      # row b: dW0[:, b mod 64] of b's block
    if not f16:
        assert (got[:, [j for j in range(width) if j != hot]] == 0).all(), "units outside the one-hot head have a gradient"
        got = got[:, hot:hot + 1]
    p64 = pts.double()
    # the stored delta is a half in the half kernels; the product with the 8-bit input is exact in fp32 there, rounded once in fp32 nets
    r_dw = (ah.to_half(r_grad).double() * p64) if f16 else (r_grad.float() * pts).double()
    zz = pts[:, None].expand_as(got)
    ah.check_elements(label + " act' (dW0)", zz, got, r_dw[:, None].expand_as(got), (p64 * dwant)[:, None].expand_as(got))
    if name == "tanh":
        assert _odd(pts, (v / K).cpu()), "tanh is not odd"
    if name == "gelu":
        assert (v / K).min().item() >= -0.17


# ---- the policy head's squash: fast_tanh against tanhf ------------------------------------------------------------------------
def _squash_cases():
    from gops_amd import hip_backend as hb
    return {
        # name: width, dtype, flags, gops_rollout_variant, fast_tanh
        "plain_tanhf": (64, "fp32", 0, 0, False),                                    # streamed fp32 kernels: libm tanhf
        "split_256": (256, "fp32", 0, 1, True),                                      # register-stationary plane-split
        "streamed_split_256": (256, "fp32", hb.VF_NO_STATIONARY_SPLIT, 4, True),
        "half64_256": (256, "fp16", 0, 8, True),
    }


@pytest.mark.parametrize("case", ("plain_tanhf", "split_256", "streamed_split_256", "half64_256"))
def test_head_squash_and_its_derivative_per_element(case, grids):
    """A closed-loop pyth_lq rollout of one step whose final observation is the wrapped action (act_helpers.route_squash): the
    squash 2 tanh(x0) from final_obs, its derivative from backward_adj(want_grad_obs=True).  The half kernels have no sweep that
    returns an observation adjoint (gops_rollout_backward_adj refuses GOPS_DTYPE_F16, asserted here): their squash is checked by value
    and branch; 1 - th^2 of their sweep is the same expression on the same stashed th as in the fp32 families."""
    from gops_amd import hip_backend as hb
    width, dtype, flags, variant, fast = _squash_cases()[case]
    x0 = grids[0].reshape(-1)
    B = x0.numel()
    ws, bs = ah.route_squash(width)
    ws, bs = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    mlp = hb.make_mlp(ws, bs, "relu")
    env = hb.make_env(hb.ENV_LQ, 3, 2, lq=ah.SQUASH_LQ, **ah.SQUASH_LIMITS)
    ro = hb.Rollout(env, mlp, batch=B, horizon=1, gamma=1.0, finite_horizon=False, dtype=dtype, variant_flags=flags)
    assert hb.lib().gops_rollout_variant(ctypes.byref(ro.desc)) == variant, "the launch would not take the kernels this case is named after"
    obs = torch.zeros(B, 3)
    obs[:, 0] = x0
    data = dict(obs=obs.to(DEV), done=torch.zeros(B, device=DEV))
    fo = ro.forward(data, want_final=True)["final_obs"].clone()
    gfo = torch.tensor([0.0, 1.0, -1.0]).repeat(B, 1).to(DEV)
    zero = torch.zeros(B, device=DEV)
    assert torch.equal(fo, ro.forward(data, want_final=True)["final_obs"]), "a second launch differs"
    if dtype == "fp16":
        with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
            ro.backward_adj(zero, grad_final_obs=gfo, want_grad_obs=True)
        g = None
    else:
        g = ro.backward_adj(zero, grad_final_obs=gfo, want_grad_obs=True).clone()
        assert torch.equal(g, ro.backward_adj(zero, grad_final_obs=gfo, want_grad_obs=True)), "a second launch differs"
        g = g.cpu()
    fo = fo.cpu()
    assert (fo[:, 0] == 0).all() and ((fo[:, 1] == 0) | (fo[:, 2] == 0)).all() and (fo[:, 1:] >= 0).all()
    got = fo[:, 1] - fo[:, 2]   # (one of the two is zero: exact)
    r_val, r_grad = ah.squash_restated(x0, fast)
    want, dwant = ah.squash_reference(x0)
    ah.check_elements(f"squash {case} value", x0, got, r_val, want)
    if g is not None:
        ah.check_elements(f"squash {case} derivative", x0, g[:, 0], r_grad, dwant)
    assert _odd(x0, got), "the squash is not odd"
    if fast:
        # which branch ran.  Below |x| = 1/8 the series is fma / multiply arithmetic alone: the kernel's bits are the restatement's.
        # From 1/8 up the exponential branch runs: act_helpers' two branches differ at more than a quarter of the grid points of
        # [1/8, 1/4) (test_activations_cpu.py), so a kernel that equals the series at ALL of them has its switch elsewhere.
        low, band = x0.abs() < 0.125, (x0.abs() >= 0.125) & (x0.abs() < 0.25)
        series = (ah.f(ah.SQUASH_SC) * ah.fast_tanh_series(x0)).float()
        assert torch.equal(got[low], series[low]), "below the switch the kernel is not on the series"
        assert not torch.equal(got[band], series[band]), "between 1/8 and 1/4 the kernel is on the series: the switch has moved"
