"""CPU: what tests/test_activations_gpu.py stands on (act_helpers.py) - the float64 definitions against torch float64 autograd, the
routing nets through the float64 oracle, the grids, and the fp32 restatements' own errors against the claims in csrc/common.h."""
import pytest
import torch

import act_helpers as ah
from oracle import adp_oracle as orc


@pytest.fixture(scope="module")
def grids():
    return ah.grid8(), ah.grid_dense()


@pytest.mark.parametrize("name", ah.ACTS)
def test_float64_definitions_match_torch_autograd(name, grids):
    z = torch.cat([g.reshape(-1) for g in grids]).double()
    z = z[z != 0] if name == "relu" else z   # (relu'(0): the kernels' and torch's 0, checked below)
    zz = z.clone().requires_grad_(True)
    a = orc._ACT[name](zz)
    d, = torch.autograd.grad(a.sum(), zz)
    a64, d64 = ah.act64(name, z)
    assert torch.isfinite(a64).all() and torch.isfinite(d64).all()
    # torch's own float64 forms cancel where ours do not (1 - tanh^2, erf on the negative side): absolute 1e-15, or 1e-12 relative
    for got, want in ((a64, a.detach()), (d64, d)):
        assert ((got - want).abs() <= 1e-15 + 1e-12 * want.abs()).all(), name
    assert ah.act64("relu", torch.zeros(2))[1].tolist() == [0.0, 0.0]


def test_squash_definition_matches_torch_autograd():
    y = torch.linspace(-9, 9, 1001, dtype=torch.float64).requires_grad_(True)
    d, = torch.autograd.grad((1.5 * torch.tanh(y) + 0.25).sum(), y)
    v64, d64 = ah.squash64(y.detach(), 1.5, 0.25)
    assert torch.allclose(v64, 1.5 * torch.tanh(y.detach()) + 0.25, rtol=0, atol=1e-15) and ((d64 - d).abs() <= 1e-15 + 1e-12 * d.abs()).all()


def test_grids(grids):
    g8, gd = grids
    assert tuple(g8.shape) == (337, 16) and tuple(gd.shape) == (4112, 16)
    flat = g8.reshape(-1)
    assert flat.unique().numel() == flat.numel() - 1   # (+0 == -0)
    mant = flat.view(torch.int32) & 0x7FFFFF
    assert int(((mant & 0xFFFF) == 0).sum()) >= 5376 + 2 and int(((mant & 0xFFF) == 0).sum()) == flat.numel()   # 8 bits; the specials <= 12
    nz = flat[flat != 0].abs()
    assert nz.min() == 2.0 ** -14 and nz.max() == 255 * 0.5
    # exact under every operand split: one half, hi / lo half planes at 2^-4, three bf16 planes
    assert torch.equal(flat.half().float(), flat) and torch.equal(ah.split22(flat).float(), flat)
    hi = flat.bfloat16().float()
    mid = (flat - hi).bfloat16().float()
    assert torch.equal(hi + mid + (flat - hi - mid).bfloat16().float(), flat)
    for v in (0.125, 6.0, 0.25):   # the switch points and their neighbours on both sides
        assert (flat == v).any() and (flat == -v).any() and ((flat > v * 0.99) & (flat < v)).any() and ((flat > v) & (flat < v * 1.01)).any()
    assert gd.abs().max() <= 12 and (gd.abs() < 1e-3).sum() > 1000


def _torch_act(name, z, layers):
    """(act o .. o act)(z) and its derivative by the oracle's own float64 activation and autograd: what the routed net is compared
    with bit for bit (ah.act64 is the same function written without cancellation: test_float64_definitions_match_torch_autograd)."""
    zz = z.double().clone().requires_grad_(True)
    a = zz
    for _ in range(layers):
        a = orc._ACT[name](a)
    d, = torch.autograd.grad(a.sum(), zz)
    return a.detach(), d


@pytest.mark.parametrize("name", ah.ACTS)
@pytest.mark.parametrize("width,layers", [(64, 1), (64, 2), (256, 2)])
def test_mlp_routing_is_exact_in_the_float64_oracle(name, width, layers, grids):
    x = grids[0].double().requires_grad_(True)
    ws, bs = ah.route_mlp(width, layers)
    y = orc.mlp_forward([w.double() for w in ws], [b.double() for b in bs], x, name)
    cols = torch.arange(width) % 16
    # (the same tensor shape as the net's hidden layer: torch's vectorised float64 functions differ in the last bit between layouts)
    want, dfull = _torch_act(name, grids[0][:, cols], layers)
    dwant = dfull[:, ah.route_mlp_units(width)]
    tiny = 2.3e-308   # bit for bit, except that the BLAS behind the oracle's linear layers may flush float64 DENORMALS (gelu(-38))
    y0 = y.detach()
    assert (y0 - want).abs().max() <= tiny and torch.equal(y0[want.abs() > tiny], want[want.abs() > tiny])
    gx, = torch.autograd.grad((y * ah.route_mlp_grad_y(x.shape[0], width).double()).sum(), x)
    assert (gx - dwant).abs().max() <= tiny and torch.equal(gx[dwant.abs() > tiny], dwant[dwant.abs() > tiny])
    assert ah.route_mlp_units(width).unique().numel() == 16 and torch.equal(ah.route_mlp_units(width) % 16, torch.arange(16))


@pytest.mark.parametrize("name", ah.ACTS)
@pytest.mark.parametrize("f16", [False, True])
def test_value_routing_is_exact_in_the_float64_oracle(name, f16, grids):
    pts = grids[0].reshape(-1)[:200]
    K, hot = 64, 37
    ws, bs = ah.route_value(K, f16, hot=hot)
    ws = [w.double().requires_grad_(True) for w in ws]
    x = ah.value_inputs(pts).double()
    v = orc.mlp_forward(ws, [b.double() for b in bs], x, name).squeeze(-1)
    want, dwant = _torch_act(name, pts, 1)
    assert torch.equal(v.detach(), (K if f16 else 1) * want)
    block = torch.zeros(200, dtype=torch.float64)
    block[64:128] = 1.0
    dw0, = torch.autograd.grad((v * block).sum(), ws[0])
    rows = dw0 if f16 else dw0[hot:hot + 1]
    assert torch.equal(rows, (pts[64:128].double() * dwant[64:128]).expand_as(rows))
    if not f16:
        assert dw0.abs().sum() == dw0[hot].abs().sum()


def test_squash_routing_is_exact_in_the_float64_oracle(grids):
    x0 = grids[0].reshape(-1).double()
    obs = torch.stack([x0, torch.zeros_like(x0), torch.zeros_like(x0)], 1).requires_grad_(True)
    ws, bs = ah.route_squash(64)
    lim = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in ah.SQUASH_LIMITS.items()}
    net = dict(w=[w.double() for w in ws], b=[b.double() for b in bs], act="relu", act_low=lim["policy_low"], act_high=lim["policy_high"])
    a = orc.wrap_action(orc.policy_forward(net, obs, None), lim)
    lq = {k: torch.as_tensor(v, dtype=torch.float64) if isinstance(v, list) else v for k, v in ah.SQUASH_LQ.items()}
    nxt, rew, _ = orc.lq_step(lq, obs, a)
    want, dwant = ah.squash_reference(grids[0].reshape(-1))
    assert torch.equal(nxt[:, 0].detach(), torch.zeros_like(x0)) and torch.equal((nxt[:, 1] - nxt[:, 2]).detach(), want)
    assert (rew == 0).all() and ((nxt[:, 1] == 0) | (nxt[:, 2] == 0)).all()
    g, = torch.autograd.grad((nxt[:, 1] - nxt[:, 2]).sum(), obs)
    assert ((g[:, 0] - dwant).abs() <= 1e-15 + 1e-12 * dwant.abs()).all() and (g[:, 0][x0 == 0] == 0).all()   # (autograd: 1 - tanh^2)
    assert torch.equal(want, -ah.squash_reference(-grids[0].reshape(-1))[0])   # odd


# The accuracy statements of csrc/common.h (comments above gelu_pair, gelu_pair_h, act_fwd_t and fast_tanh) and DESIGN.md 2.2e:
# the restatements' largest errors over both grids stay within them.  (Measured here: see the printed figures.)
CLAIMS = dict(gelu_pair=dict(phi=3.1e-7, gelu=4.5e-7, dgelu=3.5e-7), gelu_pair_h=dict(phi=1.6e-5, gelu=1.2e-5, dgelu=1.6e-5),
              fast_tanh=dict(rel=6.0e-7), elu=dict(abs=1.4e-7), selu=dict(abs=3.0e-7))


def test_restatement_errors_stay_within_the_claims_of_common_h():
    got = ah.claims()
    print(got)
    for fn, terms in CLAIMS.items():
        for k, claim in terms.items():
            assert got[fn][k] <= claim, (fn, k, got[fn][k], claim)
            assert got[fn][k] >= claim / 4, (fn, k, got[fn][k], claim)   # a claim four times too wide says nothing


@pytest.mark.parametrize("name", ah.ACTS)
def test_restated_derivative_from_the_stash_is_close_to_float64(name, grids):
    """act_bwd_t rebuilds act' from the stored activation: within 1e-6 absolute of the float64 derivative in fp32 storage (1.6e-5 +
    half rounding for the half kernels) on both grids, except at the kink of relu / elu / selu at z = +-0, where it is the
    left-hand derivative (h = 0 is not > 0)."""
    for g in grids:
        z = g.reshape(-1)
        for f16 in (False, True):
            _, d = ah.restate(name, z, f16=f16)
            _, want = ah.reference(name, z)
            tol = 2e-3 if f16 else 1e-6
            keep = torch.ones_like(z, dtype=torch.bool) if name in ("gelu", "sigmoid", "tanh") else z != 0
            assert ((d - want).abs()[keep] <= tol).all(), (name, f16, (d - want).abs()[keep].max().item())


def test_fast_tanh_branches_differ_above_the_switch(grids):
    """Between 1/8 and 1/4 the exponential branch and the series disagree in their last bits at many grid points: a kernel whose
    bits equal the series at EVERY such point has its switch in the wrong place (the GPU test asserts that)."""
    z = grids[0].reshape(-1)
    band = z[(z.abs() >= 0.125) & (z.abs() < 0.25)]
    assert band.numel() >= 256
    assert int((ah.fast_tanh_series(band) != ah.fast_tanh_big(band)).sum()) > band.numel() // 4
    assert torch.equal(ah.fast_tanh(z), -ah.fast_tanh(-z))
