"""The oracle of tests/test_optim_gpu.py checked where it can be checked without a GPU: `adam_ref64` against torch's own float64
Adam, and the rounding-count bounds against an fp32 emulation of the kernel's operation order (tests/optim_helpers.py)."""
import numpy as np
import pytest
import torch

import optim_helpers as oh

HYPER = [dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8), dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6)]


@pytest.mark.parametrize("hyper", HYPER, ids=["default", "betas-0.8-0.99"])
@pytest.mark.parametrize("grad_scale", oh.GRAD_SCALES)
def test_adam_ref64_matches_torch_float64_adam(hyper, grad_scale):
    """Five steps of `adam_ref64`, carried in float64, against torch.optim.Adam (foreach=False) on float64 CPU tensors that are handed
    the same scaled gradients: 1e-12 relative per element of p, exp_avg and exp_avg_sq."""
    n = 4096
    rng = np.random.default_rng(5)

    def spread(lo, hi, signed=True):   # (no engineered cancellation here: 1e-12 is RELATIVE to the result)
        x = 10.0 ** rng.uniform(lo, hi, n) * (rng.choice([-1.0, 1.0], n) if signed else 1.0)
        return x.astype(np.float32)
    p0, m0, v0 = spread(-4, 1), spread(-12, 8), spread(-24, 16, signed=False)
    par = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([par], foreach=False, **hyper)
    k0 = 3   # a loaded state: moments and step count of an earlier run
    opt.state[par] = dict(step=torch.tensor(float(k0)), exp_avg=torch.from_numpy(m0).double(), exp_avg_sq=torch.from_numpy(v0).double())
    P, M, V = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    for k in range(5):
        g = spread(-12, 8)
        par.grad = torch.from_numpy(g).double() * grad_scale
        opt.step()
        P, M, V, dP, D = oh.adam_ref64(P, M, V, g, t=k0 + k + 1, grad_scale=grad_scale, **hyper)
        for name, got, want in (("p", P, par.detach()), ("m", M, opt.state[par]["exp_avg"]), ("v", V, opt.state[par]["exp_avg_sq"])):
            want = want.numpy()
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (name, k, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
        assert np.allclose(dP, (P + dP) - P, rtol=0, atol=1e-12 * np.abs(P).max())


def test_adam_ref64_returns_the_inputs_of_elements_without_a_finite_scaled_gradient():
    p, m, v, g = oh.adam_grid(64, 9)
    g[[0, 5, 63]] = [np.nan, np.inf, -np.inf]
    g[7] = 3e38          # finite, fp32(g * 2) is not
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, t=4, grad_scale=2.0)
    ref = oh.adam_ref64(p, m, v, g, **hyper)
    skipped = np.zeros(64, bool)
    skipped[[0, 5, 7, 63]] = True
    assert np.array_equal(~oh.stepped(g, 2.0), skipped)
    for got, inp in zip(ref[:3], (p, m, v)):
        assert np.array_equal(got[skipped], inp[skipped].astype(np.float64)) and np.all(np.isfinite(got))
    assert np.all(ref[3][skipped] == 0) and np.all(oh.adam_ref64(p, m, v, g, **dict(hyper, grad_scale=1.0))[3][7] != 0)
    bounds = oh.adam_bounds(m, v, g, ref, lr=1e-3, betas=(0.9, 0.999), t=4, grad_scale=2.0)
    assert all(np.all(e[skipped] == 0) and np.all(np.isfinite(e)) for e in bounds)


@pytest.mark.parametrize("form", ["plain", "fma", "fma_alt"])
def test_fp32_emulation_of_the_kernel_stays_within_the_bounds(form):
    """The fp32 restatement of adam_kernel's element - uncontracted, and with the multiply-adds hipcc may contract - against
    `adam_ref64` on the grid the GPU test uses (every Adam size, steps 1 and 10001, every grad_scale, both sets of betas):
    every element of p, m, v within E_p, E_m, E_v.  What the reference and its bounds alone can be held to."""
    worst = oh.Worst()
    for hyper in HYPER:
        for t in (1, 10001):
            for gs in oh.GRAD_SCALES:
                for i, n in enumerate(oh.ADAM_SIZES):
                    p, m, v, g = oh.adam_grid(n, 100 + i, hyper["betas"], fresh=(t == 1))
                    ref = oh.adam_ref64(p, m, v, g, t=t, grad_scale=gs, **hyper)
                    got = oh.adam_emulate32(p, m, v, g, t=t, grad_scale=gs, form=form, **hyper)
                    assert all(np.all(np.isfinite(x)) for x in got)
                    bounds = oh.adam_bounds(m, v, g, ref, lr=hyper["lr"], betas=hyper["betas"], t=t, grad_scale=gs)
                    worst.check(f"{form} betas={hyper['betas']} t={t} gs={gs:.3g} n={n}", got, ref, bounds)
                    z = oh.adam_zero_case(m, v, g)
                    assert z.sum() > 0 or n < 64
                    for a, b in zip(got, (p, m, v)):
                        assert oh.bits_equal(a[z], b[z])
    worst.report(f"fp32 emulation ({form})")
    assert all(worst.r[k][0] > 0.05 for k in "pmv")   # (the bounds are not orders of magnitude away from what fp32 does)


def test_three_carried_steps_of_the_emulation_stay_within_the_added_bounds():
    """Three fp32 steps from one loaded state against three float64 steps carried in float64, the bounds of every step added up
    with the propagation of `adam_bounds(carried=)`: the rule test_optim_gpu.py applies to the device."""
    hyper = HYPER[0]
    worst = oh.Worst()
    for form in ("plain", "fma"):
        p, m, v, _ = oh.adam_grid(65537, 3)
        R, carried = (p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)), None
        for k in range(3):
            g = oh.adam_grid(65537, 30 + k)[3]
            ref = oh.adam_ref64(*R, g, t=41 + k, grad_scale=1.0 / 3.0, **hyper)
            carried = oh.adam_bounds(R[1], R[2], g, ref, lr=hyper["lr"], betas=hyper["betas"], t=41 + k, grad_scale=1.0 / 3.0, carried=carried)
            p, m, v = oh.adam_emulate32(p, m, v, g, t=41 + k, grad_scale=1.0 / 3.0, form=form, **hyper)
            R = ref[:3]
            worst.check(f"{form} step {k + 1}", (p, m, v), ref, carried)
    worst.report("fp32 emulation, three carried steps")


def test_bit_restatements_and_size_lists():
    """polyak_ref32 / value_grad_ref32 round every operation once (they differ from the float64 value rounded once at some element,
    and agree with torch's two-pass fp32 arithmetic everywhere); the size lists sit on the loop edges their comments name."""
    rng = np.random.default_rng(1)
    t, p = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    for tau in (0.005, 0.5, 1.0):
        got = oh.polyak_ref32(t, p, tau)
        assert got.dtype == np.float32
        want = torch.from_numpy(t) * torch.tensor(1.0 - tau, dtype=torch.float64).float() + torch.tensor(tau, dtype=torch.float64).float() * torch.from_numpy(p)
        assert oh.bits_equal(got, want.numpy())
    assert oh.bits_equal(oh.polyak_ref32(t, p, 1.0), p + np.float32(0.0) * t)   # tau = 1: the online value (0 * t + p)
    once = (t.astype(np.float64) * (1 - 0.005) + 0.005 * p.astype(np.float64)).astype(np.float32)
    assert not oh.bits_equal(oh.polyak_ref32(t, p, 0.005), once)
    a, b = t[:1000], p[:1000]
    gr = oh.value_grad_ref32(a, b)
    assert gr.dtype == np.float32 and oh.bits_equal(gr, (torch.tensor(2.0 / 1000, dtype=torch.float64).float() * (torch.from_numpy(a) - torch.from_numpy(b))).numpy())
    trip = 4 * 64 * 256
    assert {trip - 1, trip, trip + 1, trip + 16384 + 1, 4 * trip + 3, 1, 255, 256, 257, 1023, 1024, 1025} == set(oh.ADAM_SIZES)
    assert {1, 257, 64 * 256, 64 * 256 + 1, 4 * 64 * 256 + 1} == set(oh.POLYAK_SIZES)
    one, many = 8 * 256, 8 * 64 * 256
    assert {1, one - 1, one, one + 1, oh.LOSS_ONE_BLOCK_MAX, oh.LOSS_ONE_BLOCK_MAX + 1, many - 1, many, many + 1, 2 * many + 1} == set(oh.LOSS_SIZES)
