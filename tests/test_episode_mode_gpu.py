"""`gops_episode_rollout_mode` and `Evaluator(stochastic_mode=True)` on the MI355X: a StochaPolicy evaluated by the mode of its action
distribution in one launch, against the per-step loop (`step_loop`: torch `policy(obs)`, `get_act_dist(...).mode()`, one
`gops_env_step` per step) on the same evaluator, initial conditions and networks.

Shapes: E = 5 and E = 37 (no multiple of the 16-row tile; 37 spans three tiles), hidden (16,) and (32, 16), T = 12.

The head (`shape_head`): the last layer's mean rows are scaled up (by at most MAX_GAIN) until the means spread over about +-1.5
(tanh-Gaussian head: the tanh has to saturate) or +-0.5 (Gaussian head: its limits follow the means, a wider spread only adds gain) on
the observations the episodes visit; the log-std rows are large random values, which must not reach the action.  Gaussian head: the
means are centred on 0 and the policy's limits are their 30 % and 70 % quantiles: several means leave [low, high] and the clamp
returns a limit, several stay inside.  Tanh-Gaussian head: the means are centred on 1.83 (1 - tanh = 0.05) under narrow limits
(a fifth of the helpers'): about half of them saturate the tanh - the action lies within 5 % of the half range of `high` -, the
others sit on its shoulder, and nearly all lie outside [low, high].  Both are asserted on the means of the loop's own trace.
Why the gain is capped: the two paths are two fp32 evaluations of the same stack (rocBLAS GEMMs against the kernel's MFMA tiles)
and differ by rounding, a few 1e-7 of a mean; the closed loop multiplies that difference by (head gain x env sensitivity) at every
step.  With the rows scaled by the 50 - 100 that the narrow cartpole reset states would need, the paths drift apart by 1e-4 in twelve
steps although each step agrees to rounding (measured: first action against float64 0 / 6e-8); cartpole therefore starts from states
spread over the track, and no row is scaled by more than MAX_GAIN.

Bound of the float comparisons: the one tests/test_episode_gpu.py holds its fused kernel to against its per-step loop - the shared
`deviations` (the return against max(1, |return|), the observations against max(1, the largest |observation|)), at most
max(4 x the loop's own deviation from a record, 1e-5).  No record exists for these policies, so the bound is its floor, 1e-5, the
smallest value that rule can give; actions and rewards are held to the same figure in the same form (against max(1, the loop's
largest |value|)).  `length` and `terminated` are equal, for every row: none is left out.  Every figure is printed before it is
asserted (run with -s).  On an MI355X the largest of the 24 x 4 figures was 2.4e-6 (veh3dof, Gaussian head, (16,), E = 5: the actions),
the next 1.2e-6, most below 5e-7; the first action against float64: 2.6e-8 / 6.0e-9.  (With the Gaussian head's means spread over
+-1.5 like the tanh-Gaussian's, the same veh3dof case at E = 37 came to 9.4e-6: gain that the clamp does not need.)"""
import copy

import numpy as np
import pytest
import torch

import closed_loop_helpers as cl
from closed_loop_helpers import deviations, rows, stocha_evaluator

from gops_amd.utils.act_distribution import TanhGaussDistribution

pytestmark = pytest.mark.gpu
BOUND = 1e-5
T = 12
MAX_GAIN = 8.0
TILES = [14, 15, 16, 17, 36]   # rows of the E = 37 run, from all three of its tiles, run again at E = 5


def shape_head(nets, probe):
    """The head described in the module docstring, shaped on the observations `probe`; the limits are written into the policy."""
    pol = nets.policy
    A = pol.act_dim
    head = pol.linear_layers()[-1]
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        y = pol.policy(probe)[:, :A]
        spread = 1.5 if pol.action_distribution_cls is TanhGaussDistribution else 0.5
        scale = (spread / y.std(dim=0)).clamp(1.0, MAX_GAIN)
        head.weight[:A].mul_(scale[:, None])
        head.bias[:A].mul_(scale)
        y = pol.policy(probe)[:, :A]
        if pol.action_distribution_cls is TanhGaussDistribution:
            head.bias[:A].add_(1.83 - y.median(dim=0).values)
            pol.act_low_lim.mul_(0.2), pol.act_high_lim.mul_(0.2)
        else:
            head.bias[:A].sub_(y.median(dim=0).values)
            q = torch.quantile(y - y.median(dim=0).values, torch.tensor([0.3, 0.7], device=y.device), dim=0)
            pol.act_low_lim.copy_(q[0])
            pol.act_high_lim.copy_(torch.maximum(q[1], q[0] + 0.05))
        head.weight[A:].copy_(5.0 * torch.randn(head.weight[A:].shape, generator=g))
        head.bias[A:].copy_(5.0 * torch.randn(head.bias[A:].shape, generator=g))


def initial_conditions(ev, env, E, seed=5):
    """E reset states of the data env.  Cartpole: states spread over the track instead (position within +-1.5 of the +-2.4 bound,
    speed +-1, angle +-0.03 of the 0.21 bound, rate +-0.1); the last row starts where the first step ends the episode."""
    init = cl.initial_conditions(ev, env, E, seed)
    if env == "cartpole":
        g = torch.Generator().manual_seed(seed)
        spread = torch.tensor([1.5, 1.0, 0.03, 0.1])
        init["obs"] = ((2 * torch.rand(E, 4, generator=g) - 1) * spread).to(ev.device)
        cl.doom(env, init, [E - 1])
    return init


def make_case(env, hidden, dist):
    """(evaluator, networks, the E = 37 initial conditions).  The head is shaped on the observations these episodes visit under the
    policy as it was initialised; the evaluator is built after that, so that its description carries the limits."""
    probe, nets = stocha_evaluator(env, hidden, dist, T=T)
    init = initial_conditions(probe, env, 37)
    visited = probe.step_loop(init, trace=True, trace_fill=0.0)
    inside = torch.arange(T, device=probe.device)[None, :] < visited["length"][:, None]
    shape_head(nets, visited["trace_obs"][inside])
    ev, _ = stocha_evaluator(env, hidden, dist, T=T, nets=nets, stochastic_mode=True)
    return ev, nets, init


def raw_means(nets, res):
    """The policy's raw means on every recorded observation of `res`, [n, A]."""
    inside = torch.arange(T, device=res["length"].device)[None, :] < res["length"][:, None]
    with torch.no_grad():
        return nets.policy.policy(res["trace_obs"][inside])[:, :nets.policy.act_dim]


def compare(label, fused, loop):
    """The fused run against the loop's: books equal, floats within BOUND in the form of `deviations`."""
    assert torch.equal(fused["length"], loop["length"]), (label, fused["length"], loop["length"])
    assert torch.equal(fused["terminated"], loop["terminated"]), label
    lp = {k: v.cpu().numpy() for k, v in loop.items()}
    d_ret, d_obs = deviations(fused, lp["trace_obs"], lp["ret"].astype(np.float64), lp["length"])
    inside = np.arange(T)[None, :] < lp["length"][:, None]
    d = {}
    for k in ("trace_act", "trace_rew"):
        got, want = fused[k].cpu().numpy().reshape(inside.shape + (-1,)), lp[k].reshape(inside.shape + (-1,))
        d[k] = float((np.abs(got - want) * inside[:, :, None]).max() / max(1.0, float((np.abs(want) * inside[:, :, None]).max())))
    print(f"{label}: fused vs loop  ret {d_ret:.3e} obs {d_obs:.3e} act {d['trace_act']:.3e} rew {d['trace_rew']:.3e} | bound {BOUND:.0e}")
    assert d_ret <= BOUND and d_obs <= BOUND and d["trace_act"] <= BOUND and d["trace_rew"] <= BOUND, (label, d_ret, d_obs, d)


@pytest.mark.parametrize("hidden", [(16,), (32, 16)], ids=["h16", "h32x16"])
@pytest.mark.parametrize("dist", ["gauss", "tanh_gauss"])
@pytest.mark.parametrize("env", ["cartpole", "lq", "veh3dof"])
def test_fused_against_the_per_step_loop(env, dist, hidden):
    ev, nets, init37 = make_case(env, hidden, dist)
    low, high = nets.policy.act_low_lim, nets.policy.act_high_lim
    for E, init in ((37, init37), (5, rows(init37, [0, 1, 2, 3, 36]))):
        loop = ev.step_loop(init, trace=True, trace_fill=0.0)
        fused = ev.run_episodes(init, trace=True, trace_fill=0.0)
        assert ev.path == "fused"
        compare(f"{env} {dist} {hidden} E={E}", fused, loop)
        # several means leave the limits, and not every one does what the others do: the clamp / the saturation are run, and their complement
        mean = raw_means(nets, loop)
        n_out, n_in, n_sat = int(((mean > high) | (mean < low)).sum()), int(((mean > low) & (mean < high)).sum()), int((mean.abs() > 1.83).sum())
        print(f"    means outside [low, high] {n_out}, inside {n_in}, beyond +-1.83 {n_sat} of {mean.numel()}")
        assert n_out >= 4
        inside = torch.arange(T, device=ev.device)[None, :] < fused["length"][:, None]
        act = fused["trace_act"][inside]
        assert bool((act >= low).all()) and bool((act <= high).all())
        if dist == "gauss":   # the clamp returns the limits themselves; inside them the action is the mean
            assert n_in >= 2 and int(((act == high) | (act == low)).sum()) >= 4 and int(((act > low) & (act < high)).sum()) >= 2
        else:                 # the tanh is saturated: the action within 5 % of the half range of a limit; and some are not
            near = (act > high - 0.05 * (high - low) / 2) | (act < low + 0.05 * (high - low) / 2)
            assert n_sat >= 4 and mean.numel() - n_sat >= 2 and int(near.sum()) >= 4 and int((~near).sum()) >= 2
        if env == "cartpole":
            assert int(fused["length"][E - 1]) == 1 and float(fused["terminated"][E - 1]) == 1.0
            assert bool(((fused["length"] == T) & (fused["terminated"] == 0)).any())


@pytest.mark.parametrize("dist", ["gauss", "tanh_gauss"])
def test_first_action_against_float64(dist):
    ev, nets, init37 = make_case("cartpole", (32, 16), dist)
    init = rows(init37, [0, 1, 2, 3, 36])
    fused = ev.run_episodes(init, trace=True, trace_fill=0.0)
    assert ev.path == "fused"
    pol64 = copy.deepcopy(nets.policy).cpu().double()
    with torch.no_grad():
        want = pol64.get_act_dist(pol64(init["obs"].cpu().double())).mode()
    got = fused["trace_act"][:, 0].cpu().double()
    err = float((got - want).abs().max() / max(1.0, float(want.abs().max())))
    print(f"{dist}: first action against float64 {err:.3e} | bound {BOUND:.0e}")
    assert err <= BOUND


@pytest.mark.parametrize("dist", ["gauss", "tanh_gauss"])
def test_tile_independence_and_repeat_launches(dist):
    ev, nets, init37 = make_case("veh3dof", (32, 16), dist)
    a = {k: v.clone() for k, v in ev.run_episodes(init37, trace=True, trace_fill=0.0).items()}
    b = ev.run_episodes(init37, trace=True, trace_fill=0.0)
    assert ev.path == "fused"
    for k in a:
        assert torch.equal(a[k], b[k]), k
    small = ev.run_episodes(rows(init37, TILES), trace=True, trace_fill=0.0)
    assert ev.path == "fused"
    for k in a:
        assert torch.equal(a[k][TILES], small[k]), k


def test_routing():
    ev, nets, init37 = make_case("cartpole", (16,), "tanh_gauss")
    init = rows(init37, [0, 1, 2, 3, 36])
    ev.run_episodes(init)
    assert ev.path == "fused" and ev.kernel_refuses() is None
    off, _ = stocha_evaluator("cartpole", (16,), "tanh_gauss", T=T)   # the default keyword
    off.run_episodes(init)
    assert off.path == "loop: stochastic policy"
    wide, wnets = stocha_evaluator("cartpole", (24,), "tanh_gauss", T=T, stochastic_mode=True)   # no multiple of 16: the kernel's plan refuses
    got = wide.run_episodes(init, trace=True, trace_fill=0.0)
    assert wide.path.startswith("loop: ") and "outside the episode kernel" in wide.path
    want = wide.step_loop(init, trace=True, trace_fill=0.0)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_the_limits_override_of_the_rollout_class():
    """`hb.EpisodeRollout(mode_head=..., act_low=..., act_high=...)`: the description's own limits handed in again change nothing;
    narrower ones are the clamp's."""
    from gops_amd import hip_backend as hb
    ev, nets, init37 = make_case("lq", (16,), "gauss")
    init = rows(init37, [0, 1, 2, 3, 36])
    want = ev.run_episodes(init, trace=True, trace_fill=0.0)
    env, mlp = ev._hip_env(), nets.policy.hip_mlp()
    low, high = nets.policy.act_low_lim, nets.policy.act_high_lim
    same = hb.EpisodeRollout(env, mlp, episodes=5, max_steps=T, mode_head=hb.SAMPLE_GAUSS, act_low=low, act_high=high).run(init, trace=True, trace_fill=0.0)
    for k in want:
        assert torch.equal(same[k], want[k]), k
    narrow = hb.EpisodeRollout(env, mlp, episodes=5, max_steps=T, mode_head=hb.SAMPLE_GAUSS, act_low=low / 2, act_high=high / 2).run(init, trace=True)
    first = narrow["trace_act"][:, 0]
    assert bool((first >= low / 2).all()) and bool((first <= high / 2).all()) and bool(((first == low / 2) | (first == high / 2)).any())
    assert list(env.policy_low[:2]) == pytest.approx(low.tolist())   # the caller's description is not written to
    with pytest.raises(ValueError, match="mode_head"):
        hb.EpisodeRollout(env, mlp, episodes=5, max_steps=T, mode_head=hb.SAMPLE_DETERM)


def test_sac_container_evaluates_in_one_launch(tmp_path):
    import ac_helpers as ac
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    torch.manual_seed(0)
    kw = ac.trainer_kwargs("SAC", "gym_cartpoleconti", 4, 1.0, tmp_path, policy_min_log_std=-20, policy_max_log_std=0.5, gamma=0.99, tau=0.005,
                           auto_alpha=True)
    alg = create_alg(**kw)
    alg.networks.to("cuda")
    ev = create_evaluator(**dict(kw, env_model=create_env_model(**kw), networks=alg.networks, num_eval_episode=4, eval_save=False,
                                 is_render=False, max_episode_steps=40, stochastic_mode=True))
    assert np.isfinite(ev.run_evaluation(0))
    assert ev.path == "fused"
    assert tuple(ev.last["length"].shape) == (4,) and 1 <= int(ev.last["length"].min()) and int(ev.last["length"].max()) <= 40
