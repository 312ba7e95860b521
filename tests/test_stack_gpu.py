"""gops_stack_sample_rollout / gops_stack_episode_rollout against float64 (stack_helpers.py), teacher-forced: every stored row is
recomputed on its own from the stored window, action and noise, so nothing compounds along a trajectory.  Bounds: the recurrent kernels'
own (tests/test_rnn_gpu.py) - relative L2 < 1e-5 for outputs; rows that are copies of earlier values are bit-equal."""
import numpy as np
import pytest
import torch

import stack_helpers as sh
from conftest import rel_l2
from rnn_helpers import ppo_kwargs

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.trainer.evaluator import Evaluator
from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
from gops_amd.trainer.sampler.reset_pool import restate_sample_books

pytestmark = pytest.mark.gpu

R = 3   # pool rows
# (n_envs, T, L, H, head hidden, max_episode_steps): L = 1 - no W_hh chain; a ragged tile, T > L - the ring wraps -, a time-limit reset
# inside the launch (and instances 0 .. 3 start at theta = 0.2 moving outward: a threshold termination and its reset); the NB = 2
# instantiation, three tiles, the L bound; T shorter than what refills a window, non-power-of-two widths, two head layers
CASES = [(1, 1, 1, 16, (16,), 200), (17, 7, 5, 64, (64,), 4), (33, 12, 8, 128, (128,), 200), (16, 3, 2, 48, (32, 16), 200)]


def _setup(N, T, L, H, head, max_steps, steps=None):
    """Policy (device), its float64 copy, the rollout object, the state / pool / noise of a launch of `steps` (default T) steps."""
    steps = T if steps is None else steps
    net, ref = sh.make_policy(H, head, 100 * N + L)
    net = net.cuda()
    rng = np.random.RandomState(7 * N + T)
    draw = lambda *shape: rng.uniform(-sh.RESET_HALF_RANGE, sh.RESET_HALF_RANGE, size=shape + (4,)).astype(np.float32)  # noqa: E731
    x0, pool = draw(N), draw(R, N)
    if max_steps == 4:
        x0[:4] = np.array([0.0, 0.0, 0.2, 0.5], np.float32)
    state = dict(obs=torch.from_numpy(x0).unsqueeze(1).repeat(1, L, 1).contiguous().cuda(), t=torch.zeros(N, dtype=torch.int32).cuda(),
                 reset_count=torch.zeros(N, dtype=torch.int32).cuda())
    ro = hb.StackSampleRollout(sh.hip_env(net, L), net.hip_rnn(L), n_envs=N, steps=steps, max_episode_steps=max_steps, pool_rows=R,
                               min_log_std=sh.MIN_LOG_STD, max_log_std=sh.MAX_LOG_STD)
    noise = torch.from_numpy(rng.standard_normal((steps, N, 1)).astype(np.float32)).cuda()
    return net, ref, ro, state, dict(obs=torch.from_numpy(pool).cuda()), noise


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}-T{}-L{}-H{}-{}-max{}".format(*c))
def test_sampler_rows_teacher_forced(case):
    N, T, L, H, head, max_steps = case
    net, ref, ro, state, pool, noise = _setup(*case)
    first = state["obs"].cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in ro.run(state, pool, noise).items()}
    obs, obs2, eps = out["obs"], out["obs2"], noise.cpu().numpy()[..., 0].astype(np.float64)
    # the policy and the exploration head on the stored windows
    mean, raw = sh.head64(ref, obs.reshape(T * N, L, 4))
    ls = np.clip(raw, sh.MIN_LOG_STD, sh.MAX_LOG_STD).reshape(T, N)
    assert rel_l2(torch.from_numpy(out["act"][..., 0]), torch.from_numpy(mean.reshape(T, N) + np.exp(ls) * eps)) < 1e-5
    assert rel_l2(torch.from_numpy(out["logp"]), torch.from_numpy(-eps * eps / 2 - ls - 0.5 * np.log(2 * np.pi))) < 1e-5
    # the env step on the stored newest state and action
    xn, done = sh.step64(obs[:, :, -1], out["act"][..., 0])
    assert sh.threshold_margin(xn) > 1e-4   # fp32 and float64 cannot disagree on `done`
    assert rel_l2(torch.from_numpy(obs2[:, :, -1]), torch.from_numpy(xn)) < 1e-5
    assert np.array_equal(out["done"], done.astype(np.float32)) and (out["rew"] == 1.0).all()
    assert np.array_equal(obs2[:, :, :-1], obs[:, :, 1:])   # the shift: copies
    # the books, and where every window continues from: the step's own next window, or L copies of the instance's pool row
    books = restate_sample_books(out["done"], np.zeros(N), np.zeros(N), max_steps, R)
    for k in ("time_limited", "end"):
        assert np.array_equal(out[k], books[k]), k
    assert np.array_equal(state["t"].cpu().numpy(), books["t"]) and np.array_equal(state["reset_count"].cpu().numpy(), books["reset_count"])
    fresh = np.repeat(pool["obs"].cpu().numpy()[np.maximum(books["src"], 0), np.arange(N)][:, :, None], L, axis=2)   # [T, N, L, 4]
    after = np.where((books["src"] >= 0)[..., None, None], fresh, obs2)
    assert np.array_equal(obs[0], first) and np.array_equal(obs[1:], after[:-1]) and np.array_equal(state["obs"].cpu().numpy(), after[-1])
    if max_steps == 4:   # both kinds of reset fell inside the launch
        assert out["done"][0, :4].all() and out["time_limited"].any() and (books["src"] >= 0).sum() > 4


def test_second_call_continues_and_calls_are_reproducible():
    """Two launches of 4 steps equal one of 8 on the same noise, bit for bit (windows, counters and reset counts are carried over; the
    ring is rebuilt from the stored window); two launches on equal inputs are bit-equal."""
    case = (17, 4, 5, 64, (64,), 3)
    _, _, whole, st8, pool, noise = _setup(*case, steps=8)
    want = {k: v.clone() for k, v in whole.run(st8, pool, noise).items()}
    _, _, half, st4, _, _ = _setup(*case)
    start = {k: v.clone() for k, v in st4.items()}
    a = {k: v.clone() for k, v in half.run(st4, pool, noise[:4].contiguous()).items()}
    b = half.run(st4, pool, noise[4:].contiguous())
    assert (a["end"][3] == 1).all()   # a launch's last step ends every segment: the one column that knows where a launch stops
    a["end"][3] = want["end"][3]
    for k in want:
        assert torch.equal(torch.cat((a[k], b[k])), want[k]) and torch.isfinite(want[k]).all(), k
    assert all(torch.equal(st4[k], st8[k]) for k in st4)
    again = half.run(start, pool, noise[:4].contiguous())
    assert all(torch.equal(again[k], a[k]) for k in a if k != "end")


@pytest.mark.parametrize("E", [1, 17, 33])
def test_evaluator_episodes_against_the_float64_loop(E):
    """Returns, lengths and done flags with max_steps = 12 (fp32 / float64 drift cannot move a length); episode 0 starts at
    theta = 0.2 moving outward and terminates by threshold."""
    L, T = 5, 12
    net, ref = sh.make_policy(64, (64,), 11 + E)
    net = net.cuda()
    x0 = np.random.RandomState(E).uniform(-sh.RESET_HALF_RANGE, sh.RESET_HALF_RANGE, size=(E, 4)).astype(np.float32)
    x0[0] = np.array([0.0, 0.0, 0.2, 0.5], np.float32)
    ro = hb.StackEpisodeRollout(sh.hip_env(net, L), net.hip_rnn(L), episodes=E, max_steps=T)
    res = {k: v.cpu().numpy() for k, v in ro.run(dict(obs=torch.from_numpy(x0).cuda())).items()}
    lo, hi = float(net.act_low_lim[0]), float(net.act_high_lim[0])
    want = [sh.episode64(ref, x0[e], L, T, lo, hi) for e in range(E)]
    assert min(w[2] for w in want) > 1e-4
    assert res["length"].tolist() == [w[0] for w in want] and res["terminated"].tolist() == [w[1] for w in want]
    assert res["ret"].tolist() == [float(w[0]) for w in want] and res["terminated"][0] == 1.0 and res["length"][0] < T


def test_ppo_samples_updates_and_evaluates_on_the_stacked_env():
    """The public path: the fused sampler feeds three local_updates of the recurrent pair, the evaluator runs its episodes."""
    torch.manual_seed(7)
    alg = create_alg(**ppo_kwargs(use_gpu=True))
    alg.networks.cuda()
    model = create_env_model("gym_cartpolecontiwithstack")
    smp = OnPolicyDeviceSampler(dict(env_id="gym_cartpolecontiwithstack"), model, n_envs=17, steps_per_sample=2, max_episode_steps=5, seed=3,
                                fused=True)
    smp.networks = alg.networks
    before = [p.detach().clone() for p in alg.networks.parameters()]
    for it in range(3):
        batch, _ = smp.sample()
        assert batch["obs"].shape == (34, 5, 4) and all(torch.isfinite(v).all() for v in batch.values() if v.is_floating_point())
        alg.local_update(batch, it)
        assert torch.isfinite(alg.last_loss_terms).all()
    assert smp.path == "fused: gops_stack_sample_rollout"
    assert all(not torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(alg.networks.parameters(), before))
    ev = Evaluator(env_model=model, networks=alg.networks, cfg=dict(env_id="gym_cartpolecontiwithstack"), num_eval_episode=5, eval_save=False,
                   max_episode_steps=10, stochastic_mode=True)
    assert 1.0 <= ev.run_evaluation(0) <= 10.0 and ev.path == "fused: gops_stack_episode_rollout"
