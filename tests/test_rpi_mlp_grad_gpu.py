"""The reverse pass and the Adam moments of csrc/rollout_rpi_mlp.hip on the MI355X, per parameter tensor against a float64 shadow of one
evaluation step (rpi_mlp_helpers.shadow_step).

After ONE step from zero moments the state block holds m = (1 - beta1) g and v = (1 - beta2) g^2, so the kernel's gradient can be read
element by element (`RpiMlpEvaluator.moments()`); the stepped parameters cannot show it, Adam's first step being lr sign(g) and every
step invariant to a factor on a whole tensor's gradient.  Bounds are not chosen in advance: the eager fp32 host path's deviation from
the shadow is measured on the same inputs, per tensor, and the kernel gets 4 times that with a floor of 1e-5 (the convention of
test_episode_gpu.py); every figure is printed before it is asserted (run with -s).  Deviations are relative to the tensor's largest
reference element."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rpi_helpers import fixture, sub
from rpi_mlp_helpers import (TENSOR_NAMES, all_cases, build, case_shape, flat_params, float64_default, heldout_norm64, host_gradient,
                             layer_sizes, raw_pair64, set_params, shadow_flat_grad, shadow_step, split_params,
                             tensor_deviation, to_double)

pytestmark = pytest.mark.gpu

BETA1, BETA2, EPS = 0.9, 0.99, 1e-8
ONE_MINUS_BETA1, ONE_MINUS_BETA2 = np.float32(1 - BETA1), np.float32(1 - BETA2)   # the weights the kernel and torch's Adam use
FLOOR, FACTOR = 1e-5, 4.0
ACTS = ("elu", "gelu", "tanh", "sigmoid")
MODEL_CASES = {"osc": lambda: sub(fixture("rpi_mlp_step_osc"), "b64/"), "air": lambda: fixture("rpi_mlp_air_b64_m8"),
               "susp": lambda: fixture("rpi_mlp_susp_b65_m8")}
FIXTURE_CASES = all_cases()


def _net_override(hidden, act, batch):
    return dict(value_hidden_sizes=list(hidden), value_hidden_activation=act, reset_batch_size=batch, sample_batch_size=batch)


def _first_step(case, use_gpu, obs0, params0, draws, max_step=None, **override):
    """One local_update of one step through the algorithm from zero moments -> its gradient as the moments show it."""
    from gops_amd.algorithm.rpi import RecordedResetSource
    alg = build(case, inject=False, use_gpu=use_gpu, max_step_update_value=1, **override)
    for net in (alg.networks.value, alg.networks.value_target):
        set_params(net, params0)
    alg.obs = torch.from_numpy(obs0).clone()
    if max_step is not None:
        alg.env_model.unwrapped.max_step_per_episode = torch.from_numpy(max_step).clone()
    alg.reset_source = RecordedResetSource(draws)
    info = alg.local_update(None, 0)
    assert info["num_update_value"] == 1
    if use_gpu:
        m, v = alg._evaluator.moments().cpu().numpy()
        count = float(alg._evaluator.state[0])
    else:
        m, v, count = alg._adam["exp_avg"].numpy(), alg._adam["exp_avg_sq"].numpy(), float(alg._adam["step"])
    return SimpleNamespace(m=m, v=v, g=m / ONE_MINUS_BETA1, gg=v / ONE_MINUS_BETA2, count=count, params=flat_params(alg.networks.value))


def _bounds(host_devs):
    return [max(FLOOR, FACTOR * d) for d in host_devs]


def _fmt(values):
    return "[" + " ".join(f"{v:.2e}" for v in values) + "]"


def _check_first_step(tag, case, sizes, act, obs0, params0, draws, references, max_step=None, **override):
    """Host path and kernel on the same inputs against each (name, flat float64 gradient) of `references`."""
    host = _first_step(case, False, obs0, params0, draws, max_step, **override)
    dev = _first_step(case, True, obs0, params0, draws, max_step, **override)
    names = " ".join(TENSOR_NAMES[2 * (len(sizes) - 1)])
    failures = []
    for ref_name, g64 in references:
        for what, h, d, want in (("g", host.g, dev.g, g64), ("v", host.gg, dev.gg, g64 ** 2)):
            host_devs, dev_devs = tensor_deviation(h, want, sizes), tensor_deviation(d, want, sizes)
            bounds = _bounds(host_devs)
            print(f"GRAD {tag} act={act} ref={ref_name} {what} ({names}): host {_fmt(host_devs)} kernel {_fmt(dev_devs)} bound {_fmt(bounds)}")
            if any(a > b for a, b in zip(dev_devs, bounds)):
                failures.append((ref_name, what, dev_devs, bounds))
    assert not failures, failures
    assert dev.m[-1] == 0 and dev.v[-1] == 0, "the output bias takes no gradient: both moments stay exactly 0"
    assert dev.params[-1:].view(np.uint32) == np.asarray(params0[-1:], dtype=np.float32).view(np.uint32), "output bias moved"
    assert dev.count == 1 and host.count == 1


# ---- (a) every fixture case: against the reference's recorded grad0 and against the shadow --------------------------------------------
@pytest.mark.parametrize("case", [c for _, c in FIXTURE_CASES], ids=[i for i, _ in FIXTURE_CASES])
def test_first_step_gradient_of_the_fixtures(case, request):
    sizes, act = case_shape(case)
    probe = build(case, inject=False, use_gpu=False)
    params = split_params(case["params0"], sizes)
    g64 = shadow_flat_grad(shadow_step(to_double(probe.env_model), act, params, params, case["obs0"]))
    _check_first_step(request.node.callspec.id, case, sizes, act, case["obs0"], case["params0"], case["draws"][:2],
                      [("grad0", case["grad0"].astype(np.float64)), ("shadow", g64)], max_step=case["max_step_alg"])


# ---- (b) generated cases --------------------------------------------------------------------------------------------------------------
def draw_params(rng, sizes, hidden_bias=0.0):
    """As ApproxContainer draws them: per Linear layer uniform(+-sqrt(6 / (fan_in + fan_out))) weights, zero biases (`hidden_bias`:
    hidden biases uniform in +-hidden_bias instead)."""
    flat = []
    for l, (fan_in, fan_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        bound = np.sqrt(6.0 / (fan_in + fan_out))
        flat.append(rng.uniform(-bound, bound, fan_out * fan_in))
        flat.append(rng.uniform(-hidden_bias, hidden_bias, fan_out) if hidden_bias and l + 2 < len(sizes) else np.zeros(fan_out))
    return np.concatenate(flat)


def generated_inputs(model, hidden, act, batch, seed, hidden_bias=0.0, n_draws=2, **extra):
    """Inputs from a fixed RandomState, selected by the shadow alone.  Candidate states are uniform in the model's
    initial_state_range, four times as many as needed; the output weights are scaled so that the median |raw action| of the
    candidates is 1 (both branches of ScaleAction's clip run); the first `batch` candidates whose float64 |h_i| is at least 0.1 of the
    candidates' mean|h| are kept (a sign(h_i) two orderings may disagree on is not the kernel's fault: the filter of
    test_rpi_mlp_gpu._pair_inputs).  The reset draws pass the same filter."""
    case = MODEL_CASES[model]()
    override = dict(_net_override(hidden, act, batch), **extra)
    probe = build(case, inject=False, use_gpu=False, **{"max_step_update_value": 1, **override})
    env64, bare = to_double(probe.env_model), probe.env_model.unwrapped
    sizes = layer_sizes(bare.state_dim, hidden)
    rng = np.random.RandomState(seed)
    flat = draw_params(rng, sizes, hidden_bias)
    scale = np.asarray(bare.initial_state_range, dtype=np.float64)
    n_rows = n_draws * batch   # the start states and one set per reset draw (the held-out set feeds no gradient: unfiltered)

    def candidates(n):
        return rng.uniform(-scale, scale, (4 * n, len(scale))).astype(np.float32)

    cand = candidates(n_rows)
    with float64_default():
        params = split_params(flat, sizes)
        raw = raw_pair64(env64, params, act, torch.from_numpy(cand).double()).numpy()
    flat[-(sizes[-2] + 1):-1] /= np.median(np.abs(raw[:, 0]))
    params0 = flat.astype(np.float32)
    params = split_params(params0, sizes)
    step = shadow_step(env64, act, params, params, cand)
    keep = np.abs(step.h) >= 0.1 * np.abs(step.h).mean()
    rows, raw_action = cand[keep][:n_rows], step.pair[keep][:n_rows, 0]
    assert rows.shape[0] == n_rows, f"{rows.shape[0]} of {4 * n_rows} candidate rows survived, {n_rows} needed"
    obs0 = rows[:batch]
    if batch >= 63:
        outside = float((np.abs(raw_action[:batch]) > 1).mean())
        assert 0.1 <= outside <= 0.9, f"raw action outside [-1, 1] on {outside:.0%} of the rows"
    held_out = candidates(batch)[:batch]
    draws = np.stack([held_out] + [rows[k * batch:(k + 1) * batch] for k in range(1, n_draws)])
    return SimpleNamespace(case=case, override=override, env64=env64, sizes=sizes, act=act, obs0=obs0, params0=params0, draws=draws,
                           rng=rng, bare=bare, loss_scale=float(np.abs(step.h).mean()))


OSC_NETS = ([16], [32], [48], [64], [16, 16], [16, 64], [64, 16], [32, 48], [48, 32], [64, 64])
GENERATED = [("osc", h, a, 65) for h in OSC_NETS for a in ACTS]
GENERATED += [(m, h, a, 130) for m in ("osc", "air", "susp") for h in ([48], [32, 48]) for a in ACTS]
GENERATED += [(m, h, a, b) for m, h, a in (("susp", [64, 16], "gelu"), ("air", [16], "sigmoid")) for b in (1, 63, 64, 65, 128, 1024)]


def _case_seed(model, hidden, act, batch):
    return [20261018, ("osc", "air", "susp").index(model), ACTS.index(act), batch] + list(hidden)


@pytest.mark.parametrize("model,hidden,act,batch", GENERATED,
                         ids=[f"{m}-{'x'.join(map(str, h))}-{a}-b{b}" for m, h, a, b in GENERATED])
def test_first_step_gradient_of_generated_cases(model, hidden, act, batch, request):
    """Every supported width pair and activation at B = 65 (a second tile with one live row), three tiles with the last one partial
    on all three models, and the batch edges 1, 63, 64, 65, 128, 1024 (GOPS_RPI_MAX_BATCH: 16 tiles)."""
    inp = generated_inputs(model, hidden, act, batch, _case_seed(model, hidden, act, batch))
    params = split_params(inp.params0, inp.sizes)
    g64 = shadow_flat_grad(shadow_step(inp.env64, act, params, params, inp.obs0))
    _check_first_step(request.node.callspec.id, inp.case, inp.sizes, act, inp.obs0, inp.params0, inp.draws, [("shadow", g64)],
                      **inp.override)


# ---- a step-by-step chain across launches ---------------------------------------------------------------------------------------------
CHAIN_STEPS, CHAIN_LR = 6, 1e-3
# (model, hidden, activation, batch, thresholds): nets whose moment offsets differ from [64, 64]'s.  The thresholds sit at 1.5 times
# the initial_state_range, so that lanes started inside them can cross within the chain.
CHAINS = [("susp", [16, 64], "gelu", 65, [0.075, 0.75, 0.075, 1.5]), ("air", [48], "tanh", 130, [0.15, 0.3, 0.15])]
CHAIN_SEED = {"susp": 3, "air": 3}


def chain_inputs(model, hidden, act, batch, threshold):
    """Start parameters (hidden biases in +-0.1: the first launch already reads non-zero biases), start lanes, time limits, the
    held-out set and one reset draw per step.  About a tenth of the lanes gets a time limit of 1 to 3 (the counter is never zeroed,
    so such a lane is reset at every later step), another tenth is placed half an Euler step inside a state threshold it moves
    towards; the rest has no limit within the chain."""
    inp = generated_inputs(model, hidden, act, batch, [20261018, CHAIN_SEED[model]] + list(hidden), hidden_bias=0.1,
                           n_draws=CHAIN_STEPS + 1, state_threshold=list(threshold), learning_rate=CHAIN_LR,
                           max_step_update_value=CHAIN_STEPS)
    rng, env64, bare = inp.rng, inp.env64, inp.bare
    tenth = max(1, batch // 10)
    lanes = rng.permutation(batch)
    max_step = np.full(batch, 1000.0)
    max_step[lanes[:tenth]] = rng.randint(1, 4, tenth)
    # threshold lanes: put one column on its threshold, keep the rows that move outwards there, then pull the column back inside by
    # half of the step the shadow takes from the threshold
    params = split_params(inp.params0, inp.sizes)
    thr, rest = np.asarray(threshold), lanes[tenth:]
    idx, col, sign = np.arange(len(rest)), rng.randint(len(thr), size=len(rest)), rng.choice([-1.0, 1.0], len(rest))
    x = inp.obs0[rest].copy()
    x[idx, col] = sign * thr[col]
    idle = dict(draw=x, count=np.zeros(len(rest)), max_step=np.full(len(rest), 1000.0))
    move = shadow_step(env64, act, params, params, x, **idle).euler[idx, col] - x[idx, col]
    x[idx, col] = (sign * thr[col] - 0.5 * move).astype(np.float32)
    st = shadow_step(env64, act, params, params, x, **idle)
    ok = (sign * move > 0) & st.done & (st.done_margin >= 5e-4) & (np.abs(st.h) >= 0.1 * inp.loss_scale)
    chosen = np.flatnonzero(ok)[:tenth]
    assert len(chosen) == tenth, f"{len(chosen)} of {tenth} threshold lanes placed"
    inp.obs0[rest[chosen]] = x[chosen]
    inp.max_step = max_step
    return inp


def _snapshot(alg, ev):
    """Host copies of everything a launch reads and writes."""
    moments = ev.moments().cpu().numpy().copy()
    return SimpleNamespace(value=flat_params(alg.networks.value).copy(), target=flat_params(alg.networks.value_target).copy(),
                           lanes=ev.lanes().t().cpu().numpy().copy(), counters=ev.counters().cpu().numpy().copy(), m=moments[0],
                           v=moments[1], count=float(ev.state[0]))


def _start(inp, use_gpu):
    alg = build(inp.case, inject=False, use_gpu=use_gpu, **inp.override)
    for net in (alg.networks.value, alg.networks.value_target):
        set_params(net, inp.params0)
    alg.obs = torch.from_numpy(inp.obs0).clone()
    alg.env_model.unwrapped.max_step_per_episode = torch.from_numpy(inp.max_step).clone()
    return alg


def _launch(alg, ev, pool, steps):
    """[steps + 1, B, S] held-out set and draws -> the launch's result as a list."""
    pool_dev = torch.from_numpy(np.ascontiguousarray(pool.transpose(0, 2, 1))).to(ev.device)
    return ev.evaluate(alg._max_step_dev, pool_dev, steps, CHAIN_LR, BETA1, BETA2, EPS).tolist()


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-30)


@pytest.mark.parametrize("model,hidden,act,batch,threshold", CHAINS, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-b{c[3]}" for c in CHAINS])
def test_chain_of_single_step_launches(model, hidden, act, batch, threshold):
    """Six launches of one step each on one evaluator, the target net fixed, each checked against the shadow at the kernel's OWN
    pre-launch parameters, lanes, counters and moments (nothing accumulates, so every check is well conditioned): the moment
    updates, Adam's step from the kernel's own post-step moments (4 ulp of |w| plus 1e-6 of |update| per element; t from state[0]),
    the lanes and both counters, loss and held-out norms.  Then ONE launch of six steps from the same start on a fresh evaluator,
    whose pool gives step k the chain's k-th draw: after its n = result[0] steps its parameters, moments, lanes and counters equal
    the chain's after n launches BITWISE."""
    inp = chain_inputs(model, hidden, act, batch, threshold)
    sizes, env64 = inp.sizes, inp.env64
    alg, host = _start(inp, True), _start(inp, False)
    ev = alg._device_evaluator()
    held_out, draws = inp.draws[0], inp.draws[1:]
    target = split_params(inp.params0, sizes)
    snaps, failures, kinds = [_snapshot(alg, ev)], [], dict(done=0, truncated=0)
    for k in range(CHAIN_STEPS):
        before = snaps[-1]
        result = _launch(alg, ev, np.stack([held_out, draws[k]]), 1)
        after = _snapshot(alg, ev)
        snaps.append(after)
        assert result[0] == 1 and after.count == k + 1 and np.array_equal(after.target, before.target)
        st = shadow_step(env64, act, split_params(before.value, sizes), target, before.lanes, draw=draws[k], count=before.counters[0],
                         max_step=inp.max_step, set_state=held_out)
        assert np.abs(st.h).min() >= 1e-3 * st.loss, "a loss row within 1e-3 of zero: the inputs are ill-conditioned, not the kernel"
        g64 = shadow_flat_grad(st)
        # the host path at the same parameters and lanes: its deviations set the bounds
        set_params(host.networks.value, before.value)
        lanes32 = torch.from_numpy(before.lanes)
        g_host = torch.from_numpy(host_gradient(host, lanes32))
        m_host = torch.from_numpy(before.m).lerp(g_host, float(ONE_MINUS_BETA1)).numpy()
        v_host = (torch.from_numpy(before.v) * np.float32(BETA2) + ONE_MINUS_BETA2 * g_host * g_host).numpy()
        m64 = before.m.astype(np.float64) + (1 - BETA1) * (g64 - before.m)
        v64 = BETA2 * before.v.astype(np.float64) + (1 - BETA2) * g64 ** 2
        for what, h, d, want in (("m", m_host, after.m, m64), ("v", v_host, after.v, v64)):
            host_devs, dev_devs = tensor_deviation(h, want, sizes), tensor_deviation(d, want, sizes)
            bounds = _bounds(host_devs)
            print(f"CHAIN {model} act={act} launch {k + 1} {what}: host {_fmt(host_devs)} kernel {_fmt(dev_devs)} bound {_fmt(bounds)}")
            if any(a > b for a, b in zip(dev_devs, bounds)):
                failures.append((k + 1, what, dev_devs, bounds))
        # Adam from the kernel's own post-step moments
        t = after.count
        m, v, w0 = after.m.astype(np.float64), after.v.astype(np.float64), before.value.astype(np.float64)
        update = -CHAIN_LR / (1 - BETA1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - BETA2 ** t) + EPS)
        excess = np.abs((after.value.astype(np.float64) - w0) - update) - (4 * np.spacing(np.abs(before.value)) + 1e-6 * np.abs(update))
        print(f"CHAIN {model} launch {k + 1} adam: largest excess over 4 ulp + 1e-6 |update| {excess.max():.2e} (t = {t:g})")
        if excess.max() > 0:
            failures.append((k + 1, "adam", int(excess.argmax()), float(excess.max())))
        assert after.value[-1:].view(np.uint32) == inp.params0[-1:].view(np.uint32) and after.m[-1] == 0 and after.v[-1] == 0
        # lanes and counters
        sure = st.done_margin >= 1e-4   # (the time-limit test compares whole numbers: exact on both sides)
        assert (~sure).mean() <= 0.02, f"{(~sure).sum()} rows within 1e-4 of a threshold"
        kinds["done"] += int((st.done & sure).sum())
        kinds["truncated"] += int((st.truncated & ~st.done & sure).sum())
        lane_err = (np.abs(after.lanes - st.next_x) / np.maximum(1.0, np.abs(st.next_x)))[sure]
        print(f"CHAIN {model} launch {k + 1} lanes: largest error {lane_err.max():.2e}, resets {int(st.reset.sum())}, left out {(~sure).sum()}")
        if lane_err.max() > 1e-5:
            failures.append((k + 1, "lanes", float(lane_err.max())))
        shown = np.where(st.reset, 0.0, np.where(before.counters[1] < 0, st.count_after, before.counters[1]))
        assert np.array_equal(after.counters[0], st.count_after)
        assert np.array_equal(after.counters[1][sure], shown[sure])
        # scalars: loss, held-out norm before and after (the latter at the kernel's own stepped parameters)
        set_pair = host.networks.action_and_adversary(torch.from_numpy(held_out))
        host_loss = float(host._hamiltonian_mlp(lanes32, host.networks.action_and_adversary(lanes32)).detach().abs().mean())
        host_before = float(host._hamiltonian_mlp(torch.from_numpy(held_out), set_pair).detach().abs().mean())
        set_params(host.networks.value, after.value)
        host_after = float(host._hamiltonian_mlp(torch.from_numpy(held_out), set_pair).detach().abs().mean())
        norm_after = heldout_norm64(env64, split_params(after.value, sizes), target, act, held_out)
        for what, got, h, want in (("loss", result[1], host_loss, st.loss), ("norm before", result[2], host_before, st.norm),
                                   ("norm after", result[3], host_after, norm_after)):
            bound = max(FLOOR, FACTOR * _rel(h, want))
            print(f"CHAIN {model} launch {k + 1} {what}: host {_rel(h, want):.2e} kernel {_rel(got, want):.2e} bound {bound:.2e}")
            if _rel(got, want) > bound:
                failures.append((k + 1, what, _rel(got, want), bound))
    assert not failures, failures
    assert kinds["done"] >= 1 and kinds["truncated"] >= 1, kinds

    # one launch of up to six steps from the same start
    alg2 = _start(inp, True)
    ev2 = alg2._device_evaluator()
    result = _launch(alg2, ev2, np.concatenate([held_out[None], draws]), CHAIN_STEPS)
    n = int(result[0])
    assert 1 <= n <= CHAIN_STEPS and result[0] == n
    one, chain = _snapshot(alg2, ev2), snaps[n]
    print(f"CHAIN {model}: the single launch took {n} steps")
    assert one.count == n
    for name in ("value", "target", "m", "v", "lanes", "counters"):
        a, b = getattr(one, name), getattr(chain, name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {int((a != b).sum())} elements differ, largest {np.abs(a - b).max():.3e}"
