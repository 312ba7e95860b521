"""Shared by test_rpi_mlp_cpu.py / test_rpi_mlp_gpu.py: the fixtures of RPI with an MLP value function (tests/golden/rpi_mlp_*.npz,
written by make_golden_rpi_mlp.py from the unmodified reference), an algorithm built from a fixture's own arguments with its recorded
inputs injected, the check of one run against a fixture, and a float64 shadow of ONE evaluation step (`shadow_step`) that the
gradient tests compare the host path and the kernel with."""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch

from rpi_helpers import alg_kwargs, fixture, rel, sub, tolerance

STEP_CASES = ("b1", "b64", "b65", "n16_tanh", "n32x16_gelu", "n48_sigmoid", "n16x64_elu")
MULTI_FIXTURES = ("rpi_mlp_susp_b65_m8", "rpi_mlp_air_b64_m8", "rpi_mlp_osc_b64_m20_it3")


def all_cases():
    """(id, case dict) of every fixture case."""
    step = fixture("rpi_mlp_step_osc")
    return [(tag, sub(step, tag + "/")) for tag in STEP_CASES] + [(name, fixture(name)) for name in MULTI_FIXTURES]


def flat_params(net):
    return torch.cat([q.detach().reshape(-1) for q in net.parameters()]).cpu().numpy()


def set_params(net, flat):
    o = 0
    for q in net.parameters():
        q.data.copy_(torch.from_numpy(flat[o:o + q.numel()]).view_as(q).to(q.device))
        o += q.numel()


def build(case, inject=True, **override):
    """The algorithm of a fixture case, seeded as the generator seeded the reference; `inject`: recorded start state, time limits,
    parameters and reset draws instead of what the seed gives (the two agree - test_construction_from_the_seed_alone)."""
    from gops_amd.algorithm.rpi import RecordedResetSource
    from gops_amd.create_pkg.create_alg import create_alg
    kw, seed = alg_kwargs(case, **override)
    np.random.seed(seed)
    torch.manual_seed(seed)
    alg = create_alg(**kw)
    if inject:
        for net in (alg.networks.value, alg.networks.value_target):
            set_params(net, case["params0"])
        alg.obs = torch.from_numpy(case["obs0"]).clone()
        alg.env_model.unwrapped.max_step_per_episode = torch.from_numpy(case["max_step_alg"]).clone()
        alg.reset_source = RecordedResetSource(case["draws"])
    return alg


def check_run(case, use_gpu):
    """Every local_update of the case on one path: step counts and counters exactly, scalars (relative to max(1, |want|)) and vectors
    (relative L2) within max(1e-4, 4 d)."""
    tol = tolerance(case)
    alg = build(case, use_gpu=use_gpu)
    alg.record_trace = True
    k = 0
    for it, n in enumerate(case["num_update_value"]):
        info = alg.local_update(None, it)
        assert info["num_update_value"] == n, (it, info["num_update_value"], n)
        assert rel(alg.norm_hamiltonian_before, case["norm_before"][it]) <= tol
        trace = alg.trace.cpu().numpy()
        assert trace.shape == (n, 2)
        assert rel(trace[:, 0], case["loss"][k:k + n]) <= tol and rel(trace[:, 1], case["norm_after"][k:k + n]) <= tol
        assert np.abs(trace[:, 0] - case["loss"][k:k + n]).max() <= tol * max(1.0, np.abs(case["loss"][k:k + n]).max())
        assert rel(info["Loss/Critic loss-RL iter"], case["loss"][k + n - 1]) <= tol
        assert rel(alg.norm_hamiltonian_after, case["norm_after"][k + n - 1]) <= tol
        k += n
        assert rel(flat_params(alg.networks.value), case["params"][it]) <= tol
        for a, b in zip(alg.networks.value.parameters(), alg.networks.value_target.parameters()):
            assert torch.equal(a, b)
    assert rel(alg.obs.cpu().numpy(), case["final_obs"]) <= tol
    assert np.array_equal(alg.step_count.cpu().numpy(), case["final_count"])
    assert np.array_equal(alg.step_per_episode.cpu().numpy(), case["final_step_per_episode"])
    return alg


# ---- a float64 shadow of one evaluation step ------------------------------------------------------------------------------------
ACTIVATIONS = {"elu": torch.nn.functional.elu, "gelu": torch.nn.functional.gelu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}
TENSOR_NAMES = {4: ("W1", "b1", "WL", "bL"), 6: ("W1", "b1", "W2", "b2", "WL", "bL")}


def layer_sizes(state_dim, hidden):
    return [int(state_dim)] + [int(h) for h in hidden] + [1]


def split_params(flat, sizes):
    """The flattened parameters (`parameters()` order: weight [out, in], bias [out] per Linear layer) as float64 tensors."""
    flat = np.asarray(flat, dtype=np.float64)
    out, o = [], 0
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        out.append(torch.from_numpy(flat[o:o + fan_out * fan_in].copy()).view(fan_out, fan_in))
        o += fan_out * fan_in
        out.append(torch.from_numpy(flat[o:o + fan_out].copy()))
        o += fan_out
    assert o == flat.size
    return out


def split_flat(flat, sizes):
    """A flattened per-parameter array (gradient, moment) as float64 numpy pieces, one per parameter tensor."""
    return [q.numpy().reshape(-1) for q in split_params(flat, sizes)]


def to_double(chain):
    """A copy of a wrapper chain with every fp32 tensor attribute (Q, R, the bounds, the wrappers' limits, a model's matrices)
    widened to float64; the wrappers' `__getattr__` rules out deepcopy."""
    new = object.__new__(type(chain))
    for k, v in vars(chain).items():
        if k == "model":
            v = to_double(v)
        elif torch.is_tensor(v):
            v = v.double() if v.dtype == torch.float32 else v.clone()
        new.__dict__[k] = v
    return new


@contextlib.contextmanager
def float64_default():
    """(The models build g(x), k(x) and their zeros with the default dtype.)"""
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


def mlp64(params, act, x):
    """V(x) [B] of the net `params` (split_params) with hidden activation `act`, linear output."""
    a, fn = x, ACTIVATIONS[act]
    for l in range(0, len(params), 2):
        a = a @ params[l].t() + params[l + 1]
        if l + 2 < len(params):
            a = fn(a)
    return a.squeeze(-1)


def value_gradient64(params, act, x, create_graph=False):
    x = x.detach().clone().requires_grad_(True)
    (dv,) = torch.autograd.grad(mlp64(params, act, x).sum(), x, create_graph=create_graph)
    return dv


def raw_pair64(env64, target, act, x):
    """The target net's raw action / adversary pair [B, 2] (best_act, worst_adv: no wrapper sees them)."""
    dv = value_gradient64(target, act, x)
    return torch.cat((env64.best_act(x, dv), env64.worst_adv(x, dv)), 1)


def hamiltonian64(env64, value, act, x, pair):
    """h [B] = -reward + (dV/dx . delta_state) with the VALUE net's dV/dx and the pair wrapped inside `forward`: the formula of
    RPI._hamiltonian_mlp, differentiable in `value`."""
    _, reward, _, info = env64.forward(x, pair, torch.zeros(x.shape[0], dtype=torch.bool), {})
    return -reward.detach() + (value_gradient64(value, act, x, create_graph=True) * info["delta_state"].detach()).sum(1)


def heldout_norm64(env64, value, target, act, set_state):
    """mean|h| on the held-out states under the TARGET's pair with the VALUE net `value`."""
    with float64_default():
        set_state = torch.as_tensor(np.asarray(set_state), dtype=torch.float64)
        return float(hamiltonian64(env64, value, act, set_state, raw_pair64(env64, target, act, set_state)).detach().abs().mean())


def shadow_step(env64, act, value, target, x, draw=None, count=None, max_step=None, set_state=None):
    """One evaluation step in float64.  `env64`: to_double(alg.env_model); `value`, `target`: split_params lists; `x` [B, S]; `draw`
    [B, S] the step's reset draw; `count`, `max_step` [B] the lanes' time-limit counter before the step and their time limits;
    `set_state` [B, S] the held-out states.  Returns h [B], loss = mean|h|, grads (one array per parameter tensor, None for the output
    bias, which takes no gradient), the raw pair, and - with `draw` - the bare Euler step `euler`, the flags `done` / `truncated` /
    `reset`, `next_x`, `count_after`, and each flag's relative distance from its threshold (`done_margin`: min over the columns of
    ||x_i| - threshold_i| / threshold_i; `time_margin`: |count + 1 - max_step| / max(1, max_step), a comparison of whole numbers);
    with `set_state` the held-out mean|h| under the UNstepped value net (`norm`)."""
    f64 = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)  # noqa: E731
    with float64_default():
        x = f64(x)
        value = [q.detach().clone().requires_grad_(True) for q in value]
        pair = raw_pair64(env64, target, act, x)
        h = hamiltonian64(env64, value, act, x, pair)
        loss = h.abs().mean()
        grads = torch.autograd.grad(loss, value, allow_unused=True)
        out = SimpleNamespace(h=h.detach().numpy(), loss=float(loss.detach()), pair=pair.numpy(),
                              grads=[None if g is None else g.numpy() for g in grads])
        if draw is not None:
            bare = env64.unwrapped
            euler = x + bare._derivative(x, pair[:, 0], pair[:, 1]) * bare.dt
            threshold = f64(bare.state_threshold)
            after = f64(count) + 1
            out.done = (euler.abs() > threshold).any(1).numpy()
            out.done_margin = ((euler.abs() - threshold).abs() / threshold).min(1).values.numpy()
            out.truncated = (after > f64(max_step)).numpy()
            out.time_margin = ((after - f64(max_step)).abs() / f64(max_step).clamp(min=1.0)).numpy()
            out.reset = out.done | out.truncated
            out.euler, out.count_after = euler.numpy(), after.numpy()
            out.next_x = torch.where(torch.from_numpy(out.reset).unsqueeze(-1), f64(draw), euler).numpy()
    if set_state is not None:
        out.norm = heldout_norm64(env64, [q.detach() for q in value], target, act, set_state)
    return out


def case_shape(case):
    """(layer sizes, activation) of a fixture case."""
    kw, _ = alg_kwargs(case)
    return layer_sizes(case["obs0"].shape[1], kw["value_hidden_sizes"]), kw["value_hidden_activation"]


def host_gradient(alg, obs):
    """The eager fp32 host path's gradient of mean|h| at `obs`, flattened in parameters() order (zeros for the output bias)."""
    params = list(alg.networks.value.parameters())
    h = alg._hamiltonian_mlp(obs, alg.networks.action_and_adversary(obs))
    grads = torch.autograd.grad(h.abs().mean(), params, allow_unused=True)
    assert grads[-1] is None and all(g is not None for g in grads[:-1]), "only the output bias takes no gradient"
    return torch.cat([torch.zeros_like(q).reshape(-1) if g is None else g.reshape(-1) for q, g in zip(params, grads)]).numpy()


def tensor_deviation(got, want, sizes):
    """Per parameter tensor: max|got - want| / max|want| (0 where both vanish identically, as for the output bias)."""
    out = []
    for a, b in zip(split_flat(got, sizes), split_flat(want, sizes)):
        top = np.abs(b).max()
        out.append(float(np.abs(a - b).max() / top) if top > 0 else float(np.abs(a).max()))
    return out


def shadow_flat_grad(step):
    return np.concatenate([np.zeros(1) if g is None else g.reshape(-1) for g in step.grads])
