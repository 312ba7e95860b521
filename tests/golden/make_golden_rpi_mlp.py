"""Generate the fixtures of RPI with an MLP value function (`rpi_mlp_*.npz`) by running the UNMODIFIED reference on the CPU.

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_rpi_mlp.py
As in make_golden_rpi.py (whose helpers this module imports) the reference is observed, never changed: its `reset`, `step`,
Hamiltonian and optimizer step are wrapped by recorders that call the original.

Per case the generator also runs a float64 SHADOW of the whole case - the same loop written out here, from the same start state, the
same initial parameters and the same reset draws - and stores `fp64_distance = d`: the largest relative difference (relative L2 for
vectors) between a recorded fp32 quantity and the shadow's value, over the losses, the held-out norms, the first step's gradient and
the parameters at the end of each Newton iteration.  A seed whose shadow takes other step counts is rejected.  Asserted, and written
into `meta/conditions`:
  * every loss row satisfies |h_i| >= 1e-3 x mean|h|;
  * every continue/stop decision is at least 1e-3 relative from its threshold;
  * 4 d <= 1e-3 (Adam's first steps move each weight by about lr whatever the size of its gradient element, so an element near zero
    is noise: the shadow shows whether a case is free of it).
The multi-step oscillator case needs lanes ending by threshold and by time limit, one iteration stopped by the 0.88 rule and one
that runs to the bound; `golden_multi` looks for ONE seed with all four.
"""
import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_rpi as base  # noqa: E402  (installs the reference import path)
from make_golden_rpi import RPI, alg_kwargs, rel, save, to_double  # noqa: E402

torch.set_num_threads(1)


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).numpy().copy()


def hamiltonian_rows(net, env, obs, inp):
    x = obs.detach().clone().requires_grad_(True)
    (dv,) = torch.autograd.grad(net(x).sum(), x, create_graph=True)
    _, rew, _, info = env.forward(x.detach(), inp.detach(), torch.zeros(x.shape[0]).bool(), {})
    return -rew.detach() + (dv * info["delta_state"].detach()).sum(1)


def pair_of(net, cont_env, obs):
    x = obs.detach().clone().requires_grad_(True)
    (dv,) = torch.autograd.grad(net(x).sum(), x)
    return torch.cat((cont_env.best_act(obs.detach(), dv), cont_env.worst_adv(obs.detach(), dv)), 1)


class Shadow:
    """The reference's loop in float64 (rpi.py:174-197, sample() :289-327), fed with recorded reset draws."""

    def __init__(self, alg):
        self.env = to_double(alg.env_model)
        self.cont_env = to_double(alg.networks.env_model)
        self.value = deepcopy(alg.networks.value).double()
        self.target = deepcopy(self.value)
        self.obs = alg.obs.double().clone()
        self.opt = torch.optim.Adam(self.value.parameters(), lr=alg.learning_rate, betas=(0.9, 0.99), weight_decay=0)
        self.max_steps = alg.max_step_update_value

    def run(self, draws, iterations):
        """(The models fill buffers made by torch.zeros: the default dtype is float64 for the length of the run.)"""
        torch.set_default_dtype(torch.float64)
        try:
            return self._run(draws, iterations)
        finally:
            torch.set_default_dtype(torch.float32)

    def _run(self, draws, iterations):
        draws = iter(torch.from_numpy(np.asarray(d)).double() for d in draws)
        env, bare = self.env, self.env.unwrapped
        out = dict(num=[], loss=[], before=[], after=[], params=[], grad0=None)
        for _ in range(iterations):
            set_state = next(draws)
            set_pair = pair_of(self.target, self.cont_env, set_state)
            before = float(hamiltonian_rows(self.value, env, set_state, set_pair).abs().mean())
            out["before"].append(before)
            n = 0
            for _ in range(self.max_steps):
                n += 1
                obs = self.obs
                action = pair_of(self.target, self.cont_env, obs)
                next_obs, _, done, info = env.step(action)
                reset = done | info["TimeLimit.truncated"]
                self.obs = torch.where(reset.unsqueeze(-1), next(draws), next_obs)
                bare.parallel_state = self.obs.clone()
                env.step_per_episode = torch.where(reset, env.initial_step(), env.step_per_episode)
                self.opt.zero_grad()
                loss = hamiltonian_rows(self.value, env, obs, action).abs().mean()
                loss.backward()
                if out["grad0"] is None:
                    out["grad0"] = flat([torch.zeros_like(q) if q.grad is None else q.grad for q in self.value.parameters()])
                self.opt.step()
                after = float(hamiltonian_rows(self.value, env, set_state, set_pair).abs().mean())
                out["loss"].append(float(loss))
                out["after"].append(after)
                if not (abs(after) > 0.88 * abs(before) and n < self.max_steps):
                    break
            self.target = deepcopy(self.value)
            out["num"].append(n)
            out["params"].append(flat(self.value.parameters()))
        return out


class Recorder:
    """Wraps one reference RPI instance: reset draws, the bare step's inputs and flags, per-evaluation Hamiltonian rows, gradients."""

    def __init__(self, alg):
        self.alg = alg
        self.draws, self.evals, self.grads, self.raw_inputs, self.done, self.trunc = [], [], [], [], [], []
        bare = alg.env_model.unwrapped
        reset0, step0 = bare.reset, bare.step

        def reset():
            s = reset0()
            self.draws.append(s.numpy().copy())
            return s

        def step(action):
            out = step0(action)
            self.raw_inputs.append(action.detach().numpy().copy())
            self.done.append(out[2].numpy().copy())
            self.trunc.append(out[3]["TimeLimit.truncated"].numpy().copy())
            return out

        bare.reset, bare.step = reset, step
        ham0 = alg._RPI__calculate_hamiltonian

        def hamiltonian(obs, inp):
            holder = {}
            vlf0 = RPI._RPI__value_loss_function

            def vlf(delta_value, utility, delta_state):
                holder["rows"] = (utility + torch.diag(torch.mm(delta_value, delta_state.t()), 0)).detach().numpy().copy()
                return vlf0(delta_value, utility, delta_state)

            RPI._RPI__value_loss_function = staticmethod(vlf)
            try:
                out = ham0(obs, inp)
            finally:
                RPI._RPI__value_loss_function = staticmethod(vlf0)
            self.evals.append(dict(value=float(out.detach()), rows=holder["rows"]))
            return out

        alg._RPI__calculate_hamiltonian = hamiltonian
        opt_step0 = alg.approximate_optimizer.step
        params = list(alg.networks.value.parameters())

        def opt_step(*a, **k):
            assert params[-1].grad is None, "the output bias takes no gradient"
            assert all(q.grad is not None for q in params[:-1])
            self.grads.append(flat([torch.zeros_like(q) if q.grad is None else q.grad for q in params]))
            return opt_step0(*a, **k)

        alg.approximate_optimizer.step = opt_step


def run_case(model, batch, max_step_update_value, iterations, seed, hidden, act, out_scale=1.0, **extra):
    """-> (arrays, conditions) of `iterations` reference local_update calls and their float64 shadow; None when the shadow takes
    other step counts.  `out_scale` multiplies the output layer's weights of value and target before the run: dV/dx of a freshly
    initialised net is a few tenths, so the raw action never leaves [-1, 1] and ScaleAction's clip would stay idle (`params_seed`
    keeps what the seed alone gives, `params0` what the run starts from)."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    kw = alg_kwargs(model, batch, max_step_update_value, seed, value_func_type="MLP", value_hidden_sizes=list(hidden),
                    value_hidden_activation=act, value_output_activation="linear", **extra)
    alg = RPI(**kw)
    assert all(torch.equal(a, b) for a, b in zip(alg.networks.value.parameters(), alg.networks.value_target.parameters()))
    params_seed = flat(alg.networks.value.parameters())
    for net in (alg.networks.value, alg.networks.value_target):
        net.v[-2].weight.data.mul_(out_scale)
    shadow = Shadow(alg)
    out = {"obs0": alg.obs.numpy().copy(), "params_seed": params_seed, "params0": flat(alg.networks.value.parameters()),
           "max_step_alg": alg.env_model.max_step_per_episode.numpy().copy(),
           "max_step_container": alg.networks.env_model.max_step_per_episode.numpy().copy()}
    rec = Recorder(alg)
    num, losses, norms_b, norms_a, margins, ratios, params = [], [], [], [], [], [], []
    for it in range(iterations):
        e0, s0 = len(rec.evals), len(rec.grads)
        info = alg.local_update(None, it)
        n = info["num_update_value"]
        num.append(n)
        ev = rec.evals[e0:]
        assert len(ev) == 1 + 2 * n and len(rec.grads) - s0 == n
        norms_b.append(ev[0]["value"])
        for k in range(n):
            loss, after = ev[1 + 2 * k], ev[2 + 2 * k]
            losses.append(loss["value"])
            norms_a.append(after["value"])
            ratios.append(float(np.abs(loss["rows"]).min() / np.abs(loss["rows"]).mean()))
            margins.append(abs(abs(after["value"]) - 0.88 * abs(ev[0]["value"])) / (0.88 * abs(ev[0]["value"])))
        assert abs(info["Loss/Critic loss-RL iter"] - losses[-1]) == 0
        assert all(torch.equal(a, b) for a, b in zip(alg.networks.value.parameters(), alg.networks.value_target.parameters()))
        params.append(flat(alg.networks.value.parameters()))
    sh = shadow.run(rec.draws, iterations)
    if sh["num"] != num:
        return None
    d64 = [rel(a, b) for a, b in zip(losses, sh["loss"])] + [rel(a, b) for a, b in zip(norms_a, sh["after"])]
    d64 += [rel(a, b) for a, b in zip(norms_b, sh["before"])] + [rel(a, b) for a, b in zip(params, sh["params"])]
    d64.append(rel(rec.grads[0], sh["grad0"]))
    raw = np.concatenate(rec.raw_inputs, 0)
    cond = dict(min_row_ratio=min(ratios), min_decision_margin=min(margins), fp64_distance=float(max(d64)),
                lanes_done=int(np.sum(rec.done)), lanes_truncated=int(np.sum(rec.trunc)),
                raw_action_outside=int(np.sum(np.abs(raw[:, 0]) > 1)), raw_action_inside=int(np.sum(np.abs(raw[:, 0]) <= 1)),
                stopped_early=int(sum(n < max_step_update_value for n in num)),
                ran_to_max=int(sum(n == max_step_update_value for n in num)))
    out.update({"draws": np.stack(rec.draws), "num_update_value": np.array(num), "loss": np.array(losses),
                "norm_before": np.array(norms_b), "norm_after": np.array(norms_a), "grad0": rec.grads[0],
                "params": np.stack(params), "final_obs": alg.obs.numpy().copy(),
                "final_count": alg.env_model.unwrapped.step_per_episode.numpy().copy(),
                "final_step_per_episode": alg.env_model.step_per_episode.numpy().copy()})
    kw_json = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out["meta/cfg"] = json.dumps(dict(model=model, seed=seed, kwargs=kw_json))
    out["meta/conditions"] = json.dumps(cond)
    return out, cond


def common(c):
    return c["min_row_ratio"] >= 1e-3 and c["min_decision_margin"] >= 1e-3 and 4 * c["fp64_distance"] <= 1e-3


def find_seed(accept, *args, seeds=range(1, 300), **kw):
    for seed in seeds:
        got = run_case(*args, seed=seed, **kw)
        if got is not None and common(got[1]) and accept(got[1]):
            return got
    raise AssertionError(f"no seed in {seeds} satisfies the conditions for {args} {kw}")


def golden_steps():
    """One evaluation step on the oscillator: [64, 64] elu at B = 1, 64, 65 (one lane, a full tile, a second tile with one live
    row), then B = 64 for nets that cover every activation, one and two hidden layers, unequal widths, the smallest and the largest."""
    arrays, conds = {}, {}
    cases = [(f"b{b}", b, [64, 64], "elu") for b in (1, 64, 65)]
    cases += [("n16_tanh", 64, [16], "tanh"), ("n32x16_gelu", 64, [32, 16], "gelu"), ("n48_sigmoid", 64, [48], "sigmoid"),
              ("n16x64_elu", 64, [16, 64], "elu")]
    for tag, batch, hidden, act in cases:
        # (ScaleAction's clip active on some rows and idle on others wherever there is more than one row)
        out, cond = find_seed(lambda c: batch == 1 or (c["raw_action_outside"] > 0 and c["raw_action_inside"] > 0),
                              "osc", batch, 1, 1, hidden=hidden, act=act, out_scale=1.0 if batch == 1 else STEP_OUT_SCALE)
        arrays.update({f"{tag}/{k}": v for k, v in out.items()})
        conds[tag] = cond
    save("rpi_mlp_step_osc", arrays, conds)


def golden_multi():
    """Suspension [32, 32] elu at B = 65 and aircraft [16] tanh at B = 64, at most 8 steps; oscillator [64, 64] elu at B = 64, at most
    20 steps, three Newton iterations with short time limits and tight thresholds."""
    out, cond = find_seed(lambda c: True, "susp", 65, 8, 1, hidden=[32, 32], act="elu", lower_step=3, upper_step=200)
    save("rpi_mlp_susp_b65_m8", out, cond)
    out, cond = find_seed(lambda c: c["lanes_truncated"] > 0, "air", 64, 8, 1, hidden=[16], act="tanh", lower_step=3, upper_step=200)
    save("rpi_mlp_air_b64_m8", out, cond)

    def ok(c):
        return c["lanes_done"] > 0 and c["lanes_truncated"] > 0 and c["stopped_early"] > 0 and c["ran_to_max"] > 0
    out, cond = find_seed(ok, "osc", 64, 20, 3, hidden=[64, 64], act="elu", lower_step=3, upper_step=1000,
                          state_threshold=[1.45, 1.45], learning_rate=MULTI_LR)
    save("rpi_mlp_osc_b64_m20_it3", out, cond)


MULTI_LR = 3e-3
STEP_OUT_SCALE = 8.0

if __name__ == "__main__":
    only = set(sys.argv[1:])
    for fn in (golden_steps, golden_multi):
        if not only or fn.__name__ in only:
            fn()
