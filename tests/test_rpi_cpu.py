"""RPI on the host: registration, the three zero-sum game models and the wrapper chain against the reference's recorded outputs,
the eager policy-evaluation loop against the reference's per-step record, the reset stream, the refusals and the C ABI surface.
Fixtures: tests/golden/rpi_*.npz (make_golden_rpi.py, the unmodified reference).  Tolerance per model: max(1e-4, 4 d) with d the
fixture's own fp32-to-float64 distance (`rpi_helpers.tolerance`); scalars relative to max(1, |want|), vectors in relative L2."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from rpi_helpers import MODELS, alg_kwargs, build, fixture, rel, sub, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_IDS = {"osc": "pyth_oscillatorconti", "air": "pyth_aircraftconti", "susp": "pyth_suspensionconti"}


def step_fixture(model, batch=64):
    fx = fixture(f"rpi_step_{model}")
    case = sub(fx, f"b{batch}/")
    case["meta/conditions"] = fx["meta/conditions"]
    return fx, case


@pytest.mark.parametrize("model", MODELS)
def test_create_alg_and_env_model_build(model):
    from gops_amd.algorithm.rpi import RPI
    from gops_amd.create_pkg.create_env_model import create_env_model
    _, case = step_fixture(model)
    kw, seed = alg_kwargs(case)
    alg = build(case, inject=False)
    assert isinstance(alg, RPI) and alg.adjustable_parameters == ("max_newton_iteration",)
    n = alg.obsv_dim
    assert alg.networks.value.v.weight.shape == (1, n * (n + 1) // 2)
    env = create_env_model(**kw)
    assert env.unwrapped.state_dim == n and env.unwrapped.hip_kind == 0
    assert tuple(env.reset().shape) == (64, n) and tuple(env.max_step().shape) == (64,) and float(env.initial_step().sum()) == 0
    # a fresh container: zero weights, nn.Linear's bias, the target a copy
    from gops_amd.create_pkg.create_alg import create_approx_contrainer
    nets = create_approx_contrainer(**kw)
    assert float(nets.value.v.weight.detach().abs().sum()) == 0 and nets.value.v.bias is not None
    assert all(torch.equal(a, b) for a, b in zip(nets.value.state_dict().values(), nets.value_target.state_dict().values()))
    assert sorted(alg.state_dict()) == ["value.v.bias", "value.v.weight", "value_target.v.bias", "value_target.v.weight"]
    alg.load_state_dict(alg.state_dict())


@pytest.mark.parametrize("model", MODELS)
def test_model_functions_match_reference(model):
    fx, case = step_fixture(model)
    tol = tolerance(fx)
    alg = build(case)
    fn = sub(fx, "fn/")
    bare, wrapped = alg.env_model.unwrapped, alg.env_model
    x, a, dv = (torch.from_numpy(fn[k]) for k in ("obs", "action", "delta_value"))
    assert rel(bare.best_act(x, dv), fn["best_act"]) <= tol and rel(bare.worst_adv(x, dv), fn["worst_adv"]) <= tol
    assert tuple(bare.best_act(x[:1], dv[:1]).shape) == fn["best_act_b1"].shape
    assert rel(bare.best_act(x[:1], dv[:1]), fn["best_act_b1"]) <= tol and rel(bare.worst_adv(x[:1], dv[:1]), fn["worst_adv_b1"]) <= tol
    done = torch.zeros(64, dtype=torch.bool)
    for tag, mdl, act in (("bare", bare, a), ("wrapped", wrapped, a), ("wrapped_x3", wrapped, 3 * a)):
        nx, r, d, info = mdl.forward(x, act, done, {})
        assert not d.any()
        for key, got in (("next_obs", nx), ("reward", r), ("delta_state", info["delta_state"])):
            assert rel(got, fn[f"{tag}/{key}"]) <= tol, (tag, key)
    # the wrapper quirk: the chain changes `forward` (rows inside [-1, 1] are scaled, rows outside clipped first) ...
    raw, scaled = fn["bare/delta_state"], fn["wrapped/delta_state"]
    inside = np.abs(fn["action"][:, 0]) <= 1
    assert inside.any() and (~inside).any() and rel(raw, scaled) > 1e-2
    low, high = bare.action_lower_bound, bare.action_upper_bound
    got = wrapped.action(a)
    assert torch.allclose(got[inside], (low + (high - low) * ((a + 1) / 2))[inside], rtol=1e-6, atol=1e-7)
    assert torch.equal(got[~inside][:, 0].abs(), high[0].expand(int((~inside).sum())))
    # ... while step / best_act / worst_adv reached through it see raw values
    wrapped.unwrapped.parallel_state, wrapped.unwrapped.step_per_episode = x.clone(), torch.zeros(64)
    nx, r, d, info = wrapped.step(a)
    assert rel(nx, fn["step/next_obs"]) <= tol and rel(r, fn["step/reward"]) <= tol and np.array_equal(d.numpy(), fn["step/done"])
    assert rel(wrapped.best_act(x, dv), fn["best_act"]) <= tol
    # f_x / g_x / k_x: dx/dt = f + g u + k w
    lin = bare.f_x(x) + bare.g_x(x)[:, :, 0] * a[:, :1] + bare.k_x(x)[:, :, 0] * a[:, 1:]
    assert rel(lin, fn["bare/delta_state"]) <= tol
    # the container's eager methods
    nets = alg.networks
    nets.value_target.v.weight.data.copy_(torch.from_numpy(fn["value_target"]))
    assert rel(nets.policy(x.clone()), fn["policy"]) <= tol
    assert rel(nets.action_and_adversary(x.clone()), fn["action_and_adversary"]) <= tol


@pytest.mark.parametrize("scale,clip", [(True, False), (False, True), (False, False)])
def test_wrapper_switches(scale, clip):
    from gops_amd.create_pkg.create_env_model import create_env_model
    _, case = step_fixture("osc")
    kw, _ = alg_kwargs(case, action_scale=scale, clip_action=clip)
    env = create_env_model(**kw)
    low, high = env.unwrapped.action_lower_bound, env.unwrapped.action_upper_bound
    a = torch.tensor([[0.5, 0.1], [-7.0, 0.9], [2.0, -3.0]])
    if scale:
        want = (low + (high - low) * ((a.clip(-1, 1) + 1) / 2)).clip(low, high)
    else:
        want = a.clip(low, high) if clip else a
    assert torch.allclose(env.action(a), want)


def test_wrapper_bounds_per_column_on_the_host():
    """List-valued min_action / max_action, and `use_gpu=True`: the game models are host objects, so the chain's bounds stay on the
    CPU next to them and `forward` takes CPU observations."""
    from gops_amd.create_pkg.create_env_model import create_env_model
    _, case = step_fixture("osc")
    kw, _ = alg_kwargs(case, use_gpu=True, min_action=[-1.0, -2.0], max_action=[1.0, 2.0])
    env = create_env_model(**kw)
    low, high = env.unwrapped.action_lower_bound, env.unwrapped.action_upper_bound
    assert low.device.type == "cpu" and env.min_action.device.type == "cpu"
    a = torch.tensor([[0.5, 1.0], [-7.0, 0.9], [0.2, -3.0]])
    lo, hi = torch.tensor([-1.0, -2.0]), torch.tensor([1.0, 2.0])
    assert torch.allclose(env.action(a), low + (high - low) * ((a.clip(lo, hi) - lo) / (hi - lo)))
    x = torch.tensor([[0.3, -0.2], [1.0, 0.5], [-0.4, 0.9]])
    _, reward, _, info = env.forward(x, a, torch.zeros(3, dtype=torch.bool), {})
    assert reward.shape == (3,) and info["delta_state"].shape == (3, 2)


@pytest.mark.parametrize("model,batch", [(m, b) for m in MODELS for b in (1, 64, 65)])
def test_eager_single_step_matches_reference(model, batch):
    fx, case = step_fixture(model, batch)
    tol = tolerance(fx)
    alg = build(case)
    info = alg.local_update(None, 0)
    assert info["num_update_value"] == 1 and info["iteration"] == 0
    assert rel(info["Loss/Critic loss-RL iter"], case["loss"][0]) <= tol
    assert "Time/Algorithm time [ms]-RL iter" in info
    assert rel(alg.norm_hamiltonian_before, case["norm_before"][0]) <= tol
    assert rel(alg.norm_hamiltonian_after, case["norm_after"][0]) <= tol
    assert rel(alg.networks.value.v.weight.detach().numpy()[0], case["weights"][0]) <= tol
    assert torch.equal(alg.networks.value.v.weight, alg.networks.value_target.v.weight)


@pytest.mark.parametrize("name", ["rpi_osc_b64_m40_it3", "rpi_air_b64_m12_it2", "rpi_susp_b65_m10"])
def test_eager_loop_matches_reference(name):
    fx = fixture(name)
    tol = tolerance(fx)
    alg = build(fx)
    k = 0
    for it, n in enumerate(fx["num_update_value"]):
        info = alg.local_update(None, it)
        assert info["num_update_value"] == n                     # exact: the generator asserted a margin at every decision
        assert rel(alg.norm_hamiltonian_before, fx["norm_before"][it]) <= tol
        for s in range(n):
            assert rel(alg.trace[s, 0], fx["loss"][k + s]) <= tol, (it, s)
            assert rel(alg.trace[s, 1], fx["norm_after"][k + s]) <= tol, (it, s)
            assert rel(alg.weight_trace[s].numpy(), fx["weights"][k + s]) <= tol, (it, s)
        k += n
        assert torch.equal(alg.networks.value.v.weight, alg.networks.value_target.v.weight)
    assert rel(alg.obs.numpy(), fx["final_obs"]) <= tol
    assert np.array_equal(alg.step_count.numpy(), fx["final_count"])
    assert np.array_equal(alg.step_per_episode.numpy(), fx["final_step_per_episode"])
    assert rel(alg.networks.value_target.v.weight.detach().numpy(), fx["final_value_target"]) <= tol


def test_time_limit_counter_is_never_zeroed():
    """The reference's quirk the loop keeps: a lane past its time limit is flagged at every later step."""
    fx = fixture("rpi_osc_b64_m40_it3")
    trunc = fx["truncated"]
    first = trunc.argmax(0)
    lanes = np.where(trunc.any(0))[0]
    assert len(lanes) > 0 and all(trunc[first[b]:, b].all() for b in lanes)
    cond = json.loads(str(fx["meta/conditions"]))
    assert cond["lanes_done"] > 0 and cond["lanes_truncated"] > 0 and cond["stopped_early"] > 0 and cond["ran_to_max"] > 0
    assert cond["min_row_ratio"] >= 1e-3 and cond["min_decision_margin"] >= 1e-3


@pytest.mark.parametrize("model", MODELS)
def test_default_reset_source_reproduces_the_stream(model):
    """Seeded like the generator, construction draws max_step (algorithm), the start state, max_step (container) - then every
    reset follows the recorded stream, through `next` and through `pool` / `consume`."""
    _, case = step_fixture(model, 65)
    alg = build(case, inject=False)
    assert np.array_equal(alg.env_model.unwrapped.max_step_per_episode.numpy(), case["max_step_alg"])
    assert np.array_equal(alg.networks.env_model.unwrapped.max_step_per_episode.numpy(), case["max_step_container"])
    assert np.array_equal(alg.obs.numpy(), case["obs0"])
    src = alg.reset_source
    pool = src.pool(5)                                       # [5, S, B]: one bulk draw, column-major per reset
    assert np.array_equal(pool[:2].transpose(1, 2).numpy(), case["draws"])
    src.consume(1)
    assert np.array_equal(src.next().numpy(), case["draws"][1])
    assert np.array_equal(src.next().numpy(), pool[2].t().numpy())
    # the bulk draw leaves np.random where the same number of single resets leave it
    model = alg.env_model.unwrapped
    np.random.seed(3)
    one_by_one = torch.stack([model.reset() for _ in range(7)])
    after = np.random.get_state()
    np.random.seed(3)
    assert torch.equal(model.reset_many(7).transpose(1, 2), one_by_one)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), after))
    for used in (4, 2):                                      # every pooled draw used (no rewind), and fewer
        np.random.seed(4)
        for _ in range(used):
            model.reset()
        want = model.reset()
        np.random.seed(4)
        src.pool(4)
        src.consume(used)
        assert torch.equal(src.next(), want)


def test_refusals():
    from gops_amd.create_pkg.create_alg import create_alg
    from gops_amd.create_pkg.create_env_model import create_env_model
    _, case = step_fixture("osc")
    kw, _ = alg_kwargs(case)
    bad = [dict(value_func_type="MLP", value_hidden_sizes=[64], value_hidden_activation="relu"), dict(value_func_type="GAUSS"),
           dict(value_degree=3), dict(initial_weight=[1.0, 0.0, 1.0]), dict(is_adversary=False), dict(repeat_num=2),
           dict(obs_scale=[1.0, 2.0]), dict(obs_shift=0.1), dict(reward_scale=0.5), dict(reward_shift=1.0)]
    for extra in bad:
        with pytest.raises(NotImplementedError):
            create_alg(**{**kw, **extra})
    for extra in bad[5:]:
        with pytest.raises(NotImplementedError):
            create_env_model(**{**kw, **extra})
    for env_id in ENV_IDS.values():   # the three models serve RPI only
        for algorithm in ("FHADP", "INFADP", "MAC", "SPIL"):
            with pytest.raises(NotImplementedError, match="RPI"):
                create_alg(**{**kw, "env_id": env_id, "algorithm": algorithm})
    with pytest.raises(ValueError):
        create_alg(**{**kw, "max_step_update_value": (1 << 20) + 1})
    with pytest.raises(ValueError, match="reset pool"):   # the device path's pre-drawn pool: 2^20 x 2 x 1024 floats = 8 GiB
        create_alg(**{**kw, "use_gpu": True, "max_step_update_value": 1 << 20, "reset_batch_size": 1024, "sample_batch_size": 1024})


def test_rpi_symbols_declared_mirrored_exported():
    from gops_amd import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    for name in ("gops_rpi_state_bytes", "gops_rpi_evaluate"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in hb.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(hb.LIB_PATH), name)
    assert int(re.search(r"#define GOPS_HIP_ABI_VERSION (\d+)", header).group(1)) == 15 == hb.lib().gops_hip_version()
    codes = {k: int(v) for k, v in re.findall(r"(GOPS_RPI_[A-Z_]+) = (\d+)", header)}
    for name, value in codes.items():
        assert getattr(hb, name[len("GOPS_"):]) == value, name
    assert int(re.search(r"#define GOPS_RPI_MAX_BATCH (\d+)", header).group(1)) == hb.RPI_MAX_BATCH
    assert int(re.search(r"#define GOPS_RPI_STATE_HEADER (\d+)", header).group(1)) == hb.RPI_STATE_HEADER
    # sizes without a device: header + (S + 2) lanes of floats; nothing beyond 1024 lanes or for an unknown kind
    assert hb.lib().gops_rpi_state_bytes(hb.RPI_ENV_SUSPENSION, 65) == 4 * (32 + 6 * 65)
    assert hb.lib().gops_rpi_state_bytes(hb.RPI_ENV_OSCILLATOR, 1025) == 0 and hb.lib().gops_rpi_state_bytes(7, 64) == 0
