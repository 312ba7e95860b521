"""RPI with an MLP value function on the eager host path against the reference's recorded runs (tests/golden/rpi_mlp_*.npz,
make_golden_rpi_mlp.py), plus construction, refusals and the C ABI's new symbols.  Tolerance per case: max(1e-4, 4 d), d = the
fixture's distance between the reference's fp32 results and its float64 shadow; step counts and counters are compared exactly (the
generator asserted a relative margin >= 1e-3 at every continue/stop decision and on every loss row)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from rpi_helpers import alg_kwargs, fixture, sub
from rpi_mlp_helpers import (TENSOR_NAMES, all_cases, build, case_shape, check_run, flat_params, host_gradient, shadow_flat_grad,
                             shadow_step, split_params, tensor_deviation, to_double)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = all_cases()


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_host_path_reproduces_the_reference(case):
    alg = check_run(case, use_gpu=False)
    assert alg.weight_trace.shape == (case["num_update_value"][-1], case["params0"].size)
    assert np.array_equal(alg.weight_trace[-1].numpy(), flat_params(alg.networks.value))
    assert alg.min_row_ratio >= 1e-3


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_construction_from_the_seed_alone(case):
    """The torch and numpy generators stand where the reference's stand: initial parameters (Xavier-uniform weights in module order
    after the module's own initialisation, zero biases), start state and both time limits."""
    alg = build(case, inject=False)
    assert np.array_equal(flat_params(alg.networks.value), case["params_seed"])
    assert np.array_equal(flat_params(alg.networks.value_target), case["params_seed"])
    assert np.array_equal(alg.obs.numpy(), case["obs0"])
    assert np.array_equal(alg.env_model.max_step_per_episode.numpy(), case["max_step_alg"])
    assert np.array_equal(alg.networks.env_model.max_step_per_episode.numpy(), case["max_step_container"])


def _report(what, sizes, devs, bound):
    names = TENSOR_NAMES[2 * (len(sizes) - 1)]
    print(f"{what}: " + ", ".join(f"{n} {d:.2e}" for n, d in zip(names, devs)) + f"  (bound {bound:.1e})")


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_host_first_step_gradient_equals_grad0(case):
    """`grad0` is the unmodified reference's gradient of its first step.  The eager fp32 host path's (autograd of mean|h| over
    `_hamiltonian_mlp`) equals it per parameter tensor within 1e-6 of the tensor's largest element (measured: 0 in nine cases, 4e-8
    in the tenth); the output bias takes none."""
    alg = build(case, use_gpu=False)
    sizes, _ = case_shape(case)
    devs = tensor_deviation(host_gradient(alg, torch.from_numpy(case["obs0"]).clone()), case["grad0"], sizes)
    _report("host path against grad0", sizes, devs, 1e-6)
    assert max(devs) <= 1e-6
    assert case["grad0"][-1] == 0


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_shadow_gradient_agrees_with_grad0(case):
    """The float64 shadow of one step (rpi_mlp_helpers.shadow_step, the yardstick of test_rpi_mlp_grad_gpu.py) at the fixture's
    `obs0` and `params0` against `grad0`: per tensor within max(1e-5, 4 d) of the tensor's largest |grad0|, d = the case's
    fp32-to-float64 distance."""
    alg = build(case, use_gpu=False)
    sizes, act = case_shape(case)
    params = split_params(case["params0"], sizes)
    step = shadow_step(to_double(alg.env_model), act, params, params, case["obs0"])
    assert step.grads[-1] is None and all(g is not None for g in step.grads[:-1])
    bound = max(1e-5, 4.0 * json.loads(str(case["meta/conditions"]))["fp64_distance"])
    devs = tensor_deviation(shadow_flat_grad(step), case["grad0"], sizes)
    _report("shadow against grad0", sizes, devs, bound)
    assert max(devs) <= bound
    assert abs(step.loss - case["loss"][0]) <= bound * max(1.0, abs(case["loss"][0]))


def test_policy_takes_the_target_nets_gradient():
    case = sub(fixture("rpi_mlp_step_osc"), "b64/")
    alg = build(case)
    obs = torch.from_numpy(case["obs0"]).clone()
    x = obs.clone().requires_grad_(True)
    (dv,) = torch.autograd.grad(alg.networks.value_target(x).sum(), x)
    model = alg.networks.env_model
    pair = alg.networks.action_and_adversary(obs)
    assert torch.equal(pair, torch.cat((model.best_act(obs, dv), model.worst_adv(obs, dv)), 1))
    assert torch.equal(alg.networks.policy(obs), pair[:, :1])
    assert not obs.requires_grad


def test_refusals():
    from gops_amd.create_pkg.create_alg import create_alg
    kw, _ = alg_kwargs(sub(fixture("rpi_mlp_step_osc"), "b64/"))
    bad = [dict(value_func_type="GAUSS"), dict(value_func_type="POLY", value_degree=3), dict(initial_weight=[1.0, 0.0, 1.0]),
           dict(is_adversary=False), dict(value_hidden_activation="relu"), dict(value_hidden_activation="selu"),
           dict(value_hidden_sizes=[16, 16, 16]), dict(value_hidden_sizes=[]), dict(value_hidden_sizes=[80]),
           dict(value_hidden_sizes=[64, 24]), dict(value_hidden_sizes=[8]), dict(value_output_activation="tanh")]
    for extra in bad:
        with pytest.raises(NotImplementedError):
            create_alg(**{**kw, **extra})
    create_alg(**{**kw, "value_degree": 7})   # ignored for an MLP


def test_abi_symbols():
    from gops_amd import hip_backend as hb
    header = open(os.path.join(ROOT, "include", "gops_hip.h")).read()
    assert re.search(r"#define GOPS_HIP_ABI_VERSION 15\b", header)
    lib = os.path.join(ROOT, "gops_amd", "libgops_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ("gops_rpi_mlp_state_bytes", "gops_rpi_mlp_evaluate"):
        assert re.search(r"\b" + name + r"\(", header)
        assert name in hb.EXPORTED_SYMBOLS
        assert re.search(r" T " + name + r"\b", exported)
    # both are declared to ctypes with every argument of the header's prototype
    loaded = hb.lib()
    assert len(loaded.gops_rpi_mlp_state_bytes.argtypes) == 3 and loaded.gops_rpi_mlp_state_bytes.restype is hb.C.c_size_t
    assert len(loaded.gops_rpi_mlp_evaluate.argtypes) == 17
