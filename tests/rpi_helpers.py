"""Shared by test_rpi_cpu.py / test_rpi_gpu.py: the RPI fixtures (tests/golden/rpi_*.npz, written by make_golden_rpi.py from the
unmodified reference) and an algorithm built from a fixture's own arguments with its recorded inputs injected."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = ("osc", "air", "susp")
_cache = {}


def fixture(name):
    if name not in _cache:
        with np.load(os.path.join(GOLD, name + ".npz")) as f:
            _cache[name] = {k: f[k] for k in f.files}
    return _cache[name]


def sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def tolerance(fx):
    """max(1e-4, 4 d): d = the fixture's measured distance between the reference's fp32 results and float64."""
    return max(1e-4, 4.0 * json.loads(str(fx["meta/conditions"]))["fp64_distance"])


def alg_kwargs(fx, **override):
    cfg = json.loads(str(fx["meta/cfg"]))
    kw = dict(cfg["kwargs"])
    for k in ("action_high_limit", "action_low_limit"):
        kw[k] = np.array(kw[k], dtype=np.float32)
    kw.update(override)
    return kw, cfg["seed"]


def build(fx, inject=True, **override):
    """The algorithm of a fixture, seeded as the generator seeded the reference; `inject`: recorded start state, time limits,
    weights and reset draws instead of what the seed gives (the two agree - test_default_reset_source_reproduces_the_stream)."""
    from gops_amd.algorithm.rpi import RecordedResetSource
    from gops_amd.create_pkg.create_alg import create_alg
    kw, seed = alg_kwargs(fx, **override)
    np.random.seed(seed)
    torch.manual_seed(seed)
    alg = create_alg(**kw)
    dev = next(alg.networks.parameters()).device
    for net in (alg.networks.value, alg.networks.value_target):
        net.v.weight.data.copy_(torch.from_numpy(fx["w0"]).to(dev))
        net.v.bias.data.copy_(torch.from_numpy(fx["bias"]).to(dev))
    if inject:
        alg.obs = torch.from_numpy(fx["obs0"]).clone()
        alg.env_model.unwrapped.max_step_per_episode = torch.from_numpy(fx["max_step_alg"]).clone()
        alg.reset_source = RecordedResetSource(fx["draws"])
    return alg


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.ndim == 0:
        return abs(got - want) / max(1.0, abs(want))
    return np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
