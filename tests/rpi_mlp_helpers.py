"""Shared by test_rpi_mlp_cpu.py / test_rpi_mlp_gpu.py: the fixtures of RPI with an MLP value function (tests/golden/rpi_mlp_*.npz,
written by make_golden_rpi_mlp.py from the unmodified reference), an algorithm built from a fixture's own arguments with its recorded
inputs injected, and the check of one run against a fixture."""
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
