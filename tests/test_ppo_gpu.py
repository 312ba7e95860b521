"""PPO on the MI355X: the three kernels of csrc/ppo.hip against float64 restatements, the fixtures of tests/golden/make_golden_ppo.py
on the device, graph replay against eager launches, the on-policy device sampler and a short OnSerialTrainer run."""
import numpy as np
import pytest
import torch

from ac_helpers import EPS32, TOL, check_rows_beyond_the_batch, close
from conftest import load_golden, rel_l2
from ppo_helpers import (HYPER, KERNEL_SHAPES, LOCAL_UPDATE, ONE_STEP, TERMS, load_ppo, minibatch_of, restate_gae, restate_loss_with_seeds,
                         synthetic_minibatch)

pytestmark = pytest.mark.gpu


def _bound_check(label, got, comp, want):
    """ac_helpers.check_backup's rule for one tensor: the same formulas composed from fp32 torch ops on the device are measured
    first; the kernel may use twice their max error, and not less than 4 fp32 ulp of the tensor's largest magnitude."""
    want = want.reshape(got.shape)
    err_c = (comp.double().cpu().reshape(got.shape) - want).abs().max().item()
    err_k = (got.double().cpu() - want).abs().max().item()
    bound = max(2 * err_c, 4 * EPS32 * want.abs().max().item())
    print(f"{label}: kernel {err_k:.3e} composed {err_c:.3e} bound {bound:.3e}")
    assert err_k <= bound, (label, err_k, err_c, bound)


@pytest.mark.parametrize("M,A", KERNEL_SHAPES)
@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("value_norm", [False, True])
def test_ppo_loss_kernel_against_float64(M, A, value_clip, value_norm):
    from gops_amd import hip_backend as hb
    if M == 1 and value_norm:
        loss = hb.PpoLoss(A, HYPER["min_ls"], HYPER["max_ls"], "cuda", value_clip, True)
        t = {k: v.cuda() for k, v in synthetic_minibatch(1, A).items()}
        with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):   # the unbiased std of one return does not exist
            loss.run(t["head"], t["v"], t["act"], t["logp"], t["adv"], t["ret"], t["val"], t["logits"])
        return
    host = synthetic_minibatch(M, A)
    hyper = dict(HYPER, loss_value_clip=value_clip, loss_value_norm=value_norm)
    stats64, sh64, sv64, _ = restate_loss_with_seeds(host, hyper)
    stats32, sh32, sv32, _ = restate_loss_with_seeds(host, hyper, dtype=torch.float32, device="cuda")
    t = {k: v.cuda() for k, v in host.items()}
    loss = hb.PpoLoss(A, HYPER["min_ls"], HYPER["max_ls"], "cuda", value_clip, value_norm)
    loss.set_hyper(HYPER["clip"], HYPER["value_clip"], HYPER["c_kl"], HYPER["c_v"], HYPER["c_ent"])

    def run(out=None):
        out = out or {}
        sh, sv, st = loss.run(t["head"], t["v"], t["act"], t["logp"], t["adv"], t["ret"], t["val"], t["logits"],
                              seed_head=None if "seed_head" not in out else out["seed_head"].view(M, 2 * A), seed_v=out.get("seed_v"))
        return dict(seed_head=sh.clone(), seed_v=sv.clone(), stats=st.clone())

    got = check_rows_beyond_the_batch(run, dict(seed_head=2 * M * A, seed_v=M))
    again = run()
    torch.cuda.synchronize()
    label = f"ppo_loss M={M} A={A} clip={value_clip} norm={value_norm}"
    _bound_check(label + " seed_head", got["seed_head"], sh32, sh64)
    _bound_check(label + " seed_v", got["seed_v"], sv32, sv64)
    for i, name in enumerate(TERMS):
        _bound_check(f"{label} {name}", got["stats"][i], stats32[i], stats64[i])
    for k in got:
        assert torch.equal(got[k], again[k]), k   # a second launch is bit-identical
    raw = t["head"][:, A:]
    outside = (raw < HYPER["min_ls"]) | (raw > HYPER["max_ls"])
    assert (got["seed_head"][:, A:][outside] == 0.0).all() and (got["seed_head"][:, A:][~outside] != 0.0).all()
    assert M < 70 or (outside.any() and (~outside).any())
    assert int(loss.buf.view(torch.int32)[10 + 2 * 5 * 64].item()) == 0   # the ticket, behind results, norm and partial sums


@pytest.mark.parametrize("n", [2, 70, 8192, 8193])
def test_adv_normalize_kernel(n):
    from gops_amd import hip_backend as hb
    g = torch.Generator().manual_seed(n)
    an = hb.AdvNormalize("cuda")
    for label, x in (("spread", 3 * torch.randn(n, generator=g) + 0.5), ("mean 1e3, spread 1", 1e3 + torch.randn(n, generator=g))):
        xd = x.double()
        want = (xd - xd.mean()) / (xd.std() + 1e-8)
        comp = (x.cuda() - x.cuda().mean()) / (x.cuda().std() + 1e-8)
        pad = torch.full((n + 64,), -777.0, device="cuda")
        got = an.run(x.cuda(), 1e-8, out=pad[:n])
        again = an.run(x.cuda(), 1e-8)
        torch.cuda.synchronize()
        _bound_check(f"adv_normalize n={n} {label}", got, comp, want)
        assert (pad[n:] == -777.0).all() and torch.equal(got, again)
        assert abs(float(an.buf[1]) - float(torch.std(xd))) <= 4 * EPS32 * float(torch.std(xd))   # unbiased, no cancellation
        assert int(an.buf.view(torch.int32)[6 + 2 * 2 * 64].item()) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        an.run(torch.zeros(1, device="cuda"))


def _gae_case(N, T, seed):
    rng = np.random.RandomState(seed)
    rew, val, val_next = (rng.randn(T, N).astype(np.float32) for _ in range(3))
    done = (rng.rand(T, N) < 0.2).astype(np.float32)
    end = np.maximum(done, (rng.rand(T, N) < 0.2).astype(np.float32))
    end[T - 1] = 1
    return dict(rew=rew, val=val, val_next=val_next, done=done, end=end, gamma=0.99, gae_lambda=0.95)


@pytest.mark.parametrize("case", ["fixture", "N130_T3"])
def test_gae_kernel(case):
    """Equality with the float64 recurrence rounded to fp32 (the store's rounding is the only one); the reference's recorded values
    within 2 fp32 ulp.  N = 130: more than two waves and rows beyond a multiple of 64."""
    from gops_amd import hip_backend as hb
    from ppo_helpers import ulps32
    g = load_golden("gae_segments") if case == "fixture" else _gae_case(130, 3, 5)
    T, N = g["rew"].shape
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("rew", "val", "val_next", "done", "end")}
    pad = torch.full((2, T * N + 64), -777.0, device="cuda")
    ret, adv = hb.gae(dev["rew"], dev["val"], dev["val_next"], dev["done"], dev["end"], float(g["gamma"]), float(g["gae_lambda"]),
                      ret=pad[0, :T * N].view(T, N), adv=pad[1, :T * N].view(T, N))
    torch.cuda.synchronize()
    want_ret, want_adv = restate_gae(g["rew"], g["val"], g["val_next"], g["done"], g["end"], float(g["gamma"]), float(g["gae_lambda"]))
    assert np.array_equal(ret.cpu().numpy(), want_ret.astype(np.float32)) and np.array_equal(adv.cpu().numpy(), want_adv.astype(np.float32))
    assert (pad[:, T * N:] == -777.0).all()
    if case == "fixture":
        assert ulps32(ret.cpu().numpy(), g["ret"]) <= 2 and ulps32(adv.cpu().numpy(), g["adv"]) <= 2


@pytest.mark.parametrize("name", ONE_STEP)
def test_one_minibatch_step_against_the_reference(name):
    """The fixture's minibatch through both forwards, gops_ppo_loss and both backwards: every loss term and tb value with `close`,
    every gradient at rel-L2 < 1e-4; then the Adam step: the state dict after it."""
    alg, g, meta = load_ppo(name, use_gpu=True)
    mb = {k: v.cuda() for k, v in minibatch_of(g).items()}
    out = alg._minibatch_step(mb, 0).cpu()
    for i, k in enumerate(TERMS):
        assert close(out[i], g["loss/" + k]), (k, float(out[i]), float(g["loss/" + k]))
    tb = {"Loss/Actor loss-RL iter": out[1], "Loss/Critic loss-RL iter": out[2], "PPO/KL_divergence-RL iter": out[4]}
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), k
    for n in ("policy", "value"):
        for i, p in enumerate(getattr(alg.networks, n).parameters()):
            assert rel_l2(p.grad.cpu(), g[f"{n}_grad/{i}"]) < TOL, (n, i, rel_l2(p.grad.cpu(), g[f"{n}_grad/{i}"]))
    for k, v in alg.networks.state_dict().items():
        assert rel_l2(v.cpu(), g["sd_after/" + k]) < TOL, k


def test_local_update_against_the_reference():
    """One full local_update - 2 repeats x 2 minibatches of 35, both linear schedules, the recorded permutations: the state dict
    after it at rel-L2 < 1e-4 per entry, the last minibatch's tb values and gradients, the learning rate and clip_now."""
    alg, g, meta = load_ppo(LOCAL_UPDATE, use_gpu=True)
    data = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("in/")}
    tb = alg.local_update(data, meta["iteration"])
    for k, v in alg.networks.state_dict().items():
        assert rel_l2(v.cpu(), g["sd_after/" + k]) < TOL, (k, rel_l2(v.cpu(), g["sd_after/" + k]))
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), (k, float(tb[k[3:]]), float(g[k]))
    for n in ("policy", "value"):
        for i, p in enumerate(getattr(alg.networks, n).parameters()):
            assert rel_l2(p.grad.cpu(), g[f"{n}_grad/{i}"]) < TOL, (n, i)
    assert alg.approximate_optimizer.param_groups[0]["lr"] == float(g["lr_after"]) and alg.clip_now == float(g["clip_now_after"])


def test_graph_replay_matches_eager_launches(monkeypatch):
    """GOPS_HIP_GRAPH=1 against 0 over 3 local_updates of 2 repeats x 2 minibatches of 35 rows with schedule_clip = "linear" (the clip
    range changes under the captured graph): parameters and tb values bit-equal; one capture, every later step a replay."""
    from gops_amd.utils import hip_graph
    captures = []
    init = hip_graph.GraphedStep.__init__

    def counted(self, *a, **k):
        captures.append(1)
        init(self, *a, **k)

    monkeypatch.setattr(hip_graph.GraphedStep, "__init__", counted)

    def run(mode):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        del captures[:]
        alg, g, meta = load_ppo(LOCAL_UPDATE, use_gpu=True)
        logs = []
        for it in range(3):
            data = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("in/")}
            data["ret"] = data["ret"] + 0.1 * it
            logs.append({k: float(v) for k, v in alg.local_update(data, it).items() if not k.startswith("Time/")})
        return alg, logs, len(captures)

    eager, log_e, cap_e = run("0")
    graph, log_g, cap_g = run("1")
    assert cap_e == 0 and eager.graph_replays == 0 and eager._graph.graph is None
    assert cap_g == 1 and graph._graph.graph is not None and graph.graph_replays >= 6
    assert log_e == log_g
    for (ne, pe), (ng, pg) in zip(eager.networks.named_parameters(), graph.networks.named_parameters()):
        assert ne == ng and torch.equal(pe, pg), ne
    assert eager.clip_now == graph.clip_now != eager.clip


def _sampler_setup(cls, **kw):
    from gops_amd.create_pkg.create_env_model import create_env_model
    from ppo_helpers import ah
    torch.manual_seed(0)
    args = ah._common_kwargs("PPO", "gym_cartpoleconti", 4, 1, ([-1.0], [1.0]), [64, 64], "relu", 0, True)
    args.update(trainer="on_serial_trainer", max_iteration=8, num_repeat=2, num_mini_batch=2, mini_batch_size=64, sample_batch_size=128,
                policy_min_log_std=-3.0, policy_max_log_std=-0.5)
    from gops_amd.create_pkg.create_alg import create_alg
    alg = create_alg(**args)
    alg.networks.to("cuda")
    model = create_env_model(**args)
    smp = cls(dict(env_id="gym_cartpoleconti"), model, n_envs=8, steps_per_sample=16, max_episode_steps=5, seed=3, **kw)
    smp.networks = alg.networks
    return args, alg, smp


def test_on_policy_device_sampler():
    """ret / adv equal the float64 recurrence of the returned columns rounded to fp32 - with the values of one forward over all
    observations -; obs, act, rew, done, logp bit-equal to a plain DeviceEnvSampler with the same seed and networks."""
    from gops_amd import hip_backend as hb
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    _, alg, smp = _sampler_setup(OnPolicyDeviceSampler, gamma=0.97, gae_lambda=0.9)
    _, _, plain = _sampler_setup(DeviceEnvSampler)
    plain.networks = alg.networks
    got, _ = smp.sample()
    ref, _ = plain.sample()
    assert set(got) >= {"obs", "act", "rew", "done", "logp", "time_limited", "ret", "adv"} and "obs2" not in got
    for k in ("obs", "act", "rew", "done", "logp"):
        assert torch.equal(got[k], ref[k]), k
    T, N = 16, 8
    done, tlim = got["done"].view(T, N), got["time_limited"].view(T, N)
    assert (done != 0).any() or tlim.any()
    assert tlim.any() and not (tlim & (done != 0)).any()
    end = ((done != 0) | tlim).float()
    end[T - 1] = 1
    val = hb.MlpNet(alg.networks.value.hip_mlp(), T * N).forward(ref["obs"].contiguous()).view(T, N)
    val_next = hb.MlpNet(alg.networks.value.hip_mlp(), T * N).forward(ref["obs2"].contiguous()).view(T, N)
    want_ret, want_adv = restate_gae(got["rew"].view(T, N).cpu(), val.cpu(), val_next.cpu(), done.cpu(), end.cpu(), 0.97, 0.9)
    assert np.array_equal(got["ret"].view(T, N).cpu().numpy(), want_ret.astype(np.float32))
    assert np.array_equal(got["adv"].view(T, N).cpu().numpy(), want_adv.astype(np.float32))
    assert smp.get_total_sample_number() == T * N


def test_on_serial_trainer_runs_ppo(tmp_path):
    """Four steps of OnSerialTrainer with PPO on the on-policy device sampler, no evaluator, sample_batch_size = 128 = 2 x 64: every
    parameter stays finite and moves."""
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.on_policy_device_sampler import OnPolicyDeviceSampler
    args, alg, smp = _sampler_setup(OnPolicyDeviceSampler)
    args.update(log_save_interval=1000, apprfunc_save_interval=1000, eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    trainer = create_trainer(alg, smp, None, None, **args)
    before = {k: v.detach().clone() for k, v in alg.networks.state_dict().items()}
    for _ in range(4):
        trainer.step()
        trainer.iteration += 1
    after = alg.networks.state_dict()
    assert all(torch.isfinite(p).all() for p in after.values())
    assert all((after[k] - before[k]).abs().max() > 0 for k in before if "lim" not in k)
