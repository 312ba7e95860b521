"""GPU: DDPG / TD3 (algorithm/_actor_critic.py) and the two kernels of csrc/actor_critic.hip - `gops_ac_backup` (the Bellman backup
in one launch) and `gops_ac_critic_loss` - against a float64 restatement and the reference fixtures of
tests/golden/make_golden_td3.py.

Tolerance of the fused backup: the error of the COMPOSED path (`gops_mlp_forward` + torch elementwise ops) against the same float64
restatement on the same inputs is measured first; the fused kernel may use twice that, but not less than 4 fp32 ulp of the largest
|value| of the tensor compared (a sum of up to 256 fp32 products cannot be asked to be more exact than a few roundings of its
result).  The test prints both errors."""
import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from td3_helpers import ONE_UPDATE, TOL, alg_kwargs, batch_of, load_alg, q_names_of, restate_update

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_alg import create_alg

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23


def _alg(obs, act, hidden, activation, alg="TD3", seed=5, **over):
    """A DDPG / TD3 object on the GPU with every network randomised apart, its target head steep enough to saturate the squash."""
    meta = dict(cfg=dict(alg=alg, env_id="gym_pendulum" if obs == 3 else "pyth_lq", hidden=hidden, act=activation),
                lim=([-2.0], [2.0]) if act == 1 else ([-1.0, -0.5], [2.0, 0.5]), seed=seed, per=False,
                attrs=dict(target_noise=0.4, noise_clip=0.5))
    if obs == 4:
        meta["cfg"]["lq_config"] = "s4a2"
    torch.manual_seed(seed)
    a = create_alg(**alg_kwargs(meta, True, **over))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in a.networks.named_parameters():
            if "_target" in n:
                p.add_(0.3 * (torch.rand(p.shape, generator=g) - 0.5))
        # the target head spread to +-3 around zero on inputs like `_data`'s (tanh saturates on some rows, not on others) and the
        # twin targets centred on each other: rows on both sides of every clamp and of the minimum
        head = a.networks.policy_target.linear_layers()[-1]
        probe = torch.randn(256, obs, generator=g)
        spread = 3.0 / a.networks.policy_target.pi(probe).std(dim=0)
        head.weight.mul_(spread[:, None])
        head.bias.mul_(spread)
        head.bias.sub_(a.networks.policy_target.pi(probe).median(dim=0).values)
        if alg == "TD3":
            a2 = a.networks.policy_target(probe)
            a.networks.q2_target.linear_layers()[-1].bias.add_((a.networks.q1_target(probe, a2) - a.networks.q2_target(probe, a2)).median())
    a.networks.cuda()
    a.gamma, a.reward_scale = 0.97, 0.5
    return a


def _data(B, obs, act, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, obs, generator=g)
    d = (torch.rand(B, generator=g) < 0.2).float()
    if B > 1:
        d[0], d[-1] = 1.0, 0.0
    return dict(obs=o, act=torch.rand(B, act, generator=g) * 2 - 1, rew=torch.randn(B, generator=g), obs2=o + 0.1 * torch.randn(B, obs, generator=g),
                done=d, target_noise=torch.randn(B, act, generator=g))


def _fused(alg, batch, **kw):
    ab = alg._ac_backup(batch["obs2"].shape[0], batch["obs2"].device)
    assert ab.supported
    return ab, ab.run(batch["obs2"], batch["rew"], batch["done"], batch.get("target_noise"), target_noise=getattr(alg, "target_noise", 0.0),
                      noise_clip=getattr(alg, "noise_clip", 0.0), reward_scale=getattr(alg, "reward_scale", 1.0), gamma=alg.gamma,
                      want_a2=True, want_q=True, **kw)


def _check_backup(alg, data, label):
    batch = alg._batch(data)
    ref = restate_update(alg, data)
    comp = dict(zip(("backup", "a2", "q_targ"), alg._backup_composed(batch)))
    _, got = _fused(alg, batch)
    _, again = _fused(alg, batch)
    for k in ("backup", "a2", "q_targ"):
        want = ref[k].reshape(got[k].shape)
        err_c = (comp[k].double().cpu() - want).abs().max().item()
        err_f = (got[k].double().cpu() - want).abs().max().item()
        bound = max(2 * err_c, 4 * EPS32 * want.abs().max().item())
        print(f"{label} {k}: fused {err_f:.3e} composed {err_c:.3e} bound {bound:.3e}")
        assert err_f <= bound, (label, k, err_f, err_c, bound)
        assert torch.equal(got[k], again[k]), (label, k)
    return ref, batch


SHAPES = [(3, 1, [32], "relu"), (4, 2, [64, 48], "tanh"), (3, 1, [48, 16], "gelu")]


@pytest.mark.parametrize("B", [1, 22, 70])
@pytest.mark.parametrize("obs,act,hidden,activation", SHAPES)
def test_ac_backup_against_float64(obs, act, hidden, activation, B):
    """B = 22: one full 16-row tile and six rows of the next; 70: four tiles and a partial one; one and two hidden layers of
    different widths, three activations, both action widths; TD3 (two critics, smoothing)."""
    alg = _alg(obs, act, hidden, activation)
    data = _data(B, obs, act)
    ref, batch = _check_backup(alg, data, f"{obs}/{act} {hidden} {activation} B={B}")
    if B == 70:   # the cases the clamps need are in the batch
        raw = data["target_noise"] * alg.target_noise
        pre = alg.networks.policy_target(batch["obs2"]).cpu() + raw.clamp(-alg.noise_clip, alg.noise_clip)
        lo, hi = torch.tensor(alg.act_low_limit), torch.tensor(alg.act_high_limit)
        assert (raw > alg.noise_clip).any() and (raw < -alg.noise_clip).any() and (raw.abs() < alg.noise_clip).any()
        assert (pre > hi).any() and (pre < lo).any() and ((pre > lo) & (pre < hi)).any()
        assert (ref["q_targ"][0] < ref["q_targ"][1]).any() and (ref["q_targ"][1] < ref["q_targ"][0]).any()
        assert (data["done"] == 1).any() and (data["done"] == 0).any()


@pytest.mark.parametrize("hidden,B", [([64, 64], 2054), ([256, 256], 16390)])
def test_ac_backup_larger_tiles_and_chunked_weights(hidden, B):
    """The 32-row tiles (B >= 2048) and the 64-row tiles (B >= 16384; with 256-wide layers the weights go through LDS in chunks of
    16 output features next to 132 KiB of activations), each with a partial last tile."""
    alg = _alg(4, 2, hidden, "elu")
    _check_backup(alg, _data(B, 4, 2, seed=3), f"{hidden} B={B}")


def test_ac_backup_ddpg_one_critic():
    alg = _alg(3, 1, [32, 16], "relu", alg="DDPG")
    alg.gamma = 0.95
    data = _data(70, 3, 1)
    data.pop("target_noise")
    _check_backup(alg, data, "ddpg")


def test_rows_beyond_the_batch_stay_untouched():
    """Outputs allocated with one extra 64-row tile of sentinel behind them: the kernels write the batch's rows only."""
    S, B, pad = -777.0, 70, 64
    alg = _alg(4, 2, [64, 48], "tanh")
    batch = alg._batch(_data(B, 4, 2))
    full = lambda n: torch.full((n,), S, device="cuda")   # noqa: E731
    bk, a2, qt = full(B + pad), full((B + pad) * 2), full(2 * B + pad)
    _fused(alg, batch, out=dict(backup=bk, a2=a2, q_targ=qt))
    torch.cuda.synchronize()
    for t, n in ((bk, B), (a2, 2 * B), (qt, 2 * B)):
        assert (t[:n] != S).all() and (t[n:] == S).all()
    q = torch.randn(2, B, device="cuda")
    seed, err = full(2 * B + pad), full(B + pad)
    hb.AcCriticLoss("cuda").run(q, bk[:B].clone(), None, seed=seed, abs_err=err)
    torch.cuda.synchronize()
    assert (seed[:2 * B] != S).all() and (seed[2 * B:] == S).all() and (err[:B] != S).all() and (err[B:] == S).all()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nq,B", [(1, 1), (2, 70), (2, 9000), (1, 9000)])
def test_ac_critic_loss_against_float64(nq, B, weighted):
    """Seeds, losses, mean(q) and |q - backup| (B = 9000: the 64-block form with the ticket round); two launches are bit-equal."""
    g = torch.Generator().manual_seed(B + nq)
    q, bk = torch.randn(nq, B, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    w = (0.2 + 0.8 * torch.rand(B, generator=g)).cuda() if weighted else None
    cl = hb.AcCriticLoss("cuda")
    seed, err, stats = (t.clone() for t in cl.run(q, bk, w))
    seed2, err2, stats2 = cl.run(q, bk, w)
    assert torch.equal(seed, seed2) and torch.equal(err, err2) and torch.equal(stats, stats2)
    q64, b64 = q.double().cpu(), bk.double().cpu()
    w64 = torch.ones(B, dtype=torch.float64) if w is None else w.double().cpu()
    diff = q64 - b64
    assert rel_l2(seed.cpu(), 2 * w64 * diff / B) <= 4 * EPS32
    assert torch.equal(err.cpu(), (q[0] - bk).abs().cpu())
    losses = (w64 * diff ** 2).mean(dim=1)
    want = [losses[0].item(), losses[1].item() if nq == 2 else 0.0, q64[0].mean().item(), losses.sum().item()]
    for i, v in enumerate(want):
        assert abs(stats[i].item() - v) <= 4 * EPS32 * max(abs(v), q64[0].abs().mean().item() if i == 2 else 0.0) + 1e-30, (i, stats[i].item(), v)
    assert int(cl.buf[4 + 6 * 64:].view(torch.int32)[0].item()) == 0   # the ticket is left zero


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ONE_UPDATE)
def test_one_update_matches_the_reference(name, fused):
    """Through create_alg on the GPU: losses, every gradient and (PER) idx / abs_err of one update against the reference's."""
    alg, g, meta = load_alg(name, use_gpu=True, fused_target=fused)
    data = batch_of(g)
    extra, info = alg.get_remote_update_info(data, 0)
    assert alg.backup_path == ("fused" if fused else "composed")
    tb = extra[0] if meta["per"] else extra
    close = lambda a, b: abs(float(a) - float(b)) <= TOL * max(1.0, abs(float(b)))   # noqa: E731
    for k in [k for k in g if k.startswith("tb/")]:
        assert close(tb[k[3:]], g[k]), (k, float(tb[k[3:]]), float(g[k]))
    names = q_names_of(meta["cfg"]["alg"]) + ("policy",)
    assert set(info) == {f"{n}_grad" for n in names} | {"iteration"} and info["iteration"] == 0
    for n in names:
        for i, gr in enumerate(info[f"{n}_grad"]):
            assert rel_l2(gr.cpu(), g[f"{n}_grad/{i}"]) < TOL, (n, i, rel_l2(gr.cpu(), g[f"{n}_grad/{i}"]))
    if meta["per"]:
        assert torch.equal(extra[1].cpu(), data["idx"]) and rel_l2(extra[2].cpu(), g["abs_err"]) < TOL
    before = [p.detach().clone() for p in alg.networks.parameters()]
    alg.remote_update(info)
    assert all(torch.isfinite(p).all() for p in alg.networks.parameters())
    assert all((a - b).abs().max() > 0 for a, b in zip(alg.networks.parameters(), before))


@pytest.mark.parametrize("name", ["td3_pend_relu", "ddpg_lqs4a2_gelu"])
def test_fused_and_composed_updates_agree(name):
    """The two backups differ by fp32 rounding only (bound of the module docstring, measured on the fixture's own inputs); the
    gradients are linear in the backup: 1e-5 relative, a tenth of the parity bound, leaves two decades for their conditioning."""
    out = {}
    for fused in (True, False):
        alg, g, meta = load_alg(name, use_gpu=True, fused_target=fused)
        _, info = alg.get_remote_update_info(batch_of(g), 0)
        out[fused] = {n: [t.clone() for t in v] for n, v in info.items() if n.endswith("_grad")}
    _check_backup(alg, batch_of(g), name)
    for n in out[True]:
        for a, b in zip(out[True][n], out[False][n]):
            assert rel_l2(a.cpu(), b.cpu()) <= 1e-5, n


def test_td3_five_updates_match_the_reference():
    """Five `local_update` calls with delay_update = 2 and the reference's own noise draws handed in: every online and target
    parameter after each update (rel-L2 < 1e-4, the bound of the five-update POLY / LipsNet tests); the policy steps at
    iterations 0, 2, 4 only - at 1 and 3 it keeps its bits, while its target still moves towards it (Polyak runs every iteration,
    td3.py:234-251)."""
    alg, g, meta = load_alg("td3_pend_5updates", use_gpu=True, prefix="sd0/")
    for n in ("q1", "q2", "policy"):
        for group in getattr(alg.networks, f"{n}_optimizer").param_groups:
            group["lr"] = meta["lr"]
    assert alg.delay_update == 2 and alg.tau == 0.05
    close = lambda a, b: abs(float(a) - float(b)) <= TOL * max(1.0, abs(float(b)))   # noqa: E731
    for k in range(5):
        policy_before = [p.detach().clone() for p in alg.networks.policy.parameters()]
        target_before = [p.detach().clone() for p in alg.networks.policy_target.parameters()]
        tb = alg.local_update(batch_of(g, f"in{k}/"), k)
        assert close(tb["Loss/Critic loss-RL iter"], g[f"loss_q{k}"]) and close(tb["Loss/Actor loss-RL iter"], g[f"loss_pi{k}"]), k
        for key, p in alg.networks.state_dict().items():
            assert rel_l2(p.cpu().double(), g[f"sd{k + 1}/{key}"]) < TOL, (k, key)
        moved = any(not torch.equal(a, b) for a, b in zip(alg.networks.policy.parameters(), policy_before))
        assert moved == (k % 2 == 0), k
        assert any(not torch.equal(a, b) for a, b in zip(alg.networks.policy_target.parameters(), target_before)), k
        ref_moved = any(not np.array_equal(g[f"sd{k}/{key}"], g[f"sd{k + 1}/{key}"]) for key in alg.networks.state_dict() if key.startswith("policy.pi"))
        assert ref_moved == (k % 2 == 0)


@pytest.mark.parametrize("name", ["TD3", "DDPG"])
def test_graph_replay_equals_eager(name, monkeypatch):
    """local_update captured into HIP graphs (one per value of `iteration % delay_update == 0`; the noise draws travel with the
    batch as a graph input) walks exactly the parameter trajectory of the eager launches: 14 updates, of which at least 6 are replays."""
    B = 70

    def run(mode):
        monkeypatch.setenv("GOPS_HIP_GRAPH", mode)
        alg = _alg(3, 1, [32, 16], "relu", alg=name, seed=4)
        alg.delay_update = 2
        logs = []
        for it in range(14):
            data = _data(B, 3, 1, seed=100 + it)
            data.pop("target_noise")   # drawn by the algorithm's own generator: same seed, same draws in both runs
            logs.append(dict(alg.local_update(data, it)))
        return alg, logs

    eager, log_e = run("0")
    graph, log_g = run("1")
    assert all(c.graph is not None for c in graph._graphs.values()) and len(graph._graphs) == 2
    assert all(c.graph is None for c in eager._graphs.values())
    for (ne, pe), (ng, pg) in zip(eager.networks.named_parameters(), graph.networks.named_parameters()):
        assert ne == ng and torch.equal(pe, pg), ne
    for a, b in zip(log_e, log_g):
        for k in a:
            if not k.startswith("Time/"):
                assert float(a[k]) == float(b[k]), k


def test_per_end_to_end(tmp_path):
    """OffSerialTrainer + prioritized_replay_buffer + DeviceEnvSampler with exploration noise + TD3: local_update returns the triple,
    the priorities of the sampled leaves become (|q1 - backup| + eps)^alpha, the in-launch evaluator returns a finite value."""
    from gops_amd.create_pkg.create_buffer import create_buffer
    from gops_amd.create_pkg.create_env_model import create_env_model
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    from gops_amd.create_pkg.create_trainer import create_trainer
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    cfg = dict(env_id="pyth_idpendulum")
    torch.manual_seed(0)
    kw = dict(algorithm="TD3", trainer="off_serial_trainer", seed=0, cnn_shared=False, env_id="pyth_idpendulum", obsv_dim=6, action_dim=1,
              action_type="continu", action_low_limit=-np.ones(1, dtype=np.float32), action_high_limit=np.ones(1, dtype=np.float32),
              policy_func_type="MLP", policy_func_name="DetermPolicy", policy_hidden_sizes=[64, 64], policy_hidden_activation="relu",
              policy_act_distribution="default", policy_learning_rate=1e-3, value_func_type="MLP", value_func_name="ActionValue",
              value_hidden_sizes=[64, 64], value_hidden_activation="relu", value_learning_rate=1e-3, use_gpu=True,
              buffer_name="prioritized_replay_buffer", buffer_max_size=4096, buffer_warm_size=512, replay_batch_size=64,
              sample_interval=1, additional_info={}, max_iteration=8, log_save_interval=1000, apprfunc_save_interval=1000,
              eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    alg = create_alg(**kw)
    alg.networks.to("cuda")
    model = create_env_model(**kw)
    smp = DeviceEnvSampler(cfg, model, n_envs=128, steps_per_sample=2, max_episode_steps=50, seed=3, noise_std=0.2)
    buf = create_buffer(**kw)
    ev = create_evaluator(**dict(kw, env_model=model, networks=alg.networks, num_eval_episode=4, eval_save=False, is_render=False,
                                 max_episode_steps=40))
    trainer = create_trainer(alg, smp, buf, ev, **kw)
    seen = {}
    update = alg.local_update

    def spy(data, iteration):
        out = update(data, iteration)
        seen["out"] = out
        return out

    alg.local_update = spy
    for _ in range(6):
        trainer.step()
        trainer.iteration += 1
        tb, idx, err = seen["out"]
        assert isinstance(tb, dict) and idx.shape == (64,) and err.shape == (64,)
        want = (err.double() + buf.epsilon) ** buf.alpha
        # (duplicated leaves keep the value of the index's last occurrence: compare through a table filled in order)
        table = {}
        for i, v in zip(idx.tolist(), want.tolist()):
            table[i] = v
        got = buf.sum_tree[torch.tensor(list(table), device=buf.sum_tree.device)].tolist()
        assert got == list(table.values())
    assert alg.backup_path == "fused"
    assert all(torch.isfinite(p).all() for p in alg.networks.parameters())
    assert np.isfinite(ev.run_evaluation(0))


def test_default_takes_the_fused_backup_where_it_was_measured_faster():
    """Up to 64-wide networks: the one-launch backup; 256-wide: the composed path unless forced; `backup_path` says which."""
    data = _data(22, 3, 1)
    for hidden, over, want in (([64, 64], {}, "fused"), ([256, 256], {}, "composed"), ([256, 256], dict(fused_target="force"), "fused"),
                               ([64, 64], dict(fused_target=False), "composed")):
        alg = _alg(3, 1, hidden, "relu", **over)
        alg.get_remote_update_info(data, 0)
        assert alg.backup_path == want, (hidden, over)


def test_shape_refusals():
    """A hidden width the kernel does not hold: workspace_bytes is 0, the algorithm runs the composed path and says so; an accepted
    shape with a workspace that is too small returns GOPS_ERR_WORKSPACE."""
    alg = _alg(3, 1, [272], "relu")          # wider than the kernel's 256; `gops_mlp_forward` takes any multiple of 16
    data = _data(22, 3, 1)
    batch = alg._batch(data)
    ab = alg._ac_backup(22, batch["obs"].device)
    assert not ab.supported and hb.lib().gops_ac_backup_workspace_bytes(hb.C.byref(ab.desc), 22) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        ab.run(batch["obs2"], batch["rew"], batch["done"], batch["target_noise"])
    assert alg.fused_target
    alg.get_remote_update_info(data, 0)
    assert alg.backup_path == "composed"
    ok = _alg(3, 1, [32], "relu")
    pol = ok.networks.policy_target
    small = hb.AcBackup(pol.hip_mlp(), [ok.networks.q1_target.hip_mlp(), ok.networks.q2_target.hip_mlp()],
                        squash_low=pol.act_low_lim.cpu().numpy(), squash_high=pol.act_high_lim.cpu().numpy(), act_low=ok.act_low_limit,
                        act_high=ok.act_high_limit, batch=22, smooth=True, workspace_bytes=16)
    assert small.supported
    b = ok._batch(data)
    with pytest.raises(RuntimeError, match="GOPS_ERR_WORKSPACE"):
        small.run(b["obs2"], b["rew"], b["done"], b["target_noise"])
    # gops_ac_critic_loss keeps doubles behind its four results: a `stats` pointer off the 8-byte grid is refused before any launch
    q, buf = torch.zeros(1, 22, device="cuda"), torch.zeros(hb.AC_LOSS_STATS_FLOATS + 1, device="cuda")
    rc = hb.lib().gops_ac_critic_loss(q.data_ptr(), q.data_ptr(), None, 1, 22, q.clone().data_ptr(), None, buf.data_ptr() + 4, None)
    assert rc == -1
