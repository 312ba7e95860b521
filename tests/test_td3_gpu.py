"""GPU: DDPG / TD3 (algorithm/_actor_critic.py) and the two kernels of csrc/actor_critic.hip - `gops_ac_backup` (the Bellman backup
in one launch) and `gops_ac_critic_loss` - against a float64 restatement and the reference fixtures of
tests/golden/make_golden_td3.py.

Tolerance of the fused backup (ac_helpers.check_backup): the error of the COMPOSED path (`gops_mlp_forward` + torch elementwise
ops) against the same float64 restatement on the same inputs is measured first; the fused kernel may use twice that, but not less
than 4 fp32 ulp of the largest |value| of the tensor compared (a sum of up to 256 fp32 products cannot be asked to be more exact
than a few roundings of its result).  The test prints both errors."""
import numpy as np
import pytest
import torch

import ac_helpers as ac
from ac_helpers import EPS32, S, TD3_ONE_UPDATE, TOL, load_alg, restate_update
from conftest import rel_l2

from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
_data = ac.synthetic_batch


def _alg(obs, act, hidden, activation, alg="TD3", seed=5, **over):
    """A DDPG / TD3 object on the GPU with every network randomised apart, its target head steep enough to saturate the squash."""
    meta = ac.synthetic_meta(alg, obs, act, hidden, activation, seed, per=False, attrs=dict(target_noise=0.4, noise_clip=0.5))
    a = ac.synthetic_alg(meta, obs, act, ac.spread_target_head, **over)
    a.gamma, a.reward_scale = 0.97, 0.5
    return a


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
    ac.check_backup(_fused(alg, batch)[1], _fused(alg, batch)[1], comp, ref, ("backup", "a2", "q_targ"), label)
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
    B, pad = 70, 64
    alg = _alg(4, 2, [64, 48], "tanh")
    batch = alg._batch(_data(B, 4, 2))
    got = ac.check_rows_beyond_the_batch(lambda out: _fused(alg, batch, out=out)[1], dict(backup=B, a2=2 * B, q_targ=2 * B), pad=2 * pad)
    full = lambda n: torch.full((n,), S, device="cuda")   # noqa: E731
    q = torch.randn(2, B, device="cuda")
    seed, err = full(2 * B + pad), full(B + pad)
    hb.AcCriticLoss("cuda").run(q, got["backup"].clone(), None, seed=seed, abs_err=err)
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
@pytest.mark.parametrize("name", TD3_ONE_UPDATE)
def test_one_update_matches_the_reference(name, fused):
    """Through create_alg on the GPU: losses, every gradient and (PER) idx / abs_err of one update against the reference's."""
    alg, g, meta = load_alg(name, use_gpu=True, fused_target=fused)
    data, extra, tb, info = ac.check_one_update(alg, g, meta, fused)
    if meta["per"]:
        assert torch.equal(extra[1].cpu(), data["idx"]) and rel_l2(extra[2].cpu(), g["abs_err"]) < TOL
    ac.check_the_step_moves_everything(alg, info)


@pytest.mark.parametrize("name", ["td3_pend_relu", "ddpg_lqs4a2_gelu"])
def test_fused_and_composed_updates_agree(name):
    ac.check_fused_and_composed_agree(name, _check_backup)


def test_td3_five_updates_match_the_reference():
    """Five `local_update` calls with delay_update = 2 and the reference's own noise draws handed in: every online and target
    parameter after each update (rel-L2 < 1e-4, the bound of the five-update POLY / LipsNet tests); the policy steps at
    iterations 0, 2, 4 only - at 1 and 3 it keeps its bits, while its target still moves towards it (Polyak runs every iteration,
    td3.py:234-251)."""
    for alg, g, k, before in ac.five_updates("td3_pend_5updates"):
        assert alg.delay_update == 2 and alg.tau == 0.05
        sd = alg.networks.state_dict()
        moved = any(not torch.equal(p, before[key]) for key, p in sd.items() if key.startswith("policy."))
        assert moved == (k % 2 == 0), k
        assert any(not torch.equal(p, before[key]) for key, p in sd.items() if key.startswith("policy_target.")), k
        ref_moved = any(not np.array_equal(g[f"sd{k}/{key}"], g[f"sd{k + 1}/{key}"]) for key in sd if key.startswith("policy.pi"))
        assert ref_moved == (k % 2 == 0)


@pytest.mark.parametrize("name", ["TD3", "DDPG"])
def test_graph_replay_equals_eager(name, monkeypatch):
    def make():
        alg = _alg(3, 1, [32, 16], "relu", alg=name, seed=4)
        alg.delay_update = 2
        return alg

    ac.check_graph_replay(make, 2, monkeypatch)


def test_per_end_to_end(tmp_path):
    """OffSerialTrainer + prioritized_replay_buffer + DeviceEnvSampler with exploration noise + TD3: local_update returns the triple,
    the priorities of the sampled leaves become (|q1 - backup| + eps)^alpha, the in-launch evaluator returns a finite value."""
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    kw = ac.trainer_kwargs("TD3", "pyth_idpendulum", 6, 1.0, tmp_path, buffer_name="prioritized_replay_buffer")
    alg, buf, ev, trainer = ac.build_trainer(kw, lambda model, alg: DeviceEnvSampler(dict(env_id="pyth_idpendulum"), model, n_envs=128,
                                                                                    steps_per_sample=2, max_episode_steps=50, seed=3, noise_std=0.2), True)
    seen = {}
    update = alg.local_update

    def spy(data, iteration):
        out = update(data, iteration)
        seen["out"] = out
        return out

    def priorities_follow():
        tb, idx, err = seen["out"]
        assert isinstance(tb, dict) and idx.shape == (64,) and err.shape == (64,)
        want = (err.double() + buf.epsilon) ** buf.alpha
        # (duplicated leaves keep the value of the index's last occurrence: compare through a table filled in order)
        table = {}
        for i, v in zip(idx.tolist(), want.tolist()):
            table[i] = v
        got = buf.sum_tree[torch.tensor(list(table), device=buf.sum_tree.device)].tolist()
        assert got == list(table.values())

    alg.local_update = spy
    ac.run_trainer(trainer, alg, priorities_follow)
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
