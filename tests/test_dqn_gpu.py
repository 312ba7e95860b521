"""GPU: DQN (algorithm/dqn.py) and its two kernels of csrc/actor_critic.hip - `gops_dqn_backup` (the max-Q backup in one launch) and
`gops_dqn_loss` (the dense output-layer seed) - against a float64 restatement and the reference fixtures of
tests/golden/make_golden_dqn.py.

Tolerance of the fused backup (ac_helpers.check_backup): the error of the COMPOSED path (`gops_mlp_forward` + `torch.max`) against
the same float64 restatement on the same inputs is measured first; the fused kernel may use twice that, but not less than 4 fp32 ulp
of the largest |value| of the tensor compared.  The arg-max has no tolerance: it is checked on the kernel's own q_targ bits."""
import pytest
import torch

import ac_helpers as ac
from ac_helpers import EPS32, S, TOL, close
from conftest import rel_l2
from dqn_helpers import DQN_FIVE_UPDATES, DQN_ONE_UPDATE, dqn_batch, dqn_kwargs, load_dqn, restate_dqn, synthetic_dqn
from helpers import data_from_golden

from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
TICKET = 4 + 6 * 64   # float index of the loss kernel's ticket in its stats buffer


def _fused(alg, batch, **kw):
    db = alg._dqn_backup(batch["obs2"].shape[0], batch["obs2"].device)
    assert db.supported
    return db.run(batch["obs2"], batch["rew"], batch["done"], reward_scale=alg.reward_scale, gamma=alg.gamma, want_q=True, want_a=True, **kw)


def _check_a_star(got):
    """On the kernel's own bits: the value at a_star is the row's maximum, and no lower index holds it."""
    q, a = got["q_targ"], got["a_star"].long()
    assert a.min() >= 0 and a.max() < q.shape[1]
    assert torch.equal(q.gather(1, a[:, None]).squeeze(1), q.max(dim=1).values)


def _check_backup(alg, data, label):
    batch = alg._batch(data)
    ref = restate_dqn(alg, data)
    comp = dict(zip(("backup", "q_targ"), alg._backup_composed(batch)))
    got, again = _fused(alg, batch), _fused(alg, batch)
    ac.check_backup(got, again, comp, ref, ("backup", "q_targ"), label)
    assert torch.equal(got["a_star"], again["a_star"])
    _check_a_star(got)
    return ref, batch, got


SHAPES = [(3, 2, [32], "relu"), (4, 5, [64, 48], "tanh"), (3, 16, [48, 16], "gelu")]


@pytest.mark.parametrize("B", [1, 22, 70])
@pytest.mark.parametrize("obs,act_num,hidden,activation", SHAPES)
def test_dqn_backup_against_float64(obs, act_num, hidden, activation, B):
    """B = 1: a partial tile; 22: one full 16-row tile and six rows of the next; 70: four tiles and a partial one.  2 actions (fewer
    than the feature groups of a row), 5, and 16 (the kernel's limit: with 64-row tiles four outputs per thread)."""
    alg = synthetic_dqn(obs, act_num, hidden, activation)
    data = dqn_batch(B, obs, act_num)
    ref, _, got = _check_backup(alg, data, f"{obs}/{act_num} {hidden} {activation} B={B}")
    if B == 70:
        assert (data["done"] == 1).any() and (data["done"] == 0).any()
        if act_num <= 5:   # every action is the arg-max somewhere
            assert set(ref["a_star"].tolist()) == set(range(act_num)) == set(got["a_star"].tolist())


@pytest.mark.parametrize("obs,act_num,hidden,B", [(4, 5, [64, 64], 2054), (4, 5, [256, 256], 16390), (3, 16, [48, 16], 2054)])
def test_dqn_backup_larger_tiles_and_chunked_weights(obs, act_num, hidden, B):
    """The 32-row tiles (B >= 2048) and the 64-row tiles (B >= 16384; 256-wide layers go through LDS in chunks), each with a partial
    last tile; and all 16 actions as the arg-max of some row."""
    alg = synthetic_dqn(obs, act_num, hidden, "elu")
    ref, _, got = _check_backup(alg, dqn_batch(B, obs, act_num, seed=3), f"{act_num} {hidden} B={B}")
    assert set(ref["a_star"].tolist()) == set(range(act_num)) == set(got["a_star"].tolist())


def test_a_row_does_not_depend_on_the_batch_or_the_tile():
    """The same 22 rows at the head of batches of 22 (16-row tiles), 2054 (32-row) and 16390 (64-row): the same bits."""
    alg = synthetic_dqn(4, 5, [64, 48], "tanh")
    big = alg._batch(dqn_batch(16390, 4, 5, seed=9))
    outs = [_fused(alg, {k: v[:B].contiguous() for k, v in big.items()}) for B in (22, 2054, 16390)]
    for o in outs[1:]:
        for k in ("backup", "q_targ", "a_star"):
            assert torch.equal(o[k][:22], outs[0][k]), k


def test_a_star_takes_the_lowest_index_among_equal_maxima():
    """Head rows 1 and 3 made bit-identical and lifted above the rest: both columns hold the same bits, the arg-max is 1."""
    alg = synthetic_dqn(4, 5, [64, 48], "relu")
    head = alg.networks.q_target.linear_layers()[-1]
    with torch.no_grad():
        head.bias[1] += 10.0
        head.weight[3].copy_(head.weight[1])
        head.bias[3].copy_(head.bias[1])
    got = _fused(alg, alg._batch(dqn_batch(70, 4, 5)))
    _check_a_star(got)
    assert torch.equal(got["q_targ"][:, 1], got["q_targ"][:, 3]) and (got["a_star"] == 1).all()


def _loss_inputs(N, B, weighted):
    g = torch.Generator().manual_seed(B + N)
    idx = torch.randint(N, (B,), generator=g)
    act = (idx + 0.9 * torch.rand(B, generator=g)).float()   # the index is the truncation, as `a.to(torch.long)`
    assert torch.equal(act.to(torch.long), idx)
    q, bk = torch.randn(B, N, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    w = (0.2 + 0.8 * torch.rand(B, generator=g)).cuda() if weighted else None
    return q, act.cuda(), idx, bk, w


def test_rows_beyond_the_batch_stay_untouched():
    """Outputs allocated with sentinels behind them: both kernels write the batch's rows only."""
    B, N = 70, 5
    alg = synthetic_dqn(4, N, [64, 48], "tanh")
    batch = alg._batch(dqn_batch(B, 4, N))
    a_buf = torch.full((B + 128,), -777, dtype=torch.int32, device="cuda")
    ac.check_rows_beyond_the_batch(lambda out: _fused(alg, batch, out=dict(out, a_star=a_buf[:B])), dict(backup=B, q_targ=N * B), pad=128)
    assert (a_buf[B:] == -777).all() and (a_buf[:B] >= 0).all()
    q, act, _, bk, _ = _loss_inputs(N, B, False)
    ac.check_rows_beyond_the_batch(lambda out: hb.DqnLoss("cuda").run(q, act, bk, None, seed=out["seed"], abs_err=out["abs_err"]),
                                   dict(seed=N * B, abs_err=B))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,B", [(2, 1), (5, 70), (16, 9000)])
def test_dqn_loss_against_float64(N, B, weighted):
    """The dense seed, |q_sel - backup|, the loss and mean(q_sel) (B = 9000: the 64-block form with the ticket round); two launches
    are bit-equal."""
    q, act, idx, bk, w = _loss_inputs(N, B, weighted)
    dl = hb.DqnLoss("cuda")
    seed, err, stats = (t.clone() for t in dl.run(q, act, bk, w))
    seed2, err2, stats2 = dl.run(q, act, bk, w)
    assert torch.equal(seed, seed2) and torch.equal(err, err2) and torch.equal(stats, stats2)
    q_sel = q.cpu().gather(1, idx[:, None]).squeeze(1)
    diff = q_sel.double() - bk.double().cpu()
    w64 = torch.ones(B, dtype=torch.float64) if w is None else w.double().cpu()
    taken = torch.zeros(B, N, dtype=torch.bool).scatter_(1, idx[:, None], True)
    assert rel_l2(seed.cpu()[taken], 2 * w64 * diff / B) <= 4 * EPS32
    assert (seed.cpu()[~taken] == 0.0).all() and not torch.signbit(seed.cpu()[~taken]).any()
    assert torch.equal(err.cpu(), (q_sel - bk.cpu()).abs())
    want = [(w64 * diff ** 2).mean().item(), q_sel.double().mean().item(), 0.0]
    for i, v in enumerate(want):
        assert abs(stats[i].item() - v) <= 4 * EPS32 * max(abs(v), q_sel.double().abs().mean().item() if i == 1 else 0.0) + 1e-30, (i, stats[i].item(), v)
    assert int(dl.buf[TICKET:].view(torch.int32)[0].item()) == 0   # the ticket is left zero


@pytest.mark.parametrize("B", [70, 9000])
def test_dqn_loss_leaves_out_rows_with_a_bad_index(B):
    """One row with index act_num and one with -1: counted, a zero seed row and abs_err 0, nothing of them in the sums, and nothing
    written or read outside the rows (q_all, the seed and abs_err sit between sentinels)."""
    N, pad = 5, 64
    q, act, idx, bk, w = _loss_inputs(N, B, True)
    act[3], act[10] = float(N), -1.0
    q_buf = torch.full((pad + B * N + pad,), float("nan"), device="cuda")   # a read outside q_all would poison the sums
    q_buf[pad:pad + B * N] = q.reshape(-1)
    seed_buf, err_buf = torch.full((pad + B * N + pad,), S, device="cuda"), torch.full((pad + B + pad,), S, device="cuda")
    dl = hb.DqnLoss("cuda")
    seed, err, stats = dl.run(q_buf[pad:pad + B * N].view(B, N), act, bk, w, seed=seed_buf[pad:pad + B * N].view(B, N), abs_err=err_buf[pad:pad + B])
    torch.cuda.synchronize()
    assert stats[2].item() == 2.0
    for t, n in ((seed_buf, B * N), (err_buf, B)):
        assert (t[:pad] == S).all() and (t[pad + n:] == S).all() and (t[pad:pad + n] != S).all()
    good = torch.ones(B, dtype=torch.bool)
    good[3] = good[10] = False
    assert (seed[~good.cuda()] == 0.0).all() and (err[~good.cuda()] == 0.0).all()
    q_sel = q.cpu()[good].gather(1, idx[good][:, None]).squeeze(1)
    diff = q_sel.double() - bk.double().cpu()[good]
    want = [(w.double().cpu()[good] * diff ** 2).sum().item() / B, q_sel.double().sum().item() / B]
    assert abs(stats[0].item() - want[0]) <= 4 * EPS32 * abs(want[0])
    assert abs(stats[1].item() - want[1]) <= 4 * EPS32 * q_sel.double().abs().sum().item() / B
    assert torch.equal(err.cpu()[good], (q_sel - bk.cpu()[good]).abs())
    assert int(dl.buf[TICKET:].view(torch.int32)[0].item()) == 0


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", DQN_ONE_UPDATE)
def test_one_update_matches_the_reference(name, fused):
    """Through create_alg on the GPU: the path taken, the loss and every gradient of one update against the reference's; then the
    step moves every parameter of q and q_target."""
    alg, g, meta = load_dqn(name, use_gpu=True, fused_target=fused)
    tb, info = alg.get_remote_update_info(data_from_golden(g), 0)
    assert alg.backup_path == ("fused" if fused else "composed")
    assert set(tb) == {"Loss/Critic loss-RL iter", "Time/Algorithm time [ms]-RL iter"}
    assert close(tb["Loss/Critic loss-RL iter"], g["loss_q"]), (float(tb["Loss/Critic loss-RL iter"]), float(g["loss_q"]))
    assert set(info) == {"q_grad", "iteration"} and info["iteration"] == 0 and alg.bad_action_rows() == 0
    for i, gr in enumerate(info["q_grad"]):
        assert rel_l2(gr.cpu(), g[f"q_grad/{i}"]) < TOL, (i, rel_l2(gr.cpu(), g[f"q_grad/{i}"]))
    ac.check_the_step_moves_everything(alg, info)


def test_five_updates_match_the_reference():
    """Five `local_update` calls with tau = 0.05 and the learning rate at 1e-2: the loss and every online and target parameter after
    each update, rel-L2 < 1e-4."""
    alg, g, meta = load_dqn(DQN_FIVE_UPDATES, use_gpu=True, prefix="sd0/")
    assert alg.tau == 0.05
    for k in range(5):
        tb = alg.local_update(data_from_golden(g, f"in{k}/"), k)
        assert close(tb["Loss/Critic loss-RL iter"], g[f"loss_q{k}"]), k
        for key, p in alg.networks.state_dict().items():
            assert rel_l2(p.cpu().double(), g[f"sd{k + 1}/{key}"]) < TOL, (k, key)
    assert alg.backup_path == "fused"


@pytest.mark.parametrize("fused", [True, False])
def test_prioritized_replay_returns_the_triple(fused):
    """No reference fixture exists (the reference's PER path raises): the weighted loss, |q_sel - backup| and the gradients against the
    float64 restatement of the evident intent."""
    alg = synthetic_dqn(4, 5, [64, 48], "tanh", buffer_name="prioritized_replay_buffer", fused_target=fused)
    data = dqn_batch(70, 4, 5, weight=True)
    ref = restate_dqn(alg, data)
    (tb, idx, err), info = alg.get_remote_update_info(data, 0)
    assert torch.equal(idx, data["idx"]) and err.shape == (70,) and rel_l2(err.cpu(), ref["abs_err"]) < TOL
    assert close(tb["Loss/Critic loss-RL iter"], ref["loss"])
    for got, want in zip(info["q_grad"], ref["grads"]["q"]):
        assert rel_l2(got.cpu(), want) < TOL
    out = alg.local_update(data, 1)
    assert isinstance(out, tuple) and len(out) == 3 and torch.equal(out[1], data["idx"]) and out[2].shape == (70,)


def test_graph_replay_equals_eager(monkeypatch):
    ac.check_graph_replay(lambda: synthetic_dqn(3, 2, [32, 16], "relu", seed=4), 1, monkeypatch)


def test_default_takes_the_fused_backup_up_to_64_wide():
    """Up to 64-wide networks: the one-launch backup; 256-wide: the composed path unless forced; `backup_path` says which."""
    data = dqn_batch(22, 3, 2)
    for hidden, over, want in (([64, 64], {}, "fused"), ([256, 256], {}, "composed"), ([256, 256], dict(fused_target="force"), "fused"),
                               ([64, 64], dict(fused_target=False), "composed")):
        alg = synthetic_dqn(3, 2, hidden, "relu", **over)
        alg.get_remote_update_info(data, 0)
        assert alg.backup_path == want, (hidden, over)


@pytest.mark.parametrize("act_num,hidden", [(17, [32]), (2, [272])])
def test_shapes_the_kernel_refuses_run_composed(act_num, hidden):
    """More than 16 actions, or a hidden width beyond 256: workspace_bytes is 0, the kernel returns GOPS_ERR_UNSUPPORTED, the
    algorithm runs the composed path and says so - and still matches the float64 restatement."""
    alg = synthetic_dqn(3, act_num, hidden, "relu")
    data = dqn_batch(22, 3, act_num)
    batch = alg._batch(data)
    db = alg._dqn_backup(22, batch["obs"].device)
    assert not db.supported and hb.lib().gops_dqn_backup_workspace_bytes(hb.C.byref(db.desc), 22) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        db.run(batch["obs2"], batch["rew"], batch["done"])
    assert alg.fused_target
    ref = restate_dqn(alg, data)
    _, info = alg.get_remote_update_info(data, 0)
    assert alg.backup_path == "composed"
    for got, want in zip(info["q_grad"], ref["grads"]["q"]):
        assert rel_l2(got.cpu(), want) < TOL


def test_workspace_and_alignment_refusals():
    ok = synthetic_dqn(3, 2, [32], "relu")
    small = hb.DqnBackup(ok.networks.q_target.hip_mlp(), batch=22, workspace_bytes=16)
    assert small.supported
    b = ok._batch(dqn_batch(22, 3, 2))
    with pytest.raises(RuntimeError, match="GOPS_ERR_WORKSPACE"):
        small.run(b["obs2"], b["rew"], b["done"])
    # gops_dqn_loss keeps doubles behind its results: a `stats` pointer off the 8-byte grid is refused before any launch
    q, buf = torch.zeros(22, 2, device="cuda"), torch.zeros(hb.DQN_LOSS_STATS_FLOATS + 1, device="cuda")
    v = torch.zeros(22, device="cuda")
    rc = hb.lib().gops_dqn_loss(q.data_ptr(), v.data_ptr(), v.data_ptr(), None, 2, 22, q.clone().data_ptr(), None, buf.data_ptr() + 4, None)
    assert rc == -1


def test_end_to_end_two_action_cartpole(tmp_path):
    """OffSerialTrainer + replay buffer + DeviceEnvSampler on gym_cartpoleconti with the action table [[-1], [1]] (the two-action
    cartpole), epsilon 0.25, no evaluator: six steps; every stored action is an index, both occur, the updates took the one-launch
    backup, everything stays finite."""
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    kw = dqn_kwargs(4, 2, [64, 64], "relu", use_gpu=True, env_id="gym_cartpoleconti", action_dim=1, buffer_max_size=4096, buffer_warm_size=512,
                    replay_batch_size=64, sample_interval=1, additional_info={}, max_iteration=8, log_save_interval=1000,
                    apprfunc_save_interval=1000, eval_interval=10 ** 9, save_folder=str(tmp_path), ini_network_dir=None)
    alg, buf, _, trainer = ac.build_trainer(kw, lambda model, alg: DeviceEnvSampler(dict(env_id="gym_cartpoleconti"), model, n_envs=128,
                                                                                   steps_per_sample=2, max_episode_steps=50, seed=3,
                                                                                   action_table=[[-1.0], [1.0]], epsilon=0.25), False)
    ac.run_trainer(trainer, alg)
    stored = buf.buf["act"][:buf.size]
    assert stored.shape[1] == 1 and buf.size >= 512
    assert ((stored == 0.0) | (stored == 1.0)).all() and (stored == 0.0).any() and (stored == 1.0).any()
    assert alg.backup_path == "fused" and alg.bad_action_rows() == 0
    assert all(torch.isfinite(p).all() for p in alg.networks.parameters())
