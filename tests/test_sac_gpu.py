"""GPU: SAC and DSAC (algorithm/sac.py, dsac.py) and their kernels - `gops_soft_q_backup`, `gops_dsac_critic_loss` - against a float64
restatement and the reference fixtures of tests/golden/make_golden_sac.py.

Bound of the soft Q backup (ac_helpers.check_backup, the rule of test_td3_gpu.py / test_dsact_gpu.py): the composed path's max error
against float64 is measured on the same inputs first; the fused kernel may use twice that, but not less than 4 fp32 ulp of the
largest |value|.  The critic-loss kernel forms every value in double from its fp32 inputs and rounds once: 4 ulp rel-L2 against
float64 evaluated on the same fp32 inputs.
"""
import copy

import numpy as np
import pytest
import torch

import ac_helpers as ac
from ac_helpers import EPS32, S, SAC_FIVE_UPDATES, SAC_ONE_UPDATE, TOL, close, load_alg
from conftest import rel_l2

from gops_amd import hip_backend as hb

pytestmark = pytest.mark.gpu
OUT = ("backup", "a2", "logp", "q_targ")
CTOR = {"SAC": dict(gamma=0.97, tau=0.05, auto_alpha=True), "DSAC": dict(gamma=0.97, tau=0.05, auto_alpha=True, bound=True, delay_update=2)}


def _alg(name, obs, act, hidden, activation, seed=5, **over):
    """A SAC / DSAC object on the GPU: targets randomised apart, the heads of ac_helpers.shape_soft_heads.  act 4 (obs 6): eight head
    outputs."""
    meta = ac.synthetic_meta(name, obs, act, hidden, activation, seed, min_log_std=-3.0, max_log_std=-0.5, ctor=CTOR[name])
    return ac.synthetic_alg(meta, obs, act, ac.shape_soft_heads, **over)


def _data(B, obs, act, seed=0):
    return ac.synthetic_batch(B, obs, act, seed, z_next=(B,))


def _ref_backup(alg, data):
    """The backup of whatever `alg._backup_modules()` names, in float64 on the host."""
    pol, qs = alg._backup_modules()
    pol, qs = copy.deepcopy(pol).cpu().double(), [copy.deepcopy(q).cpu().double() for q in qs]
    d = {k: v.detach().cpu().double() for k, v in data.items()}
    alpha = float(alg.networks.log_alpha.detach().double().exp()) if alg.auto_alpha else float(alg.alpha)
    with torch.no_grad():
        a2, logp = pol.get_act_dist(pol(d["obs2"])).rsample(d["eps_next"])
        if alg._distri:
            q_targ = qs[0](d["obs2"], a2)
            q_next = q_targ[:, 0] + torch.clamp(d["z_next"], -3, 3) * q_targ[:, 1]
        else:
            q_targ = torch.stack([q(d["obs2"], a2) for q in qs])
            q_next = q_targ.min(dim=0).values
        backup = d["rew"] + (1 - d["done"]) * alg.gamma * (q_next - alpha * logp)
    return dict(backup=backup, a2=a2, logp=logp, q_targ=q_targ)


def _fused(alg, batch, want=("a2", "logp", "q_targ"), **kw):
    sb = alg._soft_q_backup(batch["obs2"].shape[0], batch["obs2"].device)
    assert sb.supported and sb.n_q == len(alg._q_names) and sb.distri == alg._distri
    return sb.run(batch["obs2"], batch["rew"], batch["done"], batch["eps_next"], batch.get("z_next"), gamma=alg.gamma, alpha=alg.alpha,
                  want=want, **kw)


def _check_backup(alg, data, label):
    batch = alg._batch(data)
    ref = _ref_backup(alg, data)
    ac.check_backup(_fused(alg, batch), _fused(alg, batch), dict(zip(OUT, alg._backup_composed(batch))), ref, OUT, label)
    return ref, batch


SHAPES = [(3, 1, [32], "relu"), (4, 2, [64, 48], "tanh"), (3, 1, [48, 16], "gelu")]
KINDS = ["SAC", "DSAC", "SAC one critic"]   # distri 0 / n_q 2, distri 1 / n_q 1, distri 0 / n_q 1


def _kind(kind, *args, **kw):
    alg = _alg(kind.split()[0], *args, **kw)
    if kind == "SAC one critic":
        alg._q_names = ("q1",)   # the backup only is asked of this object
    return alg


@pytest.mark.parametrize("B", [1, 22, 70])
@pytest.mark.parametrize("obs,act,hidden,activation", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_soft_q_backup_against_float64(kind, obs, act, hidden, activation, B):
    alg = _kind(kind, obs, act, hidden, activation)
    data = _data(B, obs, act)
    ref, batch = _check_backup(alg, data, f"{kind} {obs}/{act} {hidden} {activation} B={B}")
    assert ref["q_targ"].shape == ((B, 2) if kind == "DSAC" else (len(alg._q_names), B))
    if B == 70:   # the branch cases are in the batch
        pt = alg._backup_modules()[0]
        ls = pt.policy(batch["obs2"])[:, act:].cpu()
        assert (ls < -3.0).any() and (ls > -0.5).any() and ((ls > -3.0) & (ls < -0.5)).any()
        if kind == "SAC":
            m = ref["q_targ"]
            assert (m[0] < m[1]).any() and (m[1] < m[0]).any()
        if kind == "DSAC":
            z = data["z_next"]
            assert (z > 3).any() and (z < -3).any() and (z.abs() < 3).any()
        assert (data["done"] == 1).any() and (data["done"] == 0).any()
        mean, std = torch.chunk(pt(batch["obs2"]).cpu().double(), 2, dim=-1)
        assert (mean + std * data["eps_next"].double()).abs().max() <= 3.0


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_soft_q_backup_fixed_alpha(name):
    alg = _alg(name, 3, 1, [32, 16], "relu", auto_alpha=False, alpha=0.3)
    _check_backup(alg, _data(70, 3, 1), f"{name} fixed alpha")


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_soft_q_backup_32_row_tiles(name):
    _check_backup(_alg(name, 4, 2, [64, 64], "elu"), _data(2054, 4, 2, seed=3), f"{name} [64, 64] B=2054")


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_soft_q_backup_64_row_tiles_eight_head_outputs_chunked_weights(name):
    _check_backup(_alg(name, 6, 4, [256, 256], "elu", seed=7), _data(16390, 6, 4, seed=3), f"{name} [256, 256] act 4 B=16390")


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_soft_q_backup_does_not_depend_on_the_tile_rows(name):
    """70 rows alone (16-row tiles) and as the first rows of a batch of 2054 (32-row tiles): the same bits."""
    alg = _alg(name, 4, 2, [64, 48], "tanh")
    big = _data(2054, 4, 2, seed=2)
    small = {k: v[:70].clone() for k, v in big.items()}
    a, b = _fused(alg, alg._batch(small)), _fused(alg, alg._batch(big))
    for k in OUT:
        rows = b[k][:, :70] if (k == "q_targ" and name == "SAC") else b[k][:70]
        assert torch.equal(a[k], rows), k


def test_soft_backup_and_soft_q_backup_share_one_policy_head():
    """One policy, obs2 and eps_next through `gops_soft_backup` and through `gops_soft_q_backup` (distri, one critic): the same bits of
    a2 and logp - both kernels run the one policy head of csrc/actor_critic.hip."""
    alg = _alg("DSAC", 4, 2, [64, 48], "tanh")
    batch = alg._batch(_data(70, 4, 2))
    got = _fused(alg, batch)
    pt, (q,) = alg._backup_modules()
    twin = hb.SoftBackup(pt.hip_mlp(), [q.hip_mlp(), q.hip_mlp()], act_low=pt.act_low_lim.cpu().numpy(), act_high=pt.act_high_lim.cpu().numpy(),
                         min_log_std=pt.min_log_std, max_log_std=pt.max_log_std, batch=70, log_alpha=alg.networks.log_alpha.data,
                         device=batch["obs2"].device)
    assert twin.supported
    z2 = torch.stack((batch["z_next"], batch["z_next"]))
    ref = twin.run(batch["obs2"], batch["rew"], batch["done"], batch["eps_next"], z2, gamma=alg.gamma, alpha=alg.alpha, want=("a2", "logp"))
    for k in ("a2", "logp"):
        assert torch.equal(got[k], ref[k]), k
    assert got["logp"].abs().max() > 0 and got["a2"].std() > 0


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_soft_q_backup_saturation(name):
    """Rows with |u| > 8: every output is finite and a2 is within the limits (no parity asked where fp32 cannot resolve the log)."""
    alg = _alg(name, 4, 2, [64, 48], "tanh")
    data = _data(70, 4, 2)
    pt = alg._backup_modules()[0]
    mean, std = torch.chunk(pt(data["obs2"].cuda()).cpu(), 2, dim=-1)
    data["eps_next"][:6] = (torch.tensor([[12.0, -12.0]] * 3 + [[-30.0, 30.0]] * 3) - mean[:6]) / std[:6]   # u = +-12, +-30
    batch = alg._batch(data)
    assert ((mean.cuda() + std.cuda() * batch["eps_next"])[:6].abs() > 8).all()
    got = _fused(alg, batch)
    for k in OUT:
        assert torch.isfinite(got[k]).all(), k
    assert (got["a2"] >= pt.act_low_lim).all() and (got["a2"] <= pt.act_high_lim).all()


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_optional_outputs_and_rows_beyond_the_batch(name):
    """Outputs padded with a sentinel: rows beyond the batch stay untouched; with the optional outputs NULL the backup keeps its bits."""
    B = 70
    alg = _alg(name, 4, 2, [64, 48], "tanh")
    batch = alg._batch(_data(B, 4, 2))
    got = ac.check_rows_beyond_the_batch(lambda out: _fused(alg, batch, out=out), dict(backup=B, a2=2 * B, logp=B, q_targ=2 * B))
    alone = _fused(alg, batch, want=())
    assert set(alone) == {"backup"} and torch.equal(alone["backup"], got["backup"])


def test_soft_q_backup_return_codes():
    """distri = 1 with n_q = 2 (gops_soft_backup's case) and a 272-wide layer: 0 workspace bytes, GOPS_ERR_UNSUPPORTED; a missing
    z_next, n_q = 3 and critics of the wrong output width: GOPS_ERR_BAD_ARG; a short workspace: GOPS_ERR_WORKSPACE."""
    data = _data(22, 3, 1)
    dsac = _alg("DSAC", 3, 1, [32], "relu")
    b = dsac._batch(data)
    args = (b["obs2"], b["rew"], b["done"], b["eps_next"])
    pt, q = dsac.networks.policy_target, dsac.networks.q_target
    mk = lambda critics, distri, **kw: hb.SoftQBackup(pt.hip_mlp(), critics, distri=distri, act_low=pt.act_low_lim.cpu().numpy(),   # noqa: E731
                                                      act_high=pt.act_high_lim.cpu().numpy(), min_log_std=-3.0, max_log_std=-0.5, batch=22, **kw)
    twin = mk([q.hip_mlp(), q.hip_mlp()], True)
    assert not twin.supported and hb.lib().gops_soft_q_backup_workspace_bytes(hb.C.byref(twin.desc), 22) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        twin.run(*args, b["z_next"])
    ok = mk([q.hip_mlp()], True)
    assert ok.supported
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        ok.run(*args, None)
    ok.run(*args, b["z_next"])
    scalar_on_distri = mk([q.hip_mlp()], False)   # a two-output critic where one output is described
    assert not scalar_on_distri.supported
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        scalar_on_distri.run(*args)
    ok.desc.n_q = 3
    assert hb.lib().gops_soft_q_backup_workspace_bytes(hb.C.byref(ok.desc), 22) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_BAD_ARG"):
        ok.run(*args, b["z_next"])
    small = mk([q.hip_mlp()], True, workspace_bytes=16)
    assert small.supported
    with pytest.raises(RuntimeError, match="GOPS_ERR_WORKSPACE"):
        small.run(*args, b["z_next"])
    wide = _alg("SAC", 3, 1, [272], "relu")
    sb = wide._soft_q_backup(22, b["obs"].device)
    assert not sb.supported and hb.lib().gops_soft_q_backup_workspace_bytes(hb.C.byref(sb.desc), 22) == 0
    with pytest.raises(RuntimeError, match="GOPS_ERR_UNSUPPORTED"):
        sb.run(*args)
    torch.cuda.synchronize()


def _critic_inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    qraw = torch.randn(B, 2, generator=g)
    if B > 4:
        qraw[1, 1], qraw[2, 1] = 25.0, -2.5   # beyond softplus' threshold, and a small std (0.079)
    return qraw, qraw[:, 0] + 3.0 * torch.randn(B, generator=g)


def _critic_ref(qraw, tq, bound):
    q, raw, tq, B = qraw[:, 0].double(), qraw[:, 1].double(), tq.double(), qraw.shape[0]
    sd = torch.nn.functional.softplus(raw)
    sig = torch.where(raw > 20, torch.ones_like(raw), torch.sigmoid(raw))
    td = (3 * sd.mean()).float().double()   # handed from the moments to the seeds as fp32
    e = tq - q
    eb = torch.clamp(e, -td, td) if bound else e
    terms = [e ** 2 / (2 * sd ** 2), eb ** 2 / (2 * sd ** 2), torch.log(sd)] if bound else [e ** 2 / (2 * sd ** 2), torch.log(sd) + 0.5 * np.log(2 * np.pi)]
    seed = torch.stack((-e / sd ** 2 / B, (1 / sd - eb ** 2 / sd ** 3) * sig / B), dim=-1)
    stats = [sum(terms).mean().item(), q.mean().item(), sd.mean().item(), td.item()]
    scale = [sum(t.abs() for t in terms).mean().item(), q.abs().mean().item(), sd.mean().item(), td.item()]
    return seed, stats, scale, e.abs() > td


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("B", [1, 70, 9000])
def test_dsac_critic_loss_against_float64(B, bound):
    """B = 9000: beyond one block - two launches of 64 blocks.  Called twice on different inputs (the scratch is left reusable), and
    again on the same: the same bits; rows beyond the batch keep the sentinel; the ticket is left zero."""
    cl = hb.DsacCriticLoss("cuda")
    for call in range(2):
        qraw, tq = _critic_inputs(B, seed=call)
        want, stats, scale, binds = _critic_ref(qraw, tq, bound)
        if B > 1:
            assert binds.any() and (~binds).any()
        seed = torch.full((2 * B + 64,), S, device="cuda")
        out, st = cl.run(qraw.cuda(), tq.cuda(), bound, seed=seed[:2 * B].view(B, 2))
        got_stats = st.cpu().double().tolist()
        assert (seed[2 * B:] == S).all()
        err = rel_l2(out.cpu(), want)
        print(f"B={B} bound={bound} call {call}: seeds rel-L2 {err:.3e}")
        assert err <= 4 * EPS32
        for i, (a, b) in enumerate(zip(got_stats, stats)):
            assert abs(a - b) <= 4 * EPS32 * max(abs(b), scale[i]) + 1e-30, (i, a, b)
        assert int(cl.buf[4 + 2 * 2 * 64:].view(torch.int32)[0].item()) == 0   # the ticket is left zero
        out2, st2 = cl.run(qraw.cuda(), tq.cuda(), bound)
        assert torch.equal(out, out2) and st2.cpu().double().tolist() == got_stats
    bad = torch.zeros(hb.DSAC_STATS_FLOATS + 1, device="cuda")
    q = torch.zeros(22, 2, device="cuda")
    assert hb.lib().gops_dsac_critic_loss(q.data_ptr(), q.data_ptr(), 22, 1, q.clone().data_ptr(), bad.data_ptr() + 4, None) == -1


def _loss_q(alg, tb):
    return float(tb["Loss/Critic loss-RL iter"]) if type(alg).__name__ == "SAC" else float(alg.loss_q)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", SAC_ONE_UPDATE)
def test_one_update_matches_the_reference(name, fused):
    alg, g, meta = load_alg(name, use_gpu=True, fused_target=fused)
    data, _, tb, info = ac.check_one_update(alg, g, meta, fused)
    assert {k for k in tb if not k.startswith("Time/")} == {k[3:] for k in g if k.startswith("tb/")}   # the reference's keys
    assert close(_loss_q(alg, tb), g["loss_q"]) and close(tb["Loss/Actor loss-RL iter"], g["loss_pi"])
    batch = alg._batch(data)
    res = _fused(alg, batch) if fused else dict(zip(OUT, alg._backup_composed(batch)))
    for k, key in (("backup", "backup"), ("a2", "a2"), ("logp", "logp_next"), ("q_targ", "q_targ")):
        assert rel_l2(res[k].cpu(), g[key]) < TOL, k
    ac.check_the_step_moves_everything(alg, info)


@pytest.mark.parametrize("name", ["sac_pend_relu", "sac_lqs4a2_gelu", "dsac_pend_relu_bound", "dsac_lqs4a2_gelu_nobound"])
def test_fused_and_composed_updates_agree(name):
    ac.check_fused_and_composed_agree(name, _check_backup)


@pytest.mark.parametrize("name", SAC_FIVE_UPDATES)
def test_five_updates_match_the_reference(name):
    """Five `local_update` calls with the reference's own draws handed in: every parameter and log_alpha after each call.  SAC steps
    everything every time; DSAC (delay_update = 2) keeps the bits of policy, log_alpha and both targets on iterations 1 and 3."""
    dsac = name.startswith("dsac")
    for alg, g, k, before in ac.five_updates(name, critic_loss=not dsac):   # (the reference's DSAC reports no critic loss)
        assert type(alg).__name__ == ("DSAC" if dsac else "SAC") and alg.tau == 0.05 and (not dsac or alg.delay_update == 2)
        for key, p in alg.networks.state_dict().items():
            if "lim" not in key:
                assert torch.equal(p, before[key]) == (dsac and ac.delayed(key) and k % 2 == 1), (k, key)


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_graph_replay_equals_eager(name, monkeypatch):
    ac.check_graph_replay(lambda: _alg(name, 3, 1, [32, 16], "relu", seed=4), 1 if name == "SAC" else 2, monkeypatch)


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_default_backup_path_and_shape_refusals(name):
    """Up to 64-wide: the one-launch backup; 256-wide: composed unless forced; a 272-wide layer falls back to composed."""
    data = _data(22, 3, 1)
    for hidden, over, want in (([64, 64], {}, "fused"), ([256, 256], {}, "composed"), ([256, 256], dict(fused_target="force"), "fused"),
                               ([64, 64], dict(fused_target=False), "composed"), ([272], {}, "composed"), ([272], dict(fused_target="force"), "composed")):
        alg = _alg(name, 3, 1, hidden, "relu", **over)
        alg.get_remote_update_info(data, 0)
        assert alg.backup_path == want, (hidden, over)


@pytest.mark.parametrize("name", ["SAC", "DSAC"])
def test_end_to_end(name, tmp_path):
    """OffSerialTrainer + replay_buffer + DeviceEnvSampler (the stochastic policy's own samples) on gym_pendulum: finite losses,
    every online network moved, the targets lag behind."""
    from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
    start = {}

    def sampler(model, alg):
        start.update({k: v.detach().clone() for k, v in alg.networks.state_dict().items()})
        smp = DeviceEnvSampler(dict(env_id="gym_pendulum"), model, n_envs=128, steps_per_sample=2, max_episode_steps=50, seed=3,
                               env_step="model")   # (gym_pendulum's data environment is not restated in the step kernel)
        smp.networks = alg.networks
        return smp

    kw = ac.trainer_kwargs(name, "gym_pendulum", 3, 2.0, tmp_path, policy_min_log_std=-20, policy_max_log_std=0.5, gamma=0.99, tau=0.005,
                           auto_alpha=True, bound=True, delay_update=2)
    alg, _, _, trainer = ac.build_trainer(kw, sampler, False)
    ac.run_trainer(trainer, alg)
    assert all(np.isfinite(float(v)) for v in alg.tb_info.values())
    nets = alg.networks.state_dict()
    assert all(torch.isfinite(p).all() for p in nets.values())
    for key, p in nets.items():
        if "lim" in key:
            continue
        assert not torch.equal(p, start[key]), key
        if "_target." in key:   # moved, but by less than its online twin
            online = nets[key.replace("_target", "")]
            assert (p - start[key]).abs().max() < (online - start[key]).abs().max(), key
