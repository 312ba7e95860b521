"""What the C entry points outside the rollout / value / MLP family refuse, and with which code - without a device: every call of
the table is refused by an argument check, before the library makes any HIP call.  Each entry point appears with a null pointer,
a batch / n below its minimum and one row per distinct check it makes itself; two-fault rows fix the order of checks.  The codes
are literals (GOPS_ERR_BAD_ARG -1, GOPS_ERR_UNSUPPORTED -2, GOPS_ERR_WORKSPACE -3; 0 from a size query: "no such workspace"),
recorded from the library as it stood when every one of these entry points was a trampoline in api.hip; the same table passes
against that library and against the one that defines each entry point beside its kernels."""
import ctypes as C
import json
import os

import pytest

from desc_helpers import BAD, ELU, ODD, UNS, WS, P, env_desc as _env, mlp_desc as _mlp, ptr_struct as _all_ptrs, struct as _struct

from gops_amd import hip_backend as hb

TANH = hb.ACT_IDS["tanh"]


def _grad(n=hb.MAX_LAYERS, weight0=P):
    g = hb.GopsMlpGrad()
    for j in range(n):
        g.weight[j] = g.bias[j] = P
    g.weight[0] = weight0
    return g


def _io(**null):
    return _all_ptrs(hb.GopsStepIO, **null)


def _poly_desc(**fields):
    d = hb.GopsRolloutDesc()
    d.batch, d.horizon, d.need_grad, d.gamma = 4, 2, 1, 1.0
    d.env = _env(hb.ENV_LQ, 2, 1)
    pol = _mlp([2, 1], act=hb.POLY_FULL[1])
    pol.sizes[2] = 2   # weight columns: the features of degree 1
    pol.bias[0] = 0
    d.policy = pol
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _poly_value(**fields):
    v = _mlp([2, 1], act=hb.POLY_SYM_2, **fields)
    v.sizes[2] = 3
    v.bias[0] = 0
    return v


def _tensors(n, **fields):
    t = hb.GopsAdamTensors()
    t.n = n
    for i in range(min(max(n, 0), hb.ADAM_MAX)):
        t.numel[i] = 8
        t.param[i] = t.grad[i] = t.exp_avg[i] = t.exp_avg_sq[i] = P
    for k, (i, v) in fields.items():
        getattr(t, k)[i] = v
    return t


def _lips(**fields):
    return _struct(hb.GopsLipsNet, mlp=_mlp([3, 16, 1], act=TANH), k_scalar=P, eps=1e-4, **fields)


def _ac(**fields):
    d = hb.GopsAcBackup()
    d.policy = _mlp([3, 16, 1])
    d.q[0] = d.q[1] = _mlp([4, 16, 1])
    d.n_q = 2
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _soft(cls=hb.GopsSoftBackup, q_out=2, **fields):
    d = cls()
    d.policy = _mlp([3, 16, 2])
    d.q[0] = d.q[1] = _mlp([4, 16, q_out])
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _soft_q(**fields):
    return _soft(hb.GopsSoftQBackup, 1, **{"n_q": 1, **fields})


def _dqn(**fields):
    return _struct(hb.GopsDqnBackup, q=_mlp([3, 16, 4]), **{"act_num": 4, **fields})


def _tg(act_dim=2):
    return _struct(hb.GopsTanhGauss, act_dim=act_dim, min_log_std=-20.0, max_log_std=0.5)


def _ppo(act_dim=2, norm=0):
    return _struct(hb.GopsPpoLoss, act_dim=act_dim, loss_value_norm=norm, min_log_std=-20.0, max_log_std=0.5)


def _table():
    """(label, entry point, arguments, code) - arguments as ctypes takes them: None is a null pointer."""
    ref = C.byref
    consts = (C.c_float * hb.RPI_CONST_COUNT)()
    rin, rout = _all_ptrs(hb.GopsRolloutIn), _all_ptrs(hb.GopsRolloutOut)
    eout = _all_ptrs(hb.GopsEpisodeOut)
    T = []

    def row(label, name, args, code):
        T.append(pytest.param(name, args, code, id=f"{name[5:]}-{label}"))

    # ---- rollout_poly.hip ----
    pd, pv = _poly_desc(), _poly_value()
    row("null", "gops_poly_rollout_workspace_bytes", (None,), 0)
    row("batch0", "gops_poly_rollout_workspace_bytes", (ref(_poly_desc(batch=0)),), 0)
    for i, what in enumerate(("desc", "in", "out")):
        args = [ref(pd), ref(rin), ref(rout), P, 1 << 20, None]
        args[i] = None
        row(f"null-{what}", "gops_poly_rollout_forward", tuple(args), BAD)
    row("batch0", "gops_poly_rollout_forward", (ref(_poly_desc(batch=0)), ref(rin), ref(rout), P, 1 << 20, None), BAD)
    row("null-obs", "gops_poly_rollout_forward", (ref(pd), ref(_all_ptrs(hb.GopsRolloutIn, obs=0)), ref(rout), P, 1 << 20, None), BAD)
    row("null-workspace", "gops_poly_rollout_forward", (ref(pd), ref(rin), ref(rout), None, 1 << 20, None), WS)
    pg = _grad()
    pg.bias[0] = 0
    for i, what in ((0, "desc"), (1, "in"), (3, "grad")):
        args = [ref(pd), ref(rin), P, ref(pg), P, 1 << 20, None]
        args[i] = None
        row(f"null-{what}", "gops_poly_rollout_backward", tuple(args), BAD)
    row("batch0", "gops_poly_rollout_backward", (ref(_poly_desc(batch=0)), ref(rin), P, ref(pg), P, 1 << 20, None), BAD)
    row("no-need-grad", "gops_poly_rollout_backward", (ref(_poly_desc(need_grad=0)), ref(rin), P, ref(pg), P, 1 << 20, None), BAD)
    row("null-workspace", "gops_poly_rollout_backward", (ref(pd), ref(rin), P, ref(pg), None, 1 << 20, None), WS)
    row("null", "gops_poly_value_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_poly_value_workspace_bytes", (ref(pv), 0), 0)
    row("null", "gops_poly_value_forward", (None, 4, P, P, None), BAD)
    row("batch0", "gops_poly_value_forward", (ref(pv), 0, P, P, None), BAD)
    row("null-obs", "gops_poly_value_forward", (ref(pv), 4, None, P, None), BAD)
    row("null-value", "gops_poly_value_backward", (None, 4, P, P, ref(pg), P, 1 << 20, None), BAD)
    row("null-grad", "gops_poly_value_backward", (ref(pv), 4, P, P, None, P, 1 << 20, None), BAD)
    row("batch0", "gops_poly_value_backward", (ref(pv), 0, P, P, ref(pg), P, 1 << 20, None), BAD)
    row("null-workspace", "gops_poly_value_backward", (ref(pv), 4, P, P, ref(pg), None, 1 << 20, None), WS)

    # ---- rollout_rpi.hip ----
    osc = hb.RPI_ENV_OSCILLATOR
    row("kind0", "gops_rpi_state_bytes", (0, 4), 0)
    row("batch0", "gops_rpi_state_bytes", (osc, 0), 0)
    rpi = lambda kind=osc, B=4, steps=8, c=consts, w=P, state_bytes=1 << 20: (
        kind, B, steps, c, w, P, P, P, P, state_bytes, 1e-3, 0.9, 0.999, 1e-8, P, None, None)
    row("kind0", "gops_rpi_evaluate", rpi(kind=0), UNS)
    row("batch0", "gops_rpi_evaluate", rpi(B=0), BAD)
    row("batch-above-max", "gops_rpi_evaluate", rpi(B=hb.RPI_MAX_BATCH + 1), UNS)
    row("steps0", "gops_rpi_evaluate", rpi(steps=0), BAD)
    row("null-consts", "gops_rpi_evaluate", rpi(c=None), BAD)
    row("null-weights", "gops_rpi_evaluate", rpi(w=None), BAD)
    row("small-state", "gops_rpi_evaluate", rpi(state_bytes=16), WS)

    # ---- rollout_rpi_mlp.hip ----
    rv = _mlp([2, 16, 1])
    row("null", "gops_rpi_mlp_state_bytes", (osc, 4, None), 0)
    row("batch0", "gops_rpi_mlp_state_bytes", (osc, 0, ref(rv)), 0)
    rpm = lambda kind=osc, B=4, steps=8, c=consts, v=ref(rv), t=ref(rv), state_bytes=1 << 20: (
        kind, B, steps, c, v, t, P, P, P, state_bytes, 1e-3, 0.9, 0.999, 1e-8, P, None, None)
    row("null-value", "gops_rpi_mlp_evaluate", rpm(v=None), BAD)
    row("null-target", "gops_rpi_mlp_evaluate", rpm(t=None), BAD)
    row("kind0", "gops_rpi_mlp_evaluate", rpm(kind=0), UNS)
    row("batch0", "gops_rpi_mlp_evaluate", rpm(B=0), BAD)
    row("null-consts", "gops_rpi_mlp_evaluate", rpm(c=None), BAD)
    row("null-weight", "gops_rpi_mlp_evaluate", rpm(v=ref(_mlp([2, 16, 1], ptr=0))), BAD)
    row("small-state", "gops_rpi_mlp_evaluate", rpm(state_bytes=16), WS)

    # ---- rollout_lips.hip ----
    ln, lg = _lips(), _struct(hb.GopsLipsGrad, mlp=_grad(), k_net=_grad(), k_scalar=P)
    row("null", "gops_lips_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_lips_workspace_bytes", (ref(ln), 0), 0)
    row("null-net", "gops_lips_forward", (None, 4, P, P, None, None, P, 1 << 20, None), BAD)
    row("batch0", "gops_lips_forward", (ref(ln), 0, P, P, None, None, P, 1 << 20, None), BAD)
    row("null-obs", "gops_lips_forward", (ref(ln), 4, None, P, None, None, P, 1 << 20, None), BAD)
    row("null-workspace", "gops_lips_forward", (ref(ln), 4, P, P, None, None, None, 1 << 20, None), WS)
    row("null-net", "gops_lips_backward", (None, 4, P, P, ref(lg), P, 1 << 20, None), BAD)
    row("null-grad", "gops_lips_backward", (ref(ln), 4, P, P, None, P, 1 << 20, None), BAD)
    row("batch0", "gops_lips_backward", (ref(ln), 0, P, P, ref(lg), P, 1 << 20, None), BAD)
    row("null-k-scalar-grad", "gops_lips_backward",
        (ref(ln), 4, P, P, ref(_struct(hb.GopsLipsGrad, mlp=_grad(), k_net=_grad())), P, 1 << 20, None), BAD)
    row("null-workspace", "gops_lips_backward", (ref(ln), 4, P, P, ref(lg), None, 1 << 20, None), WS)

    # ---- rollout_episode.hip ----
    ee, ep = _env(hb.ENV_LQ, 2, 1, data_env=1), _mlp([2, 16, 1])
    row("null-env", "gops_episode_workspace_bytes", (None, ref(ep), 4, 8), 0)
    row("episodes0", "gops_episode_workspace_bytes", (ref(ee), ref(ep), 0, 8), 0)
    epi = lambda env=ref(ee), pol=ref(ep), E=4, init=ref(_io()), out=ref(eout), ws=P: (env, pol, E, 8, init, out, ws, 1 << 20, None)
    row("null-env", "gops_episode_rollout", epi(env=None), BAD)
    row("null-policy", "gops_episode_rollout", epi(pol=None), BAD)
    row("episodes0", "gops_episode_rollout", epi(E=0), BAD)
    row("model-env", "gops_episode_rollout", epi(env=ref(_env(hb.ENV_LQ, 2, 1))), BAD)
    row("mobilerobot", "gops_episode_rollout", epi(env=ref(_env(hb.ENV_MOBILEROBOT, 13, 2, data_env=1))), UNS)
    row("null-init", "gops_episode_rollout", epi(init=None), BAD)
    row("null-init-state", "gops_episode_rollout",
        epi(env=ref(_env(hb.ENV_VEH2DOF, 6, 1, pre_horizon=2, data_env=1)), pol=ref(_mlp([6, 16, 1])), init=ref(_io(state=0))), BAD)
    row("null-workspace", "gops_episode_rollout", epi(ws=None), WS)

    # ---- actor_critic.hip ----
    ac = lambda d=ref(_ac()), B=4, obs2=P, ws=P: (d, B, obs2, P, P, P, P, None, None, ws, 1 << 20, None)
    row("null", "gops_ac_backup_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_ac_backup_workspace_bytes", (ref(_ac()), 0), 0)
    row("null-desc", "gops_ac_backup", ac(d=None), BAD)
    row("batch0", "gops_ac_backup", ac(B=0), BAD)
    row("n_q0", "gops_ac_backup", ac(d=ref(_ac(n_q=0))), BAD)
    row("poly-policy", "gops_ac_backup", ac(d=ref(_ac(policy=_mlp([3, 1])))), UNS)
    row("null-obs2", "gops_ac_backup", ac(obs2=None), BAD)
    row("smooth-null-xi", "gops_ac_backup", (ref(_ac(smooth=1)), 4, P, P, P, None, P, None, None, P, 1 << 20, None), BAD)
    row("null-workspace", "gops_ac_backup", ac(ws=None), WS)
    acl = lambda q=P, n_q=2, B=4, stats=P: (q, P, None, n_q, B, P, None, stats, None)
    row("null-q", "gops_ac_critic_loss", acl(q=None), BAD)
    row("batch0", "gops_ac_critic_loss", acl(B=0), BAD)
    row("n_q0", "gops_ac_critic_loss", acl(n_q=0), BAD)
    row("n_q3", "gops_ac_critic_loss", acl(n_q=3), BAD)
    row("null-stats", "gops_ac_critic_loss", acl(stats=None), BAD)
    row("misaligned-stats", "gops_ac_critic_loss", acl(stats=ODD), BAD)
    dq = lambda d=ref(_dqn()), B=4, obs2=P, ws=P: (d, B, obs2, P, P, P, None, None, ws, 1 << 20, None)
    row("null", "gops_dqn_backup_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_dqn_backup_workspace_bytes", (ref(_dqn()), 0), 0)
    row("null-desc", "gops_dqn_backup", dq(d=None), BAD)
    row("batch0", "gops_dqn_backup", dq(B=0), BAD)
    row("act_num0", "gops_dqn_backup", dq(d=ref(_dqn(act_num=0))), BAD)
    row("act_num1", "gops_dqn_backup", dq(d=ref(_dqn(act_num=1))), UNS)
    row("null-obs2", "gops_dqn_backup", dq(obs2=None), BAD)
    row("null-workspace", "gops_dqn_backup", dq(ws=None), WS)
    dql = lambda q=P, N=4, B=4, stats=P: (q, P, P, None, N, B, P, None, stats, None)
    row("null-q", "gops_dqn_loss", dql(q=None), BAD)
    row("batch0", "gops_dqn_loss", dql(B=0), BAD)
    row("act_num0", "gops_dqn_loss", dql(N=0), BAD)
    row("misaligned-stats", "gops_dqn_loss", dql(stats=ODD), BAD)
    sb = lambda d=ref(_soft()), B=4, obs2=P, ws=P: (d, B, obs2, P, P, P, P, P, P, None, None, None, ws, 1 << 20, None)
    row("null", "gops_soft_backup_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_soft_backup_workspace_bytes", (ref(_soft()), 0), 0)
    row("null-desc", "gops_soft_backup", sb(d=None), BAD)
    row("batch0", "gops_soft_backup", sb(B=0), BAD)
    row("odd-policy-head", "gops_soft_backup", sb(d=ref(_soft(policy=_mlp([3, 16, 3])))), BAD)
    row("null-obs2", "gops_soft_backup", sb(obs2=None), BAD)
    row("null-workspace", "gops_soft_backup", sb(ws=None), WS)
    sq = lambda d=ref(_soft_q()), B=4, obs2=P, ws=P: (d, B, obs2, P, P, P, None, P, None, None, None, ws, 1 << 20, None)
    row("null", "gops_soft_q_backup_workspace_bytes", (None, 4), 0)
    row("batch0", "gops_soft_q_backup_workspace_bytes", (ref(_soft_q()), 0), 0)
    row("null-desc", "gops_soft_q_backup", sq(d=None), BAD)
    row("batch0", "gops_soft_q_backup", sq(B=0), BAD)
    row("n_q0", "gops_soft_q_backup", sq(d=ref(_soft_q(n_q=0))), BAD)
    row("distri-twin", "gops_soft_q_backup", sq(d=ref(_soft_q(n_q=2, distri=1))), UNS)
    row("distri-null-z", "gops_soft_q_backup", sq(d=ref(_soft(hb.GopsSoftQBackup, 2, n_q=1, distri=1))), BAD)
    row("null-obs2", "gops_soft_q_backup", sq(obs2=None), BAD)
    row("null-workspace", "gops_soft_q_backup", sq(ws=None), WS)

    # ---- dsact.hip ----
    dst = lambda q=P, B=4, state=P, stats=P: (q, P, P, B, 0.005, state, P, stats, None)
    row("null-q", "gops_dsact_critic_loss", dst(q=None), BAD)
    row("null-state", "gops_dsact_critic_loss", dst(state=None), BAD)
    row("batch0", "gops_dsact_critic_loss", dst(B=0), BAD)
    row("misaligned-stats", "gops_dsact_critic_loss", dst(stats=ODD), BAD)
    dsc = lambda q=P, B=4, stats=P: (q, P, B, 1, P, stats, None)
    row("null-q", "gops_dsac_critic_loss", dsc(q=None), BAD)
    row("batch0", "gops_dsac_critic_loss", dsc(B=0), BAD)
    row("misaligned-stats", "gops_dsac_critic_loss", dsc(stats=ODD), BAD)
    tgf = lambda d=ref(_tg()), B=4, head=P, stats=P: (d, B, head, P, -2.0, P, P, stats, None)
    tgb = lambda d=ref(_tg()), B=4, head=P: (d, B, head, P, P, P, P, None)
    for name, call in (("gops_tanh_gauss_forward", tgf), ("gops_tanh_gauss_backward", tgb)):
        row("null-desc", name, call(d=None), BAD)
        row("batch0", name, call(B=0), BAD)
        row("act_dim0", name, call(d=ref(_tg(0))), BAD)
        row("act_dim-above-max", name, call(d=ref(_tg(hb.MAX_ACT + 1))), BAD)
        row("null-head", name, call(head=None), BAD)
    row("misaligned-stats", "gops_tanh_gauss_forward", tgf(stats=ODD), BAD)

    # ---- ppo.hip ----
    ppo = lambda d=ref(_ppo()), M=4, head=P, stats=P: (d, M, head, P, P, P, P, P, P, P, P, P, P, stats, None)
    row("null-desc", "gops_ppo_loss", ppo(d=None), BAD)
    row("batch0", "gops_ppo_loss", ppo(M=0), BAD)
    row("act_dim0", "gops_ppo_loss", ppo(d=ref(_ppo(0))), BAD)
    row("act_dim-above-max", "gops_ppo_loss", ppo(d=ref(_ppo(hb.MAX_ACT + 1))), BAD)
    row("null-head_new", "gops_ppo_loss", ppo(head=None), BAD)
    row("value-norm-batch1", "gops_ppo_loss", ppo(d=ref(_ppo(norm=1)), M=1), BAD)
    row("misaligned-stats", "gops_ppo_loss", ppo(stats=ODD), BAD)
    row("act_dim0-and-null-head_new", "gops_ppo_loss", ppo(d=ref(_ppo(0)), head=None), BAD)
    adv = lambda a=P, n=4, stats=P: (a, n, 1e-8, P, stats, None)
    row("null-adv", "gops_adv_normalize", adv(a=None), BAD)
    row("n0", "gops_adv_normalize", adv(n=0), BAD)
    row("n1", "gops_adv_normalize", adv(n=1), BAD)
    row("misaligned-stats", "gops_adv_normalize", adv(stats=ODD), BAD)
    gae = lambda rew=P, T_=4, N=2: (rew, P, P, P, P, T_, N, 0.99, 0.95, P, P, None)
    row("null-rew", "gops_gae", gae(rew=None), BAD)
    row("steps0", "gops_gae", gae(T_=0), BAD)
    row("envs0", "gops_gae", gae(N=0), BAD)

    # ---- trpo.hip ----
    fpol = _mlp([3, 16, 4])
    fs = lambda m=ref(fpol), g=ref(_grad()), B=4, x=P: (m, g, B, x, -20.0, 0.5, P, None)
    row("null-policy", "gops_gauss_fisher_seed", fs(m=None), BAD)
    row("null-tangent", "gops_gauss_fisher_seed", fs(g=None), BAD)
    row("null-x", "gops_gauss_fisher_seed", fs(x=None), BAD)
    row("batch0", "gops_gauss_fisher_seed", fs(B=0), BAD)
    row("n_layers0", "gops_gauss_fisher_seed", fs(m=ref(_mlp([3, 16, 4], n_layers=0))), BAD)
    row("n_layers-above-max", "gops_gauss_fisher_seed", fs(m=ref(_mlp([3, 16, 4], n_layers=hb.MAX_LAYERS + 1))), BAD)
    row("n_layers0-and-null-x", "gops_gauss_fisher_seed", fs(m=ref(_mlp([3, 16, 4], n_layers=0)), x=None), BAD)
    row("odd-head", "gops_gauss_fisher_seed", fs(m=ref(_mlp([3, 16, 3]))), BAD)
    row("wide-obs", "gops_gauss_fisher_seed", fs(m=ref(_mlp([65, 16, 4]))), UNS)
    row("poly-policy", "gops_gauss_fisher_seed", fs(m=ref(_mlp([3, 4]))), UNS)
    row("null-tangent-weight", "gops_gauss_fisher_seed", fs(g=ref(_grad(weight0=0))), BAD)
    sur = lambda A=2, M=4, head=P, stats=P: (A, M, -20.0, 0.5, head, P, P, P, P, None, stats, None)
    row("batch0", "gops_trpo_surrogate", sur(M=0), BAD)
    row("act_dim0", "gops_trpo_surrogate", sur(A=0), BAD)
    row("act_dim-above-max", "gops_trpo_surrogate", sur(A=hb.MAX_ACT + 1), BAD)
    row("null-head_new", "gops_trpo_surrogate", sur(head=None), BAD)
    row("null-stats", "gops_trpo_surrogate", sur(stats=None), BAD)
    row("misaligned-stats", "gops_trpo_surrogate", sur(stats=ODD), BAD)
    cgs = {"gops_cg_init": lambda g=P, n=4, st=P: (g, P, P, P, n, 1e-10, st, None),
           "gops_cg_step": lambda g=P, n=4, st=P: (g, P, P, P, n, 0.1, 1e-10, st, None),
           "gops_cg_finish": lambda g=P, n=4, st=P: (g, P, P, n, P, st, None)}
    for name, call in cgs.items():
        row("null-vector", name, call(g=None), BAD)
        row("n0", name, call(n=0), BAD)
        row("null-state", name, call(st=None), BAD)
        row("misaligned-state", name, call(st=ODD), BAD)

    # ---- optim.hip ----
    adam = lambda t=ref(_tensors(2)), st=P: (t, st, 0.9, 0.999, 1e-8, None)
    row("null-tensors", "gops_adam_step", adam(t=None), BAD)
    row("null-state", "gops_adam_step", adam(st=None), BAD)
    row("n0", "gops_adam_step", adam(t=ref(_tensors(0))), BAD)
    row("n-above-max", "gops_adam_step", adam(t=ref(_tensors(hb.ADAM_MAX + 1))), BAD)
    row("null-moment", "gops_adam_step", adam(t=ref(_tensors(2, exp_avg_sq=(1, 0)))), BAD)
    row("numel0", "gops_adam_step", adam(t=ref(_tensors(2, numel=(1, 0)))), BAD)
    row("null-tensors", "gops_polyak_update", (None, 0.005, None), BAD)
    row("n0", "gops_polyak_update", (ref(_tensors(0)), 0.005, None), BAD)
    row("n-above-max", "gops_polyak_update", (ref(_tensors(hb.ADAM_MAX + 1)), 0.005, None), BAD)
    row("null-online", "gops_polyak_update", (ref(_tensors(2, grad=(1, 0))), 0.005, None), BAD)
    row("null-v", "gops_value_loss", (None, P, 4, None, P, None), BAD)
    row("null-stats", "gops_value_loss", (P, P, 4, None, None, None), BAD)
    row("n0", "gops_value_loss", (P, P, 0, None, P, None), BAD)
    row("null-x", "gops_mean_loss", (None, 4, 1.0, P, None), BAD)
    row("n0", "gops_mean_loss", (P, 0, 1.0, P, None), BAD)

    # ---- aux_kernels.hip ----
    step = lambda env, io=None, B=4: (ref(env) if env is not None else None, B, ref(io if io is not None else _io()), None)
    lq = _env(hb.ENV_LQ, 2, 1)
    mob = lambda **f: _env(hb.ENV_MOBILEROBOT, **{"obs_dim": 13, "act_dim": 2, "n_constraint": 1, **f})
    surr = lambda **f: _env(hb.ENV_VEH_SURR, 14, 2, **{"pre_horizon": 1, "n_surr": 1, "n_constraint": 1, **f})
    veh = lambda **f: _env(hb.ENV_VEH, 10, 2, pre_horizon=1, **f)
    row("null-env", "gops_env_step", step(None), BAD)
    row("null-io", "gops_env_step", (ref(lq), 4, None, None), BAD)
    row("batch0", "gops_env_step", step(lq, B=0), BAD)
    row("kind-none", "gops_env_step", step(_env(hb.ENV_NONE, 2, 1)), BAD)
    row("kind-above-max", "gops_env_step", step(_env(hb.ENV_MOBILEROBOT + 1, 2, 1)), BAD)
    row("mobilerobot-obs_dim", "gops_env_step", step(mob(obs_dim=12)), BAD)
    row("mobilerobot-act_dim", "gops_env_step", step(mob(act_dim=1)), BAD)
    row("mobilerobot-n_constraint", "gops_env_step", step(mob(n_constraint=0)), BAD)
    row("mobilerobot-scale_obs", "gops_env_step", step(mob(scale_obs=1)), BAD)
    row("mobilerobot-null-constraint", "gops_env_step", step(mob(), _io(constraint=0)), BAD)
    row("data-env-pendulum", "gops_env_step", step(_env(hb.ENV_PENDULUM, 3, 1, data_env=1)), UNS)
    row("data-env-veh2dof-errcstr", "gops_env_step", step(_env(hb.ENV_VEH2DOF, 6, 1, pre_horizon=2, data_env=1, cstr_err=1, n_constraint=1)), UNS)
    row("data-env-pendulum-and-null-obs", "gops_env_step", step(_env(hb.ENV_PENDULUM, 3, 1, data_env=1), _io(obs=0)), UNS)
    for k in ("obs", "action", "next_obs", "reward", "next_done"):
        row(f"null-{k}", "gops_env_step", step(lq, _io(**{k: 0})), BAD)
    row("surr-data-env", "gops_env_step", step(surr(data_env=1)), BAD)
    row("surr-n_surr0", "gops_env_step", step(surr(n_surr=0)), BAD)
    row("surr-n_surr-above-max", "gops_env_step", step(surr(n_surr=hb.MAX_SURR + 1)), BAD)
    row("surr-n_constraint2", "gops_env_step", step(surr(n_constraint=2)), BAD)
    row("surr-errcstr-n_surr1", "gops_env_step", step(surr(cstr_err=1, n_constraint=2)), BAD)
    row("surr-errcstr-n_constraint1", "gops_env_step", step(surr(cstr_err=1, n_surr=0, n_constraint=1)), BAD)
    row("surr-null-surr_state", "gops_env_step", step(surr(), _io(surr_state=0)), BAD)
    row("surr-null-next_surr_state", "gops_env_step", step(surr(), _io(next_surr_state=0)), BAD)
    row("surr-null-constraint", "gops_env_step", step(surr(), _io(constraint=0)), BAD)
    for k in ("state", "ref_points", "path_num", "u_num", "ref_time", "next_state", "next_ref_points", "next_ref_time"):
        row(f"ref-table-null-{k}", "gops_env_step", step(veh(), _io(**{k: 0})), BAD)
    row("veh2dof-null-state", "gops_env_step", step(_env(hb.ENV_VEH2DOF, 6, 1, pre_horizon=2), _io(state=0)), BAD)
    row("lq-wide", "gops_env_step", step(_env(hb.ENV_LQ, hb.MAX_LQ + 1, 1)), UNS)
    row("scale_obs-veh", "gops_env_step", step(veh(scale_obs=1)), UNS)
    row("repeat-negative", "gops_env_step", step(_env(hb.ENV_LQ, 2, 1, repeat_num=-1)), BAD)
    row("repeat-above-max", "gops_env_step", step(_env(hb.ENV_LQ, 2, 1, repeat_num=hb.MAX_REPEAT + 1)), BAD)
    row("repeat-veh", "gops_env_step", step(veh(repeat_num=2)), UNS)
    row("repeat-data-env", "gops_env_step", step(_env(hb.ENV_LQ, 2, 1, repeat_num=2, data_env=1)), UNS)
    row("scale_obs-veh-and-repeat-above-max", "gops_env_step", step(veh(scale_obs=1, repeat_num=hb.MAX_REPEAT + 1)), UNS)
    v2e = lambda **f: _env(hb.ENV_VEH2DOF, 6, 1, **{"pre_horizon": 2, "cstr_err": 1, "n_constraint": 1, **f})
    row("null-env", "gops_env_constraint", step(None), BAD)
    row("null-io", "gops_env_constraint", (ref(surr()), 4, None, None), BAD)
    row("batch0", "gops_env_constraint", step(surr(), B=0), BAD)
    row("null-constraint", "gops_env_constraint", step(surr(), _io(constraint=0)), BAD)
    row("no-constraint-model", "gops_env_constraint", step(lq), UNS)
    row("veh2dof-no-errcstr", "gops_env_constraint", step(v2e(cstr_err=0)), UNS)
    row("errcstr-null-obs", "gops_env_constraint", step(v2e(), _io(obs=0)), BAD)
    row("errcstr-veh2dof-n_constraint2", "gops_env_constraint", step(v2e(n_constraint=2)), BAD)
    row("errcstr-veh3dof-n_constraint1", "gops_env_constraint", step(surr(cstr_err=1, n_surr=0, n_constraint=1)), BAD)
    row("surr-null-state", "gops_env_constraint", step(surr(), _io(state=0)), BAD)
    row("surr-null-surr_state", "gops_env_constraint", step(surr(), _io(surr_state=0)), BAD)
    row("surr-n_surr0", "gops_env_constraint", step(surr(n_surr=0)), BAD)
    row("surr-n_surr-above-max", "gops_env_constraint", step(surr(n_surr=hb.MAX_SURR + 1)), BAD)
    row("surr-n_constraint2", "gops_env_constraint", step(surr(n_constraint=2)), BAD)
    return T


MOVED = """gops_poly_rollout_workspace_bytes gops_poly_rollout_forward gops_poly_rollout_backward gops_poly_value_workspace_bytes
gops_poly_value_forward gops_poly_value_backward gops_rpi_state_bytes gops_rpi_evaluate gops_rpi_mlp_state_bytes gops_rpi_mlp_evaluate
gops_lips_workspace_bytes gops_lips_forward gops_lips_backward gops_episode_workspace_bytes gops_episode_rollout
gops_ac_backup_workspace_bytes gops_ac_backup gops_ac_critic_loss gops_dqn_backup_workspace_bytes gops_dqn_backup gops_dqn_loss
gops_soft_backup_workspace_bytes gops_soft_backup gops_soft_q_backup_workspace_bytes gops_soft_q_backup gops_dsact_critic_loss
gops_dsac_critic_loss gops_tanh_gauss_forward gops_tanh_gauss_backward gops_ppo_loss gops_adv_normalize gops_gae
gops_gauss_fisher_seed gops_trpo_surrogate gops_cg_init gops_cg_step gops_cg_finish gops_adam_step gops_polyak_update gops_value_loss
gops_mean_loss gops_env_step gops_env_constraint""".split()

TABLE = _table()


@pytest.mark.parametrize("name, args, code", TABLE)
def test_refusal_code(name, args, code):
    assert code <= 0   # a row that is not a refusal would launch
    assert getattr(hb.lib(), name)(*args) == code


def test_table_covers_every_entry_point_beside_its_kernels():
    """Each of them with a null pointer and a batch / n below its minimum at least; and none of api.hip's own family."""
    rows = {}
    for p in TABLE:
        rows.setdefault(p.values[0], []).append(p.id)
    assert sorted(rows) == sorted(MOVED)
    assert set(MOVED) <= set(hb.EXPORTED_SYMBOLS)
    for name, ids in rows.items():
        assert any("null" in i for i in ids) or name in ("gops_rpi_state_bytes",), name   # (two integers: no pointer to leave out)
        assert any(k in i for i in ids for k in ("batch0", "-n0", "episodes0", "steps0")), name


# ---- the closed-loop pair: rollout_sample.hip and rollout_episode.hip share one admission check ----------------------------------
# Every single fault that check names, and every pair of a GOPS_ERR_UNSUPPORTED fault with a GOPS_ERR_BAD_ARG fault (the pairs fix the
# order of the tests), through the four entry points and the four workspace queries.  A fault is a set of knobs over one valid base
# description (gym_cartpoleconti as a data env, a 4-16-A net); the workspace pointer is null, so a description that passes every
# check is refused with GOPS_ERR_WORKSPACE before any HIP call.  The codes (the bytes, for a query) were recorded from the library
# as it stood when each kernel had a check of its own: tests/golden/closed_loop_refusals.json (`PYTHONPATH=. python
# tests/test_refusals_cpu.py` rewrites it from the library that is loaded).
CLOSED_LOOP_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "closed_loop_refusals.json")
CLOSED_LOOP_ENTRIES = {   # entry point: (the entry point whose single-fault codes choose its pairs, takes an action table)
    "gops_sample_workspace_bytes": ("gops_sample_rollout", False), "gops_sample_dis_workspace_bytes": ("gops_sample_rollout_dis", True),
    "gops_episode_workspace_bytes": ("gops_episode_rollout", False), "gops_episode_dis_workspace_bytes": ("gops_episode_rollout_dis", True),
    "gops_sample_rollout": ("gops_sample_rollout", False), "gops_sample_rollout_dis": ("gops_sample_rollout_dis", True),
    "gops_episode_rollout": ("gops_episode_rollout", False), "gops_episode_rollout_dis": ("gops_episode_rollout_dis", True)}
_BASE = dict(kind=hb.ENV_CARTPOLE, O=4, A=1, P=0, data_env=1, cstr_err=0, repeat_num=0, scale_obs=0, in_delta=0, hidden=(16,), out="base",
             n_layers=None, dtype=0, hidden_act=ELU, null_weight=None, null_bias=None, act_num=3, head=None, eps=0.25, table=P, N=4, T=2)


def _env_knobs(kind, O, A, P=0, **more):
    return dict(kind=kind, O=O, A=A, P=P, **more)


CLOSED_LOOP_FAULTS = {
    "none": {},
    "envs0": dict(N=0), "steps0": dict(T=0),
    # each kind neither kernel steps; a model kind as a data env and the reverse
    "kind-none": _env_knobs(hb.ENV_NONE, 4, 1), "kind-veh-surr": _env_knobs(hb.ENV_VEH_SURR, 14, 2, 1),
    "kind-mobilerobot": _env_knobs(hb.ENV_MOBILEROBOT, 13, 2), "kind-above-max": _env_knobs(hb.ENV_MOUNTAINCAR + 1, 4, 1),
    "pendulum-data-env": _env_knobs(hb.ENV_PENDULUM, 3, 1), "mountaincar-data-env": _env_knobs(hb.ENV_MOUNTAINCAR, 2, 1),
    "pendulum-model": _env_knobs(hb.ENV_PENDULUM, 3, 1, data_env=0), "mountaincar-model": _env_knobs(hb.ENV_MOUNTAINCAR, 2, 1, data_env=0),
    "cartpole-model": dict(data_env=0), "lq-model": _env_knobs(hb.ENV_LQ, 2, 1, data_env=0),
    "cstr_err": dict(cstr_err=1), "repeat2": dict(repeat_num=2),
    "one-layer": dict(hidden=()), "fp16": dict(dtype=1),
    "act_dim0": dict(A=0), "act_dim-above-max": dict(A=hb.MAX_ACT + 1), "obs_dim0": dict(O=0),
    "lq-wide": _env_knobs(hb.ENV_LQ, hb.MAX_LQ + 1, 1),
    # the per-kind shape table
    "idp-obs": _env_knobs(hb.ENV_IDP, 5, 1), "idp-act": _env_knobs(hb.ENV_IDP, 6, 2),
    "cartpole-obs": dict(O=5), "cartpole-act": dict(A=2),
    "pendulum-obs": _env_knobs(hb.ENV_PENDULUM, 4, 1, data_env=0), "pendulum-act": _env_knobs(hb.ENV_PENDULUM, 3, 2, data_env=0),
    "mountaincar-obs": _env_knobs(hb.ENV_MOUNTAINCAR, 3, 1, data_env=0), "mountaincar-act": _env_knobs(hb.ENV_MOUNTAINCAR, 2, 2, data_env=0),
    "veh-horizon0": _env_knobs(hb.ENV_VEH, 6, 2, 0), "veh-obs": _env_knobs(hb.ENV_VEH, 13, 2, 2), "veh-act": _env_knobs(hb.ENV_VEH, 14, 1, 2),
    "veh2dof-horizon0": _env_knobs(hb.ENV_VEH2DOF, 4, 1, 0), "veh2dof-obs": _env_knobs(hb.ENV_VEH2DOF, 7, 1, 2),
    "veh2dof-act": _env_knobs(hb.ENV_VEH2DOF, 6, 2, 2),
    "scale_obs-veh": _env_knobs(hb.ENV_VEH, 14, 2, 2, scale_obs=1), "scale_obs-veh2dof": _env_knobs(hb.ENV_VEH2DOF, 6, 1, 2, scale_obs=1),
    "scale_obs-wide": _env_knobs(hb.ENV_LQ, 9, 1, scale_obs=1), "scale_obs-cartpole": dict(scale_obs=1),
    "layers0": dict(n_layers=0), "layers-above-max": dict(hidden=(16,) * (hb.MAX_LAYERS - 1), n_layers=hb.MAX_LAYERS + 1),
    "time-input": dict(in_delta=1), "input-width": dict(in_delta=2),
    # output widths: base is A (act_num with a table); the Gaussian heads want 2A, the deterministic one A
    "output-plus1": dict(out="plus1"), "output-double": dict(out="double"), "output-3": dict(out=3),
    "gauss-width-A": dict(head=hb.SAMPLE_GAUSS), "gauss-width-2A": dict(head=hb.SAMPLE_GAUSS, out="double"),
    "gauss-odd-width": _env_knobs(hb.ENV_VEH, 14, 2, 2, head=hb.SAMPLE_TANH_GAUSS, out=3),
    "head-above-max": dict(head=7), "head-negative": dict(head=-1),
    "hidden-24": dict(hidden=(24,)), "hidden-8": dict(hidden=(8,)), "hidden-second-40": dict(hidden=(16, 40)),
    "activation-above-max": dict(hidden_act=TANH + 1), "activation-negative": dict(hidden_act=-1), "activation-poly": dict(hidden_act=hb.POLY_FULL[2]),
    "null-weight": dict(null_weight=0), "null-bias": dict(null_bias=1),
    "act_num1": dict(act_num=1), "act_num-above-max": dict(act_num=hb.DQN_MAX_ACTIONS + 1), "act_num0": dict(act_num=0),
    "epsilon-nan": dict(eps=float("nan")), "epsilon-negative": dict(eps=-0.01), "epsilon-above-1": dict(eps=1.01),
    "epsilon-categorical": dict(head=hb.SAMPLE_CATEGORICAL), "categorical": dict(head=hb.SAMPLE_CATEGORICAL, eps=0.0),
    "null-table": dict(table=None),
}


def _closed_loop_call(name, knobs):
    k = {**_BASE, **knobs}
    dis = CLOSED_LOOP_ENTRIES[name][1]
    env = _env(k["kind"], k["O"], k["A"], pre_horizon=k["P"], data_env=k["data_env"], cstr_err=k["cstr_err"], repeat_num=k["repeat_num"],
               scale_obs=k["scale_obs"])
    base_out = k["act_num"] if dis else k["A"]
    out_w = {"base": base_out, "plus1": base_out + 1, "double": 2 * base_out}.get(k["out"], k["out"])
    pol = _mlp([k["O"] + k["in_delta"], *k["hidden"], out_w], act=k["hidden_act"], dtype=k["dtype"])
    if k["n_layers"] is not None:
        pol.n_layers = k["n_layers"]
    if k["null_weight"] is not None:
        pol.weight[k["null_weight"]] = 0
    if k["null_bias"] is not None:
        pol.bias[k["null_bias"]] = 0
    ref, N, T = C.byref, k["N"], k["T"]
    if name.endswith("workspace_bytes"):
        return getattr(hb.lib(), name)(ref(env), ref(pol), *((k["act_num"],) if dis else ()), N, T)
    if "episode" in name:
        tail = (N, T, ref(_io()), ref(_all_ptrs(hb.GopsEpisodeOut)), None, 0, None)
        return getattr(hb.lib(), name)(ref(env), ref(pol), *((k["table"], k["act_num"]) if dis else ()), *tail)
    head = k["head"]
    desc = hb.GopsSampleDesc(head=0 if dis or head is None else head, max_episode_steps=3, pool_rows=2, min_log_std=-20.0, max_log_std=0.5)
    d = hb.GopsSampleDis(action_table=k["table"], act_num=k["act_num"], head=hb.SAMPLE_EPS_GREEDY if head is None else head,
                         epsilon=k["eps"], env_act=P)
    tail = (N, T, ref(_all_ptrs(hb.GopsSampleState)), ref(_all_ptrs(hb.GopsSamplePool)), P, ref(_all_ptrs(hb.GopsSampleOut)), None, 0, None)
    return getattr(hb.lib(), name)(ref(env), ref(pol), ref(desc), *((ref(d),) if dis else ()), *tail)


def _closed_loop_codes(name, single_of_chooser):
    """{"single": {fault: code}, "pair": {unsupported fault: {bad-arg fault: code}}} of one entry point.  A pair is taken where the
    two faults turn different knobs, so that both are present in the description."""
    single = {f: _closed_loop_call(name, knobs) for f, knobs in CLOSED_LOOP_FAULTS.items()}
    uns = [f for f, c in single_of_chooser.items() if c == UNS]
    bad = [f for f, c in single_of_chooser.items() if c == BAD]
    pair = {}
    for u in uns:
        for b in bad:
            ku, kb = CLOSED_LOOP_FAULTS[u], CLOSED_LOOP_FAULTS[b]
            if not set(ku) & set(kb):
                pair.setdefault(u, {})[b] = _closed_loop_call(name, {**ku, **kb})
    return dict(single=single, pair=pair)


@pytest.mark.parametrize("name", sorted(CLOSED_LOOP_ENTRIES))
def test_closed_loop_refusal_codes_are_those_recorded(name):
    with open(CLOSED_LOOP_GOLDEN) as f:
        golden = json.load(f)
    want = golden[name]
    assert sorted(want["single"]) == sorted(CLOSED_LOOP_FAULTS)
    assert sum(len(v) for v in want["pair"].values()) >= 100   # (the pairs are there)
    if not name.endswith("workspace_bytes"):   # a refusal each: nothing launches
        assert all(c in (BAD, UNS, WS) for c in want["single"].values())
        assert all(c in (BAD, UNS) for v in want["pair"].values() for c in v.values())
    got = _closed_loop_codes(name, golden[CLOSED_LOOP_ENTRIES[name][0]]["single"])
    diff = {f: (got["single"][f], c) for f, c in want["single"].items() if got["single"][f] != c}
    diff.update({u + "+" + b: (got["pair"][u][b], c) for u, v in want["pair"].items() for b, c in v.items() if got["pair"][u][b] != c})
    assert not diff, diff   # fault: (code now, code recorded)
    assert got == want


if __name__ == "__main__":
    first = {n: {f: _closed_loop_call(n, k) for f, k in CLOSED_LOOP_FAULTS.items()} for n in CLOSED_LOOP_ENTRIES}
    with open(CLOSED_LOOP_GOLDEN, "w") as f:
        json.dump({n: _closed_loop_codes(n, first[CLOSED_LOOP_ENTRIES[n][0]]) for n in sorted(CLOSED_LOOP_ENTRIES)}, f, indent=0, sort_keys=True)
        f.write("\n")
