"""Shared test helpers: build oracle-side envs / nets from a golden fixture."""
import numpy as np
import torch

from oracle import adp_oracle as orc

INFO_KEYS = ("state", "ref_points", "path_num", "u_num", "ref_time", "surr_state")


def oracle_env(cfg, extra, golden=None):
    """Oracle env for a fixture's config.  `golden`: the fixture - constants the reference derived
    with LAPACK when the fixture was recorded (fp32 `pinv`, whose last bits are host dependent and
    get amplified by long unstable LQ horizons) are taken from it instead of being recomputed."""
    env = orc.make_env(cfg["env_id"], lq_config=cfg.get("lq_config", "s4a2"),
                       pre_horizon=cfg.get("pre_horizon", 10), surr_veh_num=cfg.get("surr_veh_num"),
                       reward_scale=extra.get("reward_scale"), reward_shift=extra.get("reward_shift"),
                       obs_scale=extra.get("obs_scale"), obs_shift=extra.get("obs_shift"),
                       path_para=extra.get("path_para"), u_para=extra.get("u_para"),
                       repeat_num=extra.get("repeat_num"), sum_reward=extra.get("sum_reward", True),
                       mask_at_done=extra.get("mask_at_done", True))
    if golden is not None and "const/lq_inv_IA" in golden:
        env["lq"]["inv_IA"] = torch.from_numpy(np.array(golden["const/lq_inv_IA"]))
    return env


def data_from_golden(g, prefix="in/"):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith(prefix)}


def nets_from_golden(g, cfg):
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")}
    act = cfg["act"]
    nets = {}
    pol = orc.net_from_state_dict(sd, "policy.pi", act)
    pol["act_high"], pol["act_low"] = sd["policy.act_high_lim"], sd["policy.act_low_lim"]
    nets["policy"] = pol
    if "v.v.0.weight" in sd:
        nets["v"] = orc.net_from_state_dict(sd, "v.v", act)
        nets["v_target"] = orc.net_from_state_dict(sd, "v_target.v", act, requires_grad=False)
    return nets, sd


def mpg_nets_from_golden(g, cfg):
    """Oracle parameter dicts of an MPG fixture's state_dict (q1, q2, [q1_model, q2_model], targets, policy)."""
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")}
    nets = {}
    for name in ("policy", "policy_target"):
        net = orc.net_from_state_dict(sd, f"{name}.pi", cfg["act"], requires_grad=(name == "policy"))
        net["act_high"], net["act_low"] = sd[f"{name}.act_high_lim"], sd[f"{name}.act_low_lim"]
        nets[name] = net
    for name in ("q1", "q2", "q1_model", "q2_model"):
        if f"{name}.q.0.weight" in sd:
            nets[name] = orc.net_from_state_dict(sd, f"{name}.q", cfg["act"])
            nets[name + "_target"] = orc.net_from_state_dict(sd, f"{name}_target.q", cfg["act"], requires_grad=False)
    return nets, sd


def reference_init_nets(cfg, seed, obs_dim, act_dim):
    """Re-create the reference's random init: torch.manual_seed(seed) then nn.Linear layers in
    the reference's construction order (fhadp.py:42-44; infadp.py:41-45: value first)."""
    torch.manual_seed(seed)

    def linears(sizes):
        return [torch.nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]

    def to_net(layers, **kw):
        return dict(w=[l.weight.detach().clone().requires_grad_(True) for l in layers],
                    b=[l.bias.detach().clone().requires_grad_(True) for l in layers], act=cfg["act"], **kw)

    hid = list(cfg["hidden"])
    lim = dict(act_high=torch.ones(act_dim), act_low=-torch.ones(act_dim))
    nets = {}
    if cfg["alg"] == "FHADP":
        nets["policy"] = to_net(linears([obs_dim + 1] + hid + [act_dim]), **lim)
    else:
        v = linears([obs_dim] + hid + [1])
        p = linears([obs_dim] + hid + [act_dim])
        nets["v"] = to_net(v)
        nets["policy"] = to_net(p, **lim)
        vt = to_net(v)
        g = torch.Generator().manual_seed(seed + 1000)  # make_golden.perturb_targets
        with torch.no_grad():
            for w_, b_ in zip(vt["w"], vt["b"]):
                for p_ in (w_, b_):
                    p_.add_(0.05 * (torch.rand(p_.shape, generator=g) - 0.5))
        for p_ in vt["w"] + vt["b"]:
            p_.requires_grad_(False)
        nets["v_target"] = vt
    return nets


# ---- HIP side: build C-ABI descriptors from the same (oracle-side) constants -------------------
def hip_env_from_oracle(env, policy_net=None):
    from gops_amd import hip_backend as hb
    from gops_amd.env.env_ocp.resources.ref_traj_params import ref_constants
    kind = {"veh_err": hb.ENV_VEH_SURR, "lq": hb.ENV_LQ, "idp": hb.ENV_IDP, "veh": hb.ENV_VEH, "veh_surr": hb.ENV_VEH_SURR,
            "cartpole": hb.ENV_CARTPOLE, "pendulum": hb.ENV_PENDULUM, "veh2": hb.ENV_VEH2DOF, "mob": hb.ENV_MOBILEROBOT}[env["kind"]]
    surr = None
    if env["kind"] in ("veh_surr", "veh_err") or env.get("err_tol") is not None:
        surr = {k: env[k] for k in ("n_surr", "n_constraint", "veh_length", "veh_width", "road_upper", "road_lower", "reward_w")}
        surr["penalty"] = bool(env.get("penalty", False))
        surr["err_tol"] = env.get("err_tol")
    lq = None
    if env["kind"] == "lq":
        c = env["lq"]
        lq = dict(inv_IA=c["inv_IA"], B=c["B"], Q=c["Q"], R=c["R"], dt=c["dt"],
                  reward_scale=c["reward_scale"], reward_shift=c["reward_shift"])
    return hb.make_env(kind, env["obs_dim"], env["act_dim"], act_low=env["act_low"], act_high=env["act_high"],
                       min_action=env["min_action"], max_action=env["max_action"],
                       policy_low=None if policy_net is None else policy_net["act_low"],
                       policy_high=None if policy_net is None else policy_net["act_high"],
                       obs_low=env["obs_low"], obs_high=env["obs_high"], pre_horizon=env.get("P", 0),
                       reward_scale=env["reward_scale"] if env["shaping"] else None,
                       reward_shift=env["reward_shift"] if env["shaping"] else None, lq=lq, surr=surr,
                       obs_scale=env["obs_scale"] if env.get("scale_obs") else None,
                       obs_shift=env["obs_shift"] if env.get("scale_obs") else None,
                       ref_c=ref_constants(env.get("path_para"), env.get("u_para")) if "ref_params" in env else None,
                       repeat_num=env.get("repeat_num"), sum_reward=env.get("sum_reward", True),
                       mask_at_done=env.get("mask_at_done", True),
                       n_constraint=env["n_constraint"] if env["kind"] == "mob" else None)


def hip_mlp_from_net(net, device):
    from gops_amd import hip_backend as hb
    ws = [w.detach().to(device).contiguous() for w in net["w"]]
    bs = [b.detach().to(device).contiguous() for b in net["b"]]
    return hb.make_mlp(ws, bs, net["act"]), ws, bs


def to_device(data, device):
    return {k: v.to(device).contiguous() for k, v in data.items()}


def as_f64(x):
    """Deep copy of an oracle env / net / data structure in float64."""
    if torch.is_tensor(x):
        return x.detach().double() if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: as_f64(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [as_f64(v) for v in x]
    return x


def fhadp_gradient_f64(env, net, data, horizon, gamma):
    """The oracle's FHADP gradient evaluated in float64: the value both fp32 evaluations (the
    reference's and the HIP path's) approximate.  Used to size the fp32 noise floor of a case."""
    n64 = as_f64(net)
    n64["w"] = [w.requires_grad_(True) for w in n64["w"]]
    n64["b"] = [b.requires_grad_(True) for b in n64["b"]]
    return orc.fhadp_gradient(as_f64(env), n64, as_f64(data), horizon, gamma)


def fp32_noise_floor(env, net, data, horizon, gamma, ref64_flat, trials=8):
    """How far fp32 evaluations of one FHADP gradient scatter around its float64 value: the oracle
    (fp32) is re-run with every weight moved by at most one ulp; returns the largest rel-L2 distance
    to `ref64_flat` (1e-7-ish for well-conditioned cases, up to 5e-4 for the trained LQ H=80 case,
    whose clipped, unstable closed loop amplifies last-bit differences)."""
    gen = torch.Generator().manual_seed(0)
    worst = 0.0
    for _ in range(trials):
        pert = dict(net)
        pert["w"] = [(w.detach() * (1 + (torch.rand(w.shape, generator=gen) - 0.5) * 1.2e-7)).requires_grad_(True)
                     for w in net["w"]]
        pert["b"] = [b.detach().clone().requires_grad_(True) for b in net["b"]]
        grads = orc.fhadp_gradient(env, pert, data, horizon, gamma)["grads"]
        flat = torch.cat([x.reshape(-1) for x in grads]).double()
        worst = max(worst, float((flat - ref64_flat).norm() / ref64_flat.norm()))
    return worst


# ---- per-trajectory checks (tests/test_per_trajectory_gpu.py): float64 oracle with an explicit step loop ----------------------
def take_rows(data, rows):
    """The sub-batch `rows` of a replay batch (every tensor whose first axis is the batch axis)."""
    B = data["obs"].shape[0]
    idx = torch.as_tensor(list(rows), dtype=torch.long)
    out = {k: (v[idx] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B else v) for k, v in data.items()}
    if "noise" in data:   # pyth_mobilerobot's obstacle draws [H, B, 2]: the batch axis is the second one
        out["noise"] = data["noise"][:, idx]
    return out


class _appended_point:
    """While active, the oracle's vehicle models append `point` [B, 4] instead of evaluating the reference generator: the
    oracle then runs on the same appended reference points the kernels are handed (`GopsRolloutIn.ref_appended`), in any dtype."""

    def __init__(self, point):
        self.point = point

    def __enter__(self):
        self.saved = orc.ref_point, orc.ref_y, orc.ref_phi
        if self.point is not None:
            orc.ref_point = lambda t, path_num, u_num: self.point.to(t.dtype)
            orc.ref_y = lambda t, path_num, u_num: self.point[:, 1].to(t.dtype)      # (veh2dofconti appends (y, phi) only)
            orc.ref_phi = lambda t, path_num, u_num: self.point[:, 2].to(t.dtype)

    def __exit__(self, *exc):
        orc.ref_point, orc.ref_y, orc.ref_phi = self.saved


def appended_points(cfg, data):
    """The H reference points a veh3dofconti (any form) or veh2dofconti rollout appends, from the oracle's restatement of
    MultiRefTrajModel: [B, H, 4] (veh2dofconti reads columns 1 and 2 only)."""
    P, dt = cfg["pre_horizon"], 0.1
    t = data["ref_time"].clone()
    pts = []
    for _ in range(cfg["horizon"]):   # veh_step: nt = ref_time + dt (accumulated in fp32), new point at nt + P dt
        t = t + dt
        pts.append(orc.ref_point(t + P * dt, data["path_num"], data["u_num"]))
    return torch.stack(pts, 1).contiguous()


def done_margin(env, nobs):
    """Relative distance of the quantities that decide `done` (on the observation a step returns) to their bounds, per row:
    min_k | |q_k| - bound_k | / bound_k; inf for models that never terminate."""
    kind = env["kind"]
    if kind == "idp":
        tip = orc.IDP["l1"] * torch.cos(nobs[:, 1]) + orc.IDP["l2"] * torch.cos(nobs[:, 2])
        return torch.minimum((tip - 1.0).abs(), (nobs[:, 0].abs() - 15.0).abs() / 15.0)
    if kind in ("veh", "veh_surr", "veh_err") and not env.get("penalty"):
        q = nobs[:, :3].abs()
        bound = torch.tensor([10.0, 10.0, np.pi], dtype=nobs.dtype)
        return ((q - bound).abs() / bound).min(1).values
    if kind == "veh2":
        bound = torch.tensor([2.0, np.pi], dtype=nobs.dtype)
        return ((nobs[:, :2].abs() - bound).abs() / bound).min(1).values
    if kind == "cartpole":
        bound = torch.tensor([2.4, 12 * 2 * np.pi / 360], dtype=nobs.dtype)
        return ((nobs[:, [0, 2]].abs() - bound).abs() / bound).min(1).values
    if kind == "mob":   # x' < -2, |y'| > 4, constraint > 0.15 (constraint = 0.89 - distance to the obstacle)
        c = 0.89 - torch.sqrt(torch.square(nobs[:, 8] - nobs[:, 0]) + torch.square(nobs[:, 9] - nobs[:, 1]))
        return torch.stack(((nobs[:, 0] + 2.0).abs() / 2.0, (nobs[:, 1].abs() - 4.0).abs() / 4.0, (c - 0.15).abs() / 0.15), 1).min(1).values
    assert kind in ("lq", "pendulum") or env.get("penalty"), kind
    return torch.full((nobs.shape[0],), float("inf"), dtype=nobs.dtype)


def _policy_params(net):
    return [p for pair in zip(net["w"], net["b"]) for p in pair if p is not None]


def constraint_kink_gap(env, obs_in, info):
    """How far the constraint a step just returned (`info`, stepped from the observation `obs_in`) is from a point where its OWN
    formula changes branch, per row: the gap between the two smallest circle-pair distances of the surrounding-vehicle constraint
    (orc.surr_constraint takes their minimum; the detour model's road terms take a maximum over the two ego circles: the gap
    between those two), |y| = 0 for the tracking-error constraints.  inf where there is no such point."""
    kind = env["kind"]
    B = obs_in.shape[0]
    if kind == "veh_surr" and not env.get("penalty"):
        state, surr = info["state"].detach(), info["surr_state"].detach()
        d = (env["veh_length"] - env["veh_width"]) / 2
        x, y, phi = state[:, 0:1], state[:, 1:2], state[:, 2:3]
        ego = torch.stack((torch.cat((x + d * torch.cos(phi), y + d * torch.sin(phi)), 1), torch.cat((x - d * torch.cos(phi), y - d * torch.sin(phi)), 1)), 1)
        sx, sy, sphi = surr[..., 0], surr[..., 1], surr[..., 2]
        sc = torch.stack((torch.stack((sx + d * torch.cos(sphi), sy + d * torch.sin(sphi)), 2), torch.stack((sx - d * torch.cos(sphi), sy - d * torch.sin(sphi)), 2)), 2)
        dist = torch.linalg.norm(ego[:, :, None, None, :] - sc[:, None], dim=-1).reshape(B, -1)    # [B, 2 * n_surr * 2]
        two = dist.sort(1).values[:, :2]
        gap = two[:, 1] - two[:, 0]
        if env["n_constraint"] == 3:
            gap = torch.minimum(gap, (ego[:, 0, 1] - ego[:, 1, 1]).abs())
        return gap
    if kind == "veh_err":
        return torch.minimum(obs_in[:, 1].detach().abs(), obs_in[:, 3].detach().abs())
    if kind == "veh2" and env.get("err_tol") is not None:
        return obs_in[:, 0].detach().abs()
    return torch.full((B,), float("inf"), dtype=obs_in.dtype)


def constraint_outputs(cons, gamma):
    """`constraint_sums` [4, B] and `constraint_prods` [2 n_c, B] of include/gops_hip.h from the per-step constraints [H, B, n_c]."""
    H = cons.shape[0]
    g = torch.tensor([gamma ** t for t in range(H)], dtype=cons.dtype)[:, None]
    pos, neg = torch.clamp_min(cons, 0), torch.clamp_max(cons, 0)
    sums = torch.stack((((pos ** 2).sum(2) * g).sum(0), (pos.sum(2) * g).sum(0), ((-neg + 1e-8).log().sum(2) * g).sum(0),
                        (cons < 0).all(2).all(0).to(cons.dtype)))
    prods = torch.cat((orc.spil_phi(cons).prod(0).t(), (cons <= 0).all(0).t().to(cons.dtype)))
    return sums, prods


def rollout_history(env, net, data, horizon, gamma, finite_horizon, value_target=None, tail_unmasked=False):
    """The oracle's rollout (adp_oracle.rollout) as an explicit loop, in the dtype of its arguments, keeping what the loop
    passes through: per-trajectory return `v` (tail value of `value_target` included, masked at done), `rewards` [H, B],
    `done_hist` [H, B] (done after each step), `margin` [H, B] (done_margin of each step's observation for rows that entered the
    step alive, inf otherwise), `final_obs`, `final_done`.  A net dict may carry its own `forward(net, obs, virtual_t)` (POLY)."""
    obs, done, info = data["obs"], data["done"], data
    app = data.get("ref_appended")
    v = 0
    rewards, done_hist, margin, cons, gaps = [], [], [], [], []
    for step in range(horizon):
        t = step + 1 if finite_horizon else None
        a = net["forward"](net, obs, t) if "forward" in net else orc.policy_forward(net, obs, t)
        alive = ~done.bool()
        obs_in = obs
        with _appended_point(None if app is None else app[:, step]):
            obs, r, done, info = orc.env_forward(env, obs, a, done, info)
        if "constraint" in info:
            cons.append(info["constraint"])
            gaps.append(constraint_kink_gap(env, obs_in, info))
        v = v + r * (gamma ** step)
        rewards.append(r)
        done_hist.append(done)
        m = done_margin(env, obs.detach())
        margin.append(torch.where(alive, m, torch.full_like(m, float("inf"))))
    if value_target is not None:
        tail = value_target["forward"](value_target, obs) if "forward" in value_target else orc.value_forward(value_target, obs)
        v = v + (gamma ** horizon * tail if tail_unmasked else (~done) * gamma ** horizon * tail)
    out = dict(v=v, rewards=torch.stack(rewards), done_hist=torch.stack(done_hist), margin=torch.stack(margin),
               final_obs=obs, final_done=done)
    if cons:
        out["constraints"], out["kink_gap"] = torch.stack(cons), torch.stack(gaps)
        out["sums"], out["prods"] = constraint_outputs(out["constraints"], gamma)
        if "state" in info:
            out["final_state"] = info["state"]
    return out


def _net_f64(net, requires_grad=True):
    n64 = as_f64(net)
    n64["w"] = [w.requires_grad_(requires_grad) for w in n64["w"]]
    n64["b"] = [None if b is None else b.requires_grad_(requires_grad) for b in n64["b"]]
    return n64


def weighted_gradient_f64(env, nets, data, horizon, gamma, finite_horizon, gv, value_target=None):
    """The oracle's rollout in float64 with loss = (gv * v).sum() (v with INFADP's tail value when `value_target` is given):
    per-trajectory v, per-step rewards, the per-step done history, final obs / done and the policy's parameter gradients."""
    n64 = _net_f64(nets)
    vt = None if value_target is None else _net_f64(value_target, False)
    out = rollout_history(as_f64(env), n64, as_f64(data), horizon, gamma, finite_horizon, vt)
    loss = (torch.as_tensor(gv).double() * out["v"]).sum()
    grads = torch.autograd.grad(loss, _policy_params(n64), allow_unused=True)
    out = {k: x.detach() for k, x in out.items()}
    out["grads"] = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, _policy_params(n64))]
    return out


def one_row_gradients(env, nets, data, horizon, gamma, finite_horizon, rows, value_target=None):
    """d v[i] / d(policy parameters) for every i of `rows`, in the dtype of the arguments: {row: [gradient per tensor]}.  The
    trajectories of a batch do not interact, so the graph is built over the selected rows only."""
    rows = list(rows)
    out = rollout_history(env, nets, take_rows(data, rows), horizon, gamma, finite_horizon, value_target)
    params = _policy_params(nets)
    res = {}
    for k, i in enumerate(rows):
        if not out["v"][k].requires_grad:
            res[i] = [torch.zeros_like(p) for p in params]
            continue
        g = torch.autograd.grad(out["v"][k], params, retain_graph=True, allow_unused=True)
        res[i] = [torch.zeros_like(p) if x is None else x.detach() for x, p in zip(g, params)]
    return res


def one_row_gradients_f64(env, nets, data, horizon, gamma, finite_horizon, rows, value_target=None):
    """The float64 gradient of ONE trajectory's return, for every row of `rows`."""
    vt = None if value_target is None else _net_f64(value_target, False)
    return one_row_gradients(as_f64(env), _net_f64(nets), as_f64(data), horizon, gamma, finite_horizon, rows, vt)


def seeded_loss(out, seeds, dtype):
    """L = sum gv v + sum gc sums[:3] + sum gp prods[:n_c] + sum gs constraints, of a rollout_history result; `seeds`: dict with any
    of gv [B], gc [3, B], gp [n_c, B], gs [H, B, n_c] (missing or None: zero)."""
    loss = 0
    for key, of in (("gv", lambda: out["v"]), ("gc", lambda: out["sums"][:3]), ("gp", lambda: out["prods"][:out["constraints"].shape[2]]),
                    ("gs", lambda: out["constraints"])):
        if seeds.get(key) is not None:
            loss = loss + (torch.as_tensor(seeds[key]).to(dtype) * of()).sum()
    return loss


def _grads_of(loss, params):
    if not torch.is_tensor(loss) or not loss.requires_grad:
        return [torch.zeros_like(p) for p in params]
    g = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    return [torch.zeros_like(p) if x is None else x.detach() for x, p in zip(g, params)]


def seeded_gradients_f64(env, nets, data, horizon, gamma, finite_horizon, seed_sets, value_target=None, tail_unmasked=False):
    """weighted_gradient_f64 with all four gradient sources: ONE float64 pass, then the policy gradient of seeded_loss for every
    entry of `seed_sets` ({name: seeds}).  Returns (the detached history, {name: [gradient per tensor]})."""
    n64 = _net_f64(nets)
    vt = None if value_target is None else _net_f64(value_target, False)
    out = rollout_history(as_f64(env), n64, as_f64(data), horizon, gamma, finite_horizon, vt, tail_unmasked)
    params = _policy_params(n64)
    grads = {name: _grads_of(seeded_loss(out, seeds, torch.float64), params) for name, seeds in seed_sets.items()}
    return {k: x.detach() for k, x in out.items()}, grads


def one_row_seeded_gradients(env, nets, data, horizon, gamma, finite_horizon, rows, row_seeds, value_target=None, tail_unmasked=False):
    """one_row_gradients with all four sources: `row_seeds(i, k)` -> {name: seeds over the SUB-batch `rows`, non-zero in its row k
    (= row i of the batch) only}; returns {row: {name: [gradient per tensor]}}, in the dtype of the arguments.  The graph is built
    over the selected rows only."""
    rows = list(rows)
    out = rollout_history(env, nets, take_rows(data, rows), horizon, gamma, finite_horizon, value_target, tail_unmasked)
    params = _policy_params(nets)
    dtype = params[0].dtype
    return {i: {name: _grads_of(seeded_loss(out, seeds, dtype), params) for name, seeds in row_seeds(i, k).items()} for k, i in enumerate(rows)}


def fp32_seeded_noise_floor(env, nets, data, horizon, gamma, finite_horizon, seed_sets, ref64, rows, row_seeds, rows64,
                            value_target=None, tail_unmasked=False, trials=2):
    """fp32_weighted_noise_floor with all four sources: the fp32 oracle (weights as they are, then moved by at most one ulp) against
    the float64 gradients `ref64` ({name: grads} of seeded_gradients_f64) and `rows64` (one_row_seeded_gradients in float64).
    Returns ({name: largest distance, flat or any one tensor}, {row: {name: largest flat distance}})."""
    gen = torch.Generator().manual_seed(0)
    worst = {name: 0.0 for name in seed_sets}
    worst_rows = {i: {name: 0.0 for name in rows64[i]} for i in rows}
    for trial in range(trials):
        pert = dict(nets)
        scale = 0.0 if trial == 0 else 1.2e-7
        pert["w"] = [(w.detach() * (1 + (torch.rand(w.shape, generator=gen) - 0.5) * scale)).requires_grad_(True) for w in nets["w"]]
        pert["b"] = [None if b is None else b.detach().clone().requires_grad_(True) for b in nets["b"]]
        out = rollout_history(env, pert, data, horizon, gamma, finite_horizon, value_target, tail_unmasked)
        params = _policy_params(pert)
        for name, seeds in seed_sets.items():
            g = _grads_of(seeded_loss(out, seeds, torch.float32), params)
            worst[name] = max([worst[name], _dist(flat_grads(g), flat_grads(ref64[name]))] + [_dist(a.double(), b) for a, b in zip(g, ref64[name])])
        del out
        if rows:
            got = one_row_seeded_gradients(env, pert, data, horizon, gamma, finite_horizon, rows, row_seeds, value_target, tail_unmasked)
            for i in rows:
                for name, gi in got[i].items():
                    worst_rows[i][name] = max(worst_rows[i][name], _dist(flat_grads(gi), flat_grads(rows64[i][name])))
    return worst, worst_rows


def flat_grads(grads):
    return torch.cat([g.reshape(-1) for g in grads]).double().cpu()


def _dist(a, b):
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def fp32_weighted_noise_floor(env, nets, data, horizon, gamma, finite_horizon, gv, ref64, rows=(), rows64=None,
                              value_target=None, trials=2):
    """fp32_noise_floor for a weighted loss and for single rows: the fp32 oracle, re-run with every weight moved by at most
    one ulp, against the float64 results `ref64` (weighted_gradient_f64) / `rows64` (one_row_gradients_f64).  Returns
    (largest rel-L2 distance of the weighted gradient - flat or any one tensor -, {row: largest distance of that row's gradient})."""
    gen = torch.Generator().manual_seed(0)
    worst, worst_rows = 0.0, {i: 0.0 for i in rows}
    for trial in range(trials):
        pert = dict(nets)
        scale = 0.0 if trial == 0 else 1.2e-7   # (the first run is the unperturbed fp32 oracle)
        pert["w"] = [(w.detach() * (1 + (torch.rand(w.shape, generator=gen) - 0.5) * scale)).requires_grad_(True) for w in nets["w"]]
        pert["b"] = [None if b is None else b.detach().clone().requires_grad_(True) for b in nets["b"]]
        out = rollout_history(env, pert, data, horizon, gamma, finite_horizon, value_target)
        params = _policy_params(pert)
        g = torch.autograd.grad((torch.as_tensor(gv).float() * out["v"]).sum(), params, allow_unused=True)
        g = [torch.zeros_like(p) if x is None else x for x, p in zip(g, params)]
        worst = max([worst, _dist(flat_grads(g), flat_grads(ref64["grads"]))]
                    + [_dist(a.double(), b) for a, b in zip(g, ref64["grads"])])
        if rows:
            for i, gi in one_row_gradients(env, pert, data, horizon, gamma, finite_horizon, rows, value_target).items():
                worst_rows[i] = max(worst_rows[i], _dist(flat_grads(gi), flat_grads(rows64[i])))
    return worst, worst_rows


def padded_batch(cfg, seed, env, data, extra):
    """`data` followed by `extra` rows of another seed, their observations (where the observation is the state) tripled; the
    vehicle models' rows with their own appended reference points, pyth_mobilerobot's with their own obstacle draws."""
    from gops_amd.utils.synthetic import make_batch
    tail = make_batch(dict(cfg, batch=extra), seed + 77)
    if "ref_appended" in data:
        tail["ref_appended"] = appended_points(cfg, tail)
    else:
        tail["obs"] = tail["obs"] * 3.0
    out = {k: torch.cat((v, tail[k])).contiguous() for k, v in data.items() if k != "noise"}
    if "noise" in data:
        gen = torch.Generator().manual_seed(3000 + seed)
        out["noise"] = torch.cat((data["noise"], 0.05 * torch.randn(data["noise"].shape[0], extra, 2, generator=gen)), 1).contiguous()
    return out


def edge_rows(B, tile, n_workgroups):
    """The rows of a batch of B that a tiled, grid-stride kernel is most likely to get wrong: 0, tile - 1, tile, the last row of the
    last whole tile, the first and the last valid row of the ragged tile and - with more tiles than workgroups - the rows around the
    first tile a workgroup takes on its second pass (tile * n_workgroups)."""
    rows = {0, tile - 1, tile, B - 1}
    whole = B // tile
    if whole:
        rows.add(whole * tile - 1)
    if B % tile:
        rows.add(whole * tile)
    if -(-B // tile) > n_workgroups:
        t2 = tile * n_workgroups
        rows |= {t2 - 1, t2, t2 + tile - 1, t2 + tile}
    return sorted(r for r in rows if 0 <= r < B)


def edge_tiles(B, tile, n_workgroups):
    return sorted({r // tile for r in edge_rows(B, tile, n_workgroups)})


def premise_rows(B, tile, n_workgroups):
    """Where batch_with_done puts its special rows: (rows done on entry, rows to terminate inside the horizon) - each list with a
    tile-edge row, a row of the ragged (last) tile, a row of the second-pass tile where there is one, and a row in the middle."""
    nt = -(-B // tile)
    t2 = tile * n_workgroups
    mid = (nt // 2) * tile + 5
    d_cand = [tile - 1, B - 1, t2 if nt > n_workgroups else -1, mid, 5, 9, 13]
    t_cand = [tile, B - 2, t2 + tile - 1 if nt > n_workgroups else -1, mid + 1, 3, 7, 11]
    done_rows, term_rows = [], []
    for r in d_cand:
        if 0 < r < B and r not in done_rows and (len(done_rows) < 3 or r in d_cand[:4]):
            done_rows.append(r)
    for r in t_cand:
        if 0 < r < B and r not in done_rows and r not in term_rows and (len(term_rows) < 3 or r in t_cand[:4]):
            term_rows.append(r)
    return done_rows, term_rows


def _push_towards_termination(cfg, env, data, row, lam, sign):
    """Row `row` of `data` with its initial state moved to `lam` short of a termination bound, heading across it."""
    kind = env["kind"]
    if kind == "idp":      # both angles just inside tip_y = l1 cos th1 + l2 cos th2 = 1, rotating outwards
        crit = float(np.arccos(1.0 / (orc.IDP["l1"] + orc.IDP["l2"])))
        data["obs"][row, 1:3] = sign * (crit - lam)
        data["obs"][row, 4:6] = sign * 3.0
    elif kind == "cartpole":   # cart just inside |x| = 2.4, moving outwards
        data["obs"][row, 0] = sign * (2.4 - lam)
        data["obs"][row, 1] = sign * 1.5
    elif kind in ("veh", "veh_surr", "veh_err"):    # lateral error (ego frame) just inside 10 m, heading 0.5 rad off the reference's: it grows by ~0.24 m a step
        from gops_amd.utils.synthetic import veh_obs_f32
        ref0 = data["ref_points"][row, 0].numpy()
        state = data["state"][row].numpy().copy()
        ephi = np.float32(ref0[2] - sign * 0.5)
        d = np.float32(sign * (10.0 - lam))
        state[0] = ref0[0] + d * np.sin(ephi)
        state[1] = ref0[1] - d * np.cos(ephi)
        state[2] = ephi
        moved = torch.from_numpy(state[:2]) - data["state"][row, :2]
        data["state"][row] = torch.from_numpy(state)
        obs = torch.from_numpy(veh_obs_f32(state[None], data["ref_points"][row:row + 1].numpy())[0])
        if kind == "veh_surr":   # the surrounding vehicles move along with the ego vehicle: the constraint geometry stays what it was
            data["surr_state"][row, :, :2] += moved
            obs = torch.cat((obs, (data["surr_state"][row, :, :4] - data["state"][row, :4]).reshape(-1)))
        data["obs"][row] = obs
    elif kind == "veh2":   # lateral error just inside 2 m, heading 0.5 rad off the reference's: it grows by ~0.24 m a step (u = 5 m/s)
        ref = data["ref_points"][row]
        data["state"][row, 0] = ref[0, 0] + sign * (2.0 - lam)
        data["state"][row, 1] = ref[0, 1] + sign * 0.5
        st = data["state"][row]
        data["obs"][row] = torch.cat((st[:2] - ref[0], st[2:], st[:1] - ref[1:, 0]))
    elif kind == "mob":    # the obstacle `lam` outside the collision distance (constraint > 0.15 <=> closer than 0.74 m), driving at the
        y = 0.5 * sign       # ego robot at full speed: whatever the policy does, the gap closes by 0.016 m a step or more
        data["obs"][row, :5] = torch.tensor([1.0, y, 0.0, 0.4, 0.0])
        data["obs"][row, 5:8] = torch.tensor([y, 0.0, 0.4 - 0.3])
        data["obs"][row, 8:13] = torch.tensor([1.0 + 0.74 + lam, y, np.pi, 0.4, 0.0])
    else:
        raise KeyError(kind)


_PUSH_GRID = {"idp": (0.003, 0.4), "cartpole": (0.004, 0.4), "veh": (0.02, 2.8), "veh_surr": (0.02, 2.8), "veh_err": (0.02, 2.8),
              "veh2": (0.01, 2.4), "mob": (0.01, 0.3)}
DONE_MARGIN = 1e-3


def spread_tracking_errors(cfg, env, data):
    """The errcstr models constrain |lateral error| - 0.2 m: rows of make_batch start anywhere in +-1 m and cross the bound under
    an untrained policy (and the speed error, +-2 m/s, sweeps over Phi's clamp at c = -0.7).  Every second row is moved to a small lateral (0.03 .. 0.07 m) and heading (+-0.004 rad) error - clearly
    feasible over a short horizon -, the others to 0.65 .. 1 m: clearly violated, and clear of Phi's clamp at c = 0.35.  In place; observations rebuilt."""
    from gops_amd.utils.synthetic import veh_obs_f32
    B = cfg["batch"]
    gen = torch.Generator().manual_seed(77)
    u1, u2, sg = torch.rand(B, generator=gen), torch.rand(B, generator=gen), torch.where(torch.rand(B, generator=gen) < 0.5, -1.0, 1.0)
    small = torch.arange(B) % 2 == 0
    d = sg * torch.where(small, 0.03 + 0.04 * u1, 0.65 + 0.35 * u1)
    dphi = torch.where(small, 0.008 * (u2 - 0.5), 0.3 * (u2 - 0.5))
    ref0 = data["ref_points"][:, 0]
    if env["kind"] == "veh2":
        data["state"][:, 0], data["state"][:, 1] = ref0[:, 0] + d, ref0[:, 1] + dphi
        data["state"][:, 2:] = torch.where(small[:, None], 0.1 * data["state"][:, 2:], data["state"][:, 2:])
        st, ref = data["state"], data["ref_points"]
        data["obs"] = torch.cat((st[:, :2] - ref[:, 0], st[:, 2:], st[:, :1] - ref[:, 1:, 0]), 1).contiguous()
    else:
        phi = ref0[:, 2] + dphi
        data["state"][:, 3] = ref0[:, 3] - sg * (0.2 + 0.3 * u2)   # (speed error 0.2 .. 0.5 m/s: its constraint, |du| - 2, stays near -1.6)
        data["state"][:, 0], data["state"][:, 1], data["state"][:, 2] = ref0[:, 0] + d * torch.sin(phi), ref0[:, 1] - d * torch.cos(phi), phi
        data["state"][:, 4:] = torch.where(small[:, None], 0.1 * data["state"][:, 4:], data["state"][:, 4:])
        data["obs"] = torch.from_numpy(veh_obs_f32(data["state"].numpy(), data["ref_points"].numpy())).contiguous()
    data["obs2"] = data["obs"].clone()


def rows_near_origin(cfg, env, data, t_max=1.5, pool_seed=4242):
    """The surrcstr_penalty model's collision penalty has a slope of up to 240 / m in the circle distance: at the coordinates of a
    make_batch row (reference time up to 20 s: ~100 m, one fp32 ulp 7.6e-6 m) fp32 itself is 1e-3 off in the reward.  The batch is
    replaced, in place, by the rows of a larger make_batch whose reference time is below `t_max` (coordinates of a few metres)."""
    from gops_amd.utils.synthetic import make_batch
    B = cfg["batch"]
    pool = make_batch(cfg, pool_seed, batch=int(B * 20.0 / t_max * 1.5) + 64)
    idx = (pool["ref_time"] < t_max).nonzero().flatten()[:B]
    assert idx.numel() == B
    for k, v in data.items():
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B:
            data[k] = pool[k][idx].clone().contiguous()


def batch_with_done(cfg, seed, env, net, tile, n_workgroups, finite_horizon=True, shape_batch=None):
    """make_batch plus (a) rows with done = 1 on entry and (b) - for models that terminate - rows whose initial state is moved so
    that the float64 oracle, under the policy `net`, ends them strictly inside the horizon (step 1 .. H - 1) with the deciding
    quantity at least 2 * DONE_MARGIN away from its bound at every step up to there; both kinds on premise_rows(...).  veh3dofconti
    batches carry the oracle's appended reference points (`ref_appended`).  Returns (data, done_rows, term_rows)."""
    from gops_amd.utils.synthetic import make_batch
    data = make_batch(cfg, seed)
    H = cfg["horizon"]
    if shape_batch is not None:   # (a case's own initial states, before the special rows are placed)
        shape_batch(cfg, env, data)
    if env["kind"] in ("veh", "veh_surr", "veh_err", "veh2"):
        data["ref_appended"] = appended_points(cfg, data)
    if env["kind"] == "mob":   # the obstacle's draws of the rollout, fixed (GopsRolloutIn.noise)
        from gops_amd.hip_backend import MOBILEROBOT_NOISE_STD
        gen = torch.Generator().manual_seed(2000 + seed)
        data["noise"] = (torch.randn(H, cfg["batch"], 2, generator=gen) * torch.tensor(MOBILEROBOT_NOISE_STD)).contiguous()
    done_rows, term_rows = premise_rows(cfg["batch"], tile, n_workgroups)
    if env["kind"] not in _PUSH_GRID or H < 2 or env.get("penalty") or not env.get("mask_at_done", True):   # (the penalty model never reports done)
        term_rows = []
    if term_rows:
        lams = np.geomspace(*_PUSH_GRID[env["kind"]], 40)
        pool = take_rows(data, [r for r in term_rows for _ in lams])
        pool = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in pool.items()}
        for j, r in enumerate(term_rows):
            for k, lam in enumerate(lams):
                _push_towards_termination(cfg, env, pool, j * len(lams) + k, float(lam), 1.0 if (j + k) % 2 else -1.0)
        with torch.no_grad():
            hist = rollout_history(as_f64(env), as_f64(net), as_f64(pool), H, 1.0, finite_horizon)
        first = H - hist["done_hist"].sum(0)                     # 0-based step whose result is the first done (H: never)
        for j, r in enumerate(term_rows):
            want = 1 + j % (H - 1)                              # spread the terminating steps over 1 .. H - 1
            best = None
            for k in range(len(lams)):
                c = j * len(lams) + k
                step = int(first[c]) + 1                         # 1-based terminating step
                if not 1 <= step <= H - 1 or float(hist["margin"][:, c].min()) < 2 * DONE_MARGIN:
                    continue
                if best is None or abs(step - want) < abs(best[0] - want):
                    best = (step, c)
            assert best is not None, f"no initial state found that terminates row {r} inside the horizon"
            for key, v in data.items():
                if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == cfg["batch"]:
                    v[r] = pool[key][best[1]]
    data["done"][done_rows] = 1.0
    data["obs2"] = data["obs"].clone()
    return data, done_rows, term_rows
