"""GPU: the rollout kernels of the models with constraint outputs, one trajectory at a time.  tests/test_per_trajectory_gpu.py
checks every kernel family row by row for the models whose one output is the return; this module does the same for
GOPS_ENV_VEH3DOF_SURR (surrcstr, detour, surrcstr_penalty, errcstr), GOPS_ENV_VEH2DOF with cstr_err and GOPS_ENV_MOBILEROBOT -
what FHADPExterior / Interior / Lagrangian and SPIL run on - with all four gradient sources of `gops_rollout_backward`:
`grad_v`, `grad_constraint` [3, B], `grad_constraint_prod` [n_c, B] and `grad_constraint_step` [H, B, n_c].  The reference is ONE
float64 pass of the oracle (helpers.rollout_history) differentiated as

    L = sum_b gv[b] v[b] + sum_{r<3,b} gc[r,b] sums[r,b] + sum_{k,b} gp[k,b] prods[k,b] + sum_{t,b,k} gs[t,b,k] c[t,b,k].

What the other GPU tests of these models (reference fixtures of 33 to 48 rows, compared through batch means) leave out:

* 256-wide policies: the streamed plane-split forward and sweep, the fp32-MFMA sweep behind a plane-split forward, the plain
  streamed fp32 pair - and the weight-gradient GEMMs without a delta scale (a backward call with any constraint seed);
* seeds that differ from row to row, each source alone, constraint seeds with `grad_v = 0`, one row at a time;
* rows that are done on entry: MaskAtDone freezes their observation and zeroes their reward, but info["state"] and
  info["surr_state"] keep stepping, so their constraints change from step to step and HAVE a policy gradient through the
  constraint seeds (surrcstr / detour), while their gradient through `grad_v` is exactly zero.  The errcstr models read the
  frozen observation: constant constraint, zero gradient.  pyth_mobilerobot evaluates its constraint on the step it would have
  taken from the frozen observation: it changes with the obstacle's draws and has a gradient through that one step;
* the per-row outputs `constraints`, `constraint_sums`, `constraint_prods` element-wise.

The penalties are not smooth (max(c, 0), log(-c + 1e-8), Phi's clamp, the minimum over circle pairs), so a row takes part in a
seed only where fp32 can follow float64: see C_MARGIN / C_MARGIN_LOG / KINK_MARGIN below.  The other rows keep a ZERO seed (they
are not dropped): a zero seed must give no gradient.

pyth_veh3dofconti_surrcstr_penalty computes its constraint outputs on detached copies: any constraint seed with `grad_v = 0`
must give an all-zero gradient, and seeds next to `grad_v` the `grad_v`-only gradient bit for bit.  It never reports done.

Its reward's collision penalty is steep (240 / m): the case's batch lies near the origin and leaves the steep part out, see
PENALTY_DC below.  A backward call with constraint seeds keeps the weight-gradient GEMMs' delta scale for this model (api.hip),
which the bit-for-bit comparison found missing.

`mask_at_done = False`: create_env_model rejects it for pyth_veh3dofconti_surrcstr (tests/test_host_cpu.py); the library accepts
`GopsEnv.no_mask_at_done` for veh2dofconti_errcstr and pyth_mobilerobot (gops_rollout_variant >= 0): one case each.

`prepare(name)` needs no GPU and asserts the premises; tests/test_host_cpu.py runs it for every case and pins every case to its
kernel family.  Which sweep forms walk their tiles grid-stride: of the constrained kinds only pyth_mobilerobot
(rollout_bwd.hip ssb_fuse_kind); the vehicle forms take one tile per workgroup, so only mobilerobot has a second-pass case."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import (DONE_MARGIN, _net_f64, as_f64, batch_with_done, flat_grads, fp32_seeded_noise_floor, hip_env_from_oracle,
                     one_row_seeded_gradients, padded_batch, reference_init_nets, rollout_history, rows_near_origin, seeded_gradients_f64, spread_tracking_errors, to_device,
                     appended_points)
from oracle import adp_oracle as orc
from test_per_trajectory_gpu import (FWD_ATOL, FWD_RTOL, N_CU, SS_FWD, STREAMED, TOL, VF, W2, W3, _MlpLaunch, _described_mlp, _grad_errors,
                                     make_gv, selected_rows)

from gops_amd.utils.synthetic import act_dim_of, make_batch, obs_dim_of

pytestmark = pytest.mark.gpu

VF_NO_SS_BWD = 0x4   # GOPS_VF_NO_STREAMED_SPLIT_BWD

# A row takes part in a seed only if, at every step and for every constraint k of its float64 trajectory,
#   KINK_MARGIN   the constraint's own formula is away from a change of branch (helpers.constraint_kink_gap: the two smallest
#                 circle-pair distances, the two ego circles against the road, |y| = 0 of the error constraints) - every
#                 constraint seed of the row, `constraint_sums` row 0 and `grad_constraint_step` included;
#   C_MARGIN      |c|, |c + 0.7| and |c - 0.35| (max(c, 0)'s and Phi's clamp's kinks) - `constraint_sums` row 1, the Phi products,
#                 the 0 / 1 outputs;
#   C_MARGIN_LOG  |c| - `constraint_sums` row 2: d/dc log(-c + 1e-8) = 1 / c multiplies fp32's error in c.
# Chosen from the fp32 oracle against the float64 one (helpers.fp32_seeded_noise_floor; never from the kernels): with C_MARGIN =
# 1e-2 the Phi-product gradient of the surrcstr batches was 3.7e-5 to 5.5e-5 (weighted) and up to 1.7e-4 (one row) away, above
# TOL / 3; with 5e-2 every source of every case is within 2.3e-5 (weighted) and 1.9e-5 (single rows).  C_MARGIN_LOG: 1e-1 is the
# largest the errcstr models admit (c >= -0.2; at 2e-1 no feasible row is left); at 1e-1 every case meets TOL / 3.  KINK_MARGIN
# 1e-2 was not varied.  What the margins cannot remove is the cancellation in `state - reference` at coordinates of ~100 m: on
# some batches single rows miss TOL / 3, and those cases use another seed (prepare asserts the floors for every case).
KINK_MARGIN = 1e-2
C_MARGIN = 5e-2
C_MARGIN_LOG = 1e-1


# pyth_veh3dofconti_surrcstr_penalty: the reward's collision penalty 15 (tanh(max(8 - 16 dis, 0) - 4) + 1) has a slope of up to
# 240 / m in the circle distance dis.  On a make_batch batch (coordinates of ~100 m, one fp32 ulp 7.6e-6 m) the fp32 ORACLE is
# 17.8 (rewards) and 10.6 (v_pi) tolerances away from float64, and so are the kernels (17.8 / 10.5; 40 seeds: 2.9 to 18): the bar
# cannot bind there.  The case's batch is therefore (a) taken from rows with a reference time below 1.5 s
# (helpers.rows_near_origin: coordinates below 16 m, one ulp <= 9.5e-7 m), which brings the fp32 oracle to 0.8 .. 1.3
# tolerances, and (b) cleared of rows that pass through the steep part of the penalty: a row is replaced if at any step of its
# float64 trajectory slope(dis_t) * PENALTY_DC exceeds a third of that reward's tolerance, with PENALTY_DC = 1e-6 m - one ulp of
# a coordinate between 8 and 16 m, the error fp32 is granted in the distance.  Saturated (dis < ~0.2 m, penalty ~30) and far rows
# stay.  prepare asserts the fp32 oracle's forward outputs within 0.9 tolerances for this case like for every other.
PENALTY_DC = 1e-6


def _penalty_too_steep(hist):
    """Rows [B] whose collision penalty would turn an error of PENALTY_DC in the distance into more than a third of the reward's
    tolerance at some step (float64 history of the penalty model: constraints = -dis of the pose the reward is taken at)."""
    x = torch.clamp_min(8.0 + 16.0 * hist["constraints"][:, :, 0], 0.0)
    slope = 15.0 * 16.0 / torch.cosh(x - 4.0) ** 2 * (x > 0)
    return (slope * PENALTY_DC > (FWD_ATOL + FWD_RTOL * hist["rewards"].abs()) / 3).any(0)


def _c(alg, env_id, batch, horizon, hidden, act, gamma, variant, flags=0, wg=(1,), seed=3, **extra):
    return dict(alg=alg, env_id=env_id, batch=batch, horizon=horizon, hidden=hidden, act=act, gamma=gamma, variant=variant,
                flags=flags, tile=16, wg=wg, dtype=None, seed=seed, **extra)


SURR, DETOUR, PENALTY, ERR, VEH2, MOB = ("pyth_veh3dofconti_surrcstr", "pyth_veh3dofconti_detour", "pyth_veh3dofconti_surrcstr_penalty",
                                         "pyth_veh3dofconti_errcstr", "pyth_veh2dofconti_errcstr", "pyth_mobilerobot")
CASES = {
    # streamed plane-split forward + sweep (the sweep: two workgroups per CU; only mobilerobot's walks its tiles grid-stride)
    "ss_surr_n1": _c("FHADP", SURR, 203, 6, W2, "elu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, surr_veh_num=1),
    "ss_surr_p5_n2": _c("FHADP", SURR, 16 * 21 + 9, 8, W2, "gelu", 0.97, SS_FWD, wg=(1, 2), pre_horizon=5, surr_veh_num=2, seed=27),
    "ss_detour": _c("FHADP", DETOUR, 16 * 17 + 5, 7, W2, "tanh", 0.98, SS_FWD, wg=(1, 2), pre_horizon=10, seed=5),
    "ss_penalty": _c("FHADP", PENALTY, 16 * 14 + 3, 6, W2, "elu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, seed=6),
    "ss_errcstr": _c("FHADP", ERR, 16 * 19 + 11, 7, W2, "gelu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, seed=7),
    "ss_veh2_errcstr": _c("FHADP", VEH2, 16 * 12 + 7, 7, W2, "relu", 0.98, SS_FWD, wg=(1, 2), pre_horizon=10, seed=8),
    "ss_mob": _c("FHADP", MOB, 16 * 15 + 13, 8, W2, "elu", 0.97, SS_FWD, wg=(1, 2), seed=9),
    "ss_mob_walk": _c("FHADP", MOB, 2 * 4096 + 16 * 5 + 7, 3, W2, "gelu", 0.99, SS_FWD, wg=(1, 2), seed=10),
    "ss_surr_3x256": _c("FHADP", SURR, 16 * 9 + 2, 6, W3, "relu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, surr_veh_num=1, seed=11),
    "ss_mob_h1": _c("FHADP", MOB, 16 * 7 + 3, 1, W2, "relu", 0.99, SS_FWD, wg=(1, 2), seed=22),   # (a vehicle's constraint after ONE step does not depend on the action)
    # the same launches on the fp32-MFMA sweep (plane-split forward)
    "ssf_surr_f32_sweep": _c("FHADP", SURR, 203, 6, W2, "elu", 0.99, SS_FWD, flags=VF_NO_SS_BWD, pre_horizon=10, surr_veh_num=1),
    "ssf_detour_f32_sweep": _c("FHADP", DETOUR, 16 * 11 + 6, 6, W2, "gelu", 1.0, SS_FWD, flags=VF_NO_SS_BWD, pre_horizon=10, seed=12),
    # plain streamed fp32
    "plain_surr_256": _c("FHADP", SURR, 16 * 10 + 5, 6, W2, "tanh", 0.99, STREAMED, flags=VF["STREAMED_FP32"], pre_horizon=10, surr_veh_num=1, seed=34),
    "plain_veh2_errcstr_128_64": _c("FHADP", VEH2, 16 * 6 + 3, 7, (128, 64), "gelu", 0.98, STREAMED, flags=VF["STREAMED_FP32"] | VF["NO_NARROW_LDS"], pre_horizon=10, seed=14),
    # narrow policies: LDS-resident (obs-64-64-act: the written-out form) and streamed from L2
    "narrow_surr_64_64": _c("FHADP", SURR, 16 * 5 + 4, 6, (64, 64), "elu", 0.99, STREAMED, pre_horizon=10, surr_veh_num=1, seed=15),
    "narrow_errcstr_32_32": _c("FHADP", ERR, 16 * 4 + 9, 6, (32, 32), "tanh", 0.97, STREAMED, pre_horizon=10, seed=16),
    "narrow_mob_64_64_no_lds": _c("FHADP", MOB, 16 * 6 + 5, 6, (64, 64), "gelu", 0.98, STREAMED, flags=VF["NO_NARROW_LDS"], seed=17),
    # INFADP-style: no time input, a tail value net; SPIL's evaluation target does not mask the tail at done
    "ss_surr_tail": _c("INFADP", SURR, 16 * 13 + 8, 6, W2, "gelu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, surr_veh_num=1, seed=48),
    "ss_mob_tail_unmasked": _c("INFADP", MOB, 16 * 12 + 10, 6, W2, "elu", 0.98, SS_FWD, wg=(1, 2), seed=19, tail_unmasked=True),
    # no MaskAtDoneModel in the chain
    "ss_veh2_errcstr_no_mask": _c("FHADP", VEH2, 16 * 8 + 5, 6, W2, "elu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, seed=43, mask_at_done=False),
    "ss_mob_no_mask": _c("FHADP", MOB, 16 * 9 + 7, 6, W2, "tanh", 0.98, SS_FWD, wg=(1, 2), seed=21, mask_at_done=False),
}
SOURCES = ("gv", "gc", "gp", "gs")
_ROW_GC, _ROW_K = (1.0, -0.7, 0.3), (1.0, -0.5, 0.25)   # one row's seed over the rows of constraint_sums / over the constraints


# ---- a case's inputs, float64 results and premises (no GPU) ---------------------------------------------------------------------
_PREPARED = {}


def build_case(name):
    case = CASES[name]
    cfg = {k: v for k, v in case.items() if k in ("alg", "env_id", "batch", "horizon", "hidden", "act", "gamma", "pre_horizon", "surr_veh_num")}
    fh = case["alg"] == "FHADP"
    env = orc.make_env(cfg["env_id"], pre_horizon=cfg.get("pre_horizon", 10), surr_veh_num=cfg.get("surr_veh_num"),
                       mask_at_done=case.get("mask_at_done", True))
    nets = reference_init_nets(cfg, case["seed"], obs_dim_of(cfg), act_dim_of(cfg))
    return cfg, env, nets["policy"], None if fh else nets["v_target"]


def _clear_of_bounds(cfg, case, env, policy, data, keep, fh):
    """Rows (other than `keep`) that come within 2 DONE_MARGIN of a termination bound in float64 are replaced by the same row of
    another seed's batch: neither fp32 nor the kernels are asked to decide a termination that close.  The penalty model: also the
    rows of _penalty_too_steep."""
    B, H = cfg["batch"], cfg["horizon"]
    for attempt in range(1, 10):
        with torch.no_grad():
            hist = rollout_history(as_f64(env), as_f64(policy), as_f64(data), H, 1.0, fh)
        near = hist["margin"].min(0).values < 2 * DONE_MARGIN
        if env.get("penalty"):
            near = near | _penalty_too_steep(hist)
        bad = [r for r in near.nonzero().flatten().tolist() if r not in keep]
        if not bad:
            return
        other = make_batch(cfg, case["seed"] + 500 * attempt)
        if env.get("penalty"):
            rows_near_origin(cfg, env, other, pool_seed=case["seed"] + 500 * attempt)
        if "ref_appended" in data:
            other["ref_appended"] = appended_points(cfg, other)
        for k, v in data.items():
            if k in other and torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B:
                v[bad] = other[k][bad]
    raise AssertionError("rows on a termination bound")


def make_seeds(case, H, nc, masks):
    """gv [B], gc [3, B], gp [n_c, B], gs [H, B, n_c]: drawn like make_gv (mixed signs, three decades, scale 1 / B), zero where
    the row's margins do not admit the source."""
    B, tile, seed = case["batch"], case["tile"], case["seed"]
    gc = torch.stack([make_gv(B, tile, seed + 11 * (r + 1)) for r in range(3)])
    gp = torch.stack([make_gv(B, tile, seed + 37 * (k + 1)) for k in range(nc)])
    gs = torch.stack([torch.stack([make_gv(B, tile, seed + 101 * (t + 1) + 7 * k) for k in range(nc)], 1) for t in range(H)]) / H
    gc = gc * torch.stack((masks["kink"], masks["c"], masks["log"])).float()
    return dict(gv=make_gv(B, tile, seed), gc=gc.contiguous(), gp=(gp * masks["c"].float()).contiguous(), gs=(gs * masks["kink"].float()[None, :, None]).contiguous())


def seed_sets(seeds):
    sets = {"all": seeds, "cons": dict(seeds, gv=None)}
    sets.update({k: {k: seeds[k]} for k in SOURCES})
    return sets


def _t0(i, H):
    """The step a row's `grad_constraint_step` one-hot sits on: spread over 2 .. H - 1 (a vehicle's pose at step t depends on the
    actions up to t - 2: earlier steps have no policy gradient)."""
    return 2 + i % (H - 2) if H >= 3 else H - 1


def row_seed_values(i, H, nc, masks):
    """The one-row seeds of row i, per source: (index of the source's own axes, values)."""
    k3 = torch.tensor(_ROW_K[:nc])
    return dict(gv=torch.tensor(1.0), gc=torch.tensor(_ROW_GC) * torch.tensor([float(masks[m][i]) for m in ("kink", "c", "log")]),
                gp=k3 * float(masks["c"][i]), gs=k3 * float(masks["kink"][i]), t0=_t0(i, H))


def row_seeds(i, k, n, H, nc, masks):
    """{source: seeds over a batch of n rows, non-zero in row k only} with row i's values."""
    val = row_seed_values(i, H, nc, masks)
    gv, gc, gp, gs = torch.zeros(n), torch.zeros(3, n), torch.zeros(nc, n), torch.zeros(H, n, nc)
    gv[k], gc[:, k], gp[:, k], gs[val["t0"], k] = val["gv"], val["gc"], val["gp"], val["gs"]
    return dict(gv=dict(gv=gv), gc=dict(gc=gc), gp=dict(gp=gp), gs=dict(gs=gs))


def _ratio(got, want, rtol, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max()) if got.size else 0.0


def prepare(name, floors=True):
    """Inputs, float64 results and the asserted premises of a case (cached)."""
    if (name, floors) in _PREPARED:
        return _PREPARED[(name, floors)]
    case = CASES[name]
    cfg, env, policy, value = build_case(name)
    B, H, tile, fh, unmasked = cfg["batch"], cfg["horizon"], case["tile"], case["alg"] == "FHADP", bool(case.get("tail_unmasked"))
    kind, penalty, masked = env["kind"], bool(env.get("penalty")), env.get("mask_at_done", True)
    nc = env["n_constraint"]
    ntiles = -(-B // tile)
    walks = kind == "mob" and ntiles > 2 * N_CU
    n_wg = (2 if walks else 1) * N_CU
    data, done_rows, term_rows = batch_with_done(cfg, case["seed"], env, policy, tile, n_wg, finite_horizon=fh,
                                                 shape_batch=spread_tracking_errors if kind in ("veh_err", "veh2") else rows_near_origin if penalty else None)
    _clear_of_bounds(cfg, case, env, policy, data, set(done_rows) | set(term_rows), fh)
    data["obs2"] = data["obs"].clone()
    rows = selected_rows(dict(case, wg=(2,) if walks else (1,)), done_rows, term_rows) if B > 1 else [0]

    # float64, first without seeds: the trajectories decide which rows take which seed
    with torch.no_grad():
        hist = rollout_history(as_f64(env), as_f64(policy), as_f64(data), H, cfg["gamma"], fh, None if value is None else as_f64(value), unmasked)
    c = hist["constraints"]                                                          # [H, B, n_c]
    near = torch.minimum(torch.minimum(c.abs(), (c + 0.7).abs()), (c - 0.35).abs()).amin((0, 2))
    masks = dict(kink=hist["kink_gap"].amin(0) >= KINK_MARGIN)
    masks["c"] = masks["kink"] & (near >= C_MARGIN)
    masks["log"] = masks["c"] & (c.abs().amin((0, 2)) >= C_MARGIN_LOG)
    seeds = make_seeds(case, H, nc, masks)
    sets = seed_sets(seeds)
    ref, grads = seeded_gradients_f64(env, policy, data, H, cfg["gamma"], fh, sets, value, unmasked)
    rs = lambda i, k, n=len(rows): row_seeds(i, k, n, H, nc, masks)
    rows64 = one_row_seeded_gradients(as_f64(env), _net_f64(policy), as_f64(data), H, cfg["gamma"], fh, rows, rs,
                                      None if value is None else _net_f64(value, False), unmasked)

    # premises: special rows
    n_special = min(3, max(0, (B - 1) // 4))
    first_done = H - ref["done_hist"].sum(0)
    on_entry = (data["done"] != 0).nonzero().flatten().tolist()
    inside = [r for r in range(B) if r not in on_entry and 1 <= int(first_done[r]) + 1 <= H - 1]
    last_tile = (B - 1) // tile
    edge = lambda r: r % tile in (0, tile - 1)
    assert sorted(on_entry) == sorted(done_rows) and len(on_entry) >= n_special, (name, on_entry)
    assert any(edge(r) for r in on_entry) and any(r // tile == last_tile for r in on_entry), name
    terminates = not penalty and H >= 2 and masked
    if penalty:
        assert not bool(ref["done_hist"][:, [r for r in range(B) if r not in on_entry]].any()), "the penalty model never reports done"
    if terminates:
        assert set(term_rows) <= set(inside) and len(inside) >= n_special, (name, term_rows, inside)
        assert any(edge(r) for r in inside) and any(r // tile == last_tile for r in inside), name
    if walks:
        t2 = n_wg * tile
        assert any(r // tile == n_wg for r in on_entry) and any(r // tile == n_wg for r in inside), (name, t2)
    assert float(ref["margin"].min()) >= DONE_MARGIN, (name, "a row sits on a termination bound", float(ref["margin"].min()))
    if masked:
        assert bool(ref["done_hist"][:, on_entry].all())
    # ... rows that are done on entry: what their constraints do
    if masked and H >= 2 and on_entry:
        moving = (c[1:, on_entry] - c[:-1, on_entry]).abs().amax((0, 2))
        if kind in ("veh_err", "veh2"):
            assert float(moving.max()) == 0.0, (name, "errcstr: the constraint of a done row is constant")
        elif kind == "veh_surr":
            assert float(moving.min()) > 1e-3, (name, "surr forms: the constraint of a done row keeps moving", moving)
    # ... margins and caps
    full = masks["log"]
    problems = []   # (the premises about margins and floors are reported together: one run says what a case's batch lacks)
    if int(full.sum()) * 2 < B:
        problems.append(("fewer than half of the rows keep every seed", int(full.sum()), B))
    groups = {"first tile": range(min(tile, B)), "ragged tile": range(last_tile * tile, B)}
    if masked:
        groups["done on entry"] = on_entry
    if terminates:
        groups["terminating"] = inside
    if walks:
        groups["second-pass tile"] = range(n_wg * tile, min((n_wg + 1) * tile, B))
    for what, group in groups.items():
        if not any(bool(full[r]) for r in group):
            problems.append(("no row keeps every seed in", what))
    cf = c[:, full]
    if not (bool((cf > 0).any()) and bool((cf < 0).any())):
        problems.append(("seeded rows need violated and satisfied constraints",))
    if not bool((cf < 0).all(2).all(0).any()):
        problems.append(("no fully feasible seeded row: constraint_sums row 2 would carry no gradient",))
    gv = seeds["gv"]
    assert int(gv.abs().argmax()) >= tile and gv.abs().max() / gv.abs().min() > 100 and (gv > 0).any() and (gv < 0).any()
    # ... what the one-row gradients of a done row must be, on the float64 side
    for i in on_entry if masked else ():
        if i not in rows64:
            continue
        assert float(flat_grads(rows64[i]["gv"]).norm()) == 0.0, (name, i)
        for src in ("gc", "gp", "gs"):
            norm = float(flat_grads(rows64[i][src]).norm())
            if kind in ("veh_err", "veh2") or penalty:
                assert norm == 0.0, (name, i, src, norm)
        if kind == "veh_surr" and not penalty and bool(masks["kink"][i]) and _t0(i, H) >= 1:
            assert float(flat_grads(rows64[i]["gs"]).norm()) > 0.0, (name, i, "a done row of a surr form has a constraint gradient")
    if penalty:
        assert all(float(flat_grads(grads[s]).norm()) == 0.0 for s in ("cons", "gc", "gp", "gs")), name
        assert all(torch.equal(a, b) for a, b in zip(grads["all"], grads["gv"])), name

    out = dict(case=case, cfg=cfg, env=env, policy=policy, value=value, data=data, seeds=seeds, sets=sets, masks=masks, rows=rows,
               ref=ref, grads=grads, rows64=rows64, done_rows=done_rows if masked else [], term_rows=inside if terminates and masked else [],
               first_done=first_done, fh=fh, nc=nc, penalty=penalty, masked=masked, unmasked=unmasked, walks=walks, gv=seeds["gv"])
    if floors:
        # the forward bar binds only where fp32 itself meets it: the fp32 oracle's outputs against the float64 ones, as the GPU
        # test compares them (worst |error| / (atol + rtol |want|))
        with torch.no_grad():
            o32 = rollout_history(env, policy, data, H, cfg["gamma"], fh, value, unmasked)
        ml = masks["log"].numpy()
        out["fwd_floor"] = {key: _ratio(got.double().numpy(), want.numpy(), FWD_RTOL, terms * FWD_ATOL) for key, got, want, terms in (
            ("rewards", o32["rewards"], ref["rewards"], 1), ("final_obs", o32["final_obs"], ref["final_obs"], 1),
            ("v_pi", o32["v"], ref["v"], H + (0 if fh else 1)), ("constraints", o32["constraints"], ref["constraints"], 1),
            ("sums01", o32["sums"][:2], ref["sums"][:2], H * nc), ("sums2", o32["sums"][2][ml], ref["sums"][2][ml], H * nc),
            ("prods", o32["prods"][:nc], ref["prods"][:nc], H))}
        for key, ratio in out["fwd_floor"].items():
            if ratio > 0.9:
                problems.append(("fp32 oracle to float64, forward", key, ratio))
        floor, floor_rows = fp32_seeded_noise_floor(env, policy, data, H, cfg["gamma"], fh, sets, grads, rows, rs, rows64, value, unmasked)
        out["floor"], out["floor_rows"] = floor, floor_rows
        out["floor_row_worst"] = {s: max(fr[s] for fr in floor_rows.values()) for s in SOURCES}
        if max(floor.values()) > TOL / 3:
            problems.append(("fp32 oracle to float64, weighted gradients", floor))
        if max(out["floor_row_worst"].values()) > TOL / 3:
            problems.append(("fp32 oracle to float64, single rows", out["floor_row_worst"]))
    out["problems"] = problems
    assert not problems, (name, problems)
    _PREPARED[(name, floors)] = out
    return out


def rollout_desc(name):
    """The case's launch description without a device: what gops_rollout_variant is asked about."""
    from gops_amd import hip_backend as hb
    case = CASES[name]
    cfg, env, policy, value = build_case(name)
    d = hb.GopsRolloutDesc()
    d.dtype = hb.dtype_id(None)
    d.variant_flags = case["flags"]
    d.batch, d.horizon, d.finite_horizon = cfg["batch"], cfg["horizon"], int(case["alg"] == "FHADP")
    d.need_grad, d.tail_value, d.gamma = 1, int(value is not None), float(cfg["gamma"])
    d.tail_unmasked = int(bool(case.get("tail_unmasked")))
    d.env = hip_env_from_oracle(env, policy)
    d.policy = _described_mlp(policy)
    if value is not None:
        d.value = _described_mlp(value)
    return d


# ---- launches -------------------------------------------------------------------------------------------------------------------
class _Launch(_MlpLaunch):
    def rollout(self, B):
        from gops_amd import hip_backend as hb
        case, cfg = self.prep["case"], self.prep["cfg"]
        ro = hb.Rollout(self.henv, self.pol, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=self.prep["fh"],
                        need_grad=True, value=None if self.vt is None else self.vt[0], variant_flags=case["flags"],
                        tail_unmasked=self.prep["unmasked"])
        return ro, hb.lib().gops_rollout_variant(ctypes.byref(ro.desc))

    def backward(self, ro, seeds, prods):
        """`seeds`: dict with any of gv / gc / gp / gs; `prods`: the [n_c, B] Phi products the ABI's grad_constraint_prod is formed with."""
        B = ro.desc.batch
        dev_ = lambda t: None if t is None else t.float().to(self.dev).contiguous()
        gv = seeds.get("gv")
        gp = seeds.get("gp")
        gw, gb = [torch.full_like(w, float("nan")) for w in self.ws], [torch.full_like(b, float("nan")) for b in self.bs]
        ro.backward(dev_(torch.zeros(B) if gv is None else gv), gw, gb, grad_constraint=dev_(seeds.get("gc")),
                    grad_constraint_prod=None if gp is None else dev_(gp.double() * prods.double()), grad_constraint_step=dev_(seeds.get("gs")))
        torch.cuda.synchronize()
        return [t.cpu() for pair in zip(gw, gb) for t in pair]


def _scaled(seeds, f):
    return {k: (None if v is None else v * f) for k, v in seeds.items()}


def _masked(seeds, m):
    """Seeds times a per-row mask m [B]."""
    shape = dict(gv=m, gc=m[None], gp=m[None], gs=m[None, :, None])
    return {k: (None if v is None else v * shape[k]) for k, v in seeds.items()}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert torch.cuda.get_device_properties(0).multi_processor_count == N_CU, "the cases' batches are laid out for 256 CUs"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(CASES))
def test_constrained_rollout_per_trajectory(name, dev):
    prep = prepare(name)
    case, cfg, data, ref, seeds, sets, grads, masks = (prep[k] for k in ("case", "cfg", "data", "ref", "seeds", "sets", "grads", "masks"))
    B, H, tile, fh, nc, penalty = cfg["batch"], cfg["horizon"], case["tile"], prep["fh"], prep["nc"], prep["penalty"]
    launch = _Launch(prep, dev)
    ro, variant = launch.rollout(B)
    assert variant == case["variant"], "the launch would not take the kernels under test"
    ro.workspace.fill_(0xFF)
    ddev = to_device(data, dev)
    fwd = lambda r, d: {k: v.cpu() for k, v in r.forward(d, want_rewards=True, want_final=True, want_constraints=True).items()}
    res = fwd(ro, ddev)
    measured = {}

    # 1. forward, row by row
    on_entry, first_done = prep["done_rows"], prep["first_done"]
    assert np.array_equal(res["final_done"].numpy() != 0, ref["final_done"].numpy())
    assert torch.equal(res["rewards"][:, on_entry], torch.zeros(H, len(on_entry)))
    assert torch.equal(res["final_obs"][on_entry], data["obs"][on_entry])
    assert torch.equal(res["v_pi"][on_entry], torch.zeros(len(on_entry))) or prep["unmasked"]
    for r in prep["term_rows"]:
        assert torch.equal(res["rewards"][int(first_done[r]) + 1:, r], torch.zeros(H - int(first_done[r]) - 1)), r
    n_terms = H + (0 if fh else 1)
    mc, ml = masks["c"].numpy(), masks["log"].numpy()   # (the margin premises: rows whose every |c_tk| clears C_MARGIN / C_MARGIN_LOG)
    checks = [("rewards", res["rewards"], ref["rewards"], 1), ("final_obs", res["final_obs"], ref["final_obs"], 1), ("v_pi", res["v_pi"], ref["v"], n_terms),
              ("constraints", res["constraints"], ref["constraints"], 1),   # (all rows, the ones done on entry included)
              ("sums01", res["constraint_sums"][:2], ref["sums"][:2], H * nc),
              ("sums2", res["constraint_sums"][2][ml], ref["sums"][2][ml], H * nc),   # (a sum of logarithms: over the rows of the C_MARGIN_LOG premise)
              ("prods", res["constraint_prods"][:nc], ref["prods"][:nc], H)]
    if "final_state" in res:
        checks.append(("final_state", res["final_state"], ref["final_state"][:, :res["final_state"].shape[1]], 1))
    for key, got, want, terms in checks:
        got, want = got.double().numpy(), want.numpy()
        measured["fwd_" + key] = _ratio(got, want, FWD_RTOL, terms * FWD_ATOL)   # (<= 1 passes)
        print(f"{name}: {key} worst |error| / (atol + rtol |want|) = {measured['fwd_' + key]:.3f}")
    fwd_missed = {k[4:]: v for k, v in measured.items() if k.startswith("fwd_") and not v <= 1.0}   # (asserted at the end: the gradient checks run first)
    assert np.array_equal(res["constraint_sums"][3].numpy()[mc], ref["sums"][3].numpy()[mc]), (name, "feasible flag")
    assert np.array_equal(res["constraint_prods"][nc:].numpy()[:, mc], ref["prods"][nc:].numpy()[:, mc]), (name, "safe flags")

    # 2. weighted gradients: every source at once, each alone, constraint seeds with grad_v = 0 - with the float64 Phi products
    #    and with the GPU's own
    p64, pgpu = ref["prods"][:nc], res["constraint_prods"][:nc]
    g = {}
    for s, sd in sets.items():
        for tag, prods in (("", p64), ("_own_prods", pgpu)):
            if tag and "gp" not in sd:
                continue
            got = launch.backward(ro, sd, prods)
            assert all(torch.isfinite(t).all() for t in got), (name, s)
            g[s + tag] = got
            if penalty and s != "all" and s != "gv":
                assert all(float(t.abs().max()) == 0.0 for t in got), (name, s, "the penalty model's constraint outputs carry no gradient")
                continue
            measured["w_" + s + tag] = _grad_errors(got, grads[s])
    print(f"{name}: weighted gradients to float64 (flat, worst tensor): " + ", ".join(f"{k[2:]}: {v[0]:.2e} / {v[1]:.2e}" for k, v in measured.items() if k.startswith("w_")))
    print(f"{name}: fp32 oracle: " + ", ".join(f"{k}: {v:.2e}" for k, v in prep.get("floor", {}).items()))
    late = []   # (what is known to miss is asserted at the end: every other check of the case runs first)
    if penalty:
        measured["penalty_all_to_gv"] = _grad_errors(g["all"], g["gv"])
        print(f"{name}: gradient with every seed to the grad_v-only gradient: {measured['penalty_all_to_gv'][0]:.2e} / {measured['penalty_all_to_gv'][1]:.2e}")
        if not all(torch.equal(a, b) for a, b in zip(g["all"], g["gv"])):
            late.append(("constraint seeds changed the penalty model's gradient (flat, worst tensor)", measured["penalty_all_to_gv"]))
    for k, v in measured.items():
        if k.startswith("w_"):
            assert v[0] < TOL and v[1] < TOL, (name, k, v)

    # 3. linearity and call-to-call state
    g2 = launch.backward(ro, _scaled(seeds, 1e-4), p64)
    e_flat, e_worst = _grad_errors([1e4 * t for t in g2], grads["all"])
    measured["scaled_flat"] = e_flat
    assert e_flat < TOL and e_worst < TOL, (name, "backward(1e-4 seeds)", e_flat, e_worst)
    launch.backward(ro, seeds, p64)
    after = launch.backward(ro, sets["gv"], p64)                # grad_v only, straight after a call with every seed ...
    ro_fresh, _ = launch.rollout(B)
    ro_fresh.workspace.fill_(0xFF)
    fwd(ro_fresh, ddev)
    fresh = launch.backward(ro_fresh, sets["gv"], p64)          # ... and from a rollout that never saw one
    del ro_fresh
    for a, b in zip(after, fresh):
        assert torch.equal(a, b), "a seed pointer or a scale outlives its backward call"
    again = launch.backward(ro, seeds, p64)
    for a, b in zip(g["all"], again):
        assert torch.equal(a, b), "a backward call depends on the call before it"
    even = ((torch.arange(B) // tile) % 2 == 0).float()
    ga, gb = launch.backward(ro, _masked(seeds, even), p64), launch.backward(ro, _masked(seeds, 1 - even), p64)
    e_flat, e_worst = _grad_errors([a + b for a, b in zip(ga, gb)], grads["all"])
    measured["even_odd_flat"] = e_flat
    assert e_flat < TOL and e_worst < TOL, (name, "even + odd tiles", e_flat, e_worst)

    # 4. one row at a time, one source at a time
    row_err = {s: {} for s in SOURCES}
    for i in prep["rows"]:
        hot = row_seeds(i, i, B, H, nc, masks)
        for s in SOURCES:
            gi = launch.backward(ro, hot[s], p64)
            want = prep["rows64"][i][s]
            assert all(torch.isfinite(t).all() for t in gi), (name, i, s)
            if float(flat_grads(want).norm()) == 0.0:   # grad_v of a done row, any seed of an errcstr / penalty done row, a zero seed
                assert all(float(t.abs().max()) == 0.0 for t in gi), (name, i, s, "a gradient where float64 has exactly none")
                continue
            row_err[s][i] = rel_l2(flat_grads(gi), flat_grads(want))
    measured["rows"] = {s: {str(i): e for i, e in d.items()} for s, d in row_err.items()}
    measured["row_worst"] = {s: max(d.values(), default=0.0) for s, d in row_err.items()}
    for s in SOURCES:
        print(f"{name}: one-row gradients to float64, {s}: " + ", ".join(f"{i}: {e:.2e}" for i, e in row_err[s].items()))
    print(name, json.dumps({k: v for k, v in measured.items() if k != "rows"}, sort_keys=True))
    if prep["masked"] and prep["env"]["kind"] == "veh_surr" and not penalty:
        assert any(i in row_err["gs"] for i in on_entry if i in prep["rows"]), (name, "no done row's constraint gradient was compared")
    assert max(measured["row_worst"].values()) < TOL, (name, measured["row_worst"])

    # 5. rows beyond the batch are inert
    extra = tile + 3
    pad = padded_batch(cfg, case["seed"], prep["env"], data, extra)
    z = lambda t, dim: torch.cat((t, torch.zeros(*[extra if d == dim else n for d, n in enumerate(t.shape)])), dim)
    seeds_pad = dict(gv=z(seeds["gv"], 0), gc=z(seeds["gc"], 1), gp=z(seeds["gp"], 1), gs=z(seeds["gs"], 1))
    p64_pad = z(p64, 1)
    runs = []
    for fill, (d_in, s_in, p_in, n) in zip((0x00, None, 0xFF, None), ((data, seeds, p64, B), (pad, seeds_pad, p64_pad, B + extra)) * 2):
        ro_n, variant_n = launch.rollout(n)
        assert variant_n == variant
        if fill is None:
            ro_n.workspace.random_(0, 256)
        else:
            ro_n.workspace.fill_(fill)
        out = fwd(ro_n, to_device(d_in, dev))
        runs.append(([out[k][..., :B] if k in ("rewards", "constraint_sums", "constraint_prods") else (out[k][:, :B] if k == "constraints" else out[k][:B])
                      for k in ("v_pi", "rewards", "final_obs", "constraints", "constraint_sums", "constraint_prods")], launch.backward(ro_n, s_in, p_in)))
        del ro_n
    mine = [res[k] for k in ("v_pi", "rewards", "final_obs", "constraints", "constraint_sums", "constraint_prods")]
    for outs, gr in runs:
        assert all(torch.equal(a, b) for a, b in zip(outs, mine)), name
        e_flat, e_worst = _grad_errors(gr, grads["all"])
        assert e_flat < TOL and e_worst < TOL, (name, "padded batch", e_flat, e_worst)
        assert _grad_errors(gr, g["all"])[0] < TOL
    if fwd_missed:
        late.append(("forward outputs beyond rtol / atol (worst |error| / (atol + rtol |want|))", fwd_missed))
    assert not late, (name, late)
