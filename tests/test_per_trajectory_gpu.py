"""GPU: the rollout kernels one trajectory at a time.  Every kernel family (register-stationary plane-split / exact fp32, streamed
plane-split forward and sweep, plain streamed fp32, LDS-resident narrow forms, half precision on 16- and 64-row tiles, ActionRepeat,
the per-lane POLY rollout) against the float64 evaluation of the oracle with what the other GPU modules leave out:

* a `grad_v` that differs from row to row (mixed signs, three decades), so that a sweep reading the wrong row's weight - or a
  scale derived from max|grad_v| that outlives its call - changes the result;
* element-wise forward checks over ALL rows and the gradient of ONE trajectory (one-hot `grad_v`) on the rows where tiled,
  grid-stride kernels go wrong (helpers.edge_rows), instead of norms and sums over the batch;
* batches with rows that are done on entry and rows that terminate strictly inside the horizon (helpers.batch_with_done), on
  tile edges, in the ragged tile and in the first tile of a workgroup's second pass;
* rows beyond the batch (a longer batch with the same head, the workspace pre-filled with other bytes) that must not matter.

`prepare(name)` needs no GPU: it builds a case's inputs and float64 results and asserts the premises (enough special rows, a
margin between every deciding quantity and its termination bound, an fp32-to-float64 oracle distance of at most TOL / 3 for the
weighted and for every single-row gradient).  tests/test_host_cpu.py runs it for every case, and pins every case to the kernel
family it was written for (`gops_rollout_variant`)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden, rel_l2
from helpers import (DONE_MARGIN, batch_with_done, edge_rows, edge_tiles, flat_grads, fp32_weighted_noise_floor, hip_env_from_oracle,
                     hip_mlp_from_net, one_row_gradients_f64, oracle_env, reference_init_nets, take_rows, to_device,
                     weighted_gradient_f64, padded_batch)
from oracle import adp_oracle as orc

from gops_amd.utils.synthetic import act_dim_of, obs_dim_of

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # fp32 families: gradients, relative L2 (per tensor, flat, per selected row)
FWD_RTOL, FWD_ATOL = 1e-5, 2e-5   # fp32 families: per-step quantities, element-wise (v_pi: a sum of H such terms -> H * atol)
TOL_FWD_F16, TOL_GRAD_F16 = 2e-3, 1e-2   # dtype="fp16" (tests/test_f16_gpu.py)
# One row's gradient through the half-precision sweep: twice the worst distance to float64 measured on the MI355X over the rows
# these cases select (DESIGN.md section 2.2 has the table); above 10 * TOL_GRAD_F16 is a bug whatever was measured.
F16_ROW_BOUND = 2 * 1.77e-3   # worst measured: 1.77e-3 (h16_idp, row 128: the first row of the ragged tile)
N_CU = 256                      # MI355X; where the special rows go is fixed by it, so that the CPU tests see the GPU tests' batches

VF = dict(NO_STATIONARY_SPLIT=0x1, NO_STREAMED_SPLIT_FWD=0x2, STREAMED_FP32=0x10, SPLIT_TAIL_MULTI=0x100, NO_NARROW_LDS=0x400, NO_FUSED_DW0=0x4000000)
SPLIT, STAT_F32, SS_FWD, H64, STREAMED = 1, 2, 4, 8, 0   # gops_rollout_variant


def _c(alg, env_id, batch, horizon, hidden, act, gamma, variant, flags=0, tile=16, wg=(1,), dtype=None, seed=3, **extra):
    return dict(alg=alg, env_id=env_id, batch=batch, horizon=horizon, hidden=hidden, act=act, gamma=gamma, variant=variant,
                flags=flags, tile=tile, wg=wg, dtype=dtype, seed=seed, **extra)


W2, W3 = (256, 256), (256, 256, 256)
CASES = {
    # register-stationary plane-split kernels: obs-256-256-act, at most one tile per CU / grid-stride walk beyond
    "split_lq_ragged": _c("FHADP", "pyth_lq", 16 * 37 + 5, 6, W2, "gelu", 0.99, SPLIT, lq_config="s4a2"),
    "split_lq_h1": _c("FHADP", "pyth_lq", 33, 1, W2, "sigmoid", 1.0, SPLIT, lq_config="s6a3"),
    "split_idp": _c("FHADP", "pyth_idpendulum", 130, 10, W2, "gelu", 1.0, SPLIT),
    "split_veh_p10_walk": _c("FHADP", "pyth_veh3dofconti", 4096 + 16 * 9 + 3, 4, W2, "elu", 1.0, SPLIT, pre_horizon=10),
    "split_veh_p30": _c("FHADP", "pyth_veh3dofconti", 200, 8, W2, "elu", 0.99, SPLIT, pre_horizon=30),
    "split_veh_p40_stream_walk": _c("FHADP", "pyth_veh3dofconti", 4096 + 16 * 5 + 7, 3, W2, "elu", 1.0, SPLIT, pre_horizon=40),
    # ... with a tail value net (relu: the tail on exact fp32 products)
    "split_tail_lq_relu": _c("INFADP", "pyth_lq", 3000, 6, W2, "relu", 0.99, SPLIT, lq_config="s4a2", seed=8),
    "split_tail_idp_elu": _c("INFADP", "pyth_idpendulum", 90, 8, W2, "elu", 0.99, SPLIT, seed=9),
    "split_tail_veh_gelu_walk": _c("INFADP", "pyth_veh3dofconti", 4096 + 16 * 11 + 7, 4, W2, "gelu", 0.99, SPLIT,
                                   flags=VF["SPLIT_TAIL_MULTI"], pre_horizon=10, seed=8),
    # register-stationary exact fp32
    "statf32_veh_p10": _c("FHADP", "pyth_veh3dofconti", 205, 6, W2, "elu", 1.0, STAT_F32, flags=VF["NO_STATIONARY_SPLIT"] | VF["NO_STREAMED_SPLIT_FWD"], pre_horizon=10),
    "statf32_idp": _c("FHADP", "pyth_idpendulum", 77, 8, W2, "tanh", 0.97, STAT_F32, flags=VF["NO_STATIONARY_SPLIT"] | VF["NO_STREAMED_SPLIT_FWD"]),
    # streamed plane-split forward + sweep (the sweep: up to two workgroups per CU)
    "sstream_veh_3x256_walk": _c("FHADP", "pyth_veh3dofconti", 2 * 4096 + 16 * 3 + 9, 3, W3, "relu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, seed=6),
    "sstream_veh_2x256_tail_walk": _c("INFADP", "pyth_veh3dofconti", 4800, 4, W2, "elu", 0.99, SS_FWD, wg=(1, 2), pre_horizon=10, seed=5),
    "sstream_cartpole_3x256_tail": _c("INFADP", "gym_cartpoleconti", 200, 5, W3, "gelu", 0.99, SS_FWD, wg=(1, 2), seed=5),
    # (the sweep walks its tiles grid-stride, two workgroups per CU, only in the pyth_lq / cartpole / pendulum / mobilerobot forms:
    #  more than 2 * CUs tiles of those reach a workgroup's second pass; the vehicle / idpendulum forms - veh3dofconti, every
    #  GOPS_ENV_VEH3DOF_SURR form (surrcstr, detour, surrcstr_penalty, errcstr) and veh2dofconti - take one tile per workgroup:
    #  rollout_bwd.hip ssb_fuse_kind.  tests/test_constrained_per_trajectory_gpu.py has the constrained kinds)
    "sstream_lq_2x256_tail_walk": _c("INFADP", "pyth_lq", 2 * 4096 + 16 * 5 + 7, 4, W2, "gelu", 0.99, SS_FWD, wg=(1, 2), lq_config="s4a2", seed=5),
    "sstream_idp_3x256": _c("FHADP", "pyth_idpendulum", 70, 8, W3, "gelu", 1.0, SS_FWD, wg=(1, 2), seed=5),
    # plain streamed fp32
    "plain_veh_256": _c("FHADP", "pyth_veh3dofconti", 150, 6, W2, "elu", 1.0, STREAMED, flags=VF["STREAMED_FP32"], pre_horizon=10),
    "plain_idp_128_64": _c("FHADP", "pyth_idpendulum", 45, 10, (128, 64), "gelu", 0.99, STREAMED, flags=VF["STREAMED_FP32"] | VF["NO_NARROW_LDS"]),
    # narrow policies: weights resident in LDS (obs-64-64-act: the kernels written out for that shape), and streamed from L2
    "narrow_idp_64_64": _c("FHADP", "pyth_idpendulum", 40, 12, (64, 64), "gelu", 0.99, STREAMED, seed=5),
    "narrow_idp_64_64_one_row": _c("FHADP", "pyth_idpendulum", 1, 3, (64, 64), "elu", 0.99, STREAMED, seed=5),
    "narrow_lq_32_32": _c("FHADP", "pyth_lq", 17, 5, (32, 32), "tanh", 0.99, STREAMED, lq_config="s4a2", seed=5),
    "narrow_cartpole_32_32_tail": _c("INFADP", "gym_cartpoleconti", 75, 5, (32, 32), "gelu", 0.99, STREAMED, seed=5),
    "narrow_veh_64_64_no_lds": _c("FHADP", "pyth_veh3dofconti", 100, 8, (64, 64), "elu", 0.99, STREAMED, flags=VF["NO_NARROW_LDS"], pre_horizon=10, seed=5),
    # half precision, 64-row tiles (pyth_lq, 256-wide)
    "h64_lq_b63": _c("FHADP", "pyth_lq", 63, 5, W2, "gelu", 0.99, H64, tile=64, dtype="fp16", lq_config="s4a2"),
    "h64_lq_b65": _c("FHADP", "pyth_lq", 65, 5, W2, "elu", 0.99, H64, tile=64, dtype="fp16", lq_config="s4a2"),
    "h64_lq_walk": _c("FHADP", "pyth_lq", 64 * 300 + 21, 3, W2, "gelu", 0.99, H64, tile=64, dtype="fp16", lq_config="s4a2"),
    "h64_lq_dw0_by_gemm": _c("FHADP", "pyth_lq", 64 * 5 + 30, 4, W2, "gelu", 0.99, H64, flags=VF["NO_FUSED_DW0"], tile=64, dtype="fp16", lq_config="s4a2"),
    "h64_lq_tail": _c("INFADP", "pyth_lq", 64 * 3 + 11, 5, W2, "gelu", 0.99, H64, tile=64, dtype="fp16", lq_config="s4a2", seed=8),
    # half precision, 16-row tiles
    "h16_idp": _c("FHADP", "pyth_idpendulum", 130, 8, W2, "elu", 1.0, STREAMED, dtype="fp16"),
    "h16_veh_128_256": _c("FHADP", "pyth_veh3dofconti", 90, 6, (128, 256), "gelu", 0.97, STREAMED, dtype="fp16", pre_horizon=10),
    # ActionRepeat
    "repeat2_idp": _c("FHADP", "pyth_idpendulum", 53, 5, (64, 64), "gelu", 0.99, STREAMED, repeat_num=2, seed=5),
    "repeat3_lq": _c("FHADP", "pyth_lq", 100, 4, W2, "tanh", 0.99, None, repeat_num=3, lq_config="s4a2", seed=5),
    # POLY approximators on the per-lane rollout (trained / initial nets of the reference fixtures, synthetic batches)
    "poly_fhadp_one_row": _c("FHADP", "pyth_lq", 1, 6, None, None, None, None, tile=256, poly="fhadp_poly_lqs6a3_d2_bias_h30"),
    "poly_fhadp_ragged": _c("FHADP", "pyth_lq", 77, 6, None, None, None, None, tile=256, poly="fhadp_poly_lqs6a3_d2_bias_h30"),
    "poly_fhadp_blocks": _c("FHADP", "pyth_lq", 256 * 5 + 19, 8, None, None, None, None, tile=256, poly="fhadp_poly_lqs2a1_h80"),
    "poly_infadp_tail_blocks": _c("INFADP", "pyth_lq", 256 * 3 + 40, 5, None, None, None, None, tile=256, poly="infadp_poly_lqs4a2_fs5"),
}


# ---- POLY nets for the oracle's loop -------------------------------------------------------------------------------------------
def _poly_policy_forward(net, obs, virtual_t):
    from gops_amd.apprfunc.poly import make_features
    f = make_features(obs, net["degree"])
    if virtual_t is not None:
        f = torch.cat((f, virtual_t * torch.ones(obs.shape[0], 1, dtype=obs.dtype)), 1)
    return torch.nn.functional.linear(f, net["w"][0], net["b"][0])


def _poly_value_forward(net, obs):
    x = obs * net["norm"].to(obs.dtype)
    n = obs.shape[1]
    f = torch.stack([x[:, i] * x[:, j] for i in range(n) for j in range(i, n)], 1)
    return torch.nn.functional.linear(f, net["w"][0], net["b"][0]).squeeze(-1)


def _poly_net(module, value=False):
    lin = module.v if value else module.pi
    net = dict(w=[lin.weight.detach().cpu().clone().requires_grad_(not value)],
               b=[None if lin.bias is None else lin.bias.detach().cpu().clone().requires_grad_(not value)],
               forward=_poly_value_forward if value else _poly_policy_forward, degree=module.degree)
    if value:
        net["norm"] = module.norm_matrix.detach().cpu().clone()
    return net


def _load_poly(name, gpu):
    from test_poly_gpu import _kwargs
    from gops_amd.create_pkg.create_alg import create_alg
    g = load_golden(name)
    meta = golden_meta(g)
    cfg = meta["cfg"]
    kw = _kwargs(cfg, meta["extra"], meta["seed"], meta.get("lim"))
    kw["use_gpu"] = gpu
    alg = create_alg(**kw)
    alg.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("sd/")})
    if gpu:
        alg.networks.cuda()
    return alg, g, meta


# ---- a case's inputs, float64 results and premises (no GPU) ---------------------------------------------------------------------
_PREPARED = {}


def make_gv(B, tile, seed):
    """Seeded, mixed signs, three decades, the scale of a mean over the batch; its largest element outside the first tile."""
    gen = torch.Generator().manual_seed(1000 + seed)
    gv = torch.randn(B, generator=gen) * 10 ** (-3 * torch.rand(B, generator=gen)) / B
    top = int(gv.abs().argmax())
    if B > tile and top < tile:
        other = tile + (2 * (B - tile)) // 3
        gv[[top, other]] = gv[[other, top]]
    return gv


def selected_rows(case, done_rows, term_rows, n_cu=N_CU):
    B, tile = case["batch"], case["tile"]
    rows, tiles = set(), set()
    for w in case["wg"]:
        rows |= set(edge_rows(B, tile, w * n_cu))
        tiles |= set(edge_tiles(B, tile, w * n_cu))
    rows |= {r for r in list(done_rows) + list(term_rows) if r // tile in tiles}
    return sorted(rows)


def build_case(name):
    """(cfg, oracle env, policy net, tail value net or None, poly alg loader or None) of a case."""
    case = CASES[name]
    cfg = {k: v for k, v in case.items() if k in ("alg", "env_id", "batch", "horizon", "hidden", "act", "gamma", "pre_horizon", "lq_config")}
    fh = case["alg"] == "FHADP"
    if case.get("poly"):
        alg, g, meta = _load_poly(case["poly"], gpu=False)
        cfg = dict(meta["cfg"], batch=case["batch"], horizon=case["horizon"])
        env = oracle_env(meta["cfg"], meta["extra"], g)
        policy = _poly_net(alg.networks.policy)
        policy["act_high"], policy["act_low"] = alg.networks.policy.act_high_lim.cpu(), alg.networks.policy.act_low_lim.cpu()
        value = None if fh else _poly_net(alg.networks.v_target, value=True)
        return cfg, env, policy, value
    env = orc.make_env(cfg["env_id"], pre_horizon=cfg.get("pre_horizon", 10), lq_config=cfg.get("lq_config", "s4a2"),
                       repeat_num=case.get("repeat_num"))
    nets = reference_init_nets(cfg, case["seed"], obs_dim_of(cfg), act_dim_of(cfg))
    return cfg, env, nets["policy"], None if fh else nets["v_target"]


def prepare(name, floors=True):
    """Inputs, float64 results and the asserted premises of a case (cached)."""
    if (name, floors) in _PREPARED:
        return _PREPARED[(name, floors)]
    case = CASES[name]
    cfg, env, policy, value = build_case(name)
    B, H, tile, fh = cfg["batch"], cfg["horizon"], case["tile"], case["alg"] == "FHADP"
    n_wg = max(w for w in case["wg"] if w == 1 or -(-B // tile) > w * N_CU) * N_CU   # (special rows go to the LAST second-pass tile the batch reaches)
    data, done_rows, term_rows = batch_with_done(cfg, case["seed"], env, policy, tile, n_wg, finite_horizon=fh)
    gv = make_gv(B, tile, case["seed"])
    rows = selected_rows(case, done_rows, term_rows)
    ref = weighted_gradient_f64(env, policy, data, H, cfg["gamma"], fh, gv, value)
    rows64 = one_row_gradients_f64(env, policy, data, H, cfg["gamma"], fh, rows, value)

    # premises: the special rows are there, where they should be, and nothing sits on a termination bound
    n_special = min(3, max(0, (B - 1) // 4))
    first_done = H - ref["done_hist"].sum(0)                               # 0-based step whose result is the first done
    on_entry = (data["done"] != 0).nonzero().flatten().tolist()
    inside = [r for r in range(B) if r not in on_entry and 1 <= int(first_done[r]) + 1 <= H - 1]
    last_tile = (B - 1) // tile
    assert sorted(on_entry) == sorted(done_rows) and len(on_entry) >= n_special, (name, on_entry)
    terminates = env["kind"] in ("idp", "veh", "cartpole") and H >= 2
    if terminates:
        assert set(term_rows) <= set(inside) and len(inside) >= n_special, (name, term_rows, inside)
    if n_special:
        edge = lambda r: r % tile in (0, tile - 1)
        assert any(edge(r) for r in on_entry) or B <= tile, name
        assert any(r // tile == last_tile for r in on_entry), name
        if terminates:
            assert any(edge(r) for r in inside) or B <= tile, name
            assert any(r // tile == last_tile for r in inside) or B - last_tile * tile < 2, name
    assert float(ref["margin"].min()) >= DONE_MARGIN, (name, "a row sits on a termination bound", float(ref["margin"].min()))
    assert bool(ref["done_hist"][:, on_entry].all())
    top = int(gv.abs().argmax())
    assert B <= tile or top >= tile, name
    assert B < 8 or (gv.abs().max() / gv.abs().min() > 100 and (gv > 0).any() and (gv < 0).any())

    out = dict(case=case, cfg=cfg, env=env, policy=policy, value=value, data=data, gv=gv, rows=rows, ref=ref, rows64=rows64,
               done_rows=done_rows, term_rows=inside if terminates else [], first_done=first_done, fh=fh)
    if floors and case["dtype"] is None:
        # the bar only means something where fp32 itself meets it: the fp32 oracle against the float64 one
        floor, floor_rows = fp32_weighted_noise_floor(env, policy, data, H, cfg["gamma"], fh, gv, ref, rows, rows64, value)
        out["floor"], out["floor_rows"] = floor, floor_rows
        assert floor <= TOL / 3, (name, "fp32 oracle to float64, weighted gradient", floor)
        assert max(floor_rows.values()) <= TOL / 3, (name, "fp32 oracle to float64, single rows", floor_rows)
    _PREPARED[(name, floors)] = out
    return out


def _described_mlp(net):
    """A GopsMlp with the net's shape and stand-in pointers: enough for the planning code, which launches nothing."""
    from gops_amd import hip_backend as hb
    m = hb.GopsMlp()
    m.n_layers = len(net["w"])
    m.sizes[0] = net["w"][0].shape[1]
    for j, w in enumerate(net["w"]):
        m.sizes[j + 1] = w.shape[0]
        m.weight[j] = m.bias[j] = 1
    m.hidden_act = hb.ACT_IDS[net["act"]]
    return m


def rollout_desc(name):
    """The case's launch description (MLP cases) without a device: what gops_rollout_variant is asked about."""
    from gops_amd import hip_backend as hb
    case = CASES[name]
    cfg, env, policy, value = build_case(name)
    d = hb.GopsRolloutDesc()
    d.dtype = hb.dtype_id(case["dtype"])
    d.variant_flags = case["flags"]
    d.batch, d.horizon, d.finite_horizon = cfg["batch"], cfg["horizon"], int(case["alg"] == "FHADP")
    d.need_grad, d.tail_value, d.gamma = 1, int(value is not None), float(cfg["gamma"])
    d.env = hip_env_from_oracle(env, policy)
    d.policy = _described_mlp(policy)
    if value is not None:
        d.value = _described_mlp(value)
    return d


# ---- launches -------------------------------------------------------------------------------------------------------------------
class _MlpLaunch:
    def __init__(self, prep, dev):
        self.prep, self.dev = prep, dev
        self.pol, self.ws, self.bs = hip_mlp_from_net(prep["policy"], dev)
        self.vt = None if prep["value"] is None else hip_mlp_from_net(prep["value"], dev)
        self.henv = hip_env_from_oracle(prep["env"], prep["policy"])

    def rollout(self, B):
        from gops_amd import hip_backend as hb
        case, cfg = self.prep["case"], self.prep["cfg"]
        ro = hb.Rollout(self.henv, self.pol, batch=B, horizon=cfg["horizon"], gamma=cfg["gamma"], finite_horizon=self.prep["fh"],
                        need_grad=True, value=None if self.vt is None else self.vt[0], dtype=case["dtype"], variant_flags=case["flags"])
        return ro, hb.lib().gops_rollout_variant(ctypes.byref(ro.desc))

    def backward(self, ro, gv):
        gw, gb = [torch.full_like(w, float("nan")) for w in self.ws], [torch.full_like(b, float("nan")) for b in self.bs]
        ro.backward(gv.to(self.dev).contiguous(), gw, gb)
        torch.cuda.synchronize()
        return [t.cpu() for pair in zip(gw, gb) for t in pair]


class _PolyLaunch:
    def __init__(self, prep, dev):
        self.prep, self.dev = prep, dev
        self.alg, _, meta = _load_poly(prep["case"]["poly"], gpu=True)
        self.alg.gamma = prep["cfg"]["gamma"]
        if prep["fh"]:
            self.alg.pre_horizon = prep["cfg"]["horizon"]   # (the rollout's horizon; the POLY policy itself does not depend on it)
        else:
            self.alg.forward_step = prep["cfg"]["horizon"]
        self.pi = self.alg.networks.policy.pi

    def rollout(self, B):
        from gops_amd import hip_backend as hb
        ro = self.alg._rollout_for(B, self.dev) if self.prep["fh"] else self.alg._rollout_for(B, self.dev, need_grad=True)
        assert isinstance(ro, hb.PolyRollout) and ro.desc.horizon == self.prep["cfg"]["horizon"]
        return ro, None

    def backward(self, ro, gv):
        gw = [torch.full_like(self.pi.weight, float("nan"))]
        gb = [None if self.pi.bias is None else torch.full_like(self.pi.bias, float("nan"))]
        ro.backward(gv.to(self.dev).contiguous(), gw, gb)
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in gw + gb if t is not None]


def _grad_errors(got, want):
    """(flat, worst tensor) rel-L2 distance of a list of gradient tensors to the float64 ones."""
    return rel_l2(flat_grads(got), flat_grads(want)), max(rel_l2(a, b) for a, b in zip(got, want))


def _padded(prep, extra):
    """The case's batch followed by `extra` rows of another seed, their observations (where the observation is the state) tripled."""
    return padded_batch(prep["cfg"], prep["case"]["seed"], prep["env"], prep["data"], extra)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert torch.cuda.get_device_properties(0).multi_processor_count == N_CU, "the cases' batches are laid out for 256 CUs"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_per_trajectory(name, dev):
    prep = prepare(name)
    case, cfg, data, ref, gv = prep["case"], prep["cfg"], prep["data"], prep["ref"], prep["gv"]
    B, H, tile, fh = cfg["batch"], cfg["horizon"], case["tile"], prep["fh"]
    half = case["dtype"] is not None
    tol = TOL_GRAD_F16 if half else TOL
    launch = (_PolyLaunch if case.get("poly") else _MlpLaunch)(prep, dev)
    ro, variant = launch.rollout(B)
    if case["variant"] is not None:
        assert variant == case["variant"], "the launch would not take the kernels under test"
    ro.workspace.fill_(0xFF)
    ddev = to_device(data, dev)
    res = {k: v.cpu() for k, v in ro.forward(ddev, want_rewards=True, want_final=True).items()}
    measured = {}

    # 1. forward, row by row
    on_entry, first_done = prep["done_rows"], prep["first_done"]
    assert np.array_equal(res["final_done"].numpy() != 0, ref["final_done"].numpy())
    assert torch.equal(res["rewards"][:, on_entry], torch.zeros(H, len(on_entry)))
    assert torch.equal(res["final_obs"][on_entry], data["obs"][on_entry])
    assert torch.equal(res["v_pi"][on_entry], torch.zeros(len(on_entry)))   # (a tail value is masked at done too)
    for r in prep["term_rows"]:
        assert torch.equal(res["rewards"][int(first_done[r]) + 1:, r], torch.zeros(H - int(first_done[r]) - 1)), r
    n_terms = H + (0 if fh else 1)
    for key, want, terms in (("rewards", ref["rewards"], 1), ("final_obs", ref["final_obs"], 1), ("v_pi", ref["v"], n_terms)):
        got, want = res[key].double().numpy(), want.numpy()
        rtol, atol = (TOL_FWD_F16, TOL_FWD_F16 * np.abs(want).max()) if half else (FWD_RTOL, terms * FWD_ATOL)
        measured["fwd_" + key] = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())   # (<= 1 passes)
        print(f"{name}: {key} worst |error| / (atol + rtol |want|) = {measured['fwd_' + key]:.3f}")
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=f"{name}: {key}")

    # 2. weighted gradient
    g1 = launch.backward(ro, gv)
    measured["weighted_flat"], measured["weighted_worst_tensor"] = _grad_errors(g1, ref["grads"])
    print(f"{name}: weighted gradient to float64: flat {measured['weighted_flat']:.2e}, worst tensor {measured['weighted_worst_tensor']:.2e}"
          + ("" if half or "floor" not in prep else f" (fp32 oracle: {prep['floor']:.2e})"))
    assert all(torch.isfinite(g).all() for g in g1)
    assert measured["weighted_flat"] < tol and measured["weighted_worst_tensor"] < tol, (name, measured)

    # 3. linearity and call-to-call state
    g2 = launch.backward(ro, 1e-4 * gv)
    g3 = launch.backward(ro, gv)
    for a, b in zip(g1, g3):
        assert torch.equal(a, b), "a backward call depends on the call before it"
    e_flat, e_worst = _grad_errors([1e4 * g for g in g2], ref["grads"])
    measured["scaled_flat"] = e_flat
    assert e_flat < tol and e_worst < tol, (name, "backward(1e-4 gv)", e_flat, e_worst)
    even = ((torch.arange(B) // tile) % 2 == 0).float()
    ga, gb = launch.backward(ro, gv * even), launch.backward(ro, gv * (1 - even))
    e_flat, e_worst = _grad_errors([a + b for a, b in zip(ga, gb)], ref["grads"])
    measured["even_odd_flat"] = e_flat
    assert e_flat < tol and e_worst < tol, (name, "even + odd tiles", e_flat, e_worst)
    if B > tile:
        assert _grad_errors([a + b for a, b in zip(ga, gb)], g1)[0] < tol

    # 4. one row at a time
    row_err = {}
    for i in prep["rows"]:
        hot = torch.zeros(B)
        hot[i] = 1.0
        gi = launch.backward(ro, hot)
        want = prep["rows64"][i]
        if i in on_entry:
            assert all(float(g.abs().max()) == 0.0 for g in gi), (name, i, "a row that is done on entry has a gradient")
            continue
        assert all(torch.isfinite(g).all() for g in gi), (name, i)
        row_err[i] = rel_l2(flat_grads(gi), flat_grads(want))
    measured["rows"] = {str(i): e for i, e in row_err.items()}
    measured["row_worst"] = max(row_err.values(), default=0.0)
    print(f"{name}: one-row gradients to float64: " + ", ".join(f"{i}: {e:.2e}" for i, e in row_err.items()))
    print(name, json.dumps(measured, sort_keys=True))
    if half:
        assert measured["row_worst"] < 10 * TOL_GRAD_F16, (name, row_err)
        assert measured["row_worst"] < F16_ROW_BOUND, (name, row_err)
    else:
        assert measured["row_worst"] < TOL, (name, row_err)

    # 5. rows beyond the batch are inert
    extra = tile + 3
    pad = _padded(prep, extra)
    gv_pad = torch.cat((gv, torch.zeros(extra)))
    runs = []
    for fill, (d_in, g_in, n) in zip((0x00, None, 0xFF, None), ((data, gv, B), (pad, gv_pad, B + extra)) * 2):
        ro_n, variant_n = launch.rollout(n)
        assert variant_n == variant
        if fill is None:
            ro_n.workspace.random_(0, 256)
        else:
            ro_n.workspace.fill_(fill)
        out = ro_n.forward(to_device(d_in, dev), want_rewards=True, want_final=True)
        runs.append((out["v_pi"][:B].cpu(), out["rewards"][:, :B].cpu(), out["final_obs"][:B].cpu(), launch.backward(ro_n, g_in)))
        del ro_n
    for v, r, o, g in runs:
        assert torch.equal(v, res["v_pi"]) and torch.equal(r, res["rewards"]) and torch.equal(o, res["final_obs"]), name
        e_flat, e_worst = _grad_errors(g, ref["grads"])
        assert e_flat < tol and e_worst < tol, (name, "padded batch", e_flat, e_worst)
        assert _grad_errors(g, g1)[0] < tol
