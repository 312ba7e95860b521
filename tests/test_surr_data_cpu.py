"""The DATA environment pyth_veh3dofconti_surrcstr on the host: the fixtures recorded from the reference's own class, their numpy
restatement (surr_data_helpers.py) and the reset pool that draws the surrounding vehicles.

The restatement is held to 1e-6 absolute on every recorded step.  It rounds to float32 where the env rounds: where it stores (state,
reference points, surrounding vehicles, the ego vehicle's circle centres, the reward) and in the two places where the env's
arithmetic itself is float32, the ego vehicle's step and the observation's transform; the ego state and the reference points are
reproduced bit for bit.  What remains is one rounding that cannot be mirrored from a batch row: the env carries its surrounding
vehicles in float64 from step to step and hands out float32 copies, while a step from a recorded row starts from the copy, so a new
position can land on the neighbouring float32.  The fixtures keep every stored position below 16 m, where float32 is at most 9.5e-7
apart: that spacing is the largest error measured, in next_surr_state and in the observation components formed from it."""
import numpy as np
import pytest
import torch

import surr_data_helpers as sh

TOL = 1e-6
NAMES = ("surr_data_n1_p10_lane", "surr_data_n1_p1_circle", "surr_data_n4_p10_circle", "surr_data_n4_p1_sine")


def _restated(name):
    for e, s, cur, act, nxt, rew, done in sh.transitions(name):
        out = sh.step_f64(cur["state"], cur["ref_points"], cur["ref_time"], cur["path_num"], cur["u_num"], cur["surr_state"], act)
        yield (e, s), out, nxt, rew, done


def test_fixtures_cover_the_branches():
    assert sh.fixture_names() == sorted(NAMES)
    seen, clipped = set(), False
    for name in NAMES:
        cfg, eps = sh.load(name)
        seen.add((cfg["surr_veh_num"], cfg["pre_horizon"], cfg["ref_num"] // 2 == 3))
        assert sorted(eps) == sorted(sh.EPISODES)
        n, P = cfg["surr_veh_num"], cfg["pre_horizon"]
        for ep in eps.values():
            L = int(ep["length"])
            assert 1 <= L <= 20 and ep["obs"].shape == (L + 1, 6 + 4 * P + 4 * n) and ep["surr_state"].shape == (L + 1, n, 5)
            assert ep["constraint"].shape == (L + 1, 1) and ep["ref_points"].shape == (L + 1, P + 1, 4) and ep["act"].shape == (L, 2)
            assert not ep["done"][:-1].any()
            assert max(np.abs(ep[k][..., :2]).max() for k in ("state", "ref_points", "surr_state")) < 16.0
        assert eps["leave"]["done"][-1] and eps["leave"]["length"] < cfg["limit"]          # ends through `done`
        assert not eps["track"]["done"].any() and eps["track"]["length"] == cfg["limit"]   # runs to the limit
        assert (eps["approach"]["constraint"] > 0).any() and (eps["track"]["constraint"] < 0).any()
        clipped = clipped or bool((np.abs(eps["leave"]["act"]) > np.float32(sh.ACT_HIGH)).any())
    assert clipped   # the env's clip of the action is met
    assert {s[0] for s in seen} == {1, 4} and {s[1] for s in seen} == {1, 10} and {s[2] for s in seen} == {True, False}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_reward_vehicles_constraint_and_done(name):
    err = dict(reward=0.0, next_surr_state=0.0, constraint=0.0, state=0.0, ref_points=0.0)
    for at, out, nxt, rew, done in _restated(name):
        assert out["done"] == done, at
        assert out["surr_state"].dtype == np.float32 and out["state"].dtype == np.float32
        err["reward"] = max(err["reward"], abs(out["reward"] - rew))
        err["next_surr_state"] = max(err["next_surr_state"], np.abs(out["surr_state"].astype(np.float64) - nxt["surr_state"]).max())
        err["constraint"] = max(err["constraint"], abs(out["constraint"] - nxt["constraint"][0]))
        err["state"] = max(err["state"], np.abs(out["state"].astype(np.float64) - nxt["state"]).max())
        err["ref_points"] = max(err["ref_points"], np.abs(out["ref_points"].astype(np.float64) - nxt["ref_points"]).max())
        assert abs(out["ref_time"] - nxt["ref_time"]) < 1e-12
    print(name, {k: f"{v:.3g}" for k, v in err.items()})
    assert all(v <= TOL for v in err.values()), err


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_observations(name):
    worst = 0.0
    for at, out, nxt, _, _ in _restated(name):
        worst = max(worst, np.abs(out["obs"] - nxt["obs"]).max())
    print(name, f"obs {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_rows_it_starts_from(name):
    """get_constraint of every row a step starts from, the reset's included, from the row's own state."""
    worst = 0.0
    for e, s, cur, _, _, _, _ in sh.transitions(name):
        worst = max(worst, abs(sh.constraint_f64(cur["state"], cur["surr_state"]) - cur["constraint"][0]))
    assert worst <= TOL


@pytest.mark.parametrize("n_surr,P", [(4, 10), (1, 1)])
def test_reset_pool_draws_the_surrounding_vehicles(n_surr, P):
    from gops_amd.trainer.sampler.reset_pool import INFO_KEYS, draw_reset_pool
    from gops_amd.utils.synthetic import make_batch
    cfg = dict(env_id="pyth_veh3dofconti_surrcstr", pre_horizon=P, surr_veh_num=n_surr)
    R, N = 3, 70
    pool = draw_reset_pool(cfg, None, 11, R * N, "cpu")
    assert sorted(pool) == sorted(("obs", "surr_state") + INFO_KEYS)
    surr = pool["surr_state"].reshape(R, N, n_surr, 5)
    assert surr.dtype == torch.float32 and pool["obs"].shape == (R * N, 6 + 4 * P + 4 * n_surr)
    sv, ref, path = pool["surr_state"].double().numpy(), pool["ref_points"].double().numpy(), pool["path_num"].numpy()
    circle = path == 3
    assert circle.any() and (~circle).any()   # both branches of the reset are drawn
    # the path frame of the reset: the first reference point, heading the vehicles' own (the path's on the circle, else 0)
    dx, dy, phi = sv[..., 0] - ref[:, :1, 0], sv[..., 1] - ref[:, :1, 1], sv[..., 2]
    lon, lat = dx * np.cos(phi) + dy * np.sin(phi), -dx * np.sin(phi) + dy * np.cos(phi)
    eps = 1e-4   # float32 storage of positions up to ~120 m
    assert ((np.abs(lon) > 7 - eps) | (np.abs(lat) > 3 - eps)).all()       # outside the ego vehicle's box
    assert (np.abs(lon) <= 10 + eps).all() and (np.abs(lat) <= 5 + eps).all()
    assert (np.abs(lon) < 7).any() and (np.abs(lat) < 3).any()             # (either test alone admits a vehicle)
    assert ((sv[..., 3] >= 4) & (sv[..., 3] <= 6)).all() and sv[..., 3].std() > 0.3
    assert (phi[~circle] == 0).all() and (sv[~circle][..., 4] == 0).all()
    assert np.allclose(phi[circle], ref[circle][:, :1, 2], atol=0, rtol=0)
    assert np.allclose(sv[circle][..., 4], -np.arctan2(3.0, 100.0), rtol=1e-7)
    # the observation is the data env's get_obs of the drawn row
    for b in range(0, R * N, 7):
        want = sh.env_obs(pool["state"][b].numpy(), pool["ref_points"][b].numpy(), pool["surr_state"][b].numpy(), np.float64)
        assert np.abs(pool["obs"][b].double().numpy() - want).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())
    # the same seed draws the same pool; the env MODEL's pool (env_step="model") is what it was
    again = draw_reset_pool(cfg, None, 11, R * N, "cpu")
    assert all(torch.equal(pool[k], again[k]) for k in pool)
    model_pool, host = draw_reset_pool(cfg, None, 11, R * N, "cpu", data_env=False), make_batch(cfg, 11, batch=R * N)
    assert sorted(model_pool) == sorted(("obs",) + INFO_KEYS) and all(torch.equal(model_pool[k], host[k]) for k in model_pool)
    assert all(torch.equal(pool[k], host[k]) for k in INFO_KEYS)


def test_other_envs_keep_their_pools_and_refusals():
    from gops_amd.create_pkg.create_evaluator import create_evaluator
    from gops_amd.trainer.sampler.reset_pool import INFO_KEYS, draw_reset_pool
    from closed_loop_helpers import alg_kwargs
    assert INFO_KEYS == ("state", "ref_points", "path_num", "u_num", "ref_time")
    assert sorted(draw_reset_pool(dict(env_id="pyth_veh3dofconti", pre_horizon=2), None, 3, 4, "cpu")) == sorted(("obs",) + INFO_KEYS)
    cfg, kw = alg_kwargs("idp", "relu64", use_gpu=False)
    kw.update(num_eval_episode=2, eval_save=False, save_folder=None, is_render=False)
    for env_id, extra in (("gym_pendulum", dict(obsv_dim=3)), ("pyth_veh2dofconti_errcstr", dict(obsv_dim=14, pre_horizon=10))):
        with pytest.raises(RuntimeError, match="is not restated in the step kernel"):
            create_evaluator(**dict(kw, env_id=env_id, **extra))
