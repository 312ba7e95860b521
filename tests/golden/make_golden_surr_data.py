"""Generate the fixtures of the DATA environment pyth_veh3dofconti_surrcstr (`surr_data_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_surr_data.py
Every array written here is an output of the reference's own class (`gops.env.env_ocp.pyth_veh3dofconti_surrcstr.
SimuVeh3dofcontiSurrCstr`): `env.seed(seed)`, `env.reset(init_state=..., ref_time=..., ref_num=...)`, then `env.step(action)` until
`done` or LIMIT steps.  Row 0 of every per-step array is the reset's (obs, info); row s + 1 is what step s returned, so row s -> row
s + 1 under `act[s]` is one transition.  `ref_time` is kept in float64 (the env carries a Python float), everything else as the env
hands it out.

The cases cover both branches of reset() (the circle path, path_num == 3, and another path), surr_veh_num 1 and 4 and pre_horizon 1
and 10.  Each case holds three episodes:
  track      a drawn-size initial offset and moderate actions: LIMIT steps, no termination;
  leave      an initial offset close to the parent's lateral bound with a heading away from the path: `done` inside the limit;
  approach   the ego vehicle placed 2.2 m beside a surrounding vehicle the reset drew (inside the parent's done bounds): the
             bicircle constraint is violated (`constraint > 0`) on at least one row.
The maker asserts all three (a regenerated fixture cannot lose a branch) and otherwise moves on to the next seed.  The actions are
uniform in 1.2 x the action limits, so that the env's clip is exercised.  The reference time starts inside the first 0.3 s and the
maker keeps a seed only if every stored position (ego state, reference points, surrounding vehicles) stays below 16 m: there
float32 - the format the env stores them in - has a spacing of at most 9.5e-7, so a restatement that rounds where the env stores
can be held to 1e-6 absolute (tests/test_surr_data_cpu.py)."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)

from gops.env.env_ocp.pyth_veh3dofconti_surrcstr import SimuVeh3dofcontiSurrCstr  # noqa: E402

LIMIT = 10
MAX_POSITION = 16.0
STEP_KEYS = ("obs", "state", "ref_points", "surr_state", "constraint", "ref_time")

# name: (surr_veh_num, pre_horizon, ref_num = 2 * path_num + u_num)
CASES = {
    "surr_data_n4_p10_circle": (4, 10, 6),
    "surr_data_n1_p1_circle": (1, 1, 7),
    "surr_data_n4_p1_sine": (4, 1, 0),
    "surr_data_n1_p10_lane": (1, 10, 3),
}


def row(obs, info):
    return dict(obs=np.array(obs, np.float32), state=np.array(info["state"], np.float32), ref_points=np.array(info["ref_points"], np.float32),
                surr_state=np.array(info["surr_state"], np.float32), constraint=np.array(info["constraint"], np.float32),
                ref_time=np.float64(info["ref_time"]))


def episode(env, seed, init_state, ref_time, ref_num, actions):
    env.seed(seed)
    obs, info = env.reset(init_state=init_state, ref_time=ref_time, ref_num=ref_num)
    rows, rew, done_l = [row(obs, info)], [], []
    for a in actions:
        obs, r, done, info = env.step(a.copy())
        rows.append(row(obs, info))
        rew.append(np.float64(r))
        done_l.append(bool(done))
        if done:
            break
    n = len(rew)
    out = {k: np.stack([r_[k] for r_ in rows]) for k in STEP_KEYS}
    out.update(act=np.stack(actions[:n]).astype(np.float32), rew=np.array(rew, np.float64), done=np.array(done_l, np.bool_),
               path_num=np.float32(info["path_num"]), u_num=np.float32(info["u_num"]), init_state=np.array(init_state, np.float32),
               length=np.int32(n))
    return out


def beside_nearest(env, seed, ref_time, ref_num):
    """The initial offset (world frame, as reset() adds it to the first reference point) that puts the ego vehicle 2.2 m to the side
    of the first surrounding vehicle the reset drew for which that offset stays inside 4 m / 1.8 m (the parent ends the episode at
    5 m / 2 m; the reset keeps its vehicles more than 3 m to the side or 7 m along the path), or None when there is none.  Circle
    centres 2.2 m apart are closer than the two radii (2 r = 2.83 m)."""
    env.seed(seed)
    _, info = env.reset(init_state=np.zeros(6, np.float32), ref_time=ref_time, ref_num=ref_num)
    rp, surr = info["ref_points"][0].astype(np.float64), info["surr_state"].astype(np.float64)
    for d in surr[:, :2] - rp[:2]:
        dy = d[1] - np.sign(d[1]) * 2.2
        if abs(d[0]) <= 4.0 and abs(dy) <= 1.8:
            return np.array([d[0], dy, 0.0, 0.0, 0.0, 0.0], np.float32)
    return None


def record(name, n_surr, P, ref_num):
    base = zlib.crc32(name.encode()) % 1000
    for seed in range(base, base + 400):
        env = SimuVeh3dofcontiSurrCstr(pre_horizon=P, surr_veh_num=n_surr)
        rng = np.random.RandomState(seed)
        ref_time = float(rng.uniform(0.0, 0.3))
        lim = 1.2 * np.asarray(env.action_space.high, np.float64)
        actions = [rng.uniform(-lim, lim).astype(np.float32) for _ in range(LIMIT)]
        calm = [(0.3 * a).astype(np.float32) for a in actions]
        near = beside_nearest(env, seed, ref_time, ref_num)
        if near is None:
            continue
        side = 1.0 if rng.uniform() < 0.5 else -1.0
        eps = {"track": episode(env, seed, rng.uniform(-1, 1, size=6).astype(np.float32) * np.array([1, 0.5, 0.2, 1, 0.1, 0.1], np.float32),
                                ref_time, ref_num, calm),
               "leave": episode(env, seed, np.array([0.5, side * 1.6, side * 0.45, 0.5, 0.0, 0.0], np.float32), ref_time, ref_num, actions),
               "approach": episode(env, seed, near, ref_time, ref_num, calm)}
        ok = (eps["track"]["length"] == LIMIT and not eps["track"]["done"].any()
              and eps["leave"]["done"][-1] and 2 <= eps["leave"]["length"] < LIMIT
              and (eps["approach"]["constraint"] > 0).any() and eps["approach"]["length"] >= 3
              and all(np.abs(e[k][..., :2]).max() < MAX_POSITION for e in eps.values() for k in ("state", "ref_points", "surr_state")))
        if not ok:
            continue
        # asserted on what is written: the branches the tests rely on
        assert any(e["done"].any() for e in eps.values()) and any((e["constraint"] > 0).any() for e in eps.values())
        assert all(e["surr_state"].shape[1:] == (n_surr, 5) and e["obs"].shape[1] == 6 + 4 * P + 4 * n_surr for e in eps.values())
        assert (eps["track"]["path_num"] == 3) == (ref_num // 2 == 3)
        out = {"meta/cfg": json.dumps(dict(env_id="pyth_veh3dofconti_surrcstr", surr_veh_num=n_surr, pre_horizon=P, ref_num=ref_num, seed=seed,
                                           limit=LIMIT, episodes=sorted(eps), numpy=np.__version__,
                                           lengths={k: int(e["length"]) for k, e in eps.items()},
                                           violating_rows={k: int((e["constraint"] > 0).sum()) for k, e in eps.items()}))}
        for k, e in eps.items():
            out.update({f"{k}/{f}": v for f, v in e.items()})
        mg.save(name, **out)
        return
    raise AssertionError(name)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for case, args in CASES.items():
        if not only or case in only:
            record(case, *args)
