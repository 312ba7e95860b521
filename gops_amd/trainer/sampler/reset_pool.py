"""Initial conditions of the DATA environments, drawn on the host in pools and uploaded once per pool: the reset
distributions `DeviceEnvSampler` re-seeds finished instances from and `Evaluator` starts its episodes from."""
import numpy as np
import torch

from gops_amd.utils.synthetic import make_batch

INFO_KEYS = ("state", "ref_points", "path_num", "u_num", "ref_time")

NOT_RESTATED = ("the DATA environment of {env_id} is not restated in the step kernel "
                "(pyth_lq, pyth_idpendulum, pyth_veh3dofconti, pyth_veh2dofconti, pyth_mobilerobot and "
                "gym_cartpoleconti are): pass env_step='model'")


def draw_reset_pool(cfg: dict, env_model, seed: int, size: int, device, data_env: bool = True) -> dict:
    """`size` initial conditions (device tensors: obs + the info keys the model carries) of `cfg["env_id"]` for `seed`."""
    host = make_batch(cfg, seed, batch=size)
    if cfg["env_id"] == "pyth_mobilerobot" and data_env:
        # the data env's own reset distribution (pyth_mobilerobot.py:31-54, 95-106: robot and obstacle uniform in the work
        # space, w = 0, tracking errors of the robot state); make_batch's near-collision starts exist for the parity fixtures
        rng = np.random.RandomState(seed)
        ego = rng.uniform([0.0, -1.0, -0.6, 0.0, 0.0], [2.7, 1.0, 0.6, 0.3, 0.0], size=(size, 5))
        obst = rng.uniform([3.5, -3.0, np.pi / 2 - 0.3, 0.0, 0.0], [6.0, 3.0, np.pi / 2 + 0.3, 0.5, 0.0], size=(size, 5))
        ego, obst = ego.astype(np.float32), obst.astype(np.float32)   # (reset casts the drawn state first, :100-101)
        track = np.stack((ego[:, 1], ego[:, 2], ego[:, 3] - np.float32(0.3)), axis=1)   # path y = 0, phi = 0, v_desired 0.3
        host["obs"] = torch.from_numpy(np.concatenate((ego, track, obst), axis=1))
    if cfg["env_id"] == "gym_cartpoleconti" and data_env:
        # the data env's own reset distribution (env_gym/gym_cartpoleconti.py:139-147: uniform +-0.05 in every state);
        # make_batch's wide cartpole states exist to exercise the done thresholds inside short rollouts
        rng = np.random.RandomState(seed)
        host["obs"] = torch.from_numpy(rng.uniform(-0.05, 0.05, size=(size, 4)).astype(np.float32))
    pool = {key: v.to(device) for key, v in host.items() if key == "obs" or key in INFO_KEYS}
    # ScaleObservationData (scale_observation.py:53-62): the data env hands out (obs + shift) * scale
    sc, sh = getattr(env_model, "obs_scale", None), getattr(env_model, "obs_shift", None)
    if sc is not None or sh is not None:
        as_t = lambda v, d: torch.as_tensor(d if v is None else v, dtype=torch.float32, device=device)  # noqa: E731
        pool["obs"] = (pool["obs"] + as_t(sh, 0.0)) * as_t(sc, 1.0)
    return pool
