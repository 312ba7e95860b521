"""Generate the evaluation-episode fixtures (`eval_*.npz`) by running the UNMODIFIED reference.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_eval.py
Every episode is the reference's own loop (gops/trainer/evaluator.py:45-86): `create_env` (reward_scale = None, repeat_num =
None, as Evaluator.__init__ forces), `env.reset(init_state=...)`, then `policy(obs)` -> `action_distribution.mode()` ->
`env.step(action)` until `done` or the time limit.  (The gym stand-in of _ref_import.py has a TimeLimit that does not count, so
the loop counts the steps itself: the limit is 40, and the data env's own `max_episode_steps` for the one full-length episode.)

Per episode: the initial obs and info, every obs / action / reward, the length, `terminated` and the return (the reference's
`sum(reward_list)`).  Per case: the policy state_dict, the action limits and `model_consts`.

Knife-edge terminations: every episode is run again with the actions scaled by (1 + 1e-5) and by (1 - 1e-5); only episodes whose
length stays the same are kept.  At most 3 of 33 may be dropped, and at least 4 terminating and 4 time-limited episodes remain.
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import hook)

from gops.create_pkg.create_env import create_env  # noqa: E402
from gops.create_pkg.create_env_model import create_env_model  # noqa: E402

for _old, _new in (("float_", np.float64), ("int_", np.int64), ("bool8", np.bool_)):   # reference targets numpy 1.x
    if not hasattr(np, _old):
        setattr(np, _old, _new)

INFO_KEYS = ("state", "ref_points", "path_num", "u_num", "ref_time")
EPISODES, LIMIT = 33, 40

# name: (env kwargs, policy: a shipped checkpoint of make_golden.TRAINED or a seeded random-init net, candidate scale)
CASES = {
    "eval_idp_fhadp_trained": (dict(env_id="pyth_idpendulum"), "fhadp_trained_idp_h80"),
    "eval_lq_s4a2_infadp_trained": (dict(env_id="pyth_lq", lq_config="s4a2"), "infadp_trained_lqs4a2"),
    "eval_veh3dof_p10": (dict(env_id="pyth_veh3dofconti", pre_horizon=10), None),
    "eval_veh2dof_p10": (dict(env_id="pyth_veh2dofconti", pre_horizon=10), None),
    "eval_cartpole": (dict(env_id="gym_cartpoleconti"), None),
}


def build_policy(name, env_cfg, trained, env):
    """(policy module, create_action_distributions, meta) - the reference's classes."""
    seed = zlib.crc32(name.encode()) % 1000
    if trained is not None:
        run, ckpt, _ = mg.TRAINED[trained]
        rc = json.load(open(os.path.join(mg.REF_ROOT, "results", run, "config.json")))
        cfg = dict(alg=rc["algorithm"], env_id=rc["env_id"], hidden=tuple(rc["policy_hidden_sizes"]), act=rc["policy_hidden_activation"],
                   batch=4, horizon=rc.get("pre_horizon") or 1)
        if "lq_config" in rc:
            cfg["lq_config"] = rc["lq_config"]
        if rc["algorithm"] == "FHADP":
            cfg["pre_horizon"] = rc["pre_horizon"]
        low, high = np.array(rc["action_low_limit"], np.float32), np.array(rc["action_high_limit"], np.float32)
        alg = mg.build_alg(cfg, seed, action_high_limit=high, action_low_limit=low)
        alg.networks.load_state_dict(torch.load(os.path.join(mg.REF_ROOT, "results", run, "apprfunc", ckpt), map_location="cpu"))
        meta = dict(checkpoint=f"results/{run}/apprfunc/{ckpt}")
    else:
        cfg = dict(alg="INFADP", hidden=(64, 64), act="relu", batch=4, horizon=1, **env_cfg)
        low, high = np.asarray(env.action_space.low, np.float32), np.asarray(env.action_space.high, np.float32)
        alg = mg.build_alg(cfg, seed, action_high_limit=high, action_low_limit=low)
        meta = dict(checkpoint=None)
    meta.update(alg=cfg["alg"], hidden=list(cfg["hidden"]), act=cfg["act"], pre_horizon=cfg.get("pre_horizon"), seed=seed,
                act_low=low.tolist(), act_high=high.tolist())
    return alg, meta


def candidates(env_id, rng, n):
    """Reset keywords of n initial states: the reset distribution's neighbourhood first, then wider and wider states, so
    that episodes which leave the data env's bounds inside the limit are among them."""
    out = []
    for i in range(n):
        amp = (0.02, 0.1, 0.3, 0.6, 0.8, 1.0)[i % 6]
        u = rng.uniform(-1.0, 1.0, size=8)
        if env_id == "pyth_lq":   # s4a2: the observation space is the done test
            out.append(dict(init_state=(u[:4] * amp * np.array([15.0, 10.0, 15.0, 10.0])).astype(np.float32)))
        elif env_id == "pyth_idpendulum":
            out.append(dict(init_state=(u[:6] * amp * np.array([1.0, 0.35, 0.35, 1.0, 1.5, 1.5])).astype(np.float32)))
        elif env_id == "pyth_veh3dofconti":
            out.append(dict(init_state=(u[:6] * amp * np.array([1.5, 2.2, 0.8, 2.0, 0.4, 0.4])).astype(np.float32),
                            ref_time=float(20.0 * rng.uniform()), ref_num=int(rng.randint(8))))
        elif env_id == "pyth_veh2dofconti":
            out.append(dict(init_state=(u[:4] * amp * np.array([2.2, 0.8, 0.4, 0.4])).astype(np.float32),
                            ref_time=float(20.0 * rng.uniform()), ref_num=2 * int(rng.randint(4)) + 1))
        else:   # gym_cartpoleconti: reset() takes no state; it is placed after the reset
            out.append(dict(state=u[:4] * amp * np.array([2.3, 1.0, 0.2, 1.0]) * (0.05 if i % 3 == 0 else 1.0)))
    return out


def run_episode(env, alg, reset_kw, limit, act_scale=1.0):
    """evaluator.py:51-86 with the time limit counted here."""
    if "state" in reset_kw:
        ret = env.reset()
        env.unwrapped.state = np.array(reset_kw["state"], dtype=np.float64)
        ret = (np.array(env.unwrapped.state, dtype=np.float32), {"state": env.unwrapped.state.astype(np.float32)})
    else:
        ret = env.reset(**reset_kw)
    obs, info = ret if isinstance(ret, tuple) else (ret, {})
    if not info:
        info = getattr(env.unwrapped, "info", {}) or {}
    init_info = {k: np.array(info[k], dtype=np.float32).copy() for k in INFO_KEYS if k in info}
    obs_list, action_list, reward_list = [], [], []
    done = False
    while not done and len(reward_list) < limit:
        batch_obs = torch.from_numpy(np.expand_dims(obs, axis=0).astype("float32"))
        logits = alg.networks.policy(batch_obs)
        action = alg.networks.create_action_distributions(logits).mode().detach().numpy()[0]
        if act_scale != 1.0:
            action = (action * np.float32(act_scale)).astype(np.float32)
        next_obs, reward, done, _ = env.step(action)[:4]
        obs_list.append(np.array(obs, np.float32))
        action_list.append(np.array(action, np.float32))
        reward_list.append(float(reward))
        obs = next_obs
        done = bool(done)
    return dict(obs0=obs_list[0], info=init_info, obs=np.stack(obs_list), act=np.stack(action_list), rew=np.array(reward_list, np.float64),
                length=len(reward_list), terminated=float(done), ret=float(sum(reward_list)))


def record(name, env_cfg, trained):
    env = create_env(**env_cfg, reward_scale=None, repeat_num=None, gym2gymnasium=False, vector_env_num=None)
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 10000)
    env.seed(int(rng.randint(1 << 30)))
    alg, meta = build_policy(name, env_cfg, trained, env)
    with torch.no_grad():
        cands = candidates(env_cfg["env_id"], rng, 240)
        runs = [run_episode(env, alg, kw, LIMIT) for kw in cands]
        term = [i for i, r in enumerate(runs) if r["terminated"]]
        full = [i for i, r in enumerate(runs) if not r["terminated"]]
        # a third terminating (spread over the lengths that occur), the rest time-limited
        term.sort(key=lambda i: (runs[i]["length"], i))
        n_term = max(min(len(term), 12), EPISODES - len(full))
        pick = [term[(j * len(term)) // n_term] for j in range(n_term)] if n_term else []
        pick += full[:EPISODES - len(pick)]
        pick = sorted(set(pick))[:EPISODES]
        assert len(pick) == EPISODES, (name, len(term), len(full))
        kept = []
        for i in pick:
            same = all(run_episode(env, alg, cands[i], LIMIT, s)["length"] == runs[i]["length"] for s in (1.0 + 1e-5, 1.0 - 1e-5))
            if same:
                kept.append(i)
        n_t = sum(1 for i in kept if runs[i]["terminated"])
        print(name, "kept", len(kept), "of", EPISODES, "terminating", n_t, "time-limited", len(kept) - n_t,
              "lengths", sorted(runs[i]["length"] for i in kept if runs[i]["terminated"]))
        assert EPISODES - len(kept) <= 3 and n_t >= 4 and len(kept) - n_t >= 4, name
        eps = [runs[i] for i in kept]
        out = {"meta/cfg": json.dumps(dict(env=env_cfg, policy=meta, limit=LIMIT, picked=EPISODES, kept=len(kept)))}
        E = len(eps)
        out["init/obs"] = np.stack([e["obs0"] for e in eps])
        for k in eps[0]["info"]:
            out["init/" + k] = np.stack([e["info"][k] for e in eps])
        for k, dim in (("obs", eps[0]["obs"].shape[1]), ("act", eps[0]["act"].shape[1])):
            a = np.zeros((E, LIMIT, dim), np.float32)
            for j, e in enumerate(eps):
                a[j, :e["length"]] = e[k]
            out["ep/" + k] = a
        rew = np.zeros((E, LIMIT), np.float64)
        for j, e in enumerate(eps):
            rew[j, :e["length"]] = e["rew"]
        out["ep/rew"] = rew
        out["ep/length"] = np.array([e["length"] for e in eps], np.int32)
        out["ep/terminated"] = np.array([e["terminated"] for e in eps], np.float32)
        out["ep/ret"] = np.array([e["ret"] for e in eps], np.float64)
        if name == "eval_idp_fhadp_trained":   # one episode at the data env's full limit (pyth_idpendulum.py:51)
            full_limit = int(env.unwrapped.max_episode_steps)
            e = run_episode(env, alg, cands[[i for i in kept if not runs[i]["terminated"]][0]], full_limit)
            assert e["length"] == full_limit and not e["terminated"]
            out.update({"full/obs0": e["obs0"], "full/obs": e["obs"], "full/act": e["act"], "full/rew": e["rew"],
                        "full/length": np.int32(e["length"]), "full/ret": np.float64(e["ret"])})
        out.update(mg.sd_to_np(alg.networks.policy.state_dict()))
        out.update(mg.model_consts(create_env_model(**env_cfg)))
    mg.save(name, **out)


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for case, (env_kw, ckpt) in CASES.items():
        if not only or case in only:
            record(case, env_kw, ckpt)
