"""create_alg: algorithms keyed by the upper-camel file name (`fhadp.py` -> "FHADP"); each module exports
that class and `ApproxContainer` (surface of gops/create_pkg/create_alg.py:47-97).  Parallel trainers are
one process per GPU here (torch.distributed over RCCL): every trainer kind gets this rank's local object - for the
off_sync / off_async trainers behind the list-of-actor-handles shape the reference's scripts expect (`LocalActor`)."""
import inspect

from gops_amd.create_pkg._registry import Registry
from gops_amd.utils.gops_path import algorithm_path, underline2camel

registry = Registry("algorithm")
RPI_ONLY_ENVS = ("pyth_oscillatorconti", "pyth_aircraftconti", "pyth_suspensionconti")
_TRAINER_KINDS = ("off_serial", "on_serial", "on_sync", "off_sync", "off_async")


def register(algorithm: str, entry_point, approx_container_cls, **kwargs):
    registry.add(algorithm, entry_point, kwargs, algorithm=algorithm, approx_container_cls=approx_container_cls)


def _entries(stem, module):
    name = underline2camel(stem, first_upper=True)
    yield name, getattr(module, name), dict(algorithm=name, approx_container_cls=getattr(module, "ApproxContainer"))


# RPI, DDPG and TD3 are algorithms like the others; they sit in a registry of their own for one reason only: the key set of `registry`
# is pinned by tests/test_host_cpu.py (the host contract as it stood before RPI), and that test file stays as it is.  `create_alg`
# and `create_approx_contrainer` look in both.  Once the pinned set is revisited, `loop_registry` folds back into `registry`.
_LOOP_ALGORITHMS = ("rpi", "ddpg", "td3")
_ACTOR_CRITIC = ("DDPG", "TD3")   # model-free: MLP DetermPolicy + MLP ActionValue, fp32 (algorithm/_actor_critic.py)
loop_registry = Registry("algorithm")
# DSACT likewise: the key set of `loop_registry` is pinned by tests/test_td3_cpu.py (as it stood before DSAC-T), and that test file
# stays as it is.  `create_alg` and `create_approx_contrainer` look in all three; `soft_registry` folds back with `loop_registry`.
_SOFT_ALGORITHMS = ("dsact",)
soft_registry = Registry("algorithm")
# SAC and DSAC likewise: the key set of `soft_registry` is pinned by tests/test_dsact_cpu.py (as it stood before them), and that test
# file stays as it is.  `create_alg` and `create_approx_contrainer` look in all four; `soft_q_registry` folds back with the others.
_SOFT_Q_ALGORITHMS = ("sac", "dsac")
soft_q_registry = Registry("algorithm")
# PPO likewise: the key set of `soft_q_registry` is pinned by tests/test_sac_cpu.py (as it stood before PPO), and that test file stays
# as it is.  `create_alg` and `create_approx_contrainer` look in all five; `on_policy_registry` folds back with the others.
_ON_POLICY_ALGORITHMS = ("ppo",)
on_policy_registry = Registry("algorithm")
# TRPO likewise: the key set of `on_policy_registry` is pinned by tests/test_ppo_cpu.py (as it stood before TRPO), and that test file
# stays as it is.  `create_alg` and `create_approx_contrainer` look in all six; `trust_region_registry` folds back with the others.
_TRUST_REGION_ALGORITHMS = ("trpo",)
trust_region_registry = Registry("algorithm")
# DQN likewise: the key set of `trust_region_registry` is pinned by tests/test_trpo_cpu.py (as it stood before DQN), and that test file
# stays as it is.  No test pins the key set of `value_based_registry`: the next algorithm joins it (one more stem in the tuple below).
_VALUE_BASED_ALGORITHMS = ("dqn",)
value_based_registry = Registry("algorithm")
_ELSEWHERE = (_LOOP_ALGORITHMS + _SOFT_ALGORITHMS + _SOFT_Q_ALGORITHMS + _ON_POLICY_ALGORITHMS + _TRUST_REGION_ALGORITHMS
              + _VALUE_BASED_ALGORITHMS)
registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem not in _ELSEWHERE)
loop_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _LOOP_ALGORITHMS)
soft_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _SOFT_ALGORITHMS)
soft_q_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _SOFT_Q_ALGORITHMS)
on_policy_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _ON_POLICY_ALGORITHMS)
trust_region_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _TRUST_REGION_ALGORITHMS)
value_based_registry.scan(algorithm_path, "gops_amd.algorithm", _entries, keep=lambda stem: stem in _VALUE_BASED_ALGORITHMS)
# the registries beside `registry`, and of them the ones whose modules state `MANDATORY` and `refusal(kwargs)` themselves
_SIDE_REGISTRIES = (loop_registry, soft_registry, soft_q_registry, on_policy_registry, trust_region_registry, value_based_registry)
_SELF_DESCRIBED = (soft_q_registry, on_policy_registry, trust_region_registry, value_based_registry)


def _registry_of(algorithm: str) -> Registry:
    return next((r for r in _SIDE_REGISTRIES if algorithm in r), registry)


def _defaults(kwargs: dict) -> dict:
    out = dict(kwargs)
    if out.get("seed") is None:
        out["seed"] = 0
    if out.get("cnn_shared") is None:
        out["cnn_shared"] = False
    return out


class _RemoteMethod:
    """`handle.method.remote(*args)` of a Ray actor, in-process: returns the value itself."""

    def __init__(self, fn):
        self._fn = fn

    def __call__(self, *args, **kwargs):
        return self._fn(*args, **kwargs)

    def remote(self, *args, **kwargs):
        return self._fn(*args, **kwargs)


class LocalActor:
    """What the reference's example scripts expect from `create_alg` for the off_sync / off_async trainers: a list of
    actor handles whose methods are reached through `.remote(...)` (create_alg.py:87-93, e.g.
    `for alg_id in alg: alg_id.set_parameters.remote({...})`, example_train/mac/mac_mlp_cartpoleconti_async.py:153-154).
    One process per GPU here: the list has ONE entry, this rank's replica; the trainers unwrap it (`.unwrap()`)."""

    def __init__(self, obj):
        object.__setattr__(self, "_obj", obj)

    def unwrap(self):
        return self._obj

    def __getattr__(self, name):
        attr = getattr(self._obj, name)
        return _RemoteMethod(attr) if inspect.ismethod(attr) or inspect.isfunction(attr) else attr


def create_alg(**kwargs) -> object:
    reg = _registry_of(kwargs["algorithm"])
    entry = reg.lookup(kwargs["algorithm"])       # unknown algorithm: KeyError before anything else
    if reg in _SELF_DESCRIBED:   # the arguments the reference's SAC / DSAC / PPO / TRPO / DQN cannot do without: a KeyError, before any refusal
        for name in inspect.getmodule(entry.entry_point).MANDATORY:
            if name not in kwargs:
                raise KeyError(name)
    if kwargs.get("env_id") in RPI_ONLY_ENVS and kwargs["algorithm"] != "RPI":
        raise NotImplementedError(f"env {kwargs['env_id']} is a zero-sum game model that only RPI supports, not {kwargs['algorithm']}")
    poly = [k for k in ("policy", "value") if kwargs.get(k + "_func_type") == "POLY"]
    if kwargs["algorithm"] == "RPI":   # (reads the value net only; a policy_func_type in the arguments is ignored, as in the reference)
        poly = []
    if poly and kwargs["algorithm"] not in ("FHADP", "INFADP"):   # (the POLY rollout serves these two; nothing fails later)
        raise NotImplementedError(f"apprfunc type POLY ({', '.join(poly)}) is supported by FHADP and INFADP only, "
                                  f"not by {kwargs['algorithm']}")
    gauss = [k for k in ("policy", "value") if kwargs.get(k + "_func_type") == "GAUSS" and kwargs["algorithm"] != "RPI"
             and not (k == "value" and kwargs["algorithm"] == "FHADP")]   # (FHADP has no value net: the key is ignored, as for MLP)
    if gauss:   # FHADP with a GAUSS FiniteHorizonPolicy, INFADP with a GAUSS DetermPolicy and an MLP StateValue: refused here, so that nothing fails later
        reason = (f"supported by FHADP and INFADP only, not by {kwargs['algorithm']}" if kwargs["algorithm"] not in ("FHADP", "INFADP") else
                  "a GAUSS value function is outside this path: the reference itself cannot run INFADP with one (its [B, 1] value does "
                  "not broadcast into the in-place backup)" if "value" in gauss else
                  "a GAUSS policy needs an MLP value, not " + str(kwargs.get("value_func_type"))
                  if kwargs["algorithm"] == "INFADP" and kwargs.get("value_func_type") != "MLP" else None)
        if reason is not None:
            raise NotImplementedError(f"apprfunc type GAUSS ({', '.join(gauss)}): {reason}")
    lips = [k for k in ("policy", "value") if kwargs.get(k + "_func_type") == "LipsNet"]
    if lips:   # INFADP with a LipsNet DetermPolicy and an MLP StateValue is the one combination that runs; refused here, so that nothing fails later
        reason = ("a LipsNet value function does not exist (the reference has none either)" if "value" in lips else
                  "a LipsNet policy needs an MLP value, not POLY" if poly or kwargs.get("value_func_type") != "MLP" else
                  f"{kwargs['algorithm']} does not run a LipsNet policy (INFADP only)" if kwargs["algorithm"] != "INFADP" else
                  f"policy_func_name {kwargs.get('policy_func_name')!r} (DetermPolicy only)" if kwargs.get("policy_func_name") != "DetermPolicy" else
                  None)
        if reason is not None:
            raise NotImplementedError(f"apprfunc type LipsNet ({', '.join(lips)}): {reason}")
    if kwargs["algorithm"] in _ACTOR_CRITIC:   # refused here with the reason, so that nothing fails later
        from gops_amd.algorithm._actor_critic import refusal
        reason = refusal(kwargs["algorithm"], kwargs)
        if reason is not None:
            raise NotImplementedError(reason)
    if kwargs["algorithm"] in soft_registry:
        from gops_amd.algorithm.dsact import refusal
        reason = refusal(kwargs)
        if reason is not None:
            raise NotImplementedError(reason)
    if reg in _SELF_DESCRIBED:
        reason = inspect.getmodule(entry.entry_point).refusal(kwargs)
        if reason is not None:
            raise NotImplementedError(reason)
    trainer = kwargs.get("trainer")
    if trainer is not None and not trainer.startswith(_TRAINER_KINDS):
        raise RuntimeError(f"trainer {trainer} not recognized")
    alg = reg.build(kwargs["algorithm"], **_defaults(kwargs))
    if trainer is not None and trainer.startswith(("off_async", "off_sync")):
        return [LocalActor(alg)]                   # the reference returns a list of actor handles for these trainers
    return alg


def create_approx_contrainer(algorithm: str, **kwargs) -> object:
    return _registry_of(algorithm).build(algorithm, what="approx_container_cls", **_defaults(kwargs))
