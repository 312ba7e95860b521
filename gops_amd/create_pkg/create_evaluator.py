"""create_evaluator: evaluators keyed by name (surface of gops/create_pkg/create_evaluator.py:30-61).  "evaluator" builds
`gops_amd.trainer.evaluator.Evaluator` in-process - no Ray actor - from the reference's kwargs (`num_eval_episode`, `eval_save`,
`save_folder`, `seed`, `is_render`; of its own `max_episode_steps`, `fused`, `action_table`, `stochastic_mode`) plus either
`env_model` and `networks` (the learner's own) or the kwargs `create_alg` takes, from which both are built."""
from gops_amd.create_pkg._registry import Registry

registry = Registry("evaluator")


def register(evaluator_name: str, entry_point, **kwargs):
    registry.add(evaluator_name, entry_point, kwargs, evaluator_name=evaluator_name)


def _build_evaluator(**kwargs):
    from gops_amd.trainer.evaluator import Evaluator
    if kwargs.pop("is_render", False):
        raise NotImplementedError("is_render=True: gops_amd's evaluator runs its episodes on the GPU and does not render; "
                                  "use the reference's evaluator for rendering")
    env_model, networks = kwargs.pop("env_model", None), kwargs.pop("networks", None)
    if env_model is None or networks is None:
        model_kwargs = dict(kwargs, reward_scale=None, reward_shift=None, repeat_num=None)   # evaluator.py:20-25
        if env_model is None:
            from gops_amd.create_pkg.create_env_model import create_env_model
            env_model = create_env_model(**model_kwargs)
        if networks is None:
            from gops_amd.create_pkg.create_alg import create_approx_contrainer
            networks = create_approx_contrainer(**kwargs)
    cfg = kwargs.pop("cfg", None) or {k: kwargs[k] for k in ("env_id", "pre_horizon", "lq_config") if kwargs.get(k) is not None}
    return Evaluator(index=kwargs.pop("index", 0), env_model=env_model, networks=networks, cfg=cfg,
                     num_eval_episode=kwargs.pop("num_eval_episode"), eval_save=kwargs.pop("eval_save", True),
                     save_folder=kwargs.pop("save_folder", None), seed=kwargs.pop("seed", 0) or 0,
                     max_episode_steps=kwargs.pop("max_episode_steps", None), fused=kwargs.pop("fused", True),
                     action_table=kwargs.pop("action_table", None), stochastic_mode=kwargs.pop("stochastic_mode", False))


register("evaluator", _build_evaluator)


def create_evaluator(evaluator_name: str = "evaluator", **kwargs) -> object:
    return registry.build(evaluator_name, **kwargs)
