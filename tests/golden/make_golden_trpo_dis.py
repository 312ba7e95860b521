"""Generate the fixtures of TRPO on discrete actions (`trpo_dis_*.npz`) by running the UNMODIFIED reference, and
`trpo_dis_reference_error.json`.

Run in the build container only (needs the reference tree):  python tests/golden/make_golden_trpo_dis.py
Every array written here is an input, or an output of the reference's own `gops.algorithm.trpo.TRPO` on its
`gops.apprfunc.mlp.StochaPolicyDis` with the CategoricalDistribution: one `local_update` in fp32 on the CPU.  As in
make_golden_trpo.py, `_conjugate_gradient` is wrapped from outside to record `g_vec` and the solve's `x` and `r`, and the line
search is re-evaluated afterwards with the reference's own distributions (`candidates`, taken from that maker); the accepted
candidate's parameters must be the ones the reference left in the policy, bit for bit.

Batches are synthetic: normal observations, uniform action indices, random `adv` / `ret`; the policy's output layer is scaled so
that the logits have unit spread over the batch (the default initialisation leaves the probabilities all but uniform).  Asserted per
fixture: every action occurs in the batch, every tried candidate keeps |kl - delta| > 0.02 delta and |surrogate| > 1e-4, and the
two special cases really backtrack (accepted index >= 1) or reject every candidate (accepted = -1).  Seeds are searched from the
tag's checksum on until all of it holds.

`trpo_dis_reference_error.json`: per fixture and quantity, the relative error (max |a - b| / max |b|) of the fp32 reference against
the float64 restatement of tests/trpo_dis_helpers.py - the yardstick of the GPU tests' bars.
"""
import json
import os
import sys
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (installs the reference import hook)
from _make_ac_common import arrays, last_linear, meta_entry, state  # noqa: E402
from make_golden_trpo import CTOR, EPS, KL_MARGIN, SUR_MARGIN, candidates, seeds_from  # noqa: E402

from gops.algorithm.trpo import TRPO  # noqa: E402

CART = dict(obs=4, act_num=2, hidden=(64, 64), act="relu", batch=96)   # example_train/trpo/trpo_mlp_cartpole_onserial.py's shape
O3N5 = dict(obs=3, act_num=5, hidden=(16, 32), act="gelu", batch=96)
# name: (network and batch shape, constructor arguments over CTOR, what the line search must do)
CASES = {
    "trpo_dis_cart_relu": (CART, dict(), "any"),
    "trpo_dis_o3n5_gelu": (O3N5, dict(), "any"),
    "trpo_dis_backtrack": (CART, dict(delta=0.3, damping_factor=0.01), "later"),
    "trpo_dis_all_rejected": (CART, dict(delta=0.3, damping_factor=0.01, max_search=1), "none"),
}
SAME_SEED = {"trpo_dis_all_rejected": "trpo_dis_backtrack"}   # the same case with max_search = 1


def alg_kwargs(case, seed, ctor):
    return dict(algorithm="TRPO", seed=seed, cnn_shared=False, env_id="gym_cartpole", obsv_dim=case["obs"], action_type="discret",
                action_num=case["act_num"], policy_func_type="MLP", policy_func_name="StochaPolicyDis", policy_act_distribution="default",
                policy_hidden_sizes=list(case["hidden"]), policy_hidden_activation=case["act"], policy_output_activation="linear",
                policy_std_type="parameter", value_func_type="MLP", value_func_name="StateValue", value_hidden_sizes=list(case["hidden"]),
                value_hidden_activation=case["act"], value_output_activation="linear", use_gpu=False, **ctor)


def build(case, seed, over):
    ctor = dict(CTOR, **over)
    torch.manual_seed(seed)
    alg = TRPO(**alg_kwargs(case, seed, ctor))
    return alg, torch.Generator().manual_seed(seed + 1000), ctor


def shaped_batch(alg, case, g):
    """obs, act, adv, ret; the policy's output layer scaled to logits of unit spread over the batch."""
    B, O, N = case["batch"], case["obs"], case["act_num"]
    nets = alg.networks
    obs = torch.randn(B, O, generator=g)
    with torch.no_grad():
        head = last_linear(nets.policy.q)
        scale = 1.0 / nets.policy(obs).std(dim=0)
        head.weight.mul_(scale[:, None])
        head.bias.mul_(scale)
        act = torch.randint(N, (B, 1), generator=g).float()
        adv = torch.randn(B, generator=g) + 0.3
        ret = nets.value(obs) + torch.randn(B, generator=g)
    return dict(obs=obs, act=act, adv=adv, ret=ret)


def one_update_at(tag, seed):
    case, over, search = CASES[tag]
    alg, g, ctor = build(case, seed, over)
    data = shaped_batch(alg, case, g)
    if set(data["act"].long().flatten().tolist()) != set(range(case["act_num"])):
        raise AssertionError((tag, ["an action does not occur in the batch"]))
    out = {**arrays(data, "in/"), **state(alg)}
    old_policy = deepcopy(alg.networks.policy)
    tap, inner = {}, TRPO._conjugate_gradient

    def tapped(Ax, b, x, rtol, atol, max_cg):
        tap["g"] = b.detach().clone()
        xs, rs = inner(Ax, b, x, rtol, atol, max_cg)
        tap["x"], tap["r"] = xs.detach().clone(), rs.detach().clone()
        return xs, rs

    TRPO._conjugate_gradient = staticmethod(tapped)
    try:
        tb = alg.local_update({k: v.clone() for k, v in data.items()}, 0)
    finally:
        TRPO._conjugate_gradient = staticmethod(inner)
    adv = data["adv"]
    if alg.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + EPS)
    step, tried, index, weights = candidates(alg, old_policy, data, tap["g"], tap["x"], adv)
    assert torch.equal(weights, torch.nn.utils.parameters_to_vector(alg.networks.policy.parameters())), tag
    kl_gap = min(abs(kl - alg.delta) / alg.delta for _, kl in tried)
    sur_gap = min(abs(s) for s, _ in tried)
    problems = []
    if kl_gap <= KL_MARGIN:
        problems.append(f"kl within {kl_gap:.3f} delta of delta")
    if sur_gap <= SUR_MARGIN:
        problems.append(f"|surrogate| {sur_gap:.2e}")
    if (search == "later" and index < 1) or (search == "none" and index != -1):
        problems.append(f"accepted index {index}")
    if problems:
        raise AssertionError((tag, problems))
    print(f"{tag}: seed {seed}, accepted {index} of {tried}, kl margin {kl_gap:.3f} delta, |surrogate| >= {sur_gap:.3e}")
    out.update(meta_entry(cfg=dict(case, hidden=list(case["hidden"])), ctor=ctor, seed=seed, kl_margin=kl_gap, surrogate_margin=sur_gap))
    out.update(g_vec=tap["g"].numpy(), cg_x=tap["x"].numpy(), cg_r=tap["r"].numpy(), trpo_step=step.numpy(), accepted=np.int64(index),
               cand_surrogate=np.array([s for s, _ in tried]), cand_kl=np.array([k for _, k in tried]))
    out.update(state(alg, "sd_after/"))
    for k, v in tb.items():
        if not k.startswith("Time/"):
            out["tb/" + k] = np.float64(v)
    mg.save(tag, **out)
    return seed


def reference_error():
    """The fp32 reference's recorded g, x, step and final policy against the float64 restatement, per fixture."""
    import trpo_dis_helpers as td
    import trpo_helpers as th
    errors = {}
    for tag in CASES:
        alg, g, meta = td.load_trpo_dis(tag)
        got = td.restate_trpo_update(alg, th.data_of(g))
        after = [g["sd_after/policy." + k] for k in alg.networks.policy.state_dict()]
        errors[tag] = dict(g=th.rel_max(g["g_vec"], got["g"]), x=th.rel_max(g["cg_x"], got["x"]), step=th.rel_max(g["trpo_step"], got["step"]),
                           policy=th.rel_max(np.concatenate([a.reshape(-1) for a in after]), th.flat(got["policy"])))
        print(tag, errors[tag])
    with open(os.path.join(HERE, "trpo_dis_reference_error.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    only = set(sys.argv[1:])
    found = {}
    for tag in CASES:
        if not only or tag in only:
            found[tag] = seeds_from(tag, one_update_at, base=found.get(SAME_SEED.get(tag)))
    if not only or "reference_error" in only:
        reference_error()
