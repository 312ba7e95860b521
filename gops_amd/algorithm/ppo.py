"""PPO - proximal policy optimisation with the clipped surrogate - on the HIP kernels.

Same class surface as the reference's gops/algorithm/ppo.py (ApproxContainer :33-48, PPO :51-240): a Gaussian StochaPolicy and a
StateValue under ONE Adam, `num_repeat x num_mini_batch` minibatch steps per `local_update` on the on-policy columns
`obs, act, logp, ret, adv`.

Where the arithmetic runs.  Once per `local_update`: `gops_adv_normalize` and one forward of each network over the whole sample batch
(`gops_mlp_forward`).  Per repeat every column is permuted once with `index_select`, so that minibatches are contiguous slices.  One
minibatch step is, in this order, `gops_mlp_forward` for the policy, `gops_mlp_forward` for the value, `gops_ppo_loss` (all six loss
terms and the gradient seeds in one launch), the two `gops_mlp_backward` and `HipAdam.step`; that step is what `StepGraphCache`
captures and replays, with the slice as the graph's input.  The clip range, the value clip and the three coefficients live in a small
device array the loss kernel reads, refreshed before every step: `schedule_clip = "linear"` does not invalidate the graph.

Kept as the reference has them:
  * the advantages are normalised unconditionally - `advantage_norm` is never read (ppo.py:123-125);
  * `val` and `logits` come from one no-grad forward over the whole sample batch, before the first step (ppo.py:126-128);
  * the `tb_info` values are the LAST minibatch's (ppo.py:159-163);
  * `clip_now` is updated after it is used: the first minibatch of an update still runs on the previous value (ppo.py:192, 228-231);
  * the learning rate is rescheduled after each step (ppo.py:148-155).
The shuffle is `np.random.shuffle(self.indices)` on the persistent index array (ppo.py:79, 131): a run seeded like the reference draws
the same permutations.  `data["perm"]`, an integer tensor [num_repeat, sample_batch_size], overrides it.

The policy is the reference's `std_type="mlp_shared"` StochaPolicy with a GaussDistribution; `"parameter"` (the default of the
reference's PPO examples) and `"mlp_separated"` are not yet supported - `create_alg` refuses them with that reason.
"""
__all__ = ["ApproxContainer", "PPO"]

import time

import numpy as np
import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm import _on_policy
from gops_amd.algorithm._on_policy import ApproxContainer, OnPolicyBase
from gops_amd.algorithm.base import batch_to_device, cuda_device_of, grad_buffers
from gops_amd.utils.common_utils import make_adam
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags

# what the reference's constructor reads with kwargs[...] (ppo.py:99)
MANDATORY = ("learning_rate",)
COLUMNS = ("obs", "act", "logp", "adv", "ret", "val", "logits")   # of a minibatch: the graph's inputs
LOSS_TERMS = ("loss_total", "loss_surrogate", "loss_value", "loss_entropy", "approximate_kl", "clip_fraction")


def refusal(kwargs: dict):
    """Why `create_alg` cannot build PPO from these arguments, or None."""
    return _on_policy.refusal("PPO", "the loss kernel evaluates that density", kwargs)


class PPO(OnPolicyBase):
    """max_iteration, num_repeat, num_mini_batch, mini_batch_size, sample_batch_size: the reference's arguments (ppo.py:62-79); the
    attributes below its defaults (ppo.py:82-96)."""

    def __init__(self, *, max_iteration: int, num_repeat: int, num_mini_batch: int, mini_batch_size: int, sample_batch_size: int, index=0,
                 **kwargs):
        super().__init__(index, **kwargs)
        self.max_iteration = max_iteration
        self.num_repeat = num_repeat
        self.num_mini_batch = num_mini_batch
        self.mini_batch_size = mini_batch_size
        self.sample_batch_size = sample_batch_size
        self.indices = np.arange(self.sample_batch_size)

        self.clip = 0.2
        self.clip_now = self.clip
        self.EPS = 1e-8
        self.gamma = 0.99
        self.reward_scale = 0.1
        self.loss_coefficient_kl = 0.2
        self.loss_coefficient_value = 1.0
        self.loss_coefficient_entropy = 0.0

        self.schedule_adam = "none"
        self.schedule_clip = "none"
        self.advantage_norm = True
        self.loss_value_clip = True
        self.value_clip = 10.0
        self.loss_value_norm = False

        self._init_on_policy(kwargs)
        self.learning_rate = kwargs["learning_rate"]
        self.approximate_optimizer = make_adam(self.networks.parameters(), lr=self.learning_rate)
        self._graph = StepGraphCache()
        self.graph_replays = 0   # minibatch steps that ran as a graph replay

    @property
    def adjustable_parameters(self):
        return ("gamma", "reward_scale", "clip", "loss_value_clip", "value_clip", "loss_value_norm", "advantage_norm", "loss_coefficient_kl",
                "loss_coefficient_value", "loss_coefficient_entropy", "schedule_adam", "schedule_clip")

    # ---- update API ----------------------------------------------------------------------------
    def local_update(self, data: dict, iteration: int) -> dict:
        start_time = time.perf_counter()
        device = cuda_device_of(self.networks)
        nets, opt = self.networks, self.approximate_optimizer
        cols = batch_to_device(data, device, ("obs", "act", "logp", "adv", "ret"))
        S = cols["obs"].shape[0]
        cols["act"] = cols["act"].reshape(S, -1)
        cols["adv"] = self._adv_normalize(device).run(cols["adv"], self.EPS, out=self._buf("adv", (S,), device))
        cols["val"] = self._net("value@all", nets.value, S, device).forward(cols["obs"], out=self._buf("val", (S,), device)).view(S)
        head = self._net("policy@all", nets.policy, S, device).forward(cols["obs"])
        A = head.shape[1] // 2
        cols["logits"] = torch.cat((head[:, :A], torch.clamp(head[:, A:], nets.policy.min_log_std, nets.policy.max_log_std).exp()), dim=-1)

        perm = data.get("perm")
        if perm is not None:
            perm = torch.as_tensor(perm).to(device=device, dtype=torch.int64)
            assert tuple(perm.shape) == (self.num_repeat, self.sample_batch_size), "data['perm']: [num_repeat, sample_batch_size]"
        M = self.mini_batch_size
        out = None
        for r in range(self.num_repeat):
            if perm is None:
                np.random.shuffle(self.indices)
                idx = torch.from_numpy(self.indices).to(device)
            else:
                idx = perm[r]
            shuffled = {k: cols[k].index_select(0, idx) for k in COLUMNS}
            for n in range(self.num_mini_batch):
                mb = {k: v[M * n:M * (n + 1)] for k, v in shuffled.items()}
                out = self._minibatch_step(mb, iteration)
        self._step_schedulers()

        tb_info = dict()
        tb_info[tb_tags["loss_actor"]] = scalar(out, 1)
        tb_info[tb_tags["loss_critic"]] = scalar(out, 2)
        tb_info["PPO/KL_divergence-RL iter"] = scalar(out, 4)
        tb_info[tb_tags["alg_time"]] = (time.perf_counter() - start_time) * 1000
        self.tb_info = tb_info
        self.last_loss_terms = out   # device tensor [6]: LOSS_TERMS of the last minibatch
        return tb_info

    def _minibatch_step(self, mb: dict, iteration: int) -> torch.Tensor:
        """One optimisation step on a minibatch (ppo.py:138-155), eager or as a graph replay; -> the six loss terms [6] (device)."""
        opt = self.approximate_optimizer
        M, device = mb["obs"].shape[0], mb["obs"].device
        loss = self._ppo_loss(M, device)
        loss.set_hyper(self.clip_now, self.value_clip, self.loss_coefficient_kl, self.loss_coefficient_value, self.loss_coefficient_entropy)
        out = self._adam_step(self._graph, self._signature(mb), mb, self.minibatch_gradients, opt, "graph_replays")
        if self.schedule_clip == "linear":   # (after its use: ppo.py:228-231)
            decay_rate = 1 - (iteration / self.max_iteration)
            assert decay_rate >= 0, "decay_rate is less than 0!"
            self.clip_now = self.clip * decay_rate
        if self.schedule_adam == "linear":
            decay_rate = 1 - (iteration / self.max_iteration)
            assert decay_rate >= 0, "the decay_rate is less than 0!"
            for g in opt.param_groups:
                g["lr"] = self.learning_rate * decay_rate
        return out

    def minibatch_gradients(self, mb: dict) -> torch.Tensor:
        """The kernels of one minibatch without the optimizer step: both forwards, `gops_ppo_loss`, both backwards.  `mb`: COLUMNS as
        fp32 device tensors of M rows.  Leaves the gradients in `.grad`; -> LOSS_TERMS as one device tensor [6], without synchronising.
        The loss kernel reads clip, value_clip and the coefficients from its device array: `_minibatch_step` refreshes it."""
        nets = self.networks
        o = mb["obs"]
        M, device = o.shape[0], o.device
        pol, val, loss = self._net("policy@mb", nets.policy, M, device), self._net("value@mb", nets.value, M, device), self._ppo_loss(M, device)
        if loss._hyper is None:
            loss.set_hyper(self.clip_now, self.value_clip, self.loss_coefficient_kl, self.loss_coefficient_value, self.loss_coefficient_entropy)
        head = pol.forward(o, out=self._buf("head", (M, pol.out_dim), device))
        v = val.forward(o, out=self._buf("v", (M, 1), device))
        seed_head, seed_v, stats = loss.run(head, v, mb["act"], mb["logp"], mb["adv"], mb["ret"], mb["val"], mb["logits"],
                                            seed_head=self._buf("seed_head", (M, pol.out_dim), device), seed_v=self._buf("seed_v", (M, 1), device))
        gw, gb = grad_buffers(nets.policy)
        pol.backward(o, seed_head, gw, gb)
        gw, gb = grad_buffers(nets.value)
        val.backward(o, seed_v, gw, gb)
        return stats.clone()

    def _signature(self, mb):
        nets = self.networks
        return (tuple((k, tuple(v.shape)) for k, v in mb.items()), bool(self.loss_value_clip), bool(self.loss_value_norm),
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in nets.parameters()),
                self.approximate_optimizer.storage_signature(), self._storage())

    # ---- kernels' objects ------------------------------------------------------------------------
    def _ppo_loss(self, M: int, device) -> hb.PpoLoss:
        pol = self.networks.policy
        key = ("ppo_loss", str(device), bool(self.loss_value_clip), bool(self.loss_value_norm))
        loss = self._cache.get(key)   # (on every step's path: no closure for `_one`)
        if loss is None:
            loss = self._cache[key] = hb.PpoLoss(pol.act_dim, pol.min_log_std, pol.max_log_std, device, loss_value_clip=self.loss_value_clip,
                                                 loss_value_norm=self.loss_value_norm)
        return loss
