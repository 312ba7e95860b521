"""DQN - deep Q-learning on a discrete action space - on the HIP kernels.

Same class surface as the reference's gops/algorithm/dqn.py (ApproxContainer :34-61, DQN :64-191): an ActionValueDis network `q`
regressed at the taken action onto `r * reward_scale + gamma (1 - d) max_a q_target(o2)[a]`, a Polyak-averaged target, and a
`policy` that is the no-grad forward of `q` (the sampler takes its arg-max).

Where the arithmetic runs:
  * the backup - target network, maximum over its `act_num` outputs, the Bellman line - is ONE launch of `gops_dqn_backup`
    (`fused_target=True`, the default, for networks up to `FUSED_MAX_WIDTH` wide; "force": for every shape the kernel holds), or composed
    from `gops_mlp_forward` and `torch.max` (`fused_target=False`, wider networks, and whenever the kernel refuses the shape - more
    than 16 actions, hidden widths beyond 256); `backup_path` names what the last update ran;
  * the live network is `gops_mlp_forward`, then ONE launch of `gops_dqn_loss` - the dense output-layer seed `2 w (q_sel - backup) / B`
    in the taken column and zeros elsewhere, the loss, PER's `|q_sel - backup|` -, then `gops_mlp_backward`; `HipAdam`; `gops_polyak_update`.
`local_update` replays as ONE HIP graph (there is no delayed step); the batch is the graph's input.

The `act` column is the action index as a float, converted by truncation as the reference's `a.to(torch.long)`.  A row whose index
lies outside [0, act_num) would make the reference's `gather` raise; a kernel cannot raise: such a row gets a zero seed and `abs_err` 0,
adds nothing to the loss, and is counted - `bad_action_rows()` reads the count of the last update.

Prioritized replay: the reference's PER path reads `self.networks.target` (dqn.py:149), an attribute that does not exist - it raises.
Here the evident intent is implemented: the backup from `q_target`, the importance-weighted loss `mean(w (q_sel - backup)^2)`, and
`local_update` returns `(tb_info, idx, |q_sel - backup|)` like DDPG / TD3.  This path has no reference fixture: it is pinned by the
tests' float64 restatement only.
"""
__all__ = ["ApproxContainer", "DQN"]

import time
from copy import deepcopy
from typing import Tuple

import torch

from gops_amd import hip_backend as hb
from gops_amd.algorithm._actor_critic import FUSED_MAX_WIDTH, NetCache
from gops_amd.algorithm.base import AlgorithmBase, ApprBase, batch_to_device, cuda_device_of, grad_buffers, install_grads
from gops_amd.apprfunc.mlp import ActionValueDis
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.utils.common_utils import get_apprfunc_dict, make_adam
from gops_amd.utils.hip_graph import StepGraphCache
from gops_amd.utils.lazy_scalar import scalar
from gops_amd.utils.tensorboard_setup import tb_tags

# `fused_target=True` keeps DDPG / TD3's threshold `FUSED_MAX_WIDTH` (64): DQN's own measurement has the same crossover (DESIGN.md
# 4.17: update, ms fused / composed, graph replay: 64-64 nets 0.082 / 0.097 at B = 256 and 0.271 / 0.293 at B = 65536; 256-256 nets
# 0.206 / 0.142 and 1.39 / 0.638).
MANDATORY = ("value_learning_rate", "buffer_name")   # what the reference indexes (dqn.py:58,80): a KeyError without them
N_SCALARS = 4   # loss_q, mean(q_sel), rows with an index out of range, (spare): the head of the update's output vector, PER's abs_err behind it


def refusal(kwargs: dict):
    """Why `create_alg` cannot build DQN from these arguments, or None."""
    if kwargs.get("value_func_type") != "MLP":
        return f"DQN runs an MLP value network only (value_func_type {kwargs.get('value_func_type')!r})"
    if kwargs.get("value_func_name") != "ActionValueDis":
        return (f"DQN takes the action values of a discrete action space (value_func_name 'ActionValueDis'), not "
                f"{kwargs.get('value_func_name')!r}")
    if kwargs.get("action_type") != "discret":
        return f"DQN takes a discrete action space (action_type 'discret' with action_num), not {kwargs.get('action_type')!r}"
    if kwargs.get("value_output_activation", "linear") != "linear":
        return (f"DQN takes a network with a linear output layer (value_output_activation {kwargs.get('value_output_activation')!r}): "
                "the HIP kernels apply no output activation")
    if hb.dtype_id(kwargs.get("mlp_dtype")) != 0:
        return f"DQN is fp32 only (mlp_dtype {kwargs.get('mlp_dtype')!r}): its kernels have no half-precision path"
    trainer = kwargs.get("trainer")
    if trainer is not None and trainer.startswith(("off_sync", "off_async")):
        return (f"DQN runs under off_serial_trainer only: trainer {trainer!r} (data-parallel replicas) has not been run with its "
                "update_info, least of all with a prioritized buffer's (tb_info, idx, abs_err)")
    return None


class ApproxContainer(ApprBase):
    """q, its frozen target, and `policy` = the no-grad forward of q; construction order (and with it the RNG draws) follows
    dqn.py:41-58."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        q_args = get_apprfunc_dict("value", **kwargs)
        self.q = create_apprfunc(**q_args)
        self.q_target = deepcopy(self.q)
        for p in self.q_target.parameters():
            p.requires_grad = False

        def policy_q(obs):   # the policy comes straight from q, and is for sampling only
            with torch.no_grad():
                return self.q.forward(obs)

        self.policy = policy_q
        self.q_optimizer = make_adam(self.q.parameters(), lr=kwargs["value_learning_rate"])

    def create_action_distributions(self, logits):
        return self.q.get_act_dist(logits)


class DQN(NetCache, AlgorithmBase):
    """buffer_name: "prioritized_replay_buffer" makes `local_update` return (tb_info, idx, |q_sel - backup|); fused_target: the
    backup as one `gops_dqn_backup` launch for networks up to `FUSED_MAX_WIDTH` wide ("force": wherever the kernel holds the shape;
    False: always composed from `gops_mlp_forward` and `torch.max`)."""

    def __init__(self, index=0, fused_target=True, **kwargs):
        super().__init__(index, **kwargs)
        self.gamma = 0.99
        self.tau = 0.005
        self.reward_scale = 1
        self.networks = ApproxContainer(**kwargs)
        if type(self.networks.q) is not ActionValueDis:
            raise NotImplementedError(f"DQN: value network {type(self.networks.q).__name__} (MLP ActionValueDis only)")
        self.per_flag = kwargs["buffer_name"] == "prioritized_replay_buffer"
        self.fused_target = "force" if fused_target == "force" else bool(fused_target)
        self.backup_path = None   # "fused" / "composed": how the last update formed the backup
        self.tb_info = dict()
        self._cache, self._bufs, self._graphs, self._last = {}, {}, {}, None

    @property
    def adjustable_parameters(self):
        return ("gamma", "tau")

    # ---- update API ----------------------------------------------------------------------------
    def local_update(self, data: dict, iteration: int):
        start_time = time.time()
        batch = self._batch(data)
        opt = self.networks.q_optimizer

        def update(b):
            out = self._gradient_kernels(b)
            self._update()
            return out

        cache = self._graphs.setdefault("update", StepGraphCache())   # one graph: DQN has no delayed step
        out = cache.run(self._signature(batch), batch, update, before_replay=opt.sync_hyper, on_replay=opt.advance,
                        work=batch["obs"].shape[0], on_capture_fail=opt.resync_device_state)
        self._step_schedulers()
        return self._result(out, data, start_time)

    def get_remote_update_info(self, data: dict, iteration: int) -> Tuple[dict, dict]:
        start_time = time.time()
        extra_info = self._result(self._gradient_kernels(self._batch(data)), data, start_time)
        return extra_info, {"q_grad": [p.grad for p in self.networks.q.parameters()], "iteration": iteration}

    def remote_update(self, update_info: dict):
        install_grads(self.networks.q, update_info["q_grad"])
        self._update()
        self._step_schedulers()

    def bad_action_rows(self) -> int:
        """Rows of the last update's batch whose action index lay outside [0, act_num) (they were left out of the loss)."""
        return 0 if self._last is None else int(self._last[2].item())

    def _batch(self, data: dict):
        device = cuda_device_of(self.networks)
        return batch_to_device(data, device, ("obs", "act", "rew", "obs2", "done") + (("weight",) if self.per_flag else ()))

    def _result(self, out: torch.Tensor, data: dict, start_time: float):
        self._last = out
        tb_info = dict()
        tb_info[tb_tags["loss_critic"]] = scalar(out, 0)
        tb_info[tb_tags["alg_time"]] = (time.time() - start_time) * 1000
        self.tb_info = tb_info
        if self.per_flag:
            return tb_info, data["idx"], out[N_SCALARS:]
        return tb_info

    def _signature(self, batch):
        nets = self.networks
        return (self.fused_target, tuple((k, tuple(v.shape)) for k, v in batch.items()), float(self.gamma), float(self.tau),
                float(self.reward_scale),
                tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for m in (nets.q, nets.q_target) for p in m.parameters()),
                nets.q_optimizer.storage_signature(),
                tuple(sorted(obj.workspace.data_ptr() for obj in self._cache.values() if hasattr(obj, "workspace"))),
                tuple(sorted(t.data_ptr() for t in self._bufs.values())))

    def _update(self):
        nets = self.networks
        nets.q_optimizer.step()
        online, target = list(nets.q.parameters()), list(nets.q_target.parameters())   # p_targ <- (1 - tau) p_targ + tau p   (dqn.py:156-166)
        up = self._cache.get("polyak")
        if up is None or not up.matches(target, online):
            up = self._cache["polyak"] = hb.PolyakUpdater(target, online)
        up.step(self.tau)

    # ---- kernels -------------------------------------------------------------------------------
    def _dqn_backup(self, B: int, device) -> hb.DqnBackup:
        q = self.networks.q_target.hip_mlp()
        key = ("dqn_backup", B, str(device))
        db = self._cache.get(key)
        if db is None:
            db = self._cache[key] = hb.DqnBackup(q, batch=B, device=device)
        else:
            db.set_net(q)
        return db

    def _backup(self, batch) -> torch.Tensor:
        """`r * reward_scale + gamma (1 - d) max_a q_target(o2)[a]` [B], no gradient (dqn.py:104,138-140)."""
        o2 = batch["obs2"]
        B, device = o2.shape[0], o2.device
        widest = max(l.out_features for l in self.networks.q_target.linear_layers()[:-1])
        if self.fused_target and (self.fused_target == "force" or widest <= FUSED_MAX_WIDTH):
            db = self._dqn_backup(B, device)
            if db.supported:
                self.backup_path = "fused"
                return db.run(o2, batch["rew"], batch["done"], reward_scale=self.reward_scale, gamma=self.gamma)["backup"]
        self.backup_path = "composed"
        return self._backup_composed(batch)[0]

    def _backup_composed(self, batch):
        """(backup [B], q_targ [B, act_num], a_star [B]) from `gops_mlp_forward` and `torch.max`."""
        o2 = batch["obs2"]
        q_t = self._net("q_target@o2", self.networks.q_target, o2.shape[0], o2.device).forward(o2)
        q_max, a_star = torch.max(q_t, dim=1)
        return batch["rew"] * self.reward_scale + self.gamma * (1 - batch["done"]) * q_max, q_t, a_star

    def _gradient_kernels(self, batch) -> torch.Tensor:
        """Enqueue one compute_gradient; returns [loss_q, mean(q_sel), rows with an index out of range, 0] (+ abs_err [B] with PER)
        as one device tensor, without synchronising."""
        nets = self.networks
        o = batch["obs"]
        B, device = o.shape[0], o.device
        N = nets.q.act_num
        backup = self._backup(batch)
        net = self._net("q@data", nets.q, B, device)
        q_all = net.forward(o, out=self._buf("q_all", (B, N), device))
        key = ("dqn_loss", str(device))
        dl = self._cache.get(key)
        if dl is None:
            dl = self._cache[key] = hb.DqnLoss(device)
        seed, abs_err, stats = dl.run(q_all, batch["act"].reshape(-1), backup, batch.get("weight") if self.per_flag else None,
                                      seed=self._buf("seed", (B, N), device), abs_err=self._buf("abs_err", (B,), device))
        gw, gb = grad_buffers(nets.q)
        net.backward(o, seed, gw, gb)
        head = torch.cat([stats, stats[:1] * 0])
        return torch.cat([head, abs_err]) if self.per_flag else head
