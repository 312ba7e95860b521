"""RPI: relaxed policy iteration for continuous-time zero-sum games (reference: gops/algorithm/rpi.py; Li J, Li SE, Guan Y et al.,
"Ternary Policy Iteration Algorithm for Nonlinear Robust Control", arXiv 2007.06810).

Each `local_update` is one Newton iteration: the value weights take up to `max_step_update_value` Adam steps on the Hamiltonian
loss mean|U(x, u', w') + dV/dx . f(x, u', w')| of states the target weights' action / adversary pair drives, until the Hamiltonian
norm on a held-out set has fallen to 0.88 of its value at the start; then the target takes the weights.

The value function is a POLY StateValue of degree 2 or an MLP StateValue (one or two hidden layers, widths multiples of 16 up to 64,
elu / gelu / tanh / sigmoid, linear output).

Two execution paths with one meaning:
  * `use_gpu=True`: the whole policy evaluation is ONE launch (`hip_backend.RpiEvaluator`, csrc/rollout_rpi.hip, for POLY;
    `hip_backend.RpiMlpEvaluator`, csrc/rollout_rpi_mlp.hip, for an MLP), one host sync per `local_update`;
  * `use_gpu=False`: the same loop in eager fp32 torch on the host (`_evaluate_host`, with the analytic dV/dx of the degree-2
    features; `_evaluate_host_mlp`, with autograd for dV/dx and the double backward).
Both take their reset states from `self.reset_source`.  The default one draws from `np.random` in the reference's order; the device
path pre-draws a pool for `max_step_update_value + 1` resets (one bulk draw, at most MAX_POOL_BYTES) and, once the launch has reported
n steps, rewinds the generator and consumes n + 1, so the global stream stays the reference's.

The reference is the yardstick, quirks included:
  * the Hamiltonian's `forward` runs through the wrapper chain (ScaleAction from [-1, 1] onto the model's bounds - action and
    adversary column alike - then ClipAction), while `step`, `best_act` and `worst_adv` see raw values;
  * the counter the time-limit test reads lives on the bare model and is only ever incremented: rpi.py:321 assigns the zeroed counter
    through the wrapper chain, where it lands on the outermost wrapper object.  A lane past its time limit is therefore reset at every
    step from then on.  `step_count` is that counter; `step_per_episode` is the one the algorithm assigns (what
    `alg.env_model.step_per_episode` shows in the reference);
  * `max_step_per_episode` is drawn at construction (twice: algorithm and container each build a model) and never again.
Out of scope (NotImplementedError): GAUSS value functions, a POLY degree other than 2, `initial_weight`, `is_adversary=False`, and for
an MLP: relu / selu (their first derivative jumps, so dV/dx - and the action and adversary derived from it - is discontinuous: two
fp32 orderings cannot be held to a tolerance across the jump), three or more hidden layers, widths above 64 or no multiple of 16, a
non-linear output activation."""
__all__ = ["ApproxContainer", "RPI"]

import time
from copy import deepcopy

import numpy as np
import torch

from gops_amd.algorithm.base import AlgorithmBase, ApprBase
from gops_amd.create_pkg.create_apprfunc import create_apprfunc
from gops_amd.create_pkg.create_env_model import create_env_model
from gops_amd.utils.act_distribution import DiracDistribution
from gops_amd.utils.common_utils import get_apprfunc_dict
from gops_amd.utils.tensorboard_setup import tb_tags

ADAM_BETAS, ADAM_EPS = (0.9, 0.99), 1e-8
CONTINUE_FACTOR = 0.88
MAX_POOL_BYTES = 1 << 30   # device path: bound on the pre-drawn reset pool (the defaults, 10001 x 2 x 64 floats, take 5 MB)


MLP_ACTIVATIONS, MLP_MAX_WIDTH, MLP_WIDTH_STEP = ("elu", "gelu", "tanh", "sigmoid"), 64, 16


def _refuse_unsupported(kwargs):
    kind = kwargs.get("value_func_type")
    if kind not in ("POLY", "MLP"):
        raise NotImplementedError(f"RPI: value_func_type {kind!r} is not supported (POLY or MLP)")
    if kind == "POLY" and kwargs.get("value_degree") != 2:
        raise NotImplementedError(f"RPI: value_degree {kwargs.get('value_degree')!r} is not supported (2 only)")
    if kind == "MLP":   # (value_degree is ignored)
        sizes, act = list(kwargs.get("value_hidden_sizes") or []), kwargs.get("value_hidden_activation")
        if act not in MLP_ACTIVATIONS:
            raise NotImplementedError(f"RPI: value_hidden_activation {act!r} is not supported (one of {', '.join(MLP_ACTIVATIONS)}: "
                                      "dV/dx must be continuous)")
        if not 1 <= len(sizes) <= 2:
            raise NotImplementedError(f"RPI: {len(sizes)} hidden layers are not supported (one or two)")
        if any(h < MLP_WIDTH_STEP or h > MLP_MAX_WIDTH or h % MLP_WIDTH_STEP for h in sizes):
            raise NotImplementedError(f"RPI: value_hidden_sizes {sizes} are not supported (multiples of {MLP_WIDTH_STEP} up to {MLP_MAX_WIDTH})")
        if kwargs.get("value_output_activation", "linear") != "linear":
            raise NotImplementedError(f"RPI: value_output_activation {kwargs.get('value_output_activation')!r} is not supported (linear only)")
    if kwargs.get("initial_weight", None) is not None:
        raise NotImplementedError("RPI: initial_weight is not supported (the reference itself fails there); load a state_dict instead")
    if not kwargs.get("is_adversary", False):
        raise NotImplementedError("RPI: is_adversary=False is not supported (the loss needs the adversary column)")


def value_gradient(weight: torch.Tensor, norm: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
    """dV/dx [B, S] of V(x) = sum_{i<=j} w_ij y_i y_j, y = x * norm (apprfunc/poly.py StateValue, degree 2)."""
    n = obs.shape[1]
    sym = obs.new_zeros(n, n)
    iu = torch.triu_indices(n, n)
    sym[iu[0], iu[1]] = weight.reshape(-1)
    sym = sym + sym.t()   # off-diagonal w_ij on both sides, 2 w_ii on the diagonal
    return ((obs * norm) @ sym) * norm


def mlp_value_gradient(net, obs: torch.Tensor) -> torch.Tensor:
    """dV/dx [B, S] of an MLP StateValue at `obs` (autograd; no graph is kept)."""
    with torch.enable_grad():
        x = obs.detach().clone().requires_grad_(True)
        (dv,) = torch.autograd.grad(net(x).sum(), x)
    return dv


class ApproxContainer(ApprBase):
    """The value function and its target.  POLY StateValue of degree 2: weights zero, bias as nn.Linear initialises it.  MLP
    StateValue: after the module's own initialisation every Linear layer, in module order, draws its weight from
    uniform(+-sqrt(6 / (fan_in + fan_out))) and zeroes its bias (reference rpi.py:64-71)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        _refuse_unsupported(kwargs)
        self.env_model = create_env_model(**kwargs)
        self.value = create_apprfunc(**get_apprfunc_dict("value", **kwargs))
        self.is_mlp = kwargs["value_func_type"] == "MLP"
        if self.is_mlp:
            for m in self.value.v:
                if isinstance(m, torch.nn.Linear):
                    fan_out, fan_in = m.weight.shape
                    bound = np.sqrt(6.0 / (fan_in + fan_out))
                    m.weight.data.uniform_(-bound, bound)
                    m.bias.data.fill_(0)
        else:
            self.value.v.weight.data.fill_(0)
        self.value_target = deepcopy(self.value)

    def _pair(self, batch_obs):
        net = self.value_target
        dev = batch_obs.device
        if self.is_mlp:
            dv = mlp_value_gradient(net, batch_obs)
        else:
            dv = value_gradient(net.v.weight.detach(), net.norm_matrix.to(dev), batch_obs.detach())
        cpu = batch_obs.detach().cpu(), dv.cpu()   # the game models are host objects
        return self.env_model.best_act(*cpu).to(dev), self.env_model.worst_adv(*cpu).to(dev)

    def policy(self, batch_obs):
        return self._pair(batch_obs)[0]

    def action_and_adversary(self, batch_obs):
        return torch.cat(self._pair(batch_obs), dim=1)

    @staticmethod
    def create_action_distributions(logits):
        return DiracDistribution(logits)


class NumpyResetSource:
    """Reset states from `np.random`, drawn exactly as the reference's `env_model.reset()` draws them."""

    def __init__(self, model):
        self.model = model
        self._mark = None

    def next(self) -> torch.Tensor:
        return self.model.reset()

    def pool(self, n: int) -> torch.Tensor:
        """The next `n` resets as [n, S, B] (the kernel's layout) WITHOUT consuming them: `consume(k)` afterwards advances the
        stream by k resets.  One bulk draw (`reset_many`), not n * S calls of np.random."""
        self._mark, self._drawn = np.random.get_state(), n
        return self.model.reset_many(n)

    def consume(self, k: int):
        if k != self._drawn:   # (all n used: the stream already stands where n resets leave it)
            np.random.set_state(self._mark)
            self.model.reset_many(k)


class RecordedResetSource:
    """Reset states from a recorded stream [n, B, S] (tests inject the reference's own draws through this)."""

    def __init__(self, draws):
        self.draws = torch.as_tensor(np.asarray(draws), dtype=torch.float32)
        self.pos = 0

    def next(self) -> torch.Tensor:
        self.pos += 1
        return self.draws[self.pos - 1].clone()

    def pool(self, n: int) -> torch.Tensor:
        """Up to `n` recorded resets as [n, S, B]; a stream that ends early is padded with its last entry (a run that reads the
        padding has already left the recorded trajectory)."""
        got = self.draws[self.pos:self.pos + n]
        if got.shape[0] < n:
            got = torch.cat([got, got[-1:].expand(n - got.shape[0], *got.shape[1:])])
        return got.transpose(1, 2).contiguous()

    def consume(self, k: int):
        self.pos += k


class RPI(AlgorithmBase):
    def __init__(self, index: int = 0, max_newton_iteration: int = 50, max_step_update_value: int = 10000, print_interval: int = 1,
                 learning_rate: float = 1e-3, **kwargs) -> None:
        super().__init__(index, **kwargs)
        _refuse_unsupported(kwargs)
        self.max_newton_iteration = max_newton_iteration
        self.max_step_update_value = int(max_step_update_value)
        if not 1 <= self.max_step_update_value <= (1 << 20):
            raise ValueError("RPI: max_step_update_value must be within 1 .. 2**20")
        self.print_interval = print_interval
        self.num_update_value = 0
        self.norm_hamiltonian_before = 0
        self.norm_hamiltonian_after = self.max_step_update_value ** 3
        self.set_state = None
        self.grad_step = np.ones([int(self.max_newton_iteration), 1], dtype="float32")
        self.is_adversary = kwargs["is_adversary"]
        self.use_gpu = bool(kwargs.get("use_gpu", False))
        self.record_trace = False   # device path: keep (loss, norm_after) of every step in `self.trace` (tests)
        self.trace = None
        self.weight_trace = None    # host path: the weights (MLP: all parameters, flattened in parameters() order) after every step of the last local_update
        self.min_row_ratio = None   # host path: min over its loss rows of |h_i| / mean|h|

        self.env_model = create_env_model(**kwargs)
        self.obsv_dim = self.env_model.state_dim
        self.act_dim = self.env_model.action_dim
        self._obs = self.env_model.reset()
        self.done = None
        self.env_model.unwrapped.parallel_state = self._obs.clone()
        self.networks = ApproxContainer(**kwargs)
        self.learning_rate = learning_rate
        self.reset_source = NumpyResetSource(self.env_model.unwrapped)
        # Adam (betas (0.9, 0.99), no weight decay) on the value weights; the (output) bias takes no gradient and never moves
        self.is_mlp = self.networks.is_mlp
        n_feat = sum(q.numel() for q in self.networks.value.parameters()) if self.is_mlp else self.networks.value.v.weight.numel()
        self._adam = dict(step=0, exp_avg=torch.zeros(n_feat), exp_avg_sq=torch.zeros(n_feat))
        self._evaluator = None
        if self.use_gpu:
            # the device path pre-draws every reset the launch may read: [max_step_update_value + 1, S, B] floats on host and device
            pool_bytes = 4 * (self.max_step_update_value + 1) * self.obsv_dim * self.env_model.unwrapped.sample_batch_size
            if pool_bytes > MAX_POOL_BYTES:
                raise ValueError(f"RPI(use_gpu=True): the reset pool of max_step_update_value + 1 = {self.max_step_update_value + 1} "
                                 f"draws would take {pool_bytes / 2 ** 30:.1f} GiB (limit {MAX_POOL_BYTES / 2 ** 30:.0f} GiB); lower "
                                 "max_step_update_value or the batch size")
            if not torch.cuda.is_available():
                raise RuntimeError("RPI(use_gpu=True) needs an MI355X; torch.cuda is unavailable (use_gpu=False runs the host path)")
            self.networks.to(torch.device("cuda", torch.cuda.current_device()))

    @property
    def adjustable_parameters(self):
        return ("max_newton_iteration",)

    # ---- state of the parallel lanes ------------------------------------------------------------------------------------------
    @property
    def obs(self) -> torch.Tensor:
        return self._obs if self._evaluator is None else self._evaluator.lanes().t().contiguous()

    @obs.setter
    def obs(self, value):
        assert self._evaluator is None, "the lanes' states live in the device state block once the first launch has run"
        self._obs = value
        self.env_model.unwrapped.parallel_state = value.clone()

    @property
    def step_count(self) -> torch.Tensor:
        """Steps each lane has taken since construction: what the time-limit test compares with `max_step_per_episode`."""
        return self.env_model.unwrapped.step_per_episode if self._evaluator is None else self._evaluator.counters()[0]

    @property
    def step_per_episode(self) -> torch.Tensor:
        """The counter the algorithm assigns at a reset (the reference's `alg.env_model.step_per_episode`)."""
        if self._evaluator is None:
            return self.env_model.step_per_episode
        shown = self._evaluator.counters()
        return torch.where(shown[1] < 0, shown[0], shown[1])

    def continue_evaluation(self):
        return (abs(self.norm_hamiltonian_after) > CONTINUE_FACTOR * abs(self.norm_hamiltonian_before)
                and self.num_update_value < self.max_step_update_value)

    # ---- the host path --------------------------------------------------------------------------------------------------------
    def _hamiltonian_rows(self, weight, obs, pair):
        """h [B] and d(dV/dx . f)/dw [B, F] at `obs` for the action / adversary `pair` (wrapped inside `forward`)."""
        norm = self.networks.value.norm_matrix
        done = torch.zeros(obs.shape[0], dtype=torch.bool)
        _, reward, _, info = self.env_model.forward(obs, pair, done, {})
        delta = info["delta_state"]
        h = -reward + (value_gradient(weight, norm, obs) * delta).sum(1)
        y, nd = obs * norm, delta * norm
        iu = torch.triu_indices(obs.shape[1], obs.shape[1])
        dh_dw = nd[:, iu[0]] * y[:, iu[1]] + nd[:, iu[1]] * y[:, iu[0]]
        return h, dh_dw

    def _adam_step(self, weight, grad):
        st, (beta1, beta2) = self._adam, ADAM_BETAS
        st["step"] += 1
        st["exp_avg"].lerp_(grad, 1 - beta1)
        st["exp_avg_sq"].mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        step_size = self.learning_rate / (1 - beta1 ** st["step"])
        denom = (st["exp_avg_sq"].sqrt() / (1 - beta2 ** st["step"]) ** 0.5).add_(ADAM_EPS)
        weight.addcdiv_(st["exp_avg"], denom, value=-step_size)

    @torch.no_grad()
    def _evaluate_host(self):
        nets, model = self.networks, self.env_model.unwrapped
        weight = nets.value.v.weight.data.view(-1)
        self.set_state = self.reset_source.next()
        set_pair = nets.action_and_adversary(self.set_state)
        self.norm_hamiltonian_before = float(self._hamiltonian_rows(weight, self.set_state, set_pair)[0].abs().mean())
        loss, trace, weights, ratios = 0.0, [], [], []
        for _ in range(self.max_step_update_value):
            self.num_update_value += 1
            # sample(): one bare step under the target's raw pair, then the reset select
            obs = self._obs
            pair = nets.action_and_adversary(obs)
            next_obs, _, self.done, info = model.step(pair)
            reset = self.done | info["TimeLimit.truncated"]
            self._obs = torch.where(reset.unsqueeze(-1), self.reset_source.next(), next_obs)
            model.parallel_state = self._obs.clone()
            self.env_model.step_per_episode = torch.where(reset, model.initial_step(), self.env_model.step_per_episode)
            # loss, gradient and Adam step at the pre-step states
            h, dh_dw = self._hamiltonian_rows(weight, obs, pair)
            loss = float(h.abs().mean())
            ratios.append(float(h.abs().min()) / loss)
            self._adam_step(weight, (torch.sign(h).unsqueeze(1) * dh_dw).mean(0))
            self.norm_hamiltonian_after = float(self._hamiltonian_rows(weight, self.set_state, set_pair)[0].abs().mean())
            trace.append((loss, self.norm_hamiltonian_after))
            weights.append(weight.clone())
            if not self.continue_evaluation():
                break
        self.trace, self.weight_trace = torch.tensor(trace, dtype=torch.float32), torch.stack(weights)
        self.min_row_ratio = min(ratios)   # smallest |h_i| / mean|h| of a loss row: how far every sign(h_i) is from flipping
        return loss

    def _hamiltonian_mlp(self, obs, pair):
        """h [B] of the VALUE net at `obs` for the action / adversary `pair` (wrapped inside `forward`), differentiable in the
        net's parameters: dV/dx by autograd with the graph kept."""
        with torch.no_grad():
            _, reward, _, info = self.env_model.forward(obs, pair, torch.zeros(obs.shape[0], dtype=torch.bool), {})
        x = obs.detach().clone().requires_grad_(True)
        (dv,) = torch.autograd.grad(self.networks.value(x).sum(), x, create_graph=True)
        return -reward + (dv * info["delta_state"]).sum(1)

    def _adam_step_mlp(self, params, grads):
        """torch.optim.Adam's single-tensor step per parameter; a parameter without a gradient (the output bias) is skipped."""
        st, (beta1, beta2) = self._adam, ADAM_BETAS
        st["step"] += 1
        step_size = self.learning_rate / (1 - beta1 ** st["step"])
        bc2_sqrt = (1 - beta2 ** st["step"]) ** 0.5
        o = 0
        for q, grad in zip(params, grads):
            n = q.numel()
            if grad is not None:
                m, v, grad = st["exp_avg"][o:o + n], st["exp_avg_sq"][o:o + n], grad.reshape(-1)
                m.lerp_(grad, 1 - beta1)
                v.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                q.data.view(-1).addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(ADAM_EPS), value=-step_size)
            o += n

    def _evaluate_host_mlp(self):
        nets, model = self.networks, self.env_model.unwrapped
        params = list(nets.value.parameters())
        self.set_state = self.reset_source.next()
        set_pair = nets.action_and_adversary(self.set_state)
        norm = lambda: float(self._hamiltonian_mlp(self.set_state, set_pair).detach().abs().mean())  # noqa: E731
        self.norm_hamiltonian_before = norm()
        loss, trace, weights, ratios = 0.0, [], [], []
        for _ in range(self.max_step_update_value):
            self.num_update_value += 1
            # sample(): one bare step under the target's raw pair, then the reset select
            obs = self._obs
            pair = nets.action_and_adversary(obs)
            with torch.no_grad():
                next_obs, _, self.done, info = model.step(pair)
                reset = self.done | info["TimeLimit.truncated"]
                self._obs = torch.where(reset.unsqueeze(-1), self.reset_source.next(), next_obs)
                model.parallel_state = self._obs.clone()
                self.env_model.step_per_episode = torch.where(reset, model.initial_step(), self.env_model.step_per_episode)
            # loss, gradient (the double backward) and Adam step at the pre-step states
            h = self._hamiltonian_mlp(obs, pair)
            loss_t = h.abs().mean()
            grads = torch.autograd.grad(loss_t, params, allow_unused=True)
            loss = float(loss_t.detach())
            ratios.append(float(h.detach().abs().min()) / loss)
            with torch.no_grad():
                self._adam_step_mlp(params, grads)
            self.norm_hamiltonian_after = norm()
            trace.append((loss, self.norm_hamiltonian_after))
            weights.append(torch.cat([q.detach().reshape(-1) for q in params]))
            if not self.continue_evaluation():
                break
        self.trace, self.weight_trace = torch.tensor(trace, dtype=torch.float32), torch.stack(weights)
        self.min_row_ratio = min(ratios)
        return loss

    # ---- the device path ------------------------------------------------------------------------------------------------------
    def _device_evaluator(self):
        if self._evaluator is None:
            from gops_amd import hip_backend as hb
            model, dev = self.env_model.unwrapped, next(self.networks.parameters()).device
            consts = self.env_model.rpi_constants()
            if self.is_mlp:
                ev = hb.RpiMlpEvaluator(model.rpi_kind, model.sample_batch_size, model.state_dim, consts, self.networks.value.hip_mlp(),
                                        self.networks.value_target.hip_mlp(), dev)
            else:
                norm = self.networks.value.norm_matrix.cpu().numpy()
                consts[hb.RPI_C_NORM:hb.RPI_C_NORM + len(norm)] = norm
                ev = hb.RpiEvaluator(model.rpi_kind, model.sample_batch_size, model.state_dim, consts, dev)
            ev.lanes().copy_(self._obs.t())
            count = model.step_per_episode.to(dev)
            shown = self.env_model.__dict__.get("step_per_episode")   # assigned on the wrapper yet? (a host-path run before)
            ev.counters().copy_(torch.stack([count, torch.full_like(count, -1.0) if shown is None else shown.to(dev)]))
            if self.is_mlp:
                ev.moments().copy_(torch.stack([self._adam["exp_avg"], self._adam["exp_avg_sq"]]))
                ev.state[0] = float(self._adam["step"])
            else:
                n_feat = self._adam["exp_avg"].numel()
                ev.state[:n_feat] = self._adam["exp_avg"].to(dev)
                ev.state[10:10 + n_feat] = self._adam["exp_avg_sq"].to(dev)
                ev.state[20] = float(self._adam["step"])
            self._max_step_dev = model.max_step_per_episode.to(device=dev, dtype=torch.float32)
            self._evaluator = ev
        return self._evaluator

    def _evaluate_device(self):
        ev = self._device_evaluator()
        n = self.max_step_update_value
        pool = self.reset_source.pool(n + 1)                 # [n + 1, S, B] on the host: coalesced over lanes as it stands
        pool_dev = pool.to(ev.device)
        self.set_state = pool[0].t().contiguous()
        trace = torch.zeros(n, 2, dtype=torch.float32, device=ev.device) if self.record_trace else None
        if self.is_mlp:   # (the nets' weights travel as the pointers of the evaluator's two GopsMlp records)
            result = ev.evaluate(self._max_step_dev, pool_dev, n, self.learning_rate, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, trace)
        else:
            weight, target = self.networks.value.v.weight.data, self.networks.value_target.v.weight.data
            result = ev.evaluate(weight.view(-1), target.view(-1), self._max_step_dev, pool_dev, n, self.learning_rate,
                                 ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, trace)
        steps, loss, before, after = result.tolist()                           # the one host sync of this local_update
        self.num_update_value = int(steps)
        self.norm_hamiltonian_before, self.norm_hamiltonian_after = before, after
        self.reset_source.consume(self.num_update_value + 1)
        self.trace = None if trace is None else trace[:self.num_update_value]
        return loss

    # ---- the update API -------------------------------------------------------------------------------------------------------
    def local_update(self, data_ignored, iteration):
        self.num_update_value = 0
        start_time = time.time()
        loss = self._evaluate_device() if self.use_gpu else self._evaluate_host_mlp() if self.is_mlp else self._evaluate_host()
        self.networks.value_target.load_state_dict(self.networks.value.state_dict())
        end_time = time.time()
        grad_info = dict()
        grad_info["iteration"] = iteration
        grad_info["num_update_value"] = self.num_update_value
        grad_info[tb_tags["loss_critic"]] = loss
        grad_info[tb_tags["alg_time"]] = (end_time - start_time) * 1000  # ms
        if iteration % self.print_interval == 0:
            if iteration < len(self.grad_step):
                self.grad_step[iteration, 0] = self.num_update_value
            print(f"Newton ite: {iteration}, grad step = {self.num_update_value:d}")
        return grad_info
