"""BatchOptController - shooting MPC for MANY states at once, solved on the device.

`OptController` (opt_controller.py) solves one state per call inside scipy's L-BFGS-B: every cost evaluation is a batch-1 rollout
launch followed by a device-to-host copy of the cost and of the Jacobian.  Here B states are B rows of ONE open-loop rollout, and
the solver itself lives on the device (`hb.MpcSolver`: `gops_mpc_init / _step / _finish`, csrc/mpc_lbfgs.hip), so one iteration of
all B problems is four calls and no host read:

    1. Rollout.forward(head_pre = the trial actions)                 cost   = - v_pi (+ gamma^T terminal_cost(state_T))
    2. backward_open_loop (backward_open_loop_adj with a terminal cost)   d cost / d action [B, T, A]
    3. the fold of that gradient over each control interval               [B, n],  n = num_ctrl_points * act_dim
    4. MpcSolver.step                                                     Armijo test, (s, y) pair, convergence tests, next trial

The host reads the B status words once every `check_every` iterations (one synchronisation) and stops when no problem is running
or after `max_iter` cost evaluations.  Between two reads a row that has finished is still part of the rollout (at its accepted
point, which the step kernel keeps writing into its trial row) but is no longer moved.  The raw env description is `OptController`'s (identity action scaling, no observation clip,
`no_mask_at_done`), the box is the model's action bounds, and the warm start across calls is its shift: drop the first control
point, repeat the last - per row.

`run_episodes` drives the controller in closed loop for B episodes at once: between two solves the plan is handed over on the
device (`MpcSolver.advance`, gops_mpc_advance: first action out, plan shifted, block re-initialised - one launch), the env model is
stepped with the action held, and rows whose episode has ended are frozen; the status polls stay the only host reads.

Path constraints (`model.get_constraint`; pyth_veh3dofconti_surrcstr / _detour / _errcstr, pyth_veh2dofconti_errcstr) are opt-in:
`path_constraints="augmented_lagrangian"` wraps the L-BFGS in an augmented-Lagrangian outer loop that also lives on the device
(`gops_mpc_al_eval / _update / _advance`).  One inner iteration is then forward with the per-step constraint values,
`MpcSolver.al_eval` (objective, seed, violation), ONE backward seeded with `grad_v = -1` and `grad_constraint_step = seed`, the fold
and `MpcSolver.step`; every `check_every` evaluations one more forward puts the constraint values of the accepted points in place
and `MpcSolver.al_update` moves the multipliers of the rows whose inner solve has ended and re-arms them, before the one status poll.
The errcstr models emit c(obs_t) at step t, so c(obs_T) needs one padded step: it comes from a SECOND rollout of T + 1 steps, as in
`OptController._cstr_actions`, which contributes the constraint values and their gradient only - the cost and its gradient stay
those of the T-step rollout, bit for bit.  The initial state's constraint has no Jacobian: it is evaluated once
(`hb.env_constraint`), reported, and takes no part in the penalty.

Scope: shooting mode.  Without the keyword a model with path constraints is refused at construction, as before; with it
pyth_veh3dofconti_surrcstr_penalty stays refused (its constraint carries no gradient).  Collocation, fp16 and graph capture of the
loop are not provided.  What the solver does differently from scipy's L-BFGS-B - projected Armijo
backtracking instead of the Cauchy point, subspace minimisation and the More-Thuente search; tolerances held in fp32 - is in
include/gops_hip.h and DESIGN.md.
"""
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from gops_amd import hip_backend as hb
from gops_amd.sys_simulator.opt_controller import _INFO, _STATE_OBS_KINDS


class BatchOptController:
    def __init__(self, model, num_pred_step: int, ctrl_interval: int = 1, gamma: float = 1.0, use_terminal_cost: bool = False,
                 terminal_cost=None, max_iter: int = 500, pgtol: float = hb.MPC_HYPER_DEFAULTS["pgtol"],
                 ftol: float = hb.MPC_HYPER_DEFAULTS["ftol"], history: int = hb.MPC_MAX_HISTORY, check_every: int = 8, device=None,
                 path_constraints: Optional[str] = None, al_hyper: Optional[Dict] = None):
        """`max_iter`: the largest number of cost EVALUATIONS (rollout forward + backward of all rows) of one solve - every
        backtracking trial counts, unlike scipy's `maxiter` / OptController's, which count accepted iterations.  `pgtol`, `ftol`:
        the stopping tolerances of gops_mpc_step (scipy's L-BFGS-B defaults), held in fp32.  `check_every`: cost evaluations between
        two host reads of the status words.  `path_constraints`: None (a model with get_constraint is refused) or
        "augmented_lagrangian"; `al_hyper`: rho0, growth, rho_max, shrink_target, cstr_tol, max_outer, lambda_tol
        (hb.MPC_AL_HYPER_DEFAULTS for the ones not given)."""
        assert num_pred_step % ctrl_interval == 0, "ctrl_interval should be a factor of num_pred_step."
        base = model.unwrapped
        self.model, self.base = model, base
        self.terminal_cost = None
        if use_terminal_cost:
            self.terminal_cost = terminal_cost if terminal_cost is not None else getattr(model, "get_terminal_cost", None)
            assert self.terminal_cost is not None, "Choose to use terminal cost, but there is no available terminal cost function."
            if base.hip_kind not in _STATE_OBS_KINDS:
                raise NotImplementedError("a terminal cost needs the adjoint of the final observation, which the kernels provide for "
                                          "the models whose observation is the state")
        elif terminal_cost is not None:
            warnings.warn("Choose not to use terminal cost, but a terminal cost function is given. This will be ignored.")
        self.obs_dim, self.action_dim, self.sim_dt = base.obs_dim, base.action_dim, base.dt
        self.gamma, self.ctrl_interval, self.num_pred_step = gamma, ctrl_interval, num_pred_step
        self.num_ctrl_points = num_pred_step // ctrl_interval
        self.n = self.num_ctrl_points * self.action_dim
        self.max_iter, self.check_every, self.history = int(max_iter), int(check_every), int(history)
        self.hyper = dict(pgtol=float(pgtol), ftol=float(ftol))
        # the RAW model, exactly as OptController describes it
        env = hb.make_env(base.hip_kind, base.obs_dim, base.action_dim, act_low=base.action_lower_bound.cpu(),
                          act_high=base.action_upper_bound.cpu(), min_action=base.action_lower_bound.cpu(),
                          max_action=base.action_upper_bound.cpu(), pre_horizon=getattr(base, "pre_horizon", 0),
                          **base.hip_constants())
        env.no_mask_at_done = 1
        self._env = env
        self.path_constraints, self.al_hyper = path_constraints, dict(al_hyper or {})
        self._al = False
        self._refuse()
        if path_constraints is not None:
            unknown = set(self.al_hyper) - set(hb.MPC_AL_HYPER_DEFAULTS)
            if unknown:
                raise ValueError(f"BatchOptController: unknown al_hyper {sorted(unknown)}")
            self._al, self._nc, self._cstr_err = True, int(env.n_constraint), bool(env.cstr_err)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._lo = base.action_lower_bound.cpu().to(torch.float32).repeat(self.num_ctrl_points)
        self._hi = base.action_upper_bound.cpu().to(torch.float32).repeat(self.num_ctrl_points)
        self._per_batch: Dict[int, Dict] = {}
        self._terminal_vmap = True
        self._guess: Optional[torch.Tensor] = None
        self.last_result: Optional[Dict] = None
        self.last_episodes: Optional[Dict] = None
        self._data_env = None

    def _refuse(self):
        """What the batched solver does not handle, said at construction and again by `run_episodes`."""
        base = self.base
        constrained = getattr(base, "get_constraint", None) is not None and hb.has_constraints(self._env)
        if self.path_constraints is not None:
            if self.path_constraints != "augmented_lagrangian":
                raise ValueError(f"BatchOptController: path_constraints={self.path_constraints!r}; None or 'augmented_lagrangian'")
            if not constrained:
                raise ValueError(f"BatchOptController: path_constraints given, but {type(base).__name__} defines no get_constraint")
            if self._env.surr_penalty:
                raise NotImplementedError("BatchOptController: the constraint of pyth_veh3dofconti_surrcstr_penalty carries no gradient "
                                          "(the model computes it on detached copies): no multiplier method can act on it")
        elif constrained:
            raise NotImplementedError(f"BatchOptController: {type(base).__name__} has path constraints (get_constraint); the batched "
                                      "solver handles box constraints only by default - pass path_constraints='augmented_lagrangian', or use "
                                      "OptController(mode='shooting') for it")
        if not 1 <= self.n <= hb.MPC_MAX_DIM:
            raise NotImplementedError(f"BatchOptController: {self.n} decision variables per state; the device solver takes 1 .. {hb.MPC_MAX_DIM}")

    def reset(self):
        """Forget the warm start and the last episodes: the next call starts every row from zero actions."""
        self._guess = None
        self.last_episodes = None

    def _objects(self, B: int) -> Dict:
        o = self._per_batch.get(B)
        if o is None:
            T, A, dev = self.num_pred_step, self.action_dim, self.device
            o = dict(rollout=hb.Rollout(self._env, None, batch=B, horizon=T, gamma=self.gamma, finite_horizon=False, need_grad=True,
                                        device=dev, raw_actions=True),
                     solver=hb.MpcSolver(B, self.n, self._lo, self._hi, dev, history=self.history,
                                         constraints=(T, self._nc) if self._al else None),
                     actions=torch.zeros(B, T, A, dtype=torch.float32, device=dev),
                     minus_one=torch.full((B,), -1.0, dtype=torch.float32, device=dev),
                     done=torch.zeros(B, dtype=torch.float32, device=dev))
            if self.base.hip_kind == hb.ENV_MOBILEROBOT:   # a deterministic cost: the obstacle follows its expected motion
                o["noise"] = torch.zeros(T, B, 2, dtype=torch.float32, device=dev)
            o["solver"].set_hyper(**self.hyper)
            if self._al:
                o["solver"].set_al_hyper(**self.al_hyper)
                o["zero"] = torch.zeros(B, dtype=torch.float32, device=dev)
                if self._cstr_err:   # c(obs_T) needs one padded step: the constraint side runs on a rollout of its own
                    o["crollout"] = hb.Rollout(self._env, None, batch=B, horizon=T + 1, gamma=self.gamma, finite_horizon=False,
                                               need_grad=True, device=dev, raw_actions=True)
                    o["cactions"] = torch.zeros(B, T + 1, A, dtype=torch.float32, device=dev)
                    o["cseed"] = torch.zeros(T + 1, B, self._nc, dtype=torch.float32, device=dev)   # row 0 (the initial state) stays 0
            self._per_batch[B] = o
        return o

    def _data(self, o: Dict, x, info: Optional[Dict]) -> Dict:
        as_dev = lambda v: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32, device=self.device).contiguous()
        data = {"obs": as_dev(x), "done": o["done"]}
        if "noise" in o:
            data["noise"] = o["noise"]
        for k in _INFO:
            if info and k in info:
                data[k] = as_dev(info[k])
        return data

    def _terminal(self, final_obs: torch.Tensor):
        """(gamma^T terminal_cost(state_T) [B], its gradient [B, obs_dim]) with autograd on the device.  The function is written for
        ONE state (opt_controller.py:312-317; pyth_lq's x'Px): it is mapped over the rows with torch.func.vmap - one host call per
        cost evaluation whatever B is - and only a function vmap cannot trace (data-dependent branches, .item()) is called row by
        row, B host calls per evaluation."""
        xT = final_obs.detach().clone().requires_grad_(True)
        if self._terminal_vmap:
            try:
                tc = torch.func.vmap(self.terminal_cost)(xT)
            except Exception:   # not traceable: the same values, row by row
                self._terminal_vmap = False
        if not self._terminal_vmap:
            tc = torch.stack([self.terminal_cost(xT[b]) for b in range(xT.shape[0])])
        tc = tc.reshape(-1) * (self.gamma ** self.num_pred_step)
        (g,) = torch.autograd.grad(tc.sum(), xT)
        return tc.detach().to(torch.float32), g.to(torch.float32).contiguous()

    def _evaluate(self, o: Dict, data: Dict):
        """Cost and gradient of every row at the solver's trial point, left in solver.f / solver.g."""
        B, n_cp, ci, A = o["actions"].shape[0], self.num_ctrl_points, self.ctrl_interval, self.action_dim
        solver, ro = o["solver"], o["rollout"]
        o["actions"].view(B, n_cp, ci, A).copy_(solver.x_trial.view(B, n_cp, 1, A).expand(B, n_cp, ci, A))   # held over each interval
        res = ro.forward(data, head_pre=o["actions"], want_final=self.terminal_cost is not None)
        torch.neg(res["v_pi"], out=solver.f)
        if self.terminal_cost is not None:
            tc, gfo = self._terminal(res["final_obs"])
            solver.f.add_(tc)
            g, _ = ro.backward_open_loop_adj(o["minus_one"], grad_final_obs=gfo)
        else:
            g = ro.backward_open_loop(o["minus_one"])
        g = g.view(B, n_cp, ci, A)
        out = solver.g.view(B, n_cp, A)
        out.copy_(g[:, :, 0])
        for k in range(1, ci):   # the fold, one interval step at a time: element-wise, so a row's bits do not depend on B
            out.add_(g[:, :, k])

    def _evaluate_al(self, o: Dict, data: Dict, backward: bool = True):
        """The augmented Lagrangian and its gradient of every row at the solver's trial point, left in solver.f / solver.g; the
        rollout cost in solver.f_al_in, the constraint values [T, B, n_c] in o["c"].  `backward=False`: values only."""
        B, n_cp, ci, A, T = o["actions"].shape[0], self.num_ctrl_points, self.ctrl_interval, self.action_dim, self.num_pred_step
        solver, ro = o["solver"], o["rollout"]
        o["actions"].view(B, n_cp, ci, A).copy_(solver.x_trial.view(B, n_cp, 1, A).expand(B, n_cp, ci, A))
        if not self._cstr_err:   # the step kernels emit c(state_{t+1}) at step t: one rollout gives cost and constraints
            res = ro.forward(data, head_pre=o["actions"], want_constraints=True)
            torch.neg(res["v_pi"], out=solver.f_al_in)
            o["c"] = res["constraints"]
            solver.al_eval(o["c"])
            if not backward:
                return
            g = ro.backward_open_loop(o["minus_one"], grad_constraint_step=solver.seed)
        else:
            res = ro.forward(data, head_pre=o["actions"])
            torch.neg(res["v_pi"], out=solver.f_al_in)
            o["cactions"][:, :T].copy_(o["actions"])
            o["cactions"][:, T].copy_(o["actions"][:, T - 1])
            cro = o["crollout"]
            o["c"] = cro.forward(data, head_pre=o["cactions"], want_constraints=True)["constraints"][1:]   # c(obs_1 .. obs_T)
            solver.al_eval(o["c"])
            if not backward:
                return
            g = ro.backward_open_loop(o["minus_one"])
            o["cseed"][1:].copy_(solver.seed)
            g = g + cro.backward_open_loop(o["zero"], grad_constraint_step=o["cseed"])[:, :T]   # (the padded action moves no emitted value)
        g = g.view(B, n_cp, ci, A)
        out = solver.g.view(B, n_cp, A)
        out.copy_(g[:, :, 0])
        for k in range(1, ci):
            out.add_(g[:, :, k])

    def _iterate_al(self, o: Dict, data: Dict) -> int:
        """`_iterate` with the outer loop: every `check_every` evaluations one forward at the points the step kernel left in x_trial
        (the accepted point of every row whose inner solve has ended), `al_update`, and the one poll."""
        solver, evals = o["solver"], 0
        while evals < self.max_iter:
            for _ in range(min(self.check_every, self.max_iter - evals)):
                self._evaluate_al(o, data)
                solver.step()
                evals += 1
            self._evaluate_al(o, data, backward=False)
            solver.al_update(o["c"])
            status, outer = solver.finish()[2], solver.outer[:, 0]
            live = (outer == hb.MPC_AL_RUNNING) & (status != hb.MPC_NONFINITE) & (status != hb.MPC_FROZEN)
            if not bool(live.any().item()):   # the one synchronisation per check_every iterations
                break
        return evals

    def _iterate(self, o: Dict, data: Dict) -> int:
        """Evaluate / step from the initialised block until no row is running or `max_iter`; -> the cost evaluations made."""
        if self._al:
            return self._iterate_al(o, data)
        solver, evals = o["solver"], 0
        while evals < self.max_iter:
            for _ in range(min(self.check_every, self.max_iter - evals)):
                self._evaluate(o, data)
                solver.step()
                evals += 1
            plan, cost, status, iterations = solver.finish()
            if not bool((status == hb.MPC_RUNNING).any().item()):   # the one synchronisation per check_every iterations
                break
        return evals

    def solve(self, x, info: Optional[Dict] = None) -> Dict:
        """-> dict(action [B, act_dim], plan [B, num_ctrl_points, act_dim], cost [B], status [B] (hb.MPC_*), iterations [B],
        evaluations: cost evaluations made) for the states x [B, obs_dim]; tensors on the device."""
        x = np.asarray(x) if not torch.is_tensor(x) else x
        assert x.ndim == 2 and x.shape[1] == self.obs_dim, "x: [B, obs_dim]"
        B = int(x.shape[0])
        o = self._objects(B)
        solver = o["solver"]
        data = self._data(o, x, info)
        guess = self._guess if self._guess is not None and self._guess.shape[0] == B else torch.zeros(B, self.n, dtype=torch.float32,
                                                                                                      device=self.device)
        solver.init(guess)
        if self._al:
            solver.al_reset()
        evals = self._iterate(o, data)
        plan, cost, status, iterations = (t.clone() for t in solver.finish()[:4])
        A = self.action_dim
        self._guess = torch.cat((plan[:, A:], plan[:, -A:]), 1).contiguous()   # drop the first control point, repeat the last
        plan = plan.view(B, self.num_ctrl_points, A)
        self.last_result = dict(action=plan[:, 0].clone(), plan=plan, cost=cost, status=status, iterations=iterations, evaluations=evals)
        if self._al:   # cost: the ROLLOUT cost of the last forward (the accepted point of every row whose inner solve has ended)
            c0 = hb.env_constraint(self._env, data["obs"], {k: data[k] for k in ("state", "surr_state") if k in data})
            self.last_result.update(cost=solver.f_al_in.clone(), constraint_violation=solver.viol.clone(), outer_status=solver.outer[:, 0].clone(),
                                    outer_iterations=solver.outer[:, 1].clone(), multipliers=solver.lam.clone(), initial_constraint=c0)
        return self.last_result

    def __call__(self, x, info: Optional[Dict] = None) -> torch.Tensor:
        """The first optimal action of every row [B, act_dim]."""
        return self.solve(x, info)["action"]

    def _step_env(self, env_step: str):
        """The env constants the closed loop is advanced with: "model" - the raw model the plan is optimised on; "data" - the data
        environment's step (its termination tests and terminal penalty) where the step kernel has it restated."""
        if env_step == "model":
            return self._env
        if env_step != "data":
            raise ValueError("env_step must be 'model' (the env model's step) or 'data' (the data environment's)")
        base = self.base
        if base.hip_kind not in hb.DATA_ENV_KINDS:
            from gops_amd.trainer.sampler.reset_pool import NOT_RESTATED
            raise NotImplementedError(NOT_RESTATED.format(env_id=type(base).__name__))
        if self._data_env is None:
            lo, hi = base.action_lower_bound.cpu(), base.action_upper_bound.cpu()
            self._data_env = hb.make_env(base.hip_kind, base.obs_dim, base.action_dim, act_low=lo, act_high=hi, min_action=lo, max_action=hi,
                                         obs_low=base.obs_lower_bound.cpu(), obs_high=base.obs_upper_bound.cpu(),
                                         pre_horizon=getattr(base, "pre_horizon", 0), data_env=True, ref_c=getattr(base, "ref_c", None),
                                         **base.hip_constants())
        return self._data_env

    def run_episodes(self, x0, steps: int, info: Optional[Dict] = None, env_step: str = "model") -> Dict:
        """B closed-loop episodes of `steps` control steps from the states x0 [B, obs_dim], the plan handed from one solve to the next
        on the device (`MpcSolver.advance`): per control step the evaluate / step loop of `solve`, one hand-over launch (first action
        out, plan shifted by one control point, block re-initialised), `ctrl_interval` env steps with the action held, and the books
        kept by element-wise device operations.  The host reads the status words as `solve` does and nothing else.  A row whose step
        reports done is frozen: its state is held, its later actions are 0, its return and length stop, its status reads
        hb.MPC_FROZEN and it is not solved again.  With path constraints the hand-over is `MpcSolver.al_advance` (multipliers shifted by
        one control interval, rho back to rho0) and the result gains max_constraint [B]: the largest info["constraint"] value the env
        steps of the episode reported while the row was live.  -> dict(return [B], length [B] (env steps), done [B] bool,
        actions [steps, B, act_dim], obs [steps + 1, B, obs_dim], status [steps, B] int32 (hb.MPC_*), record [B, 4] int32 (last
        status, summed iterations, summed evaluations, solves), evaluations: cost evaluations made); tensors on the device."""
        self._refuse()
        step_env = self._step_env(env_step)
        x0 = np.asarray(x0) if not torch.is_tensor(x0) else x0
        assert x0.ndim == 2 and x0.shape[1] == self.obs_dim, "x0: [B, obs_dim]"
        B, A, dev, steps = int(x0.shape[0]), self.action_dim, self.device, int(steps)
        o = self._objects(B)
        solver = o["solver"]
        data = self._data(o, x0, info)
        obs = data["obs"].clone()
        step_info = {k: v for k, v in data.items() if k not in ("obs", "done", "noise")}
        if self.base.hip_kind == hb.ENV_MOBILEROBOT:   # the obstacle follows its expected motion, as in the plan's rollout
            step_info["noise"] = torch.zeros(B, 2, dtype=torch.float32, device=dev)
        zeros = torch.zeros(B, dtype=torch.float32, device=dev)
        frozen, ret, length = zeros.clone(), zeros.clone(), zeros.clone()
        record = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        actions = torch.zeros(steps, B, A, dtype=torch.float32, device=dev)
        obs_out = torch.zeros(steps + 1, B, self.obs_dim, dtype=torch.float32, device=dev)
        status = torch.zeros(steps, B, dtype=torch.int32, device=dev)
        obs_out[0].copy_(obs)
        solver.init(torch.zeros(B, self.n, dtype=torch.float32, device=dev))
        if self._al:
            solver.al_reset()
        max_c = torch.full((B,), float("-inf"), dtype=torch.float32, device=dev)
        evals = 0
        for k in range(steps):
            data["obs"] = obs
            data.update({key: v for key, v in step_info.items() if key != "noise"})
            evals += self._iterate(o, data)
            if self._al:
                solver.al_advance(frozen, actions[k], record, shift=self.ctrl_interval)
            else:
                solver.advance(frozen, actions[k], record)
            status[k].copy_(record[:, 0])
            for _ in range(self.ctrl_interval):
                obs2, rew, done, info2 = hb.env_step(step_env, obs, actions[k], zeros, step_info)
                live = 1.0 - frozen
                ret = ret + rew * live
                length = length + live
                held = frozen != 0
                if self._al:
                    max_c = torch.where(held, max_c, torch.maximum(max_c, info2["constraint"].max(1).values))
                obs = torch.where(held.unsqueeze(1), obs, obs2)
                for key, v in info2.items():
                    if key in step_info and v is not step_info[key]:
                        step_info[key] = torch.where(held.view(-1, *[1] * (v.dim() - 1)), step_info[key], v)
                frozen = torch.maximum(frozen, (done != 0).to(torch.float32))
            solver.status_words().masked_fill_(frozen != 0, hb.MPC_FROZEN)   # the rows this step ended are not solved again
            obs_out[k + 1].copy_(obs)
        self._guess = None   # (the block holds the next warm start; solve() starts from its own)
        self.last_episodes = {"return": ret, "length": length, "done": frozen != 0, "actions": actions, "obs": obs_out, "status": status,
                              "record": record, "evaluations": evals}
        if self._al:
            self.last_episodes["max_constraint"] = max_c
        return self.last_episodes
