"""optimizer_gradient / optimizer_rpgd — the gradient-based optimizers over the adjoint of the rollout + cost kernel
(SURVEY.md §8f N4).

Constructor keywords = the keys of ``Control_Toolkit_ASF/config_optimizers.yml:49-62`` (section ``gradient-tf``) and
``:63-86`` (section ``rpgd``).  The classes themselves live in the absent Control_Toolkit submodule (TensorFlow
GradientTape through predictor + cost function, Keras Adam); their behaviour here is the one those keys name and is NOT
pinned by anything in-tree ([recalled] in SURVEY.md Appendix B terms):

* both keep ``num_rollouts`` candidate input plans per env and improve ALL of them in parallel with Adam on
  d cost / d inputs (cpmppi_rollout_cost_grad + cpmppi_adam_step: per-plan gradient-norm clipping to ``gradmax_clip``,
  clip to the control limits), then apply the first input of the cheapest plan and shift every plan;
* ``gradient``: ``gradient_steps`` iterations per control step, plans initialised from N(0, ``initial_action_stdev``);
* ``rpgd`` (resampling parallel gradient descent): ``outer_its`` iterations per control step; every ``resamp_per``
  control steps only the best ``opt_keep_k_ratio`` of the plans survive (with their Adam moments), the others are
  re-drawn from the sampling distribution (``SAMPLING_DISTRIBUTION`` normal(``sample_mean``, ``sample_stdev``) or
  uniform, one random point every ``period_interpolation_inducing_points`` steps, linear in between);
  plans are shifted by ``shift_previous``.

Everything that scales with rollouts x horizon runs in HIP kernels (sampling, forward + reverse sweep, Adam, top-k);
torch is used for the per-plan bookkeeping (gather of survivors, shift).  ``num_envs`` problem instances advance in one
launch.

``fused=True`` (off by default) makes the whole control step ONE library call, cpmppi_rpgd_step: iterations, final cost,
choice of the best plan, resampling and shift in one kernel, the plans and moments updated in place.  ``step`` then only
uploads the state; ``step_device`` takes device tensors and, with a device step counter, touches the host not at all - the
form a captured closed loop replays (harness.py).  The staged path above stays what it was.

``gru_adjoint=True`` (off by default) lets both run on the neural predictor (``gru_model=`` and / or a
``GRU-6IN-32H1-32H2-5OUT*`` ``predictor_specification``, under optimizer_mppi's rules): every gradient launch of a control step is
cpmppi_rollout_cost_grad_gru and every cost launch cpmppi_rollout_cost_gru, from each env's memory ``h`` [E,2,32], which is zero
after a reset and advances once per control step with the state seen and the control applied.  Without the flag the network is
refused by name, as before; with it, ``fused=True`` (cpmppi_rpgd_step integrates the ODE) and quadratic_boundary_grad (no such
cost in the GRU kernels) are.

``gru_fused=True`` (off by default; needs the network) is the fused step over the network: ONE cpmppi_rpgd_step_gru per control
step - every iteration's forward sweep from each env's memory, reverse sweep and Adam row, then the final costs, the ranking, the
resampling and the shift in one kernel, what the staged ``gru_adjoint=True`` step computes - followed by cpmppi_gru_advance, which
moves the memory on in place with the state seen and the control chosen.  The flag is itself the opt-in to the adjoint
(``gru_adjoint=True`` beside it changes nothing) and makes the object a fused one (``fused`` is true, ``step_device``, a device
step counter): the closed loop of the shipped controller over a learned model launches, or replays as a captured graph, like
the fused ODE step's (harness.py).  At most 128 plans per env; quadratic_boundary_grad is refused as under ``gru_adjoint=True``.

``rows=`` (with ``fused=True``; ``configs.rpgd_rows`` packs them) gives every env its OWN controller setting: a float32 array
[num_envs, 16] holding, per env, quadratic_boundary_grad_minimal's seven cost weights, Adam's learning rate and the gradient clip.
The fused step is then cpmppi_rpgd_step_rows, and the constructor's ``learning_rate`` and ``gradmax_clip`` (and the cost weights of
the handle) are unused for the step.  The rows live on as the device tensor ``self.rows``, which every launch and every replay of a
captured loop reads when it runs: rewrite it in place to change the settings.  They travel inside the object, so ``capture()``,
``run_schedule(optimizer=...)``, ``generate_dataset(optimizer=...)`` and ``along_trajectories`` take it as any fused optimizer.
The sampling width stays one value per optimizer (``sample_stdev`` / ``initial_action_stdev``): the plans are drawn with the
handle's.  Refused by name: ``rows`` with the staged step (its launches read the handle's scalars), with the network
(``gru_model`` / ``gru_fused``), in another shape, or with another cost.
"""
import math

import torch

from ._lib import TUNING_ROW_FLOATS
from ._optimizer_base import _OptimizerBase, is_gru_specification
from .optimizer_cem import GRU_FUSED_NEEDS_MODEL

ROWS_NEED_FUSED = ("rows= needs fused=True: the staged step's launches (cpmppi_rollout_cost_grad, cpmppi_adam_step) read the handle's "
                   "scalars; the fused step reads a row per env (cpmppi_rpgd_step_rows)")
ROWS_OR_GRU = ("rows= with gru_model / gru_fused: the fused step over the network (cpmppi_rpgd_step_gru) reads no rows; per-env rows "
               "are built for the ODE predictors")
GRU_FUSED_OR_FUSED = ("gru_fused=True and fused=True: fused=True is the step that integrates the ODE (cpmppi_rpgd_step), gru_fused=True "
                      "the one over the network (cpmppi_rpgd_step_gru): give one of them")


class _GradientBase(_OptimizerBase):
    optimizer_name = "gradient"
    _unknown_predictor = "the adjoint kernel differentiates the ODE_v0 and ODE predictors"
    _gru_refusal = ("the gradient optimizers (gradient, rpgd) need the gradient of the cost and run on the ODE_v0 and ODE predictors "
                    "by default (the fused step has no adjoint kernel for the GRU predictor): pass gru_adjoint=True to differentiate "
                    "through the network in the staged step (cpmppi_rollout_cost_grad_gru); cem, cem-gmm and random-action run "
                    "on the GRU without it")

    def __init__(self, cost_function, control_limits, seed, mpc_horizon, mpc_timestep, num_rollouts, sample_stdev, period,
                 num_envs, cost_function_specification, cost_weights, intermediate_steps, phys, device,
                 variable_parameters, optimizer_logging, horizon_reduce, per_env_pole_mass, fused=False, gru_model=None,
                 gru_adjoint=False, gru_fused=False, rows=None):
        if gru_fused and fused:
            raise ValueError(GRU_FUSED_OR_FUSED)
        if rows is not None and (gru_model is not None or gru_fused):
            raise ValueError(ROWS_OR_GRU)
        if rows is not None and not fused:
            raise ValueError(ROWS_NEED_FUSED)
        # the handle's sampler draws knots ~ N(0, SQRTRHOINV / sqrt(dt)): set it to the requested stdev
        super().__init__(cost_function, control_limits, seed, num_envs, cost_function_specification, cost_weights,
                         variable_parameters, phys, device, optimizer_logging, mpc_horizon, mpc_timestep, num_rollouts,
                         intermediate_steps, control_mode="clip", shift_mode="none", math_mode="fast",
                         horizon_reduce=horizon_reduce, SQRTRHOINV=float(sample_stdev) * math.sqrt(float(mpc_timestep)),
                         period_interpolation_inducing_points=int(period), per_env_pole_mass=bool(per_env_pole_mass),
                         gru_model=gru_model, gru_adjoint=bool(gru_adjoint) or bool(gru_fused))   # (gru_fused: itself the opt-in)
        self.count = 0               # control steps taken
        self.draws = 0               # sampler launches (the Philox offset)
        self.fused = bool(fused)     # one cpmppi_rpgd_step per control step instead of the staged launches
        self._check_gru_adjoint(self.fused)
        self.gru_fused = bool(gru_fused)   # one cpmppi_rpgd_step_gru + cpmppi_gru_advance per control step: a fused object as well
        self.fused = self.fused or self.gru_fused
        self.rows = self._check_rows(rows)   # [num_envs, 16] per-env settings of the fused step; on the engine's device from configure() on

    def _check_rows(self, rows):
        if rows is None:
            return None
        if self.cfg.cost_function_specification != "quadratic_boundary_grad_minimal":
            raise ValueError("rows= holds the cost vector of quadratic_boundary_grad_minimal, not "
                             f"{self.cfg.cost_function_specification!r}")
        if tuple(rows.shape) != (self.num_envs, TUNING_ROW_FLOATS):
            raise ValueError(f"rows must be [num_envs={self.num_envs}, {TUNING_ROW_FLOATS}] (configs.rpgd_rows), got {tuple(rows.shape)}")
        return rows

    def configure(self, dt=None, predictor_specification=None, num_envs=None, **kwargs):
        if self.rows is not None and is_gru_specification(predictor_specification):
            raise ValueError(ROWS_OR_GRU)
        super().configure(dt=dt, predictor_specification=predictor_specification, num_envs=num_envs, **kwargs)
        if self.rows is not None:
            self.rows = self.engine.tensor(self._check_rows(self.rows))  # (the env count may be configure's)

    def _gru_selected(self, predictor_specification):
        neural = super()._gru_selected(predictor_specification)
        if self.gru_fused and not neural:
            raise ValueError(GRU_FUSED_NEEDS_MODEL)
        return neural

    def _set_timestep(self, dt):
        if dt != self.cfg.mpc_timestep:          # the sampling stdev stays what the constructor was asked for
            s = self.cfg.SQRTRHOINV / math.sqrt(self.cfg.mpc_timestep)
            self.cfg.mpc_timestep = dt
            self.cfg.SQRTRHOINV = s * math.sqrt(dt)

    # -- sampling ------------------------------------------------------------------------------------------------
    def _draw(self):
        """[E,N,H] plans from the sampling distribution (device)."""
        _, z = self.engine.sample(self.seed, offset=self.draws, knots=False, delta_u=True)
        self.draws += 1
        return self._shape_samples(z).clamp_(self.action_low, self.action_high).contiguous()

    def _shape_samples(self, z):
        return z

    def optimizer_reset(self):
        self.Q = self._draw()
        self.m, self.v = torch.zeros_like(self.Q), torch.zeros_like(self.Q)
        self.adam_it = 0
        self.count = 0
        self._first = True
        self._reset_memory()
        if self.fused:
            eng, E = self.engine, self.num_envs
            # what the fused step writes per control step: the controls, the final costs, the best plan (persistent buffers)
            self._u, self._S, self._plan = eng.zeros(E), eng.empty(E, self.num_rollouts), eng.empty(E, self.mpc_horizon)
            self._draw0 = self.draws                     # the first redraw's Philox offset (device mode counts on from it)
            self._prepared = self._prepared_key = self._attr_host = self._attr_dev = None

    # -- one control step ----------------------------------------------------------------------------------------
    def _descend(self, s_t, tp, te, L, iterations):
        eng = self.engine
        if self.h is not None:       # gru_adjoint: every gradient and cost launch of the step under the network, from the env's memory
            kw = dict(predictor="GRU", h0=self.h)
        else:
            kw = dict(L=L, previous_input=self._previous_input)
        for _ in range(iterations):
            _, G = eng.rollout_cost_grad(s_t, self.Q, tp, te, **kw)
            self.adam_it += 1
            eng.adam_step(self.Q, G, self.m, self.v, self.adam_it, self.learning_rate, self.adam_beta_1, self.adam_beta_2,
                          self.adam_epsilon, self.gradmax_clip)
        if self.h is not None:
            return eng.rollout_cost(s_t, self.Q, tp, te, **kw)
        return eng.rollout_cost(s_t, self.Q, tp, te, L=L) if self.cfg.cost_function_specification != "quadratic_boundary_grad" \
            else eng.rollout_cost_grad(s_t, self.Q, tp, te, L=L, previous_input=self._previous_input)[0]

    def _shift(self, by):
        if by <= 0:
            return
        for name in ("Q", "m", "v"):
            x = getattr(self, name)
            tail = x[:, :, -1:].expand(-1, -1, by) if name == "Q" else torch.zeros_like(x[:, :, :by])
            setattr(self, name, torch.cat([x[:, :, by:], tail], dim=2).contiguous())

    def _finish(self, S, single, as_tensor, s_t):
        E = S.shape[0]
        best = torch.argmin(S, dim=1)
        rows = torch.arange(E, device=S.device)
        u = self.Q[rows, best, 0].clone()
        self._previous_input = u.clone()
        self._advance_memory(s_t, u)                     # (the network's memory, once per control step, from the control applied)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": u.cpu().numpy(), "J_logged": S.cpu().numpy(),
                                   "u_logged": self.Q[rows, best].cpu().numpy()}
        self.count += 1
        return self._result(u, single, as_tensor)

    # -- the fused control step (cpmppi_rpgd_step) ----------------------------------------------------------------------
    def _fused_plan(self):
        """What the fused step does besides Adam: iterations, keep_k, resamp_per, shift and the redraw's distribution."""
        raise NotImplementedError

    def reserve_fused(self):
        """The fused step's workspace (cpmppi_rpgd_reserve; over the network cpmppi_rpgd_gru_reserve): after it a step never
        allocates - required before a capture."""
        if self.gru_fused:
            self.engine.rpgd_gru_reserve()
        else:
            self.engine.rpgd_reserve()

    def _fused_call(self, s, tp, te, L, previous_input, count_dev):
        """One cpmppi_rpgd_step on device tensors.  The argument block is built once per set of buffers; with ``count_dev`` the
        call changes nothing on the host, without it the host counters advance as the staged step's do.
        ``gru_fused``: one cpmppi_rpgd_step_gru from the memory ``h`` - the network knows no pole length and its costs read no
        previous input, so ``L`` and ``previous_input`` go unread -, then cpmppi_gru_advance on (the state seen, the control
        chosen): the memory is handed on the same way by ``step``, ``step_device`` and the device loop."""
        if self.gru_fused:
            L = previous_input = None
        key = self._fused_key(s, tp, te, L, previous_input, count_dev)
        if key != self._prepared_key:
            common = dict(learning_rate=self.learning_rate, beta1=self.adam_beta_1, beta2=self.adam_beta_2,
                          epsilon=self.adam_epsilon, gradmax_clip=self.gradmax_clip, seed=self.seed, draw_offset=self._draw0,
                          count_dev=count_dev, Q_out=self._u, S_out=self._S, plan_out=self._plan, **self._fused_plan())
            if self.gru_fused:
                self._prepared = self.engine.prepare_rpgd_step_gru(s, self.Q, self.m, self.v, tp, te, self.h, **common)
            else:
                if self.rows is not None:
                    common["rows"] = self.rows
                self._prepared = self.engine.prepare_rpgd_step(s, self.Q, self.m, self.v, tp, te, L, previous_input, **common)
            self._prepared_key = key
        if count_dev is not None:
            self._prepared.run()
        else:
            plan = self._fused_plan()
            iters = self.warmup_iterations if (self.warmup and self._first) else plan["iterations"]
            self._first = False
            self._prepared.run(count=self.count, adam_iteration=self.adam_it, draw_offset=self.draws, iterations=iters)
            self.adam_it += iters
            self.count += 1
            if plan["resamp_per"] > 0 and plan["keep_k"] < self.num_rollouts and self.count % plan["resamp_per"] == 0:
                self.draws += 1
        if self.gru_fused:
            self.engine.gru_advance(s, self._u, self.h)
        return self._u


class optimizer_gradient(_GradientBase):
    """config_optimizers.yml:49-62 (gradient-tf)."""
    optimizer_name = "gradient"

    def __init__(self, predictor=None, cost_function=None, control_limits=None, computation_library=None, seed=None,
                 mpc_horizon=35, mpc_timestep=0.02, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999,
                 adam_epsilon=1.0e-7, rtol=1.0e-3, gradient_steps=5, num_rollouts=40, initial_action_stdev=0.5,
                 gradmax_clip=5, warmup=False, warmup_iterations=250, optimizer_logging=False,
                 calculate_optimal_trajectory=False, num_envs=1, cost_function_specification=None, cost_weights=None,
                 intermediate_steps=10, horizon_reduce="sum", phys=None, device=0, variable_parameters=None,
                 per_env_pole_mass=False, fused=False, gru_model=None, gru_adjoint=False, gru_fused=False, rows=None, **kwargs):
        self.learning_rate, self.adam_beta_1, self.adam_beta_2 = float(learning_rate), float(adam_beta_1), float(adam_beta_2)
        self.adam_epsilon, self.gradmax_clip, self.rtol = float(adam_epsilon), float(gradmax_clip), float(rtol)
        self.gradient_steps, self.warmup, self.warmup_iterations = int(gradient_steps), bool(warmup), int(warmup_iterations)
        self.initial_action_stdev = float(initial_action_stdev)
        super().__init__(cost_function, control_limits, seed, mpc_horizon, mpc_timestep, num_rollouts, initial_action_stdev,
                         10, num_envs, cost_function_specification, cost_weights, intermediate_steps, phys, device,
                         variable_parameters, optimizer_logging, horizon_reduce, per_env_pole_mass, fused, gru_model, gru_adjoint,
                         gru_fused, rows)

    def _fused_plan(self):
        return {"iterations": self.gradient_steps, "keep_k": self.num_rollouts, "resamp_per": 0, "shift": 1}

    def _draw(self):
        """Independent N(0, initial_action_stdev) per time-step, clipped (cpmppi_cem_sample)."""
        eng = self.engine
        mid = 0.5 * (self.action_low + self.action_high)
        Q = eng.cem_sample(eng.zeros(self.num_envs, self.mpc_horizon) + mid,
                           eng.zeros(self.num_envs, self.mpc_horizon) + self.initial_action_stdev, self.seed, offset=self.draws)
        self.draws += 1
        return Q

    def step(self, s, time=None, as_tensor=False):
        if self.fused:
            return self._step_fused(s, as_tensor)
        s_t, single, E, tp, te, L = self._begin_step(s)
        iters = self.warmup_iterations if (self.warmup and self._first) else self.gradient_steps
        self._first = False
        S = self._descend(s_t, tp, te, L, iters)
        out = self._finish(S, single, as_tensor, s_t)
        self._shift(1)
        return out


class optimizer_rpgd(_GradientBase):
    """config_optimizers.yml:63-86 (rpgd)."""
    optimizer_name = "rpgd"

    def __init__(self, predictor=None, cost_function=None, control_limits=None, computation_library=None, seed=None,
                 mpc_horizon=35, mpc_timestep=0.02, SAMPLING_DISTRIBUTION="normal", period_interpolation_inducing_points=4,
                 learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1.0e-8, gradmax_clip=5, rtol=1.0e-3,
                 num_rollouts=16, opt_keep_k_ratio=0.75, outer_its=4, resamp_per=10, sample_stdev=0.5, sample_mean=0.0,
                 sample_whole_control_space=False, uniform_dist_max=0.8, uniform_dist_min=-0.8, shift_previous=1,
                 warmup=False, warmup_iterations=250, optimizer_logging=False, calculate_optimal_trajectory=False,
                 num_envs=1, cost_function_specification=None, cost_weights=None, intermediate_steps=10,
                 horizon_reduce="sum", phys=None, device=0, variable_parameters=None, per_env_pole_mass=False, fused=False,
                 gru_model=None, gru_adjoint=False, gru_fused=False, rows=None, **kwargs):
        if SAMPLING_DISTRIBUTION not in ("normal", "uniform"):
            raise ValueError(f"SAMPLING_DISTRIBUTION={SAMPLING_DISTRIBUTION!r}; expected 'normal' or 'uniform'")
        self.learning_rate, self.adam_beta_1, self.adam_beta_2 = float(learning_rate), float(adam_beta_1), float(adam_beta_2)
        self.adam_epsilon, self.gradmax_clip, self.rtol = float(adam_epsilon), float(gradmax_clip), float(rtol)
        self.outer_its, self.resamp_per, self.shift_previous = int(outer_its), int(resamp_per), int(shift_previous)
        self.warmup, self.warmup_iterations = bool(warmup), int(warmup_iterations)
        self.distribution, self.sample_mean, self.sample_stdev = SAMPLING_DISTRIBUTION, float(sample_mean), float(sample_stdev)
        self.sample_whole_control_space = bool(sample_whole_control_space)
        self.uniform_dist_min, self.uniform_dist_max = float(uniform_dist_min), float(uniform_dist_max)
        self.opt_keep_k = max(1, int(float(opt_keep_k_ratio) * int(num_rollouts)))
        stdev = self.sample_stdev if SAMPLING_DISTRIBUTION == "normal" else 1.0
        super().__init__(cost_function, control_limits, seed, mpc_horizon, mpc_timestep, num_rollouts, stdev,
                         period_interpolation_inducing_points, num_envs, cost_function_specification, cost_weights,
                         intermediate_steps, phys, device, variable_parameters, optimizer_logging, horizon_reduce,
                         per_env_pole_mass, fused, gru_model, gru_adjoint, gru_fused, rows)

    def _uniform_range(self):
        return (self.action_low, self.action_high) if self.sample_whole_control_space else \
            (self.uniform_dist_min, self.uniform_dist_max)

    def _fused_plan(self):
        lo, hi = self._uniform_range()
        return {"iterations": self.outer_its, "keep_k": self.opt_keep_k, "resamp_per": self.resamp_per,
                "shift": self.shift_previous, "distribution": self.distribution, "sample_mean": self.sample_mean,
                "uniform_lo": lo, "uniform_hi": hi}

    def _shape_samples(self, z):
        if self.distribution == "normal":
            return z + self.sample_mean if self.sample_mean != 0.0 else z
        lo, hi = self._uniform_range()
        return lo + (hi - lo) * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))     # N(0,1) -> U(lo, hi)

    def step(self, s, time=None, as_tensor=False):
        if self.fused:
            return self._step_fused(s, as_tensor)
        s_t, single, E, tp, te, L = self._begin_step(s)
        iters = self.warmup_iterations if (self.warmup and self._first) else self.outer_its
        self._first = False
        S = self._descend(s_t, tp, te, L, iters)
        out = self._finish(S, single, as_tensor, s_t)
        if self.resamp_per > 0 and self.count % self.resamp_per == 0 and self.opt_keep_k < self.num_rollouts:
            # survivors: the opt_keep_k cheapest plans (stable top-k on the device), moments kept; the rest re-drawn
            _, _, elite = self.engine.cem_update(S, self.Q, self.opt_keep_k, 0.0, return_elites=True)
            idx = elite.long().unsqueeze(-1).expand(-1, -1, self.mpc_horizon)
            fresh = self._draw()
            k = self.opt_keep_k
            for name in ("Q", "m", "v"):
                x = getattr(self, name)
                rest = fresh[:, k:] if name == "Q" else torch.zeros_like(x[:, k:])
                setattr(self, name, torch.cat([torch.gather(x, 1, idx), rest], dim=1).contiguous())
        self._shift(self.shift_previous)
        return out
