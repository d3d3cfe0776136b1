"""optimizer_cem — cross-entropy-method optimizer over the same fused rollout + cost kernel.

Constructor keywords = the keys of ``Control_Toolkit_ASF/config_optimizers.yml:1-11`` (section ``cem-tf``).  The class
itself lives in the absent Control_Toolkit submodule, so the update is the one those keys name: ``cem_outer_it`` times
{sample ``num_rollouts`` sequences from N(mean, stdev) clipped to the control limits, roll out + cost, refit mean and
stdev to the ``cem_best_k`` cheapest, floor stdev at ``cem_stdev_min``}; apply ``mean[0]``; shift mean (append the
mid-point of the limits) and stdev (append sqrt(0.5)).  Sampling, rollout, cost and the top-k refit all run on the GPU
(cpmppi_cem_sample, cpmppi_rollout_cost, cpmppi_cem_update); ``num_envs`` problem instances advance in one launch.

``fused=True`` (off by default; cem, cem-naive-grad and cem-grad-bharadhwaj) makes the whole control step ONE library call,
cpmppi_cem_step: the outer iterations of sampling, refinement, cost, ranking and refit, then the shift, in one kernel, mean and
stdev updated in place.  ``step`` then only uploads the state; ``step_device`` takes device tensors and, with a device step
counter, touches the host not at all - the form a captured closed loop replays (harness.py).  The fused step costs its samples
with the adjoint kernel's forward sweep (sin / cos on every substep) and hands the control of the step before to the cost
(``previous_input``, read by quadratic_boundary_grad); the staged path above stays what it was.

cem, cem-gmm and random-action also run on the neural predictor (``gru_model=`` and / or a ``GRU-6IN-32H1-32H2-5OUT*``
``predictor_specification``, under optimizer_mppi's rules): they only need the costs of given plans, which
cpmppi_rollout_cost_gru computes with the network in the rollout loop.  Each env keeps the network's memory ``h`` [E,2,32]:
zero after a reset, handed to every cost launch of a control step, then advanced with the state seen and the control applied.
The two hybrids need the cost's gradient: they refuse the network unless asked with ``gru_adjoint=True``, which makes their
refinement cpmppi_rollout_cost_grad_gru from the same memory; ``fused=True`` refuses it either way (cpmppi_cem_step integrates
the ODE, and has no adjoint kernel for the GRU).

``gru_fused=True`` (cem alone; needs the network) is the fused step over the network: ONE cpmppi_cem_step_gru per control step -
sampling, the GRU rollouts from each env's memory, ranking and refit for all outer iterations in one kernel, bit for bit what the
staged step above computes - followed by cpmppi_gru_advance, which moves the memory on in place with the state seen and the
control chosen.  The object is then a fused one (``fused`` is true, ``step_device``, a device step counter): the closed loop over
a learned model launches, or replays as a captured graph, like the fused ODE step's (harness.py).  cem-gmm and random-action are
not fusable and the two hybrids have no fused GRU adjoint: they refuse the flag by name.
"""
import math

import torch

from ._optimizer_base import _OptimizerBase, is_gru_specification

GRU_NO_ADJOINT = ("{} needs the gradient of the cost and runs on the ODE_v0 and ODE predictors by default (the fused step has no adjoint "
                  "kernel for the GRU predictor): pass gru_adjoint=True to differentiate through the network in the staged step "
                  "(cpmppi_rollout_cost_grad_gru); cem, cem-gmm and random-action run on the GRU without it")
GRU_NOT_FUSED = ("fused=True integrates the ODE (cpmppi_cem_step): the GRU predictor runs in the staged step of cem, cem-gmm and "
                 "random-action, fused=False")
GRU_FUSED_ONLY_CEM = ("gru_fused=True: the fused CEM control step over the GRU predictor (cpmppi_cem_step_gru) is built for cem, "
                      "not for {}: {}")
GRU_FUSED_OR_FUSED = ("gru_fused=True and fused=True: fused=True is the step that integrates the ODE (cpmppi_cem_step), gru_fused=True "
                      "the one over the network (cpmppi_cem_step_gru): give one of them")
GRU_FUSED_NEEDS_MODEL = ("gru_fused=True is the fused step over the GRU predictor: it needs gru_model= (weights or a model folder) "
                         "and / or a GRU-6IN-32H1-32H2-5OUT predictor_specification")
_NO_FUSED_GRU_ADJOINT = ("there is no fused GRU adjoint; gru_adjoint=True differentiates through the network in the staged step")


class optimizer_cem(_OptimizerBase):
    optimizer_name = "cem"
    _unknown_predictor = "the sampling optimizers run on the ODE_v0 and ODE predictors"
    _fusable = True                  # cpmppi_cem_step is built for this class (not for cem-gmm and random-action)
    _gru_fused_refusal = None        # why cpmppi_cem_step_gru cannot run this class (cem alone has none)

    def __init__(self, predictor=None, cost_function=None, control_limits=None, computation_library=None, seed=None,
                 mpc_horizon=35, mpc_timestep=0.02, cem_outer_it=3, cem_initial_action_stdev=0.5, num_rollouts=200,
                 cem_stdev_min=0.01, cem_best_k=40, warmup=False, warmup_iterations=250, optimizer_logging=False,
                 calculate_optimal_trajectory=False, num_envs=1, cost_function_specification=None, cost_weights=None,
                 math_mode="fast", intermediate_steps=10, phys=None, device=0, variable_parameters=None, per_env_pole_mass=False,
                 fused=False, gru_model=None, gru_adjoint=False, gru_fused=False, **kwargs):
        if gru_fused and self._gru_fused_refusal:
            raise ValueError(GRU_FUSED_ONLY_CEM.format(self.optimizer_name, self._gru_fused_refusal))
        if gru_fused and fused:
            raise ValueError(GRU_FUSED_OR_FUSED)
        super().__init__(cost_function, control_limits, seed, num_envs, cost_function_specification, cost_weights,
                         variable_parameters, phys, device, optimizer_logging, mpc_horizon, mpc_timestep, num_rollouts,
                         intermediate_steps, control_mode="clip", shift_mode="none", math_mode=math_mode,
                         per_env_pole_mass=bool(per_env_pole_mass), gru_model=gru_model, gru_adjoint=gru_adjoint)
        self.cem_outer_it, self.cem_best_k = int(cem_outer_it), int(cem_best_k)
        self.cem_initial_action_stdev, self.cem_stdev_min = float(cem_initial_action_stdev), float(cem_stdev_min)
        self.warmup, self.warmup_iterations = bool(warmup), int(warmup_iterations)
        self.step_counter = 0
        self.fused = bool(fused)     # one cpmppi_cem_step per control step instead of the staged launches
        if self.fused and not self._fusable:
            raise ValueError(f"fused=True: the fused CEM control step (cpmppi_cem_step) is built for cem, cem-naive-grad and "
                             f"cem-grad-bharadhwaj, not for {self.optimizer_name}")
        if self._gru_refusal:        # (the hybrids: what their opt-in to the GRU adjoint cannot be combined with)
            self._check_gru_adjoint(self.fused)
        if self.fused and gru_model is not None:
            raise ValueError(GRU_NOT_FUSED)
        self.gru_fused = bool(gru_fused)   # one cpmppi_cem_step_gru + cpmppi_gru_advance per control step: a fused object as well
        self.fused = self.fused or self.gru_fused

    def _gru_selected(self, predictor_specification):
        if self.fused and not self.gru_fused and (is_gru_specification(predictor_specification) or self.gru_model is not None):
            raise ValueError(GRU_NOT_FUSED)
        neural = super()._gru_selected(predictor_specification)
        if self.gru_fused and not neural:
            raise ValueError(GRU_FUSED_NEEDS_MODEL)
        return neural

    def _cost(self, s_t, Q, tp, te, L):
        """Costs [E,N] of the plans Q [E,N,H]: under the ODE, or - with the network - under the GRU from each env's memory."""
        if self.h is not None:
            return self.engine.rollout_cost(s_t, Q, tp, te, predictor="GRU", h0=self.h)
        return self.engine.rollout_cost(s_t, Q, tp, te, L=L)

    def _refine(self, Q, s_t, tp, te, L):
        """Hook of the CEM + gradient hybrids: improve the samples before they are ranked."""
        return Q

    def _gradient(self, s_t, Q, tp, te, L):
        """d cost / d Q [E,N,H] of the samples, under the predictor _cost uses (the hybrids' refinement)."""
        if self.h is not None:
            return self.engine.rollout_cost_grad(s_t, Q, tp, te, predictor="GRU", h0=self.h)[1]
        return self.engine.rollout_cost_grad(s_t, Q, tp, te, L=L)[1]

    def optimizer_reset(self):
        E, H = self.num_envs, self.mpc_horizon
        self.dist_mue = self.engine.zeros(E, H) + 0.5 * (self.action_low + self.action_high)
        self.stdev = self.engine.zeros(E, H) + self.cem_initial_action_stdev
        self.step_counter = 0
        self._first = True
        self._reset_memory()
        if self.fused:
            eng = self.engine
            # what the fused step writes per control step: the controls, the last costs, the mean before the shift
            self._u, self._S, self._plan = eng.zeros(E), eng.empty(E, self.num_rollouts), eng.empty(E, H)
            self._previous_input = None
            self._prepared = self._prepared_key = self._attr_host = self._attr_dev = None

    # -- the fused control step (cpmppi_cem_step) -------------------------------------------------------------------------
    def _fused_refine(self):
        """The hybrids: the refine kind and its hyper-parameters, as cem_step's keywords."""
        return {}

    def reserve_fused(self):
        """The fused step's workspace (cpmppi_cem_reserve): after it a step never allocates - required before a capture."""
        self.engine.cem_reserve(refine=self._fused_refine().get("refine"))

    def _fused_call(self, s, tp, te, L, previous_input, count_dev):
        """One cpmppi_cem_step on device tensors.  The argument block is built once per set of buffers; with ``count_dev`` the
        call changes nothing on the host (iteration i of step c draws at Philox offset c * cem_outer_it + i), without it
        ``step_counter`` advances by the iterations taken, as the staged step's does.
        ``gru_fused``: one cpmppi_cem_step_gru from the memory ``h`` - the network knows no pole length and its costs read no
        previous input, so ``L`` and ``previous_input`` go unread -, then cpmppi_gru_advance on (the state seen, the control
        chosen): the memory is handed on the same way by ``step``, ``step_device`` and the device loop."""
        if self.gru_fused:
            L = previous_input = None
        key = self._fused_key(s, tp, te, L, previous_input, count_dev)
        if key != self._prepared_key:
            common = dict(iterations=self.cem_outer_it, best_k=self.cem_best_k, stdev_min=self.cem_stdev_min, shift=1,
                          mean_fill=0.5 * (self.action_low + self.action_high), stdev_fill=math.sqrt(0.5), seed=self.seed, offset=0,
                          count_dev=count_dev, Q_out=self._u, S_out=self._S, plan_out=self._plan)
            if self.gru_fused:
                self._prepared = self.engine.prepare_cem_step_gru(s, self.dist_mue, self.stdev, tp, te, self.h, **common)
            else:
                self._prepared = self.engine.prepare_cem_step(s, self.dist_mue, self.stdev, tp, te, L, previous_input, **common,
                                                              **self._fused_refine())
            self._prepared_key = key
        if count_dev is not None:
            self._prepared.run()
        else:
            iters = self.warmup_iterations if (self.warmup and self._first) else self.cem_outer_it
            self._first = False
            self._prepared.run(offset=self.step_counter, iterations=iters)
            self.step_counter += iters
        if self.gru_fused:
            self.engine.gru_advance(s, self._u, self.h)
        return self._u

    def _shift(self):
        """Mean and stdev one control step on: the mid-point of the limits / sqrt(0.5) appended.  -> that mid-point."""
        mid = 0.5 * (self.action_low + self.action_high)
        self.dist_mue = torch.cat([self.dist_mue[:, 1:], torch.full_like(self.dist_mue[:, :1], mid)], dim=1).contiguous()
        self.stdev = torch.cat([self.stdev[:, 1:], torch.full_like(self.stdev[:, :1], math.sqrt(0.5))], dim=1).contiguous()
        return mid

    def step(self, s, time=None, as_tensor=False):
        if self.fused:
            return self._step_fused(s, as_tensor)
        s_t, single, E, tp, te, L = self._begin_step(s)
        eng = self.engine
        iters = self.warmup_iterations if (self.warmup and self._first) else self.cem_outer_it
        self._first = False
        for _ in range(iters):
            Q = eng.cem_sample(self.dist_mue, self.stdev, self.seed, offset=self.step_counter)
            Q = self._refine(Q, s_t, tp, te, L)
            S = self._cost(s_t, Q, tp, te, L)
            self.dist_mue, self.stdev = eng.cem_update(S, Q, self.cem_best_k, self.cem_stdev_min)
            self.step_counter += 1
        u = self.dist_mue[:, 0].clone()
        self._advance_memory(s_t, u)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": u.cpu().numpy(), "J_logged": S.cpu().numpy(),
                                   "u_logged": self.dist_mue.cpu().numpy()}
        self._shift()
        return self._result(u, single, as_tensor)


class optimizer_cem_gmm(optimizer_cem):
    """``cem-gmm-tf`` (config_optimizers.yml:12-20): CEM whose sampling distribution is a Gaussian MIXTURE — one
    component per elite of the previous iteration, centred on that elite sequence, equal weights, all sharing the
    per-time-step standard deviation refitted to the elites (floored at ``cem_stdev_min``).  The first iteration after a
    reset samples around the mid-point sequence with ``cem_initial_action_stdev`` (a single component).  Applied control:
    the first input of the best sequence found; the elites are shifted by one step for the next control step.
    [recalled semantics: the class lives in the absent Control_Toolkit submodule; unpinned, stated in DESIGN.md]"""
    optimizer_name = "cem-gmm"
    _fusable = False                 # (the mixture needs the previous iteration's elites as centres)
    _gru_fused_refusal = "cem-gmm is not fusable (the mixture needs the previous iteration's elites as centres)"

    def optimizer_reset(self):
        super().optimizer_reset()
        self.centres = self.dist_mue[:, None, :].contiguous()           # [E, 1, H]: one component until elites exist

    def step(self, s, time=None, as_tensor=False):
        s_t, single, E, tp, te, L = self._begin_step(s)
        eng = self.engine
        ar = torch.arange(E, device=self.dist_mue.device)[:, None]
        for _ in range(self.cem_outer_it):
            Q = eng.cem_gmm_sample(self.centres, self.stdev, self.seed, offset=self.step_counter)
            S = self._cost(s_t, Q, tp, te, L)
            self.dist_mue, self.stdev, el = eng.cem_update(S, Q, self.cem_best_k, self.cem_stdev_min, return_elites=True)
            self.centres = Q[ar, el.long()].contiguous()                # [E, K, H], cheapest first (stable order)
            self.step_counter += 1
        u = self.centres[:, 0, 0].clone()                               # first input of the best sequence
        self._advance_memory(s_t, u)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": u.cpu().numpy(), "J_logged": S.cpu().numpy(),
                                   "u_logged": self.centres[:, 0].cpu().numpy()}
        mid = self._shift()
        self.centres = torch.cat([self.centres[:, :, 1:], torch.full_like(self.centres[:, :, :1], mid)], dim=2).contiguous()
        return self._result(u, single, as_tensor)


class optimizer_cem_naive_grad(optimizer_cem):
    """``cem-naive-grad-tf`` (config_optimizers.yml:21-31): CEM whose samples take ONE plain gradient step
    ``Q <- clip(Q - learning_rate * clip_by_norm(dJ/dQ, gradmax_clip))`` (cpmppi_rollout_cost_grad + cpmppi_sgd_step)
    before the elites are chosen.  [recalled semantics, class absent from the tree]"""
    optimizer_name = "cem-naive-grad"
    _gru_refusal = GRU_NO_ADJOINT.format("cem-naive-grad")
    _gru_fused_refusal = _NO_FUSED_GRU_ADJOINT

    def __init__(self, *args, learning_rate=0.1, gradmax_clip=10, cem_outer_it=1, cem_stdev_min=0.1, **kwargs):
        super().__init__(*args, cem_outer_it=cem_outer_it, cem_stdev_min=cem_stdev_min, **kwargs)
        self.learning_rate, self.gradmax_clip = float(learning_rate), float(gradmax_clip)

    def _refine(self, Q, s_t, tp, te, L):
        G = self._gradient(s_t, Q, tp, te, L)
        return self.engine.sgd_step(Q, G, self.learning_rate, self.gradmax_clip)

    def _fused_refine(self):
        return {"refine": "sgd", "learning_rate": self.learning_rate, "gradmax_clip": self.gradmax_clip}


class optimizer_cem_grad_bharadhwaj(optimizer_cem):
    """``cem-grad-bharadhwaj-tf`` (config_optimizers.yml:32-48; Bharadhwaj et al. 2020, "Model-predictive control via
    cross-entropy and gradient-based optimization"): every CEM sample takes an Adam step on dJ/dQ before the elites
    are chosen; the Adam moments belong to the sample slots and persist over the outer iterations of a control step.
    [recalled semantics, class absent from the tree]"""
    optimizer_name = "cem-grad-bharadhwaj"
    _gru_refusal = GRU_NO_ADJOINT.format("cem-grad-bharadhwaj")
    _gru_fused_refusal = _NO_FUSED_GRU_ADJOINT

    def __init__(self, *args, learning_rate=0.05, adam_beta_1=0.9, adam_beta_2=0.999, adam_epsilon=1.0e-8, num_rollouts=32,
                 cem_best_k=8, cem_outer_it=2, cem_initial_action_stdev=2, cem_stdev_min=1.0e-6, gradmax_clip=5, **kwargs):
        super().__init__(*args, num_rollouts=num_rollouts, cem_best_k=cem_best_k, cem_outer_it=cem_outer_it,
                         cem_initial_action_stdev=cem_initial_action_stdev, cem_stdev_min=cem_stdev_min, **kwargs)
        self.learning_rate, self.adam_beta_1, self.adam_beta_2 = float(learning_rate), float(adam_beta_1), float(adam_beta_2)
        self.adam_epsilon, self.gradmax_clip = float(adam_epsilon), float(gradmax_clip)

    def _fused_refine(self):
        return {"refine": "adam", "learning_rate": self.learning_rate, "beta1": self.adam_beta_1, "beta2": self.adam_beta_2,
                "epsilon": self.adam_epsilon, "gradmax_clip": self.gradmax_clip}

    def step(self, s, time=None, as_tensor=False):
        self._m = self._v = None                    # fresh moments every control step
        self._it = 0
        return super().step(s, time, as_tensor)

    def _refine(self, Q, s_t, tp, te, L):
        if self._m is None:
            self._m, self._v = torch.zeros_like(Q), torch.zeros_like(Q)
        G = self._gradient(s_t, Q, tp, te, L)
        self._it += 1
        return self.engine.adam_step(Q, G, self._m, self._v, self._it, self.learning_rate, self.adam_beta_1, self.adam_beta_2,
                                     self.adam_epsilon, self.gradmax_clip)


class optimizer_random_action(optimizer_cem):
    """``random-action-tf`` (config_optimizers.yml:98-102): ``num_rollouts`` input plans drawn uniformly from the control
    limits every control step, the first input of the cheapest one is applied; nothing is carried over.
    [recalled semantics, class absent from the tree]"""
    optimizer_name = "random-action"
    _fusable = False
    _gru_fused_refusal = "random-action is not fusable (it draws uniform plans and keeps no distribution)"

    def __init__(self, *args, num_rollouts=640, **kwargs):
        kwargs.pop("cem_outer_it", None)
        super().__init__(*args, num_rollouts=num_rollouts, cem_outer_it=1, cem_best_k=1, **kwargs)

    def step(self, s, time=None, as_tensor=False):
        s_t, single, E, tp, te, L = self._begin_step(s)
        eng = self.engine
        # N(0,1) from the device Philox sampler (clip limits far away), mapped to U(low, high) through the normal CDF
        wide = eng.zeros(E, self.mpc_horizon)
        z = self._normal(wide, self.step_counter)
        lo, hi = self.action_low, self.action_high
        Q = (lo + (hi - lo) * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))).clamp_(lo, hi).contiguous()
        self.step_counter += 1
        S = self._cost(s_t, Q, tp, te, L)
        best = torch.argmin(S, dim=1)
        u = Q[torch.arange(E, device=S.device), best, 0].clone()
        self._advance_memory(s_t, u)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": u.cpu().numpy(), "J_logged": S.cpu().numpy()}
        return self._result(u, single, as_tensor)

    def _normal(self, zeros_EH, offset):
        # the sampler clips to the control limits, so draw with a small stdev and rescale: z = (x / 0.01), |x| <= 1 keeps
        # |z| <= 100, i.e. no clipping of a standard normal
        x = self.engine.cem_sample(zeros_EH + 0.5 * (self.action_low + self.action_high),
                                   zeros_EH + 0.01 * 0.5 * (self.action_high - self.action_low), self.seed, offset=offset)
        return (x - 0.5 * (self.action_low + self.action_high)) / (0.01 * 0.5 * (self.action_high - self.action_low))
