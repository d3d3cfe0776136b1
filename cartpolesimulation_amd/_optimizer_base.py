"""_OptimizerBase — what optimizer_mppi, the CEM family and the gradient family share: the constructor block every optimizer
gets from ``controller_mpc.configure`` (control limits, seed, cost inherited from the cost-function object, MPPIConfig, engine
bookkeeping), the ``dt`` / ``num_envs`` / predictor part of ``configure``, and the per-step prologue (state -> [E,6], per-env
attributes) and epilogue (controls -> [1] / [E,1]).  The optimizers' own signatures, defaults and attributes are theirs.

The neural predictor (``gru_model=`` / a ``GRU-6IN-32H1-32H2-5OUT*`` specification) is settled here too, for the optimizers that
run on it - mppi in its fused step, cem, cem-gmm and random-action through the cost-only GRU rollout, the gradient family
(gradient, rpgd, cem-naive-grad, cem-grad-bharadhwaj) through the GRU adjoint when asked with ``gru_adjoint=True`` - and for
those that refuse it by name: which of specification and model selects it, the model's upload, the memory ``h`` [E,2,32] per env and its hand-over
from one control step to the next.
"""
import os
import time as _time

import numpy as np

from .configs import MPPIConfig, PhysicalParameters, ode_predictor_type


GRU_SPECIFICATION = "GRU-6IN-32H1-32H2-5OUT"      # SI_Toolkit_ASF/config_predictors.yml:8-13: the names of the neural predictor


def is_gru_specification(spec):
    return spec is not None and str(spec).startswith(GRU_SPECIFICATION)


def _vec(x, E, default):
    if x is None:
        return np.full(E, default, dtype=np.float32)
    x = np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float32).reshape(-1)
    return np.full(E, x[0], dtype=np.float32) if x.size == 1 else x.astype(np.float32)


class _OptimizerBase:
    _cost_name_attributes = ("cost_name",)           # where a cost-function object keeps its name
    _unknown_predictor = "this optimizer runs on the ODE_v0 and ODE predictors"
    _gru_refusal = None                               # a class that cannot run on the GRU predictor: why not (its own sentence)

    def __init__(self, cost_function, control_limits, seed, num_envs, cost_function_specification, cost_weights,
                 variable_parameters, phys, device, optimizer_logging, mpc_horizon, mpc_timestep, num_rollouts,
                 intermediate_steps, gru_model=None, gru_adjoint=False, **config):
        """``config``: the remaining MPPIConfig fields, which differ from optimizer to optimizer.  ``gru_model``: dict of
        GRU-6IN-32H1-32H2-5OUT weights or a model-folder path -> the neural predictor in the rollout loop.  ``gru_adjoint``:
        the opt-in of a class that needs the cost's gradient (one with a ``_gru_refusal``) to the GRU adjoint,
        cpmppi_rollout_cost_grad_gru; without it such a class refuses the network as before."""
        self.gru_adjoint = bool(gru_adjoint)
        if gru_model is not None and self._gru_refusal and not self.gru_adjoint:
            raise NotImplementedError(self._gru_refusal)
        self.gru_model = gru_model
        self.h = None                                      # its memory per env [E,2,32] (controller_mppi_cartpole.py:566-567 update)
        low, high = (-1.0, 1.0) if control_limits is None else (float(np.asarray(control_limits[0]).reshape(-1)[0]),
                                                                  float(np.asarray(control_limits[1]).reshape(-1)[0]))
        self.action_low, self.action_high = low, high
        if seed is None:                                   # others/globals_and_utils.py:198-214 (time xor pid)
            seed = (_time.time_ns() ^ os.getpid()) & 0x7FFFFFFFFFFFFFFF
        self.seed = int(seed)
        self.num_envs = int(num_envs)
        if cost_function is not None and cost_function_specification is None:
            for name in self._cost_name_attributes:
                cost_function_specification = cost_function_specification or getattr(cost_function, name, None)
            cost_weights = cost_weights or getattr(cost_function, "weights", None)
        self.variable_parameters = variable_parameters if variable_parameters is not None else \
            getattr(cost_function, "variable_parameters", None)
        self.cfg = MPPIConfig(seed=self.seed, mpc_horizon=int(mpc_horizon), mpc_timestep=float(mpc_timestep),
                              num_rollouts=int(num_rollouts), intermediate_steps=int(intermediate_steps),
                              cost_function_specification=cost_function_specification or "quadratic_boundary_grad_minimal",
                              cost_weights=dict(cost_weights or {}), action_low=low, action_high=high, **config)
        self.phys = phys or PhysicalParameters()
        self.device = device
        self.num_rollouts, self.mpc_horizon = self.cfg.num_rollouts, self.cfg.mpc_horizon
        self.optimizer_logging = optimizer_logging
        self.logging_values = {}
        self.engine = None

    # -- configure ------------------------------------------------------------------------------------------------
    def configure(self, dt=None, predictor_specification=None, num_envs=None, **kwargs):
        # (a GRU specification leaves the ODE integrator of the constructor alone: the network runs inside the rollout kernel)
        self._configure_problem(dt, None if is_gru_specification(predictor_specification) else predictor_specification, num_envs)
        neural = self._gru_selected(predictor_specification)
        self.engine = self._new_engine()
        self._attach_gru(neural)
        self.optimizer_reset()

    def _gru_selected(self, predictor_specification):
        """Specification and ``gru_model`` together -> does the network predict?  A specification without a model and a model
        beside an ODE specification are errors, a model alone selects the GRU; a class without a GRU path refuses both."""
        neural = is_gru_specification(predictor_specification)
        if (neural or self.gru_model is not None) and self._gru_refusal and not self.gru_adjoint:
            raise NotImplementedError(self._gru_refusal)
        if isinstance(self.gru_model, (str, bytes)) or hasattr(self.gru_model, "__fspath__"):
            from .model_folder import load_gru_model          # an SI_Toolkit model folder (net-info, normalisation, weights)
            self.gru_model = load_gru_model(self.gru_model)
        if neural and self.gru_model is None:
            raise ValueError("a GRU predictor_specification needs gru_model=dict(weights) or a model folder path "
                             "(no GRU model files ship in-tree)")
        if self.gru_model is not None and not (neural or predictor_specification is None):
            raise ValueError(f"gru_model was given but predictor_specification={predictor_specification!r} selects the ODE "
                             "predictor: the model would be ignored")
        return self.gru_model is not None

    def _check_gru_adjoint(self, fused):
        """What ``gru_adjoint=True`` cannot be combined with (the gradient family's constructors ask): the fused control steps
        and the one cost of the ODE adjoint that the GRU kernels do not have."""
        if not self.gru_adjoint:
            return
        if fused:
            raise ValueError("gru_adjoint=True with fused=True: cpmppi_rpgd_step and cpmppi_cem_step integrate the ODE; the GRU "
                             "adjoint (cpmppi_rollout_cost_grad_gru) runs in the staged step, fused=False")
        if self.cfg.cost_function_specification == "quadratic_boundary_grad":
            raise ValueError("gru_adjoint=True with quadratic_boundary_grad: the GRU kernels are built for "
                             "quadratic_boundary_grad_minimal and default")

    def _attach_gru(self, neural):
        """The new engine gets the model, every env a zero memory; without the network there is none."""
        if neural:
            self.engine.set_gru(self.gru_model)
            self.h = self.engine.zeros(self.num_envs, 2, 32)
        else:
            self.h = None

    def _reset_memory(self):
        if self.h is not None:
            self.h.zero_()

    def _advance_memory(self, s_t, u):
        """Advance the network's memory with the state just seen and the control just chosen (update_internal_state): s_t [E,6],
        u [E].  The memory travels as [E,2,32] (the rollout kernels' layout) and through gru_predict as [2,E,32]."""
        if self.h is None:
            return
        _, h_new = self.engine.gru_predict(s_t, u.reshape(self.num_envs, 1), h0=self.h.transpose(0, 1).contiguous(),
                                           return_hidden=True)
        self.h = h_new.transpose(0, 1).contiguous()

    def _configure_problem(self, dt, predictor_specification, num_envs):
        if dt is not None:
            self._set_timestep(float(dt))
        if num_envs is not None:
            self.num_envs = int(num_envs)
        ptype = ode_predictor_type(predictor_specification, self._unknown_predictor)
        if ptype is not None:                             # (no specification: the constructor's predictor_type stands)
            self.cfg.predictor_type = ptype

    def _set_timestep(self, dt):
        self.cfg.mpc_timestep = dt

    def _new_engine(self):
        from .engine import MPPIEngine                    # (looked up at every call: the CPU tests put a stand-in there)
        return MPPIEngine(self.num_envs, self.cfg, self.phys, device=self.device)

    # -- one control step -----------------------------------------------------------------------------------------
    @property
    def _mass_rows(self):
        """apply_pole_mass_of's row count, one entry per env (handed over only with the flag: an engine without it takes none)."""
        return {"rows": self.num_envs} if self.cfg.per_env_pole_mass else {}

    def _attributes(self, E):
        """-> target_position, target_equilibrium, L as float32 host vectors [E], read off variable_parameters."""
        vp = self.variable_parameters
        return (_vec(getattr(vp, "target_position", None), E, 0.0), _vec(getattr(vp, "target_equilibrium", None), E, 1.0),
                _vec(getattr(vp, "L", None), E, self.phys.L))

    def _begin_step(self, s):
        """s[6] (one env) or s[E,6] -> (s_t [E,6], single, E, tp, te, L) on the engine's device.  The attributes are uploaded
        ONCE per control step: every sampler / cost / gradient launch of its iterations reuses the tensors."""
        if self.engine is None:
            self.configure()
        eng = self.engine
        eng.apply_pole_mass_of(self.variable_parameters, **self._mass_rows)   # (predictors_customization.py:55-58; only "ODE" reads it)
        s_t = eng.tensor(s)
        single = s_t.dim() == 1
        s_t = s_t.reshape(-1, 6)
        E = s_t.shape[0]
        if E != self.num_envs:
            raise ValueError(f"optimizer configured for {self.num_envs} envs, got {E} states")
        tp, te, L = (eng.tensor(x) for x in self._attributes(E))
        return s_t, single, E, tp, te, L

    # -- the fused control step: one library call (the optimizers that build one set `fused` and give `_fused_call`) -------
    _previous_input = None

    def _fused_call(self, s, tp, te, L, previous_input, count_dev):
        """One fused step on device tensors -> the controls buffer; with ``count_dev`` the host counts nothing."""
        raise NotImplementedError

    def _fused_key(self, s, tp, te, L, previous_input, count_dev):
        """The device tensors of a fused step, checked -> what tells one set of buffers from another (an argument block is built
        once per set)."""
        import torch
        E = self.num_envs
        for name, t, shape in (("s", s, (E, 6)), ("target_position", tp, (E,)), ("target_equilibrium", te, (E,)), ("L", L, (E,)),
                               ("previous_input", previous_input, (E,))):
            if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()
                                      and tuple(t.shape) == shape):
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on the engine's device")
        return tuple(0 if t is None else t.data_ptr() for t in (s, tp, te, L, previous_input, count_dev))

    def reserve_fused(self):
        """The fused step's workspace: after it a step never allocates - required before a step is captured into a graph."""
        raise NotImplementedError

    @property
    def controls(self):
        """The fused step's output [E]: the persistent device tensor every step writes (a closed loop's plant reads it in place)."""
        return self._u

    def step_device(self, s, target_position, target_equilibrium, L=None, previous_input=None, count_dev=None):
        """The fused control step on DEVICE tensors: s [E,6], the per-env vectors [E] (L, previous_input: or None), and
        optionally ``count_dev``, an int64 device scalar holding the control steps taken so far (incremented by the step).
        Nothing is read back and nothing is uploaded, so the call can be captured into a graph (reserve the workspace with
        ``reserve_fused()`` and apply the pole mass before).  -> the controls [E]: a persistent device tensor that the
        next step overwrites."""
        if not self.fused:
            raise ValueError(f"{type(self).__name__}.step_device needs fused=True")
        if count_dev is not None and self.warmup:
            raise ValueError("warmup=True runs warmup_iterations on the first step, which a device step counter cannot tell "
                             "from the others: use the host counters (count_dev=None) or warmup=False")
        if self.engine is None:
            self.configure()
        return self._fused_call(s, target_position, target_equilibrium, L, previous_input, count_dev)

    def _step_fused(self, s, as_tensor):
        if self.engine is None:
            self.configure()
        eng = self.engine
        eng.apply_pole_mass_of(self.variable_parameters, **self._mass_rows)
        s_t = eng.tensor(s)
        single = s_t.dim() == 1
        s_t = s_t.reshape(-1, 6)
        E = s_t.shape[0]
        if E != self.num_envs:
            raise ValueError(f"optimizer configured for {self.num_envs} envs, got {E} states")
        host = self._attributes(E)                       # uploaded only when a value has changed
        if self._attr_host is None or not all(np.array_equal(a, b) for a, b in zip(host, self._attr_host)):
            self._attr_host, self._attr_dev = host, tuple(eng.tensor(x) for x in host)
        u = self._fused_call(s_t, *self._attr_dev, self._previous_input, None)
        self._previous_input = u                         # (the step reads its env's entry before it writes it)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": u.cpu().numpy(), "J_logged": self._S.cpu().numpy(),
                                   "u_logged": self._plan.cpu().numpy()}
        return self._result(u.clone() if as_tensor else u, single, as_tensor)

    def _result(self, u, single, as_tensor):
        """The controls u[E] (device tensor, or already on the host) as the caller wants them: the tensor itself, or a host
        array of its own, [1] for a [6] state and [E,1] for [E,6]."""
        if as_tensor:
            return u
        q = u if isinstance(u, np.ndarray) else u.cpu().numpy()
        E = q.shape[0]
        return q[:1].copy() if single else q.reshape(E, 1).copy()
