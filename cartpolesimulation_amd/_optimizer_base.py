"""_OptimizerBase — what optimizer_mppi, the CEM family and the gradient family share: the constructor block every optimizer
gets from ``controller_mpc.configure`` (control limits, seed, cost inherited from the cost-function object, MPPIConfig, engine
bookkeeping), the ``dt`` / ``num_envs`` / predictor part of ``configure``, and the per-step prologue (state -> [E,6], per-env
attributes) and epilogue (controls -> [1] / [E,1]).  The optimizers' own signatures, defaults and attributes are theirs.
"""
import os
import time as _time

import numpy as np

from .configs import MPPIConfig, PhysicalParameters, ode_predictor_type


def _vec(x, E, default):
    if x is None:
        return np.full(E, default, dtype=np.float32)
    x = np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float32).reshape(-1)
    return np.full(E, x[0], dtype=np.float32) if x.size == 1 else x.astype(np.float32)


class _OptimizerBase:
    _cost_name_attributes = ("cost_name",)           # where a cost-function object keeps its name
    _unknown_predictor = "this optimizer runs on the ODE_v0 and ODE predictors"

    def __init__(self, cost_function, control_limits, seed, num_envs, cost_function_specification, cost_weights,
                 variable_parameters, phys, device, optimizer_logging, mpc_horizon, mpc_timestep, num_rollouts,
                 intermediate_steps, **config):
        """``config``: the remaining MPPIConfig fields, which differ from optimizer to optimizer."""
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
        self._configure_problem(dt, predictor_specification, num_envs)
        self.engine = self._new_engine()
        self.optimizer_reset()

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

    def _result(self, u, single, as_tensor):
        """The controls u[E] (device tensor, or already on the host) as the caller wants them: the tensor itself, or a host
        array of its own, [1] for a [6] state and [E,1] for [E,6]."""
        if as_tensor:
            return u
        q = u if isinstance(u, np.ndarray) else u.cpu().numpy()
        E = q.shape[0]
        return q[:1].copy() if single else q.reshape(E, 1).copy()
