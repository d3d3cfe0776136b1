"""optimizer_mppi — the optimizer seam on the fused HIP path (cpmppi_step).

Constructor keyword arguments are the keys of ``config_optimizers.yml:87-97`` (section ``mppi``) plus the objects
``controller_mpc.configure`` passes to every optimizer (``predictor, cost_function, control_limits,
computation_library, optimizer_logging, calculate_optimal_trajectory``) — SURVEY.md §8(b).  The absent upstream
``Control_Toolkit.Optimizers.optimizer_mppi`` fixes neither horizon aggregation, shift, clipping nor which ``u`` enters
the correction term (§8c u1-u5); they are explicit options here (defaults = the recalled upstream behaviour; the
in-tree legacy behaviour is ``configs.legacy_mppi_config``).

Differences from a drop-in that only replaced the arithmetic: ``num_envs`` independent problem instances are stepped
in ONE launch (``step`` accepts ``s[6]`` or ``s[E,6]``), and perturbations come from a counter-based device RNG unless
``noise="sfc64"`` asks for numpy's SFC64 stream (bit-identical knots to the reference's sampler for a given seed).
"""
import numpy as np
import torch

from ._optimizer_base import _OptimizerBase, _vec, is_gru_specification
from .sampling import SAMPLING_TYPES, sample_delta_u_sfc64, sample_knots_sfc64

# cost plugins with a control-change-rate term against the control applied last (Q_ccrc, CartPole/__init__.py:517-518)
PREVIOUS_INPUT_COSTS = ("quadratic_boundary_grad", "quadratic_boundary", "quadratic_boundary_nonconvex")


class optimizer_mppi(_OptimizerBase):
    optimizer_name = "mppi"
    _cost_name_attributes = ("cost_name", "cost_function_name")
    _unknown_predictor = "built predictors: ODE_v0, ODE and GRU-6IN-32H1-32H2-5OUT-*"

    def __init__(self, predictor=None, cost_function=None, control_limits=None, computation_library=None, seed=None,
                 cc_weight=1.0, R=1.0, LBD=100.0, mpc_horizon=35, num_rollouts=3500, NU=1000.0, SQRTRHOINV=0.03,
                 period_interpolation_inducing_points=10, optimizer_logging=False, calculate_optimal_trajectory=False,
                 mpc_timestep=0.02, num_envs=1, noise="philox", cost_function_specification=None, cost_weights=None,
                 horizon_reduce="sum", control_mode="clip", shift_mode="repeat_last", correction_u="u_run",
                 math_mode="fast", intermediate_steps=10, phys=None, device=0, variable_parameters=None, gru_model=None,
                 SAMPLING_TYPE="interpolated", predictor_type="ODE_v0", per_env_pole_mass=False, **kwargs):
        self.predictor, self.cost_function = predictor, cost_function
        self.lib = computation_library
        if noise not in ("philox", "sfc64"):
            raise ValueError("noise must be 'philox' (device RNG) or 'sfc64' (numpy stream, reference-identical knots)")
        self.noise = noise
        # config_controllers.yml:28 (mppi-cartpole SAMPLING_TYPE).  The device sampler implements "interpolated"; the other
        # modes exist on numpy's SFC64 stream (sampling.sample_delta_u_sfc64), i.e. with noise="sfc64"
        if SAMPLING_TYPE not in SAMPLING_TYPES:
            raise ValueError(f"SAMPLING_TYPE must be one of {SAMPLING_TYPES}")
        if SAMPLING_TYPE != "interpolated" and noise != "sfc64":
            raise ValueError(f"SAMPLING_TYPE={SAMPLING_TYPE!r} is built on the numpy SFC64 stream only: pass noise='sfc64'")
        self.sampling_type = SAMPLING_TYPE
        super().__init__(cost_function, control_limits, seed, num_envs, cost_function_specification, cost_weights,
                         variable_parameters, phys, device, optimizer_logging, mpc_horizon, mpc_timestep, num_rollouts,
                         intermediate_steps, cc_weight=cc_weight, R=R, LBD=LBD, NU=NU, SQRTRHOINV=SQRTRHOINV,
                         period_interpolation_inducing_points=int(period_interpolation_inducing_points),
                         horizon_reduce=horizon_reduce, control_mode=control_mode, shift_mode=shift_mode,
                         correction_u=correction_u, math_mode=math_mode, predictor_type=predictor_type,
                         per_env_pole_mass=bool(per_env_pole_mass), gru_model=gru_model)
        self.calculate_optimal_trajectory = calculate_optimal_trajectory
        self.optimal_trajectory = None
        self.u_nom = None
        self.step_counter = 0
        self._hblock = self._hview = self._dblock = self._h2d_done = self._hq = self._q_done = None
        self._prepared = self._prepared_key = None     # pinned staging of the host seam
        self._fast = None                              # single-env host call: preallocated arrays + argument objects

    # ------------------------------------------------------------------
    def configure(self, dt=None, predictor_specification=None, num_envs=None, **kwargs):
        # (a GRU specification leaves the ODE integrator of the constructor alone: the network runs inside the fused kernel)
        self._configure_problem(dt, None if is_gru_specification(predictor_specification) else predictor_specification, num_envs)
        neural = self._gru_selected(predictor_specification)
        self.engine = self._new_engine()
        E, N, H = self.num_envs, self.num_rollouts, self.mpc_horizon
        self._attach_gru(neural)
        self.u_nom = self.engine.zeros(E, H)
        self._Q = self.engine.zeros(E)
        self._Q_host = None
        self.S = self.engine.empty(E, N) if self.optimizer_logging else None
        self._rng = np.random.Generator(np.random.SFC64(self.seed))
        self.optimizer_reset()

    @property
    def Q(self):
        """Device tensor [E]: the controls chosen by the last step.  After a host-state step (cpmppi_step_host delivers
        them to the host only) it is refreshed from that host copy on first use."""
        if self._Q_host is not None:
            self._Q.copy_(torch.from_numpy(self._Q_host))
            self._Q_host = None
        return self._Q

    @Q.setter
    def Q(self, value):
        self._Q, self._Q_host = value, None

    def optimizer_reset(self):
        """u_nom = midpoint of the control limits; restart the noise stream."""
        if self.u_nom is not None:
            self.u_nom.fill_(0.5 * (self.action_low + self.action_high))
        self._reset_memory()
        self.step_counter = 0
        self._rng = np.random.Generator(np.random.SFC64(self.seed))

    # ------------------------------------------------------------------
    def _upload(self, s_np, E):
        """[E,6] host state + per-env attributes -> device views of one block uploaded with one asynchronous copy."""
        if self._hblock is None or self._hblock.numel() != 9 * E:
            self._hblock = torch.empty(9 * E, dtype=torch.float32).pin_memory()
            self._hview = self._hblock.numpy()
            self._dblock = torch.empty(9 * E, dtype=torch.float32, device=self.u_nom.device)
            self._h2d_done = torch.cuda.Event()
        else:
            self._h2d_done.synchronize()                      # (the previous upload has left the pinned block)
        hv = self._hview
        hv[:6 * E] = s_np.reshape(-1)
        hv[6 * E:7 * E], hv[7 * E:8 * E], hv[8 * E:9 * E] = self._attributes(E)
        self._dblock.copy_(self._hblock, non_blocking=True)
        self._h2d_done.record()
        d = self._dblock
        return d[:6 * E].view(E, 6), d[6 * E:7 * E], d[7 * E:8 * E], d[8 * E:9 * E]

    def _step_host_single(self, s):
        """One env, state on the host: the call `Q = controller.step(s, time, updated_attributes)` makes once per control
        period (CartPole/__init__.py:509-520).  Everything that does not change from call to call is built once - the
        six-float state buffer, the three one-element attribute arrays, the result, their ctypes pointers - so that the
        Python side of a control step is a handful of scalar stores and one foreign call (~4 us instead of ~10)."""
        f = self._fast
        if f is None:
            import ctypes as C
            eng = self.engine
            f = self._fast = {"s": np.zeros((1, 6), np.float32), "tp": np.zeros(1, np.float32), "te": np.ones(1, np.float32),
                              "L": np.full(1, self.phys.L, np.float32), "q": np.zeros(1, np.float32),
                              "last": [self, self, self], "call": eng.lib.cpmppi_step_host, "h": eng._h,
                              "u": C.c_void_p(self.u_nom.data_ptr()), "u_ptr": self.u_nom.data_ptr(), "stream": eng._stream}
            for k in ("s", "tp", "te", "L", "q"):
                f["p_" + k] = C.c_void_p(f[k].ctypes.data)
        if self.u_nom.data_ptr() != f["u_ptr"]:                # (the plan tensor was replaced)
            self._fast = None
            return self._step_host_single(s)
        sv = f["s"]
        try:
            sv[0] = s                                           # [6] (or [1, 6]) of anything numpy can read
        except ValueError:
            sv[0] = np.asarray(s, dtype=np.float32).reshape(6)
        vp, last = self.variable_parameters, f["last"]
        for i, (name, key) in enumerate((("target_position", "tp"), ("target_equilibrium", "te"), ("L", "L"))):
            x = getattr(vp, name, None)
            if isinstance(x, (float, int, np.floating)):        # immutable: the same object as last time = the same value
                if x is last[i]:
                    continue
                last[i] = x
                f[key][0] = x
            elif x is not None:                                 # arrays / tensors may be assigned in place: converted every time
                last[i] = None
                f[key][0] = np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float32).reshape(-1)[0]
        rc = f["call"](f["h"], 1, f["p_s"], f["p_tp"], f["p_te"], f["p_L"], f["u"], self.seed, self.step_counter, 0, f["p_q"],
                       f["stream"]())
        if rc != 0:
            self.engine._check(rc)
        q = f["q"].copy()
        self._Q_host = q
        self.step_counter += 1
        return q if np.ndim(s) == 1 else q.reshape(1, 1)

    def step(self, s, time=None, as_tensor=False):
        """s[6] (one env) or s[E,6] -> first control of the updated nominal sequence, shape [1] or [E,1]."""
        if self.engine is None:
            self.configure()
        eng = self.engine
        if self.cfg.predictor_type == "ODE":
            eng.apply_pole_mass_of(self.variable_parameters, **self._mass_rows)      # (predictors_customization.py:55-58)
        host_state = not hasattr(s, "is_cuda")
        if (host_state and self.u_nom.is_cuda and self.noise == "philox" and self.h is None and not as_tensor
                and not self.optimizer_logging and not self.calculate_optimal_trajectory
                and self.cfg.cost_function_specification not in PREVIOUS_INPUT_COSTS):
            # the simulator's call (CartPole/__init__.py:509-520) in its plain form: host state in, host Q out, in-kernel
            # noise - ONE library call (cpmppi_step_host: staging, launch, the controls delivered into pinned memory)
            if self.num_envs == 1:
                return self._step_host_single(s)
            s_np = np.ascontiguousarray(np.asarray(s, dtype=np.float32))
            single = s_np.ndim == 1
            s_np = s_np.reshape(-1, 6)
            E = s_np.shape[0]
            if E != self.num_envs:
                raise ValueError(f"optimizer configured for {self.num_envs} envs, got {E} states")
            tp, te, L = self._attributes(E)
            q = np.empty(E, dtype=np.float32)
            eng.step_host(s_np, self.u_nom, tp, te, L, self.seed, self.step_counter, q)
            self._Q_host = q
            self.step_counter += 1
            return q[:1] if single else q.reshape(E, 1)
        if host_state and self.u_nom.is_cuda:                 # (a CPU test double of the engine takes the plain path below)
            # the simulator's call (CartPole/__init__.py:509-520): state and attributes live on the host.  They go up as ONE
            # pinned block in ONE asynchronous copy (state, target_position, target_equilibrium, L: four separate pageable
            # uploads cost ~50 us per control step, more than the rollout kernel's share for small problems)
            s_np = np.asarray(s, dtype=np.float32)
            single = s_np.ndim == 1
            s_np = s_np.reshape(-1, 6)
            E = s_np.shape[0]
            if E != self.num_envs:
                raise ValueError(f"optimizer configured for {self.num_envs} envs, got {E} states")
            s_t, tp, te, L = self._upload(s_np, E)
        else:
            s_t, single, E, tp, te, L = self._begin_step(s)    # (its own pole-mass call finds the value unchanged)
        kw = {}
        if self.noise == "sfc64" and self.sampling_type != "interpolated":
            kw["delta_u"] = sample_delta_u_sfc64(self._rng, E, self.num_rollouts, self.mpc_horizon, self.cfg.sigma,
                                                 self.sampling_type)
        elif self.noise == "sfc64":
            kw["knots"] = sample_knots_sfc64(self._rng, E, self.num_rollouts, self.cfg)
        else:
            kw.update(seed=self.seed, offset=self.step_counter)
        if self.h is not None:
            kw.update(predictor="GRU", h0=self.h)
        # the control applied last, which the simulator hands over as "Q_applied_-1" / "Q_ccrc" (CartPole/__init__.py:517-518):
        # the previous_input of the control-change-rate term of quadratic_boundary_grad
        vp = self.variable_parameters
        prev = getattr(vp, "Q_applied_-1", None)
        if prev is None:
            prev = getattr(vp, "Q_ccrc", None)
        if prev is not None and self.cfg.cost_function_specification in PREVIOUS_INPUT_COSTS:
            kw["previous_input"] = _vec(prev, E, 0.0)
        if host_state and self.u_nom.is_cuda and set(kw) == {"seed", "offset"}:
            # the simulator's call with in-kernel noise: every pointer is the same from call to call (staging block, u_nom,
            # Q), so the argument block is built once and only the Philox step counter changes
            key = (id(eng), s_t.data_ptr(), self.u_nom.data_ptr(), self.Q.data_ptr(), None if self.S is None else self.S.data_ptr(),
                   E, self.seed)
            if self._prepared is None or self._prepared_key != key:
                self._prepared = eng.prepare_step(s_t, self.u_nom, tp, te, L=L, Q_out=self.Q, S_out=self.S, **kw)
                self._prepared_key = key
            self._prepared.run(offset=self.step_counter)
        else:
            eng.step(s_t, self.u_nom, tp, te, L=L, Q_out=self.Q, S_out=self.S, **kw)
        self.step_counter += 1
        self._advance_memory(s_t, self.Q)
        if self.optimizer_logging:
            self.logging_values = {"Q_logged": self.Q.cpu().numpy(), "J_logged": self.S.cpu().numpy(),
                                   "u_logged": self.u_nom.cpu().numpy()}
        if self.calculate_optimal_trajectory:
            self.optimal_trajectory = eng.predict(s_t, self.u_nom, L=L).cpu().numpy()
        if as_tensor or not self.Q.is_cuda:
            return self._result(self.Q, single, as_tensor)
        # the single D2H copy float(controller.step(...)) forces (CartPole/__init__.py:509): into a pinned buffer, then wait
        if self._hq is None or self._hq.numel() != E:
            self._hq = torch.empty(E, dtype=torch.float32).pin_memory()
            self._q_done = torch.cuda.Event()
        self._hq.copy_(self.Q, non_blocking=True)
        self._q_done.record()
        self._q_done.synchronize()
        q = self._hq.numpy().copy()
        return q[:1] if single else q.reshape(E, 1)
