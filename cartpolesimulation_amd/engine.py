"""MPPIEngine — thin host wrapper around one libcpmppi handle.  PyTorch-ROCm is used only for device buffers and streams.

All array arguments are float32 ROCm tensors (numpy arrays are uploaded); every call is enqueued on torch's current
stream of the engine's device, so ``torch.cuda.Event`` brackets the kernels correctly.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as _L
from .configs import MPPIConfig, PhysicalParameters, build_c_config, cost_vector


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def is_dense(t, dtype=torch.float32, tail=None):
    """The half of the argument check that needs no device: `t` is a contiguous `dtype` tensor [rows, *tail] (tail None: of any
    shape)."""
    return (torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous()
            and (tail is None or tuple(t.shape[1:]) == tuple(tail)))


def device_tensor(name, t, dtype=torch.float32, tail=None, note=""):
    """`t`, or ValueError: "<name> must be a contiguous float32 ROCm tensor [rows, 6]<note>" for dtype float32 and tail (6,)."""
    if not (is_dense(t, dtype, tail) and t.is_cuda):
        shape = "" if tail is None else " [rows%s]" % "".join(f", {x}" for x in tail)
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} ROCm tensor{shape}{note}")
    return t


def _same_shape(**tensors):
    """adam_step / sgd_step: every argument a contiguous float32 tensor of the first one's shape."""
    first = next(iter(tensors.values()))
    if not all(is_dense(t) and t.shape == first.shape for t in tensors.values()):
        raise ValueError(f"{', '.join(tensors)} must be contiguous float32 device tensors of one shape [E,N,H]")


_IN_PLACE = " (it is updated in place)"


def gpu_device(device):
    """``device`` (an index, a name or a torch.device) as the torch.device of a GPU; refused where PyTorch-ROCm sees none."""
    if not torch.cuda.is_available():
        raise RuntimeError("cartpolesimulation_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU fallback.")
    return torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)


class MPPIEngine:
    # what the methods read and no constructor argument sets (here, so that from_handle and a handle-less stand-in have them too)
    _h, _borrowed = None, False                                 # from_handle: somebody else destroys the handle
    _fixed_stream = _fixed_stream_obj = None                    # use_stream: the raw handle / the torch stream (keeps it alive)
    _m_rows = _m_rows_own = None                                # set_pole_mass_rows: the registered tensor / the engine's own buffer
    _m_pole_obj = None                                          # apply_pole_mass_of: the scalar object last applied
    has_gru = False                                             # set_gru: a network is attached

    def __init__(self, E, mppi: MPPIConfig = None, phys: PhysicalParameters = None, device=0):
        self._init_common(E, mppi, phys, device)
        self._h = C.c_void_p()
        rc = self.lib.cpmppi_create(C.byref(self._cfg), self.device.index, C.byref(self._h))
        if rc != 0:
            raise _L.CpmppiError(rc, self.lib.cpmppi_last_error(None).decode())

    @classmethod
    def from_handle(cls, handle, E, mppi: MPPIConfig = None, phys: PhysicalParameters = None, device=0):
        """An engine over a handle somebody else owns (an env group's: pipeline.EnvGroups / cpmppi_groups_create); `close()` then
        only forgets it."""
        self = cls.__new__(cls)
        self._init_common(E, mppi, phys, device)
        self._h = C.c_void_p(handle)
        self._borrowed = True
        return self

    def _init_common(self, E, mppi, phys, device):
        self.device = gpu_device(device)
        self.lib = _L.load()
        self.mppi = mppi or MPPIConfig()
        self.phys = phys or PhysicalParameters()
        self.E, self.N, self.H = int(E), int(self.mppi.num_rollouts), int(self.mppi.mpc_horizon)
        self.P = self.mppi.num_knots
        self._cfg = build_c_config(self.E, self.mppi, self.phys)
        self._m_pole = float(np.float32(self.phys.m_pole))

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if self._h is not None and self._h.value:
            if not self._borrowed:
                self.lib.cpmppi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise _L.CpmppiError(rc, self.lib.cpmppi_last_error(self._h).decode())

    def use_stream(self, stream):
        """Enqueue every later call of this engine on `stream` (a torch.cuda.Stream; None = torch's current stream again) -
        env groups that run side by side each keep their own stream (pipeline.py) without a stream context per call.
        -> the stream it was fixed to before (None: none), for a caller that puts it back."""
        previous = self._fixed_stream_obj
        self._fixed_stream = None if stream is None else C.c_void_p(stream.cuda_stream)
        self._fixed_stream_obj = stream
        return previous

    def launch_stream(self):
        """The torch stream this engine's launches go to: the fixed one of `use_stream`, else the device's current stream."""
        return self._fixed_stream_obj if self._fixed_stream_obj is not None else torch.cuda.current_stream(self.device)

    def _stream(self):
        if self._fixed_stream is not None:
            return self._fixed_stream
        # the caller's current stream as a raw handle (torch.cuda.current_stream() builds a Stream object: ~5 us per call,
        # three calls per control step at the host seam)
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return C.c_void_p(raw(self.device.index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def tensor(self, x, shape=None):
        """float32 contiguous tensor on the engine's device (uploads numpy / python data)."""
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        elif x.dtype == torch.float32 and x.device == self.device and x.is_contiguous():
            return x if shape is None else x.reshape(shape)      # (the common case inside optimizer loops: nothing to convert)
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None:
            x = x.reshape(shape)
        return x

    def _as_BH(self, Q):
        """Control sequences [B,H], also accepted as [B,H,1] (the reference's predictor signature)."""
        Q = self.tensor(Q)
        return Q[:, :, 0].contiguous() if Q.dim() == 3 else Q

    def _predict_inputs(self, s0, Q):
        """predict / gru_predict: -> (s0 [B,6] - one state [6] is given to every row -, Q [B,H], B, H)."""
        Q = self._as_BH(Q)
        B, H = Q.shape
        s0 = self.tensor(s0)
        if s0.dim() == 1:
            s0 = s0.unsqueeze(0).expand(B, 6).contiguous()
        return s0, Q, B, H

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ seams
    def predict(self, s0, Q, L=None, horizon=None):
        """predict_core: s0[B,6], Q[B,H] -> traj[B,H+1,6]."""
        s0, Q, B, H = self._predict_inputs(s0, Q)
        if s0.shape != (B, 6):
            raise ValueError(f"s0 must be [{B},6] (or [6]), got {tuple(s0.shape)}")
        if L is not None:
            L = self.tensor(L).reshape(-1)
            if L.numel() == 1:
                L = L.expand(B).contiguous()
        traj = self.empty(B, H + 1, 6)
        self._check(self.lib.cpmppi_predict(self._h, B, H, _ptr(s0), _ptr(Q), _ptr(L), _ptr(traj), self._stream()))
        return traj

    def trajectory_cost(self, traj, inputs, target_position, target_equilibrium, u_nom=None, u_prev=None,
                        want=("stage", "terminal", "total")):
        traj = self.tensor(traj)
        inputs = self._as_BH(inputs)
        B, H = inputs.shape
        if traj.shape != (B, H + 1, 6):
            raise ValueError(f"traj must be [{B},{H + 1},6], got {tuple(traj.shape)}")
        stage = self.empty(B, H) if "stage" in want else None
        term = self.empty(B) if "terminal" in want else None
        total = self.empty(B) if "total" in want else None
        u_nom, u_prev = self.tensor(u_nom), self.tensor(u_prev)
        self._check(self.lib.cpmppi_trajectory_cost(self._h, B, H, _ptr(traj), _ptr(inputs), float(target_position),
                                                    float(target_equilibrium), _ptr(u_nom), _ptr(u_prev), _ptr(stage),
                                                    _ptr(term), _ptr(total), self._stream()))
        return stage, term, total

    def set_cost(self, name, overrides=None):
        cost_id, w = cost_vector(name, overrides)
        arr = (C.c_float * len(w))(*w)
        self._check(self.lib.cpmppi_set_cost_weights(self._h, cost_id, arr, len(w)))

    def apply_pole_mass_of(self, variable_parameters, rows=None):
        """predictor_ODE takes the pole's mass from variable_parameters at every step (predictors_customization.py:55-58;
        the simulator sends 'm_pole' with every controller.step, CartPole/__init__.py:516); predictor_ODE_v0 does not.
        With ``MPPIConfig.per_env_pole_mass`` an m_pole that differs between rows is computed with per row (set_pole_mass_rows;
        ``rows``: how many the caller's next launch has - the predictors' batch, the optimizers' num_envs), as the reference's
        predictor broadcasts it; a scalar or a uniform host array stays the handle's one mass and clears the rows."""
        if self.mppi.predictor_type != "ODE":
            return
        m = getattr(variable_parameters, "m_pole", None)
        if m is None:
            return
        if isinstance(m, (float, int, np.floating)):            # immutable: the same object as last time means the same value
            if m is self._m_pole_obj:
                return
            self._m_pole_obj = m                                # (arrays / tensors may be assigned in place: converted every time)
        per_row = self.mppi.per_env_pole_mass
        if per_row and torch.is_tensor(m) and m.is_cuda and m.numel() > 1:
            self._m_pole_obj = None
            return self.set_pole_mass_rows(m, rows)             # (registered as it is: no copy, no look at its values)
        a = np.asarray(m.cpu() if hasattr(m, "cpu") else m, dtype=np.float32).reshape(-1)
        if a.size == 0 or not np.all(a == a[0]):
            if per_row and a.size:
                self._m_pole_obj = None
                return self.set_pole_mass_rows(a, rows)
            raise NotImplementedError(f"m_pole must be the same for every env of a handle (got {a[:4]}...); "
                                      "MPPIConfig(per_env_pole_mass=True) computes with a mass per row")
        if per_row:
            self.set_pole_mass_rows(None)
        self.set_pole_mass(float(a[0]))

    def set_pole_mass(self, m_pole):
        """The pole mass every later call computes with (predictor_ODE: variable_parameters.m_pole).  No-op when unchanged."""
        m = float(np.float32(m_pole))
        if m != self._m_pole:
            self._check(self.lib.cpmppi_set_pole_mass(self._h, m))
            self._m_pole = m

    def set_pole_mass_rows(self, m, rows=None):
        """cpmppi_set_pole_mass_rows: the pole mass predictor_ODE computes with PER ROW - per env for step / rollout_cost /
        rollout_cost_grad / step_host, per rollout for predict - wherever that call's L would be indexed.  ``None``: back to the
        handle's one mass (set_pole_mass).  A contiguous float32 tensor on the engine's device is registered AS IT IS - no copy, no
        host synchronisation; every later launch reads its values when it runs, so it may be rewritten in place (stream-ordered)
        and must outlive the launches; the engine keeps a reference.  Anything else (a host array, a list) is checked - finite,
        > 0 - uploaded into a buffer of the engine's own and registered.  ``rows``: the row count the caller's launches will have;
        an array of another length is refused here (the library refuses a launch with more rows than were registered)."""
        if m is None:
            if self._m_rows is not None:
                self._check(self.lib.cpmppi_set_pole_mass_rows(self._h, None, 0))
                self._m_rows = None
            return
        if self.mppi.predictor_type != "ODE":
            raise ValueError(f"a per-row pole mass is read by predictor_type 'ODE' only (this engine: {self.mppi.predictor_type!r}; "
                             "predictor_ODE_v0 never reads the attribute)")
        if rows is not None and int(np.prod(np.shape(m))) != int(rows):
            raise ValueError(f"m_pole has {int(np.prod(np.shape(m)))} entries, the call has {int(rows)} rows")
        if torch.is_tensor(m) and m.is_cuda:
            if not (m.dtype == torch.float32 and m.is_contiguous() and m.dim() == 1 and m.numel() > 0 and m.device == self.device):
                raise ValueError("m_pole rows on the device must be a contiguous float32 tensor [rows] on the engine's device")
            t = m
        else:
            a = np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=np.float32)
            if a.ndim != 1 or a.size == 0:
                raise ValueError(f"m_pole rows must be a vector [rows], got shape {a.shape}")
            if not (np.isfinite(a).all() and (a > 0).all()):
                raise ValueError("every pole mass must be a positive, finite number")
            own = self._m_rows_own
            if own is None or own.numel() != a.size:
                own = self._m_rows_own = self.empty(a.size)
            own.copy_(torch.from_numpy(np.ascontiguousarray(a)), non_blocking=False)
            t = own
        cur = self._m_rows
        if cur is None or cur.data_ptr() != t.data_ptr() or cur.numel() != t.numel():
            self._check(self.lib.cpmppi_set_pole_mass_rows(self._h, _ptr(t), t.numel()))
        self._m_rows = t

    def sample(self, seed, offset=0, env_offset=0, E=None, knots=True, delta_u=False):
        E = self.E if E is None else int(E)
        kn = self.empty(E, self.N, self.P) if knots else None
        du = self.empty(E, self.N, self.H) if delta_u else None
        self._check(self.lib.cpmppi_sample(self._h, E, int(seed), int(offset), int(env_offset), _ptr(kn), _ptr(du),
                                           self._stream()))
        return kn, du

    def tiled_empty(self, E=None):
        """An uninitialised perturbation buffer in the library's tiled layout (include/cpmppi.h) for E envs."""
        E = self.E if E is None else int(E)
        return torch.empty(int(self.lib.cpmppi_tiled_floats(self._h, E)), dtype=torch.float32, device=self.device)

    def sample_tiled(self, seed=0, offset=0, env_offset=0, E=None, knots=None, out=None):
        """a17 straight into the tiled layout: Philox knots, or caller ``knots`` [E,N,P] interpolated."""
        kn = None if knots is None else self.tensor(knots)
        if kn is not None and kn.dim() == 2:
            kn = kn.unsqueeze(0)
        E = (self.E if E is None else int(E)) if kn is None else kn.shape[0]
        out = self.tiled_empty(E) if out is None else out
        self._check(self.lib.cpmppi_sample_tiled(self._h, E, int(seed), int(offset), int(env_offset), _ptr(kn), _ptr(out),
                                                 self._stream()))
        return out

    def tile_delta_u(self, delta_u, out=None):
        """delta_u [E,N,H] (reference layout) -> the tiled layout."""
        du = self.tensor(delta_u)
        if du.dim() == 2:
            du = du.unsqueeze(0)
        E = du.shape[0]
        if du.shape != (E, self.N, self.H):
            raise ValueError(f"delta_u must be [E,{self.N},{self.H}], got {tuple(du.shape)}")
        out = self.tiled_empty(E) if out is None else out
        self._check(self.lib.cpmppi_tile_delta_u(self._h, E, _ptr(du), _ptr(out), self._stream()))
        return out

    def untile(self, tiled, E=None):
        """The tiled buffer viewed back as delta_u [E,N,H] (host-side index arithmetic; tests and debugging)."""
        E = self.E if E is None else int(E)
        G, Hq = (self.N + 63) // 64, (self.H + 3) // 4
        t = tiled.reshape(E, G, Hq, 64, 4).permute(0, 1, 3, 2, 4).reshape(E, G * 64, Hq * 4)
        return t[:, :self.N, :self.H].contiguous()

    def interpolate(self, knots):
        knots = self.tensor(knots)
        if knots.dim() == 2:
            knots = knots.unsqueeze(0)
        E = knots.shape[0]
        if knots.shape != (E, self.N, self.P):
            raise ValueError(f"knots must be [E,{self.N},{self.P}], got {tuple(knots.shape)}")
        du = self.empty(E, self.N, self.H)
        self._check(self.lib.cpmppi_interpolate(self._h, E, _ptr(knots), _ptr(du), self._stream()))
        return du

    def reward_weighted_average(self, S, delta_u):
        S, delta_u = self.tensor(S), self.tensor(delta_u)
        if S.dim() == 1:
            S, delta_u = S.unsqueeze(0), delta_u.unsqueeze(0)
        E = S.shape[0]
        if S.shape != (E, self.N) or delta_u.shape != (E, self.N, self.H):
            raise ValueError("S must be [E,N] and delta_u [E,N,H] for this engine's N, H")
        out = self.empty(E, self.H)
        self._check(self.lib.cpmppi_reward_weighted_average(self._h, E, _ptr(S), _ptr(delta_u), _ptr(out),
                                                            self._stream()))
        return out

    def plant_advance(self, s, Q, L=None, n_substeps=10, dt_sim=0.002, states_log=None, Q_log=None, row=0, row_dev=None):
        """In-place plant update of s[E,6] under held controls Q[E].  With ``states_log`` [T+1,E,6] / ``Q_log`` [T,E] the
        same launch records the control period: Q_log[row] = Q, states_log[row+1] = the advanced state; ``row_dev`` (an
        int64 device tensor: the step counter of ``step(offset_dev=...)``, already advanced) replaces ``row`` by its
        value - 1."""
        E = device_tensor("s", s, note=_IN_PLACE).shape[0]
        Q = self.tensor(Q).reshape(E)
        L = self.tensor(L).reshape(E) if L is not None else None
        if states_log is None and Q_log is None:
            self._check(self.lib.cpmppi_plant_advance(self._h, E, _ptr(s), _ptr(Q), _ptr(L), int(n_substeps),
                                                      float(dt_sim), self._stream()))
            return s
        for name, t, tail in (("states_log", states_log, (E, 6)), ("Q_log", Q_log, (E,))):
            if t is not None:
                device_tensor(name, t, tail=tail)
        # control periods the logs can take; the kernel itself refuses to write outside them (device counter case)
        log_rows = min(([states_log.shape[0] - 1] if states_log is not None else []) + ([Q_log.shape[0]] if Q_log is not None else []))
        if row_dev is None:
            if not 0 <= row < log_rows:
                raise IndexError(f"row {row} outside the logs")
        else:
            device_tensor("row_dev", row_dev, torch.int64)
        self._check(self.lib.cpmppi_plant_advance_record(self._h, E, _ptr(s), _ptr(Q), _ptr(L), int(n_substeps), float(dt_sim),
                                                         _ptr(states_log), _ptr(Q_log), int(max(log_rows, 0)), int(row),
                                                         _ptr(row_dev), self._stream()))
        return s

    def plant_step(self, s, Q, n_substeps, dt_sim=0.002, period=0, period_dev=None, period_steps=None, L=None, states_log=None,
                   dd_log=None, save_every=None, Q_log=None, target_position_table=None, target_equilibrium_table=None,
                   L_table=None, sched_stride=1, target_position_out=None, target_equilibrium_out=None, L_out=None, m_pole=None,
                   m_pole_table=None, L_controller_table=None, Q_disturbance_table=None, Q_bias=0.0, Q_applied_out=None,
                   s_measured=None, state_history=None, latency=0.0, measurement_noise_table=None, angle_offset_table=None,
                   informed_table=None, _prepare=False):
        """cpmppi_plant_step: one control period of the simulated cartpoles with the experiment schedule and the recording in the
        same launch (include/cpmppi.h).  ``s`` [E,6] in place under held ``Q`` [E]; logs ``states_log`` [rows,E,6], ``dd_log``
        [rows,E,2], ``Q_log`` [periods,E]; schedule tables [sched_rows,E] sampled every ``sched_stride`` simulation steps; ``*_out``
        [E] receive the row the NEXT controller call reads.  ``n_substeps`` = 0 records only.  ``m_pole`` [E] / ``m_pole_table``
        [sched_rows,E]: the PLANT's pole mass (default: the config's); ``L_controller_table``: what ``L_out`` publishes instead of
        ``L_table`` (the pole length the controller is told, CartPole/controller_informer.py).  ``Q_disturbance_table`` [periods,E]
        + ``Q_bias``: the plant is driven by (Q + table[period]) + Q_bias (the simulator's additive control disturbance);
        ``Q_applied_out`` [E] receives that control (the next controller call's ``previous_input``).
        The measurement chain (CartPole.add_noise_and_latency): ``s_measured`` [E,6] receives what the next controller call sees -
        the state ``latency`` seconds back (``state_history`` [>= latency / dt_sim + 2, E, 6], zeros with cos = 1 before the run),
        plus ``measurement_noise_table`` [calls,E,4], plus ``angle_offset_table`` [sched_rows,E] float64 on the angle (taken out again
        where ``informed_table`` [sched_rows,E] uint8 says so; None = everywhere)."""
        E = device_tensor("s", s, note=_IN_PLACE).shape[0]

        def dev(name, t, tail, dtype=torch.float32):
            return None if t is None else device_tensor(name, t, dtype, tail)

        a = _L.cpmppi_plant_args()
        Q = self.tensor(Q).reshape(E)
        Lt = self.tensor(L).reshape(E) if L is not None else None
        a.E, a.s, a.Q, a.L = E, s.data_ptr(), Q.data_ptr(), (Lt.data_ptr() if Lt is not None else None)
        a.n_substeps, a.period_steps, a.dt_sim = int(n_substeps), int(period_steps if period_steps is not None else n_substeps), float(dt_sim)
        a.period = int(period)
        if period_dev is not None:
            a.period_dev = device_tensor("period_dev", period_dev, torch.int64).data_ptr()
        states_log, dd_log, Q_log = dev("states_log", states_log, (E, 6)), dev("dd_log", dd_log, (E, 2)), dev("Q_log", Q_log, (E,))
        rows = [t.shape[0] for t in (states_log, dd_log) if t is not None]
        a.states_log = states_log.data_ptr() if states_log is not None else None
        a.dd_log = dd_log.data_ptr() if dd_log is not None else None
        a.save_rows = min(rows) if rows else 0
        a.save_every = int(save_every) if save_every else 0
        if Q_log is not None:
            a.Q_log, a.ctrl_rows = Q_log.data_ptr(), Q_log.shape[0]
            if period_dev is None and not 0 <= int(period) < Q_log.shape[0]:
                raise IndexError(f"period {period} outside Q_log")
        tabs = [dev(n, t, (E,)) for n, t in (("target_position_table", target_position_table),
                                             ("target_equilibrium_table", target_equilibrium_table), ("L_table", L_table),
                                             ("m_pole_table", m_pole_table), ("L_controller_table", L_controller_table))]
        sched = [t.shape[0] for t in tabs if t is not None]
        if sched and min(sched) != max(sched):
            raise ValueError("the schedule tables must have the same number of rows")
        (a.target_position_table, a.target_equilibrium_table, a.L_table, a.m_pole_table,
         a.L_controller_table) = [t.data_ptr() if t is not None else None for t in tabs]
        qd = dev("Q_disturbance_table", Q_disturbance_table, (E,))
        if qd is not None:
            if Q_log is not None and qd.shape[0] != Q_log.shape[0]:
                raise ValueError("Q_disturbance_table and Q_log must have the same number of rows (one per controller call)")
            a.Q_disturbance_table, a.ctrl_rows, a.Q_bias = qd.data_ptr(), qd.shape[0], float(Q_bias)
        sm = dev("s_measured", s_measured, (6,))
        if sm is not None and sm.shape[0] != E:
            raise ValueError("s_measured must be [E,6]")
        hist = dev("state_history", state_history, (E, 6))
        nz = dev("measurement_noise_table", measurement_noise_table, (E, 4))
        off = dev("angle_offset_table", angle_offset_table, (E,), torch.float64)
        inf = dev("informed_table", informed_table, (E,), torch.uint8)
        if sm is not None:
            steps = float(latency) / float(dt_sim)
            a.latency_steps = int(steps)
            a.latency_frac = steps - int(steps)
            a.s_measured = sm.data_ptr()
            if hist is not None:
                a.state_history, a.history_len = hist.data_ptr(), hist.shape[0]
            if nz is not None:
                if Q_log is not None and nz.shape[0] != Q_log.shape[0]:
                    raise ValueError("measurement_noise_table and Q_log must have the same number of rows (one per controller call)")
                a.measurement_noise_table, a.ctrl_rows = nz.data_ptr(), nz.shape[0]
            for t in (off, inf):
                if t is not None:
                    if sched and t.shape[0] != sched[0]:
                        raise ValueError("the schedule tables must have the same number of rows")
                    sched.append(t.shape[0])
            a.angle_offset_table = off.data_ptr() if off is not None else None
            a.informed_table = inf.data_ptr() if inf is not None else None
        qa = dev("Q_applied_out", Q_applied_out.reshape(E, 1) if Q_applied_out is not None else None, (1,))
        a.Q_applied_out = qa.data_ptr() if qa is not None else None
        mt = self.tensor(m_pole).reshape(E) if m_pole is not None else None
        a.m_pole = mt.data_ptr() if mt is not None else None
        a.sched_rows, a.sched_stride = (sched[0] if sched else 0), int(sched_stride)
        outs = [dev(n, t.reshape(E, 1) if t is not None else None, (1,)) for n, t in (
            ("target_position_out", target_position_out), ("target_equilibrium_out", target_equilibrium_out), ("L_out", L_out))]
        a.target_position_out, a.target_equilibrium_out, a.L_out = [t.data_ptr() if t is not None else None for t in outs]
        keep = (s, Q, Lt, mt, qd, qa, sm, hist, nz, off, inf, period_dev, states_log, dd_log, Q_log, tabs, outs)
        if _prepare:
            return PreparedPlantStep(self, a, keep)
        self._check(self.lib.cpmppi_plant_step(self._h, C.byref(a), self._stream()))
        del keep
        return s

    def prepare_plant_step(self, *args, **kwargs):
        """The argument block of ``plant_step(...)`` built and validated ONCE (a closed loop calls it every control period with the
        same buffers): ``.run(period=..., n_substeps=...)`` only updates those two fields and enqueues the launch."""
        return self.plant_step(*args, _prepare=True, **kwargs)

    # ------------------------------------------------------------------ GRU predictor (BASELINE configs[4])
    GRU_KEYS = ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_out", "b_out")

    def set_gru(self, model):
        """Attach a GRU-6IN-32H1-32H2-5OUT model: dict of float32 arrays in the torch.nn.GRU layout
        (w_ih0[96,6], w_hh0[96,32], b_ih0[96], b_hh0[96], w_ih1[96,32], w_hh1, b_ih1, b_hh1, w_out[5,32], b_out[5]) and
        optional in_scale/in_shift[6], out_scale/out_shift[5]."""
        shapes = dict(w_ih0=(96, 6), w_hh0=(96, 32), b_ih0=(96,), b_hh0=(96,), w_ih1=(96, 32), w_hh1=(96, 32),
                      b_ih1=(96,), b_hh1=(96,), w_out=(5, 32), b_out=(5,), in_scale=(6,), in_shift=(6,),
                      out_scale=(5,), out_shift=(5,))
        keep = {}
        for k, shp in shapes.items():
            if k in model and model[k] is not None:
                a = np.ascontiguousarray(np.asarray(model[k].detach().cpu() if torch.is_tensor(model[k]) else model[k],
                                                    dtype=np.float32))
                if a.shape != shp:
                    raise ValueError(f"GRU weight {k} must have shape {shp}, got {a.shape}")
                keep[k] = a
            elif k in self.GRU_KEYS:
                raise ValueError(f"GRU weight {k} missing")
        fp = lambda k: keep[k].ctypes.data_as(C.POINTER(C.c_float)) if k in keep else None
        m = _L.cpmppi_gru_model()
        m.inputs, m.hidden, m.layers, m.outputs = 6, 32, 2, 5
        for l in range(2):
            m.w_ih[l], m.w_hh[l], m.b_ih[l], m.b_hh[l] = fp(f"w_ih{l}"), fp(f"w_hh{l}"), fp(f"b_ih{l}"), fp(f"b_hh{l}")
        m.w_out, m.b_out = fp("w_out"), fp("b_out")
        m.in_scale, m.in_shift, m.out_scale, m.out_shift = fp("in_scale"), fp("in_shift"), fp("out_scale"), fp("out_shift")
        self._check(self.lib.cpmppi_set_gru(self._h, C.byref(m)))
        self.has_gru = True

    def gru_predict(self, s0, Q, h0=None, return_hidden=False):
        """Neural predictor seam: s0[B,6] | [6], Q[B,H], h0[2,B,32] -> traj[B,H+1,6] (and final hidden [2,B,32])."""
        s0, Q, B, H = self._predict_inputs(s0, Q)
        h0 = self.tensor(h0, (2, B, 32)) if h0 is not None else None
        traj = self.empty(B, H + 1, 6)
        h_out = self.empty(2, B, 32) if return_hidden else None
        self._check(self.lib.cpmppi_gru_predict(self._h, B, H, _ptr(s0), _ptr(Q), _ptr(h0), _ptr(traj), _ptr(h_out),
                                                self._stream()))
        return (traj, h_out) if return_hidden else traj

    def gru_advance(self, s, Q, h):
        """cpmppi_gru_advance: each env's memory ``h`` [E,2,32] (the layout ``step(h0=...)`` reads) moved on IN PLACE by one cell
        step on the state seen ``s`` [E,6] and the control chosen ``Q`` [E] - the hand-over between two control periods
        (update_internal_state).  All three are contiguous float32 tensors on the device; one launch, nothing allocated, so the
        call can be captured.  -> ``h``."""
        E = device_tensor("h", h, tail=(2, 32), note=_IN_PLACE).shape[0]
        if device_tensor("s", s, tail=(6,)).shape[0] != E or device_tensor("Q", Q).shape != (E,):
            raise ValueError(f"s must be [{E},6] and Q [{E}] for h [{E},2,32]")
        if E == 0 or E > self.E:
            raise ValueError(f"h must be [0<E<={self.E},2,32], got {tuple(h.shape)}")
        self._check(self.lib.cpmppi_gru_advance(self._h, E, _ptr(s), _ptr(Q), _ptr(h), self._stream()))
        return h

    # ------------------------------------------------------------------ cost-only launch and CEM
    def _per_env(self, x, E):
        x = self.tensor(x).reshape(-1)
        return x.expand(E).contiguous() if x.numel() == 1 else x

    def _rollout_inputs(self, s0, inputs, target_position, target_equilibrium, L):
        """rollout_cost / rollout_cost_grad: -> (E, s0 [E,6], inputs [E,N,H], target position, target equilibrium, L or None [E])."""
        inputs = self.tensor(inputs)
        E = inputs.shape[0]
        if inputs.shape != (E, self.N, self.H):
            raise ValueError(f"inputs must be [E,{self.N},{self.H}]")
        s0 = self.tensor(s0, (E, 6))
        tp, te = self._per_env(target_position, E), self._per_env(target_equilibrium, E)
        Lt = self._per_env(L, E) if L is not None else None
        return E, s0, inputs, tp, te, Lt

    def rollout_cost(self, s0, inputs, target_position, target_equilibrium, L=None, predictor="ODE_v0", h0=None):
        """inputs[E,N,H] -> S[E,N]: trajectory cost of given control sequences (no update).  ``predictor="GRU"`` rolls them out
        with the network of ``set_gru`` (cpmppi_rollout_cost_gru): ``h0`` [E,2,32] is each env's memory, shared by its rollouts
        (None: zeros); the network knows no pole length, so ``L`` is refused."""
        if predictor not in ("ODE_v0", "GRU"):
            raise ValueError("predictor must be 'ODE_v0' or 'GRU'")
        if predictor != "GRU" and h0 is not None:
            raise ValueError("h0 is the memory of the GRU predictor: pass predictor='GRU'")
        if predictor == "GRU":
            if L is not None:
                raise ValueError("predictor='GRU' takes no L: the network is the plant model")
        E, s0, inputs, tp, te, Lt = self._rollout_inputs(s0, inputs, target_position, target_equilibrium, L)
        S = self.empty(E, self.N)
        if predictor == "GRU":
            h0 = self.tensor(h0, (E, 2, 32)) if h0 is not None else None
            self._check(self.lib.cpmppi_rollout_cost_gru(self._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(h0),
                                                         _ptr(S), self._stream()))
            return S
        self._check(self.lib.cpmppi_rollout_cost(self._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(Lt), _ptr(S),
                                                 self._stream()))
        return S

    def rollout_cost_grad(self, s0, inputs, target_position, target_equilibrium, L=None, previous_input=None, predictor="ODE_v0",
                          h0=None):
        """inputs[E,N,H] -> (S[E,N], grad[E,N,H]): trajectory cost and its derivative w.r.t. the inputs.  ``predictor="GRU"``
        differentiates the rollout through the network of ``set_gru`` (cpmppi_rollout_cost_grad_gru): ``h0`` [E,2,32] is each
        env's memory (None: zeros); the network knows no pole length and its two costs read no previous input, so ``L`` and
        ``previous_input`` are refused."""
        if predictor not in ("ODE_v0", "GRU"):
            raise ValueError("predictor must be 'ODE_v0' or 'GRU'")
        if predictor != "GRU" and h0 is not None:
            raise ValueError("h0 is the memory of the GRU predictor: pass predictor='GRU'")
        if predictor == "GRU":
            if L is not None:
                raise ValueError("predictor='GRU' takes no L: the network is the plant model")
            if previous_input is not None:
                raise ValueError("predictor='GRU' takes no previous_input: neither of its costs (quadratic_boundary_grad_minimal, "
                                 "default) reads the control applied before")
        E, s0, inputs, tp, te, Lt = self._rollout_inputs(s0, inputs, target_position, target_equilibrium, L)
        S, grad = self.empty(E, self.N), self.empty(E, self.N, self.H)
        if predictor == "GRU":
            h0 = self.tensor(h0, (E, 2, 32)) if h0 is not None else None
            self._check(self.lib.cpmppi_rollout_cost_grad_gru(self._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(h0),
                                                              _ptr(S), _ptr(grad), self._stream()))
            return S, grad
        pi = self._per_env(previous_input, E) if previous_input is not None else None
        self._check(self.lib.cpmppi_rollout_cost_grad(self._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(Lt),
                                                      _ptr(pi), _ptr(S), _ptr(grad), self._stream()))
        return S, grad

    def adam_step(self, Q, grad, m, v, iteration, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0):
        """One Adam iteration on Q[E,N,H] in place (m, v: caller-owned moments, zero before iteration 1)."""
        _same_shape(Q=Q, grad=grad, m=m, v=v)
        self._check(self.lib.cpmppi_adam_step(self._h, Q.shape[0], _ptr(Q), _ptr(grad), _ptr(m), _ptr(v), int(iteration),
                                              float(learning_rate), float(beta1), float(beta2), float(epsilon),
                                              float(gradmax_clip), self._stream()))
        return Q

    def sgd_step(self, Q, grad, learning_rate, gradmax_clip=0.0):
        """Q <- clip(Q - lr * clip_by_norm(grad)) in place."""
        _same_shape(Q=Q, grad=grad)
        self._check(self.lib.cpmppi_sgd_step(self._h, Q.shape[0], _ptr(Q), _ptr(grad), float(learning_rate),
                                             float(gradmax_clip), self._stream()))
        return Q

    def cem_sample(self, mean, stdev, seed, offset=0, env_offset=0):
        mean, stdev = self.tensor(mean), self.tensor(stdev)
        E = mean.shape[0]
        Q = self.empty(E, self.N, self.H)
        self._check(self.lib.cpmppi_cem_sample(self._h, E, _ptr(mean), _ptr(stdev), int(seed), int(offset), int(env_offset),
                                               _ptr(Q), self._stream()))
        return Q

    def cem_gmm_sample(self, centres, stdev, seed, offset=0, env_offset=0, return_components=False):
        """centres [E,K,H], stdev [E,H] -> Q [E,N,H]: each rollout drawn around one (uniformly chosen) centre."""
        centres, stdev = self.tensor(centres), self.tensor(stdev)
        E, K = centres.shape[0], centres.shape[1]
        if centres.shape != (E, K, self.H) or stdev.shape != (E, self.H):
            raise ValueError(f"centres must be [E,K,{self.H}] and stdev [E,{self.H}]")
        Q = self.empty(E, self.N, self.H)
        comp = torch.empty(E, self.N, dtype=torch.int32, device=self.device) if return_components else None
        self._check(self.lib.cpmppi_cem_gmm_sample(self._h, E, _ptr(centres), K, _ptr(stdev), int(seed), int(offset),
                                                   int(env_offset), _ptr(Q), _ptr(comp), self._stream()))
        return (Q, comp) if return_components else Q

    def cem_update(self, S, Q, best_k, stdev_min, return_elites=False):
        S, Q = self.tensor(S), self.tensor(Q)
        E = S.shape[0]
        mean, stdev = self.empty(E, self.H), self.empty(E, self.H)
        elites = torch.empty(E, best_k, dtype=torch.int32, device=self.device) if return_elites else None
        self._check(self.lib.cpmppi_cem_update(self._h, E, _ptr(S), _ptr(Q), int(best_k), float(stdev_min), _ptr(mean),
                                               _ptr(stdev), _ptr(elites), self._stream()))
        return (mean, stdev, elites) if return_elites else (mean, stdev)

    def last_launch(self):
        """The rollout-kernel instantiation the most recent step launched (cpmppi_last_launch): dict of the template
        arguments plus `kernel`, its name as rocprofv3 prints it."""
        info = _L.cpmppi_launch_info()
        self._check(self.lib.cpmppi_last_launch(self._h, C.byref(info)))
        d = {n: int(getattr(info, n)) for n, _ in info._fields_}
        # (predictor "ODE" with a per-env pole mass registered runs the kernel's second compilation, rollout_cost_rows_kernel)
        rows = d["ode_predictor"] and self._m_rows is not None
        d["kernel"] = ("rollout_cost%s_kernel<%d, %s, %d, %d, %d%s>" % (
            "_rows" if rows else "", d["cost_id"], "true" if d["math_mode"] == _L.MATH_FAST else "false", (0, 1, 2, 3)[d["noise_kind"]],
            d["rollouts_per_lane"], d["build_variant"], ", PREDICTOR_ODE" if d["ode_predictor"] else ""))
        return d

    def set_profiling(self, enable=True, group=1):
        """HIP-event timing on the launch stream.  ``group`` = 1: every rollout kernel is bracketed; ``group`` = n > 1: one
        bracket around every n consecutive steps, reported as the average per step (an event costs ~5 us on the stream;
        group when small launches are timed by wall clock at the same time)."""
        self._check(self.lib.cpmppi_set_profiling(self._h, int(group) if enable else 0))

    def get_profile(self, max_steps=4096):
        """-> (rollout_ms[n], finalize_ms[n]) of the steps since the last call (synchronises on their events)."""
        a = (C.c_float * max_steps)()
        b = (C.c_float * max_steps)()
        n = C.c_uint32(0)
        self._check(self.lib.cpmppi_get_profile(self._h, a, b, max_steps, C.byref(n)))
        k = min(n.value, max_steps)
        return np.array(a[:k], dtype=np.float64), np.array(b[:k], dtype=np.float64)

    # ------------------------------------------------------------------ the fused rpgd / gradient-tf control step
    def rpgd_reserve(self, E=None):
        """cpmppi_rpgd_reserve: the workspace of ``rpgd_step`` for up to E envs (default: all).  After it the step never
        allocates - required before a step is captured into a graph."""
        self._check(self.lib.cpmppi_rpgd_reserve(self._h, self.E if E is None else int(E)))

    def rpgd_step(self, s0, Q, m, v, target_position, target_equilibrium, L=None, previous_input=None, *, iterations,
                  learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0, keep_k=None, resamp_per=0, shift=1,
                  distribution="normal", sample_mean=0.0, uniform_lo=0.0, uniform_hi=0.0, seed=0, draw_offset=0, env_offset=0,
                  count=0, adam_iteration=0, count_dev=None, Q_out=None, S_out=None, plan_out=None, order_out=None,
                  _prepare=False):
        """cpmppi_rpgd_step: one whole rpgd / gradient-tf control step on the plans ``Q`` and the Adam moments ``m``, ``v``
        [E,N,H], all three updated IN PLACE (include/cpmppi.h states the step).  ``count_dev``: int64 device scalar, the control
        steps taken so far - read by the kernel in place of ``count`` / ``adam_iteration`` / ``draw_offset`` and incremented
        after the step (graph replay).  -> (Q_out[E], S_out, plan_out, order_out), the last three as given (or None)."""
        E = device_tensor("Q", Q, tail=(self.N, self.H), note=_IN_PLACE).shape[0]
        if E > self.E:
            raise ValueError(f"Q must be [E<={self.E},{self.N},{self.H}], got {tuple(Q.shape)}")
        for name, t in (("m", m), ("v", v)):
            if device_tensor(name, t, tail=(self.N, self.H), note=_IN_PLACE).shape[0] != E:
                raise ValueError(f"{name} must have Q's shape")
        if distribution not in ("normal", "uniform"):
            raise ValueError(f"distribution={distribution!r}; expected 'normal' or 'uniform'")
        s0 = self.tensor(s0, (E, 6))
        tp, te = self._per_env(target_position, E), self._per_env(target_equilibrium, E)
        Lt = self._per_env(L, E) if L is not None else None
        prev = self._per_env(previous_input, E) if previous_input is not None else None
        if Q_out is None:
            Q_out = self.empty(E)
        for name, t, dtype, tail in (("Q_out", Q_out, torch.float32, ()), ("S_out", S_out, torch.float32, (self.N,)),
                                     ("plan_out", plan_out, torch.float32, (self.H,)), ("order_out", order_out, torch.int32, (self.N,))):
            if t is not None and device_tensor(name, t, dtype, tail).shape[0] != E:
                raise ValueError(f"{name} must have {E} rows")
        a = _L.cpmppi_rpgd_args()
        a.E = E
        a.s0, a.target_position, a.target_equilibrium = s0.data_ptr(), tp.data_ptr(), te.data_ptr()
        a.L = Lt.data_ptr() if Lt is not None else None
        a.previous_input = prev.data_ptr() if prev is not None else None
        a.Q, a.m, a.v = Q.data_ptr(), m.data_ptr(), v.data_ptr()
        a.iterations, a.adam_iteration = int(iterations), int(adam_iteration)
        a.learning_rate, a.beta1, a.beta2 = float(learning_rate), float(beta1), float(beta2)
        a.epsilon, a.gradmax_clip = float(epsilon), float(gradmax_clip)
        a.keep_k, a.resamp_per, a.shift = int(self.N if keep_k is None else keep_k), int(resamp_per), int(shift)
        a.distribution = _L.RPGD_UNIFORM if distribution == "uniform" else _L.RPGD_NORMAL
        a.sample_mean, a.uniform_lo, a.uniform_hi = float(sample_mean), float(uniform_lo), float(uniform_hi)
        a.seed, a.draw_offset, a.env_offset, a.count = int(seed), int(draw_offset), int(env_offset), int(count)
        if count_dev is not None:
            if device_tensor("count_dev", count_dev, torch.int64).numel() != 1:
                raise ValueError("count_dev must have one element")
            a.count_dev = count_dev.data_ptr()
        a.Q_out = Q_out.data_ptr()
        a.S_out = S_out.data_ptr() if S_out is not None else None
        a.plan_out = plan_out.data_ptr() if plan_out is not None else None
        a.order_out = order_out.data_ptr() if order_out is not None else None
        out = (Q_out, S_out, plan_out, order_out)
        if _prepare:
            return PreparedRpgdStep(self, a, (s0, tp, te, Lt, prev, Q, m, v, count_dev) + out, out)
        self._check(self.lib.cpmppi_rpgd_step(self._h, C.byref(a), self._stream()))
        return out

    def prepare_rpgd_step(self, *args, **kwargs):
        """The argument block of ``rpgd_step(...)`` built and validated ONCE: ``.run(count=, adam_iteration=, draw_offset=,
        iterations=)`` updates the host counters and enqueues the launch; with ``count_dev`` nothing changes between steps."""
        return self.rpgd_step(*args, _prepare=True, **kwargs)

    # ------------------------------------------------------------------ the fused CEM control step
    _CEM_REFINE = {None: _L.CEM_REFINE_NONE, "none": _L.CEM_REFINE_NONE, "sgd": _L.CEM_REFINE_SGD, "adam": _L.CEM_REFINE_ADAM}

    def _cem_refine(self, refine):
        if refine not in self._CEM_REFINE:
            raise ValueError(f"refine={refine!r}; expected None, 'sgd' or 'adam'")
        return self._CEM_REFINE[refine]

    def cem_reserve(self, E=None, refine=None):
        """cpmppi_cem_reserve: the workspace of ``cem_step`` for up to E envs (default: all), with the check-points, gradient and
        moments of a refining step (``refine`` 'sgd' / 'adam').  After it the step never allocates - required before a step is
        captured into a graph."""
        self._check(self.lib.cpmppi_cem_reserve(self._h, self.E if E is None else int(E), self._cem_refine(refine)))

    def cem_step(self, s0, mean, stdev, target_position, target_equilibrium, L=None, previous_input=None, *, iterations, best_k,
                 stdev_min, refine=None, learning_rate=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0, shift=1,
                 mean_fill=0.0, stdev_fill=0.0, seed=0, offset=0, env_offset=0, count_dev=None, Q_out=None, S_out=None,
                 plan_out=None, samples_out=None, order_out=None, _prepare=False):
        """cpmppi_cem_step: one whole control step of cem / cem-naive-grad (``refine='sgd'``) / cem-grad-bharadhwaj (``'adam'``) on
        the sampling distribution ``mean``, ``stdev`` [E,H], both updated IN PLACE (include/cpmppi.h states the step).
        ``count_dev``: int64 device scalar, the control steps taken so far - iteration i then draws at Philox offset
        ``offset + count * iterations + i``; incremented after the step (graph replay).
        -> (Q_out[E], S_out, plan_out, samples_out, order_out), the last four as given (or None)."""
        E = device_tensor("mean", mean, tail=(self.H,), note=_IN_PLACE).shape[0]
        if E > self.E:
            raise ValueError(f"mean must be [E<={self.E},{self.H}], got {tuple(mean.shape)}")
        if device_tensor("stdev", stdev, tail=(self.H,), note=_IN_PLACE).shape[0] != E:
            raise ValueError("stdev must have mean's shape")
        s0 = self.tensor(s0, (E, 6))
        tp, te = self._per_env(target_position, E), self._per_env(target_equilibrium, E)
        Lt = self._per_env(L, E) if L is not None else None
        prev = self._per_env(previous_input, E) if previous_input is not None else None
        if Q_out is None:
            Q_out = self.empty(E)
        for name, t, dtype, tail in (("Q_out", Q_out, torch.float32, ()), ("S_out", S_out, torch.float32, (self.N,)),
                                     ("plan_out", plan_out, torch.float32, (self.H,)),
                                     ("samples_out", samples_out, torch.float32, (self.N, self.H)),
                                     ("order_out", order_out, torch.int32, (self.N,))):
            if t is not None and device_tensor(name, t, dtype, tail).shape[0] != E:
                raise ValueError(f"{name} must have {E} rows")
        a = _L.cpmppi_cem_args()
        a.E = E
        a.s0, a.target_position, a.target_equilibrium = s0.data_ptr(), tp.data_ptr(), te.data_ptr()
        a.L = Lt.data_ptr() if Lt is not None else None
        a.previous_input = prev.data_ptr() if prev is not None else None
        a.mean, a.stdev = mean.data_ptr(), stdev.data_ptr()
        a.iterations, a.best_k, a.stdev_min, a.refine = int(iterations), int(best_k), float(stdev_min), self._cem_refine(refine)
        a.learning_rate, a.beta1, a.beta2 = float(learning_rate), float(beta1), float(beta2)
        a.epsilon, a.gradmax_clip = float(epsilon), float(gradmax_clip)
        a.shift, a.mean_fill, a.stdev_fill = int(shift), float(mean_fill), float(stdev_fill)
        a.seed, a.offset, a.env_offset = int(seed), int(offset), int(env_offset)
        if count_dev is not None:
            if device_tensor("count_dev", count_dev, torch.int64).numel() != 1:
                raise ValueError("count_dev must have one element")
            a.count_dev = count_dev.data_ptr()
        a.Q_out = Q_out.data_ptr()
        for name, t in (("S_out", S_out), ("plan_out", plan_out), ("samples_out", samples_out), ("order_out", order_out)):
            setattr(a, name, t.data_ptr() if t is not None else None)
        out = (Q_out, S_out, plan_out, samples_out, order_out)
        if _prepare:
            return PreparedCemStep(self, a, (s0, tp, te, Lt, prev, mean, stdev, count_dev) + out, out)
        self._check(self.lib.cpmppi_cem_step(self._h, C.byref(a), self._stream()))
        return out

    def prepare_cem_step(self, *args, **kwargs):
        """The argument block of ``cem_step(...)`` built and validated ONCE: ``.run(offset=, iterations=)`` updates the host's
        Philox offset and iteration count and enqueues the launch; with ``count_dev`` nothing changes between steps."""
        return self.cem_step(*args, _prepare=True, **kwargs)

    # ------------------------------------------------------------------ the fused hot path
    def step(self, s0, u_nom, target_position, target_equilibrium, L=None, delta_u=None, knots=None, seed=None,
             offset=0, env_offset=0, u_prev=None, Q_out=None, S_out=None, predictor="ODE_v0", h0=None,
             previous_input=None, offset_dev=None, delta_u_tiled=None, u_nom_out=None, gather_into=None, _prepare=False):
        """One MPPI optimizer step for E envs.  ``u_nom`` [E,H] is updated IN PLACE, or — with ``u_nom_out`` [E,H] — only
        read, the updated sequence going to ``u_nom_out`` (two buffers used alternately: shard.NativeGather).

        Exactly one noise source: ``delta_u`` [E,N,H], ``knots`` [E,N,P], ``seed`` (in-kernel Philox) or
        ``delta_u_tiled`` (a buffer from sample_tiled / tile_delta_u).
        ``gather_into`` [world, E*H] (needs a communicator, shard.NativeGather): cpmppi_step_gather — the step plus the
        all-gather of the sequences it writes, ordered on the device, nothing but the kernel on the launch stream.
        Returns (Q_out[E], S_out or None).
        """
        E = device_tensor("u_nom", u_nom, note=_IN_PLACE).shape[0]
        if u_nom.shape != (E, self.H) or E > self.E:
            raise ValueError(f"u_nom must be [E<={self.E},{self.H}], got {tuple(u_nom.shape)}")
        given = [x is not None for x in (delta_u, knots, seed, delta_u_tiled)]
        if sum(given) != 1:
            raise ValueError("give exactly one of delta_u, knots, seed, delta_u_tiled")
        a = _L.cpmppi_step_args()
        s0 = self.tensor(s0, (E, 6))
        tp, te = self._per_env(target_position, E), self._per_env(target_equilibrium, E)
        Lt = self._per_env(L, E) if L is not None else None
        noise = None
        if delta_u_tiled is not None:
            noise = device_tensor("delta_u_tiled", delta_u_tiled)
            if noise.numel() < int(self.lib.cpmppi_tiled_floats(self._h, E)):
                raise ValueError("delta_u_tiled must have cpmppi_tiled_floats(E) elements")
            a.noise_kind = _L.NOISE_DELTA_U_TILED
        elif delta_u is not None:
            noise = self.tensor(delta_u, (E, self.N, self.H))
            a.noise_kind = _L.NOISE_DELTA_U
        elif knots is not None:
            noise = self.tensor(knots, (E, self.N, self.P))
            a.noise_kind = _L.NOISE_KNOTS
        else:
            a.noise_kind = _L.NOISE_PHILOX
            a.seed, a.offset, a.env_offset = int(seed), int(offset), int(env_offset)
        u_prev = self.tensor(u_prev, (E, self.H)) if u_prev is not None else None
        if Q_out is None:
            Q_out = self.empty(E)
        a.E = E
        a.s0, a.u_nom, a.u_prev = s0.data_ptr(), u_nom.data_ptr(), (u_prev.data_ptr() if u_prev is not None else None)
        a.target_position, a.target_equilibrium = tp.data_ptr(), te.data_ptr()
        a.L = Lt.data_ptr() if Lt is not None else None
        a.noise = noise.data_ptr() if noise is not None else None
        a.Q_out = Q_out.data_ptr()
        a.S_out = S_out.data_ptr() if S_out is not None else None
        if predictor not in ("ODE_v0", "GRU"):
            raise ValueError("predictor must be 'ODE_v0' or 'GRU'")
        a.predictor = _L.PREDICTOR_GRU if predictor == "GRU" else _L.PREDICTOR_ODE_V0
        h0 = self.tensor(h0, (E, 2, 32)) if h0 is not None else None
        a.h0 = h0.data_ptr() if h0 is not None else None
        previous_input = self._per_env(previous_input, E) if previous_input is not None else None
        a.previous_input = previous_input.data_ptr() if previous_input is not None else None
        if u_nom_out is not None:
            if device_tensor("u_nom_out", u_nom_out).shape != u_nom.shape:
                raise ValueError("u_nom_out must have u_nom's shape")
            a.u_nom_out = u_nom_out.data_ptr()
        if offset_dev is not None:           # int64 device scalar: Philox step counter kept on the device (graph replay)
            if device_tensor("offset_dev", offset_dev, torch.int64).numel() != 1:
                raise ValueError("offset_dev must have one element")
            a.offset_dev = offset_dev.data_ptr()
        if _prepare:
            # every tensor the argument block points into is kept alive by the returned object
            return PreparedStep(self, a, (s0, u_nom, tp, te, Lt, noise, u_prev, Q_out, S_out, h0, previous_input, offset_dev, u_nom_out),
                                Q_out, S_out)
        if gather_into is not None:
            self._check(self.lib.cpmppi_step_gather(self._h, C.byref(a), gather_into.data_ptr(), self._stream()))
        else:
            self._check(self.lib.cpmppi_step(self._h, C.byref(a), self._stream()))
        # keep the temporaries alive until the launch is enqueued (stream-ordered frees are safe in torch's allocator)
        return Q_out, S_out

    def step_host(self, s0, u_nom, target_position, target_equilibrium, L, seed, offset, Q_host, env_offset=0):
        """cpmppi_step_host: float32 numpy arrays on the HOST for the state [E,6], the per-env vectors [E] and the result
        ``Q_host`` [E] (written in place); ``u_nom`` [E,H] stays on the device.  One library call per control step:
        staging, copy up, launch (in-kernel Philox noise), copy down, wait.  Synchronous."""
        E = u_nom.shape[0]
        for name, x, shape in (("s0", s0, (E, 6)), ("target_position", target_position, (E,)),
                               ("target_equilibrium", target_equilibrium, (E,)), ("Q_host", Q_host, (E,))) + \
                (() if L is None else (("L", L, (E,)),)):
            if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous and x.shape == shape):
                raise ValueError(f"{name} must be a C-contiguous float32 numpy array of shape {shape}")
        self._check(self.lib.cpmppi_step_host(self._h, E, s0.ctypes.data, target_position.ctypes.data, target_equilibrium.ctypes.data,
                                              None if L is None else L.ctypes.data, u_nom.data_ptr(), int(seed), int(offset),
                                              int(env_offset), Q_host.ctypes.data, self._stream()))
        return Q_host

    def prepare_step(self, *args, **kwargs):
        """The argument block of ``step(...)`` built and validated ONCE, for callers whose buffers persist from step to step
        (the host seam's staging block, a closed loop): ``.run(offset=...)`` only updates the Philox step counter and
        enqueues the launch - the per-call argument handling of ``step`` is ~10 us of a 55 us control step."""
        return self.step(*args, _prepare=True, **kwargs)


class PreparedPlantStep:
    """A validated cpmppi_plant_step argument block plus the tensors it points into (MPPIEngine.prepare_plant_step)."""

    def __init__(self, engine, args, keep):
        self.engine, self.args, self._keep = engine, args, keep

    def run(self, period=None, n_substeps=None):
        if period is not None:
            self.args.period = int(period)
        if n_substeps is not None:
            self.args.n_substeps = int(n_substeps)
        e = self.engine
        e._check(e.lib.cpmppi_plant_step(e._h, C.byref(self.args), e._stream()))


class PreparedStep:
    """A validated cpmppi_step argument block plus the tensors it points into (MPPIEngine.prepare_step)."""

    def __init__(self, engine, args, keep, Q_out, S_out):
        self.engine, self.args, self._keep, self.Q_out, self.S_out = engine, args, keep, Q_out, S_out

    def run(self, offset=None, gather_into=None):
        if offset is not None:
            self.args.offset = int(offset)
        e = self.engine
        if gather_into is not None:
            e._check(e.lib.cpmppi_step_gather(e._h, C.byref(self.args), gather_into.data_ptr(), e._stream()))
        else:
            e._check(e.lib.cpmppi_step(e._h, C.byref(self.args), e._stream()))
        return self.Q_out, self.S_out


class PreparedRpgdStep:
    """A validated cpmppi_rpgd_step argument block plus the tensors it points into (MPPIEngine.prepare_rpgd_step)."""

    def __init__(self, engine, args, keep, out):
        self.engine, self.args, self._keep, self.out = engine, args, keep, out

    def run(self, count=None, adam_iteration=None, draw_offset=None, iterations=None):
        a = self.args
        if count is not None:
            a.count = int(count)
        if adam_iteration is not None:
            a.adam_iteration = int(adam_iteration)
        if draw_offset is not None:
            a.draw_offset = int(draw_offset)
        if iterations is not None:
            a.iterations = int(iterations)
        e = self.engine
        e._check(e.lib.cpmppi_rpgd_step(e._h, C.byref(a), e._stream()))
        return self.out


class PreparedCemStep:
    """A validated cpmppi_cem_step argument block plus the tensors it points into (MPPIEngine.prepare_cem_step)."""

    def __init__(self, engine, args, keep, out):
        self.engine, self.args, self._keep, self.out = engine, args, keep, out

    def run(self, offset=None, iterations=None):
        a = self.args
        if offset is not None:
            a.offset = int(offset)
        if iterations is not None:
            a.iterations = int(iterations)
        e = self.engine
        e._check(e.lib.cpmppi_cem_step(e._h, C.byref(a), e._stream()))
        return self.out
