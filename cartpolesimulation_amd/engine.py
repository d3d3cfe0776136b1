"""MPPIEngine — thin host wrapper around one libcpmppi handle.  PyTorch-ROCm is used only for device buffers and streams.

All array arguments are float32 ROCm tensors (numpy arrays are uploaded); every call is enqueued on torch's current
stream of the engine's device, so ``torch.cuda.Event`` brackets the kernels correctly.
"""
import ctypes as C
import functools

import numpy as np
import torch

from . import _lib as _L
from .configs import MPPIConfig, PhysicalParameters, build_c_config, cost_vector
from .model_folder import DENSE_KEYS, DENSE_SHAPES, GRU_KEYS, GRU_SHAPES


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
# the caller's current stream as a raw handle (torch.cuda.current_stream() builds a Stream object: ~5 us per call, three calls per
# control step at the host seam)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _run_once(build):
    """An entry point of MPPIEngine from its builder ``_build_<name>``, whose signature and description are the entry point's:
    build the call, run it once, -> its result.  (``prepare_<name>`` is the other half: build, return the call.)"""
    @functools.wraps(build)
    def entry(self, *args, **kwargs):
        return build(self, *args, **kwargs).run()
    entry.__name__ = build.__name__[len("_build_"):]
    entry.__qualname__ = build.__qualname__.replace(build.__name__, entry.__name__)
    return entry


def _addr(t):
    """What a pointer field of an argument block is set to: the tensor's address, None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def _counter(name, t):
    """-> the address of `t`, a step counter kept on the device (int64, one element; graph replay); None for None."""
    if t is not None and device_tensor(name, t, torch.int64).numel() != 1:
        raise ValueError(f"{name} must have one element")
    return _addr(t)


def _is_gru(predictor):
    if predictor not in ("ODE_v0", "GRU"):
        raise ValueError("predictor must be 'ODE_v0' or 'GRU'")
    return predictor == "GRU"


def _rollout_is_gru(predictor, h0, L, previous_input=None):
    """rollout_cost / rollout_cost_grad: -> whether the network of set_gru rolls out; it alone has a memory, and it knows no pole
    length and (its two costs) no previous input."""
    gru = _is_gru(predictor)
    if not gru and h0 is not None:
        raise ValueError("h0 is the memory of the GRU predictor: pass predictor='GRU'")
    if gru and L is not None:
        raise ValueError("predictor='GRU' takes no L: the network is the plant model")
    if gru and previous_input is not None:
        raise ValueError("predictor='GRU' takes no previous_input: neither of its costs (quadratic_boundary_grad_minimal, "
                         "default) reads the control applied before")
    return gru


def _set_adam(a, learning_rate, beta1, beta2, epsilon, gradmax_clip):
    """The Adam / SGD hyper-parameters of a cpmppi_rpgd_args or cpmppi_cem_args block."""
    a.learning_rate, a.beta1, a.beta2 = float(learning_rate), float(beta1), float(beta2)
    a.epsilon, a.gradmax_clip = float(epsilon), float(gradmax_clip)


# plant_step's optional device tensors: field -> (shape after the leading axis, "E" standing for the env count; None: a vector
# [E]; dtype)
_PLANT_TENSORS = {
    "states_log": (("E", 6), torch.float32), "dd_log": (("E", 2), torch.float32), "Q_log": (("E",), torch.float32),
    "target_position_table": (("E",), torch.float32), "target_equilibrium_table": (("E",), torch.float32),
    "L_table": (("E",), torch.float32), "m_pole_table": (("E",), torch.float32), "L_controller_table": (("E",), torch.float32),
    "Q_disturbance_table": (("E",), torch.float32), "s_measured": ((6,), torch.float32),
    "state_history": (("E", 6), torch.float32), "measurement_noise_table": (("E", 4), torch.float32),
    "angle_offset_table": (("E",), torch.float64), "informed_table": (("E",), torch.uint8),
    "Q_applied_out": (None, torch.float32), "target_position_out": (None, torch.float32),
    "target_equilibrium_out": (None, torch.float32), "L_out": (None, torch.float32),
}


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
    _tuning = None                                              # set_tuning_rows: the registered tensor
    has_gru = False                                             # set_gru: a network is attached
    has_dense = False                                           # set_dense: the neural imitator is attached
    _train_keep = _fit_keep = _dense_keep = (None, None)        # gru_train_step / ode_fit_step / dense_train_step: the last two batches (_run_keeping)

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
        if _RAW_STREAM is not None:
            return C.c_void_p(_RAW_STREAM(self.device.index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def tensor(self, x, shape=None):
        """float32 contiguous tensor on the engine's device (uploads numpy / python data)."""
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        elif x.dtype == torch.float32 and x.device == self.device and x.is_contiguous():
            # (the common case inside optimizer loops: nothing to convert, and no view to make of a tensor of that shape)
            return x if shape is None or x.shape == shape else x.reshape(shape)
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

    def set_tuning_rows(self, rows):
        """cpmppi_set_tuning_rows: the controller's tuning PER ENV - quadratic_boundary_grad_minimal's seven cost entries, LBD and
        sigma, one row of ``_lib.TUNING_ROW_FLOATS`` floats per env (``configs.tuning_rows`` packs them) - read by every later fused
        ODE step with Philox noise where that step indexes L.  ``None``: back to the engine's configuration.  A contiguous float32
        tensor [rows, 16] on the engine's device is registered AS IT IS - no copy; every later launch (and every replay of a
        captured one) reads its values when it runs, so it may be rewritten in place (stream-ordered) and must outlive the
        launches; the engine keeps a reference.  A host array is uploaded first."""
        if rows is None:
            if self._tuning is not None:
                self._check(self.lib.cpmppi_set_tuning_rows(self._h, None, 0))
                self._tuning = None
            return None
        t = self.tensor(rows)
        if t.dim() != 2 or t.shape[1] != _L.TUNING_ROW_FLOATS or t.shape[0] == 0:
            raise ValueError(f"tuning rows must be [rows, {_L.TUNING_ROW_FLOATS}] (configs.tuning_rows), got {tuple(t.shape)}")
        self._check(self.lib.cpmppi_set_tuning_rows(self._h, _ptr(t), t.shape[0]))
        self._tuning = t
        return t

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

    def _build_plant_step(self, s, Q, n_substeps, dt_sim=0.002, period=0, period_dev=None, period_steps=None, L=None,
                          states_log=None, dd_log=None, save_every=None, Q_log=None, target_position_table=None,
                          target_equilibrium_table=None, L_table=None, sched_stride=1, target_position_out=None,
                          target_equilibrium_out=None, L_out=None, m_pole=None, m_pole_table=None, L_controller_table=None,
                          Q_disturbance_table=None, Q_bias=0.0, Q_applied_out=None, s_measured=None, state_history=None, latency=0.0,
                          measurement_noise_table=None, angle_offset_table=None, informed_table=None):
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
        where ``informed_table`` [sched_rows,E] uint8 says so; None = everywhere).  -> ``s``."""
        E = device_tensor("s", s, note=_IN_PLACE).shape[0]
        a = _L.cpmppi_plant_args()
        Q = self.tensor(Q).reshape(E)
        Lt = self.tensor(L).reshape(E) if L is not None else None
        keep = [s, Q, Lt, period_dev]

        def dev(point=True, **tensors):
            """Check the optional tensors given by field name against _PLANT_TENSORS, keep them and (`point`) put their addresses
            into the block.  -> them (a vector [E] as [E,1]), in the order given."""
            got = []
            for name, t in tensors.items():
                if t is not None:
                    tail, dtype = _PLANT_TENSORS[name]
                    if tail is None:
                        t, tail = t.reshape(E, 1), (1,)
                    device_tensor(name, t, dtype, tuple(E if x == "E" else x for x in tail))
                    keep.append(t)
                    if point:
                        setattr(a, name, t.data_ptr())
                got.append(t)
            return got

        a.E, a.s, a.Q, a.L = E, s.data_ptr(), Q.data_ptr(), _addr(Lt)
        a.n_substeps, a.period_steps, a.dt_sim = int(n_substeps), int(period_steps if period_steps is not None else n_substeps), float(dt_sim)
        a.period = int(period)
        if period_dev is not None:
            a.period_dev = device_tensor("period_dev", period_dev, torch.int64).data_ptr()
        states_log, dd_log, Q_log = dev(states_log=states_log, dd_log=dd_log, Q_log=Q_log)
        rows = [t.shape[0] for t in (states_log, dd_log) if t is not None]
        a.save_rows = min(rows) if rows else 0
        a.save_every = int(save_every) if save_every else 0
        if Q_log is not None:
            a.ctrl_rows = Q_log.shape[0]
            if period_dev is None and not 0 <= int(period) < Q_log.shape[0]:
                raise IndexError(f"period {period} outside Q_log")
        tabs = dev(target_position_table=target_position_table, target_equilibrium_table=target_equilibrium_table, L_table=L_table,
                   m_pole_table=m_pole_table, L_controller_table=L_controller_table)
        sched = [t.shape[0] for t in tabs if t is not None]
        if sched and min(sched) != max(sched):
            raise ValueError("the schedule tables must have the same number of rows")
        qd, = dev(Q_disturbance_table=Q_disturbance_table)
        if qd is not None:
            if Q_log is not None and qd.shape[0] != Q_log.shape[0]:
                raise ValueError("Q_disturbance_table and Q_log must have the same number of rows (one per controller call)")
            a.ctrl_rows, a.Q_bias = qd.shape[0], float(Q_bias)
        sm, = dev(s_measured=s_measured)
        if sm is not None and sm.shape[0] != E:
            raise ValueError("s_measured must be [E,6]")
        # the rest of the measurement chain is checked always and read only with s_measured
        hist, nz, off, inf = dev(point=sm is not None, state_history=state_history, measurement_noise_table=measurement_noise_table,
                                 angle_offset_table=angle_offset_table, informed_table=informed_table)
        if sm is not None:
            steps = float(latency) / float(dt_sim)
            a.latency_steps = int(steps)
            a.latency_frac = steps - int(steps)
            if hist is not None:
                a.history_len = hist.shape[0]
            if nz is not None:
                if Q_log is not None and nz.shape[0] != Q_log.shape[0]:
                    raise ValueError("measurement_noise_table and Q_log must have the same number of rows (one per controller call)")
                a.ctrl_rows = nz.shape[0]
            for t in (off, inf):
                if t is not None:
                    if sched and t.shape[0] != sched[0]:
                        raise ValueError("the schedule tables must have the same number of rows")
                    sched.append(t.shape[0])
        dev(Q_applied_out=Q_applied_out)
        mt = self.tensor(m_pole).reshape(E) if m_pole is not None else None
        keep.append(mt)
        a.m_pole = _addr(mt)
        a.sched_rows, a.sched_stride = (sched[0] if sched else 0), int(sched_stride)
        dev(target_position_out=target_position_out, target_equilibrium_out=target_equilibrium_out, L_out=L_out)
        return PreparedCall(self, self.lib.cpmppi_plant_step, a, keep, s, ("period", "n_substeps"))

    plant_step = _run_once(_build_plant_step)

    def prepare_plant_step(self, *args, **kwargs):
        """The argument block of ``plant_step(...)`` built and validated ONCE (a closed loop calls it every control period with the
        same buffers): ``.run(period=..., n_substeps=...)`` only updates those two fields and enqueues the launch."""
        return self._build_plant_step(*args, **kwargs)

    # ------------------------------------------------------------------ GRU predictor (BASELINE configs[4])
    GRU_KEYS, GRU_SHAPES = GRU_KEYS, GRU_SHAPES                  # (model_folder's: the order of the flat parameter vector)

    def set_gru(self, model):
        """Attach a GRU-6IN-32H1-32H2-5OUT model: dict of float32 arrays in the torch.nn.GRU layout
        (w_ih0[96,6], w_hh0[96,32], b_ih0[96], b_hh0[96], w_ih1[96,32], w_hh1, b_ih1, b_hh1, w_out[5,32], b_out[5]) and
        optional in_scale/in_shift[6], out_scale/out_shift[5].  A training run on this engine (``gru_train_begin``) ends here: its
        master copy and Adam state belong to the model before this one, so ``gru_train_step`` and ``gru_train_get`` are refused
        until ``gru_train_begin`` starts a run from this model.

        ``CpmppiError`` ("cpmppi_set_gru: ...") for a NaN or an infinity in any of the fourteen arrays ("non-finite value in
        <key>") and for a weight beyond what the f16 image of the FAST kernels stores ("weights beyond the f16 range"): the
        largest accepted magnitude is 41588.83 in the r and z rows of w_ih / w_hh, 20794.414 in their n rows (the rows are stored
        pre-scaled by log2(e) and 2 log2(e)) and 59999.996 in w_out.  A refused call changes nothing: the engine keeps the model
        it held - ``has_gru`` stays as it was - and a training run goes on.  FAST kernels need every normalised input and every
        fed-back output within +-65504 (beyond it they give NaN where PRECISE stays finite); nothing checks that at run time."""
        shapes = dict(zip(GRU_KEYS, GRU_SHAPES), in_scale=(6,), in_shift=(6,), out_scale=(5,), out_shift=(5,))
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

    # ------------------------------------------------------------------ Brunton test: predictor error over recordings
    def _recordings(self, states, Q):
        """brunton / gru_washout: -> (states [R,T,6], Q [R,T], R, T) on the device."""
        states, Q = self.tensor(states), self.tensor(Q)
        if states.dim() != 3 or states.shape[2] != 6 or states.shape[0] == 0 or states.shape[1] == 0:
            raise ValueError(f"states must be [R,T,6] with R, T >= 1, got {tuple(states.shape)}")
        R, T = states.shape[0], states.shape[1]
        if Q.dim() == 3 and Q.shape[2] == 1:                    # (the reference's [.., 1] control axis)
            Q = Q[:, :, 0].contiguous()
        if Q.shape != (R, T):
            raise ValueError(f"Q must be [{R},{T}] for states [{R},{T},6], got {tuple(Q.shape)}")
        return states, Q, R, T

    def gru_washout(self, states, Q, h0=None, out=None):
        """cpmppi_gru_washout: the network's memory along recordings ``states`` [R,T,6], ``Q`` [R,T] - row 0 holds ``h0`` [R,2,32]
        (None: zeros), row t+1 the memory after one cell step on (states[:,t], Q[:,t]): what T-1 ``gru_advance`` calls leave, bit
        for bit, in one launch.  -> ``out`` [R,T,2,32] (None: allocated here), the ``h_rows`` of ``brunton``."""
        states, Q, R, T = self._recordings(states, Q)
        h0 = self.tensor(h0, (R, 2, 32)) if h0 is not None else None
        if out is None:
            out = self.empty(R, T, 2, 32)
        elif device_tensor("out", out, tail=(T, 2, 32)).shape[0] != R:
            raise ValueError(f"out must be [{R},{T},2,32], got {tuple(out.shape)}")
        self._check(self.lib.cpmppi_gru_washout(self._h, R, T, _ptr(states), _ptr(Q), _ptr(h0), _ptr(out), self._stream()))
        return out

    def _build_brunton(self, states, Q, L=None, *, horizon, start=0, count=None, predictor="ODE_v0", h_rows=None, stats_out=None,
                       pred_out=None, return_predictions=False):
        """cpmppi_brunton: the open-loop error of a predictor over recordings ``states`` [R,T,6], ``Q`` [R,T] (include/cpmppi.h
        states the test).  From each of the ``count`` rows from ``start`` on (None: every start whose whole ``horizon`` lies inside
        the recording) the predictor is rolled forward on the recorded controls.  ``predictor="ODE_v0"``: the engine's ODE
        predictor, ``L`` [R,T] the pole length per row (None: the config's); ``"GRU"``: the network of ``set_gru`` with the memory
        ``h_rows`` [R,T,2,32] of ``gru_washout`` (None: zeros); it knows no pole length, so ``L`` is refused.
        -> (stats [horizon,6,3] float64 on the device: sum |e|, sum e^2, max |e| per horizon step and feature over the R*count
        starts; predictions [R*count,horizon+1,6] - ``pred_out``, or allocated with ``return_predictions`` - else None)."""
        gru = _is_gru(predictor)
        if gru and L is not None:
            raise ValueError("predictor='GRU' takes no L: the network is the plant model")
        if not gru and h_rows is not None:
            raise ValueError("h_rows is the memory of the GRU predictor: pass predictor='GRU'")
        states, Q, R, T = self._recordings(states, Q)
        horizon, start = int(horizon), int(start)
        count = T - start - horizon if count is None else int(count)
        if not 1 <= horizon <= self.H:
            raise ValueError(f"horizon must be in 1..{self.H} (the engine's mpc_horizon), got {horizon}")
        if start < 0 or count < 1 or start + count + horizon > T:
            raise ValueError(f"start {start} + count {count} + horizon {horizon} must lie inside the recording's {T} rows, count >= 1")
        L = self.tensor(L, (R, T)) if L is not None else None
        h_rows = self.tensor(h_rows, (R, T, 2, 32)) if h_rows is not None else None
        if stats_out is None:
            stats_out = torch.empty(horizon, 6, 3, dtype=torch.float64, device=self.device)
        elif device_tensor("stats_out", stats_out, torch.float64, (6, 3)).shape[0] != horizon:
            raise ValueError(f"stats_out must be [{horizon},6,3]")
        if pred_out is None and return_predictions:
            pred_out = self.empty(R * count, horizon + 1, 6)
        elif pred_out is not None and device_tensor("pred_out", pred_out, tail=(horizon + 1, 6)).shape[0] != R * count:
            raise ValueError(f"pred_out must be [{R * count},{horizon + 1},6]")
        a = _L.cpmppi_brunton_args()
        a.R, a.T, a.start, a.count, a.horizon = R, T, start, count, horizon
        a.predictor = _L.PREDICTOR_GRU if gru else _L.PREDICTOR_ODE_V0
        a.states, a.Q, a.L, a.h_rows = states.data_ptr(), Q.data_ptr(), _addr(L), _addr(h_rows)
        a.stats_out, a.pred_out = stats_out.data_ptr(), _addr(pred_out)
        return PreparedCall(self, self.lib.cpmppi_brunton, a, (states, Q, L, h_rows, stats_out, pred_out), (stats_out, pred_out), ())

    brunton = _run_once(_build_brunton)

    def prepare_brunton(self, *args, **kwargs):
        """The argument block of ``brunton(...)`` built and validated ONCE: ``.run()`` enqueues the two launches again on the same
        buffers (a benchmark loop, a capture - after one plain run, which allocates the workspace)."""
        return self._build_brunton(*args, **kwargs)

    # ------------------------------------------------------------------ fitting the ODE predictor's physical parameters
    @staticmethod
    def ode_fit_mask(trainable):
        """Names out of ``_lib.ODE_FIT_NAMES`` (one, or a sequence; or the bit mask itself) -> the ``trainable`` bit mask."""
        if isinstance(trainable, (int, np.integer)):
            mask = int(trainable)
        else:
            names = (trainable,) if isinstance(trainable, str) else tuple(trainable)
            unknown = [n for n in names if n not in _L.ODE_FIT_NAMES]
            if unknown:
                raise ValueError(f"trainable {unknown}: the parameters a fit can train are {', '.join(_L.ODE_FIT_NAMES)} "
                                 "(TrackHalfLength is not offered: only the bounce test reads it)")
            mask = sum({1 << _L.ODE_FIT_NAMES.index(n) for n in names})
        if not 0 < mask < (1 << _L.ODE_FIT_PARAMS):
            raise ValueError(f"trainable: a non-empty set of {', '.join(_L.ODE_FIT_NAMES)}, got {trainable!r}")
        return mask

    def _window_batch(self, windows, R, T, rows_behind, rule):
        """``windows`` [B,2] integers (r, t0) on the HOST, each with ``rows_behind`` rows behind t0 inside its recording (``rule``: the
        caller's words for that sum) -> (the uint32 host copy the library checks, its int32 upload, B)."""
        w = np.asarray(windows.cpu() if torch.is_tensor(windows) else windows)
        if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] == 0 or not np.issubdtype(w.dtype, np.integer):
            raise ValueError(f"windows must be integers [B,2] = (recording, first row) with B >= 1, got {w.dtype} {w.shape}")
        if w.min() < 0 or w[:, 0].max() >= R or w[:, 1].max() + rows_behind > T - 1:
            raise ValueError(f"every window (r, t0) must satisfy r < {R} and t0 + {rule} <= {T - 1}")
        w_host = np.ascontiguousarray(w, dtype=np.uint32)
        return w_host, torch.as_tensor(w_host.astype(np.int32)).to(self.device), w.shape[0]

    def _loss_outputs(self, loss_out, grad_out, grad, n, dtype):
        """-> (``loss_out``: float64, one element; ``grad_out``: ``dtype`` [n], None with ``grad=False``), allocated here when None."""
        if loss_out is None:
            loss_out = torch.empty(1, dtype=torch.float64, device=self.device)
        elif device_tensor("loss_out", loss_out, torch.float64).numel() != 1:
            raise ValueError("loss_out must have one element")
        if grad and grad_out is None:
            grad_out = torch.empty(n, dtype=dtype, device=self.device)
        elif grad_out is not None and (not grad or device_tensor("grad_out", grad_out, dtype).shape != (n,)):
            raise ValueError(f"grad_out must be {'float64 ' if dtype == torch.float64 else ''}[{n}] (and grad=True)")
        return loss_out, grad_out

    def _run_keeping(self, slot, call):
        """``call.run()``, its batch held in ``slot`` beside the one of the call before: the launches read a batch after the Python
        call returns, and a refused call must not free the batch of the launches still in flight."""
        setattr(self, slot, (getattr(self, slot)[1], call.keep))
        return call.run()

    def _ode_fit_args(self, states, Q, windows, horizon, trainable, feature_scale, L=None, loss_out=None, grad_out=None, grad=True,
                      per_window_out=None):
        """The argument block of cpmppi_ode_fit_loss_grad / cpmppi_ode_fit_step, checked: -> (block, what it points into, loss_out,
        grad_out).  ``windows`` [B,2] integers (r, t0) on the HOST: uploaded here, and handed to the library as its host copy."""
        states, Q, R, T = self._recordings(states, Q)
        horizon, mask = int(horizon), self.ode_fit_mask(trainable)
        if not 1 <= horizon <= self.H:
            raise ValueError(f"horizon must be in 1..{self.H} (the engine's mpc_horizon), got {horizon}")
        w_host, w_dev, B = self._window_batch(windows, R, T, horizon, horizon)
        scale = np.asarray(feature_scale, np.float32).reshape(-1)
        if scale.shape != (5,) or not np.isfinite(scale).all():
            raise ValueError("feature_scale must hold five finite numbers (angleD, angle_cos, angle_sin, position, positionD)")
        if L is not None and (mask >> _L.ODE_FIT_NAMES.index("L")) & 1:
            raise ValueError("L is trainable and L rows are given: the rows would replace the parameter")
        L = self.tensor(L, (R, T)) if L is not None else None
        loss_out, grad_out = self._loss_outputs(loss_out, grad_out, grad, _L.ODE_FIT_PARAMS, torch.float64)
        if per_window_out is not None and device_tensor("per_window_out", per_window_out, tail=(1 + _L.ODE_FIT_PARAMS,)).shape[0] != B:
            raise ValueError(f"per_window_out must be [{B},{1 + _L.ODE_FIT_PARAMS}]")
        a = _L.cpmppi_ode_fit_args()
        a.B, a.R, a.T, a.horizon, a.trainable = B, R, T, horizon, mask
        a.states, a.Q, a.L, a.windows, a.windows_host = states.data_ptr(), Q.data_ptr(), _addr(L), w_dev.data_ptr(), w_host.ctypes.data
        a.feature_scale = (C.c_float * 5)(*scale.tolist())
        a.loss_out, a.grad_out, a.per_window_out = loss_out.data_ptr(), _addr(grad_out), _addr(per_window_out)
        return a, (states, Q, L, w_dev, w_host, loss_out, grad_out, per_window_out), loss_out, grad_out

    def ode_fit_reserve(self, B):
        """cpmppi_ode_fit_reserve: the workspace of ``ode_fit_loss_grad`` / ``ode_fit_step`` for up to ``B`` windows, so that a later
        call can be captured."""
        self._check(self.lib.cpmppi_ode_fit_reserve(self._h, int(B)))

    def _build_ode_fit_loss_grad(self, states, Q, windows, horizon, trainable=("u_max",), feature_scale=(1.0,) * 5, L=None, grad=True, *,
                                 loss_out=None, grad_out=None, per_window_out=None):
        """cpmppi_ode_fit_loss_grad: the open-loop error of the engine's ODE predictor over ``windows`` [B,2] = (recording, first row)
        of ``states`` [R,T,6], ``Q`` [R,T] (include/cpmppi.h states it) - the mean over B x ``horizon`` x 5 of the squared error of
        angleD, angle_cos, angle_sin, position, positionD times ``feature_scale`` - at the fit's running parameters (the engine's own
        before ``ode_fit_begin``), and its derivative with respect to theta, p = base exp(theta), of the ``trainable`` parameters.
        -> (loss [1] float64 on the device, d loss / d theta [8] float64 in the order of ``_lib.ODE_FIT_NAMES`` - None with
        ``grad=False``, the loss alone, bit for bit the loss of the gradient call)."""
        a, keep, loss_out, grad_out = self._ode_fit_args(states, Q, windows, horizon, trainable, feature_scale, L, loss_out, grad_out,
                                                         grad, per_window_out)
        return PreparedCall(self, self.lib.cpmppi_ode_fit_loss_grad, a, keep, (loss_out, grad_out), ())

    ode_fit_loss_grad = _run_once(_build_ode_fit_loss_grad)

    def prepare_ode_fit_loss_grad(self, *args, **kwargs):
        """The argument block of ``ode_fit_loss_grad(...)`` built and validated ONCE: ``.run()`` enqueues the two launches again on the
        same buffers (a capture - after one plain run or ``ode_fit_reserve``, which allocate the workspace)."""
        return self._build_ode_fit_loss_grad(*args, **kwargs)

    def ode_fit_begin(self):
        """cpmppi_ode_fit_begin: a fit starts from the engine's own physical parameters (with its scalar pole mass) - theta, Adam's
        moments and the step counter zero.  The engine's physics is never changed by a fit."""
        self._check(self.lib.cpmppi_ode_fit_begin(self._h))

    def ode_fit_set_theta(self, theta):
        """cpmppi_ode_fit_set_theta: theta [8] in the order of ``_lib.ODE_FIT_NAMES``; p = base exp(theta) follows on the device."""
        t = np.ascontiguousarray(np.asarray(theta, np.float32).reshape(-1))
        if t.shape != (_L.ODE_FIT_PARAMS,):
            raise ValueError(f"theta must hold {_L.ODE_FIT_PARAMS} numbers ({', '.join(_L.ODE_FIT_NAMES)})")
        self._check(self.lib.cpmppi_ode_fit_set_theta(self._h, t.ctypes.data_as(C.POINTER(C.c_float))))

    def _build_ode_fit_step(self, states, Q, windows, horizon, trainable=("u_max",), feature_scale=(1.0,) * 5, L=None, *, lr, beta1=0.9,
                            beta2=0.999, eps=1e-8, loss_out=None):
        """cpmppi_ode_fit_step: the loss and gradient of ``ode_fit_loss_grad`` over this batch of ``windows``, one Adam update of the
        trainable theta and the rewrite of the parameters the next step reads, all on the device.
        -> the batch's loss BEFORE the update, [1] float64 on the device."""
        a, keep, loss_out, _ = self._ode_fit_args(states, Q, windows, horizon, trainable, feature_scale, L, loss_out, None, False)
        lib, hyper = self.lib, (float(lr), float(beta1), float(beta2), float(eps))
        return PreparedCall(self, lambda h, ref, stream: lib.cpmppi_ode_fit_step(h, ref, *hyper, stream), a, keep, loss_out, ())

    def ode_fit_step(self, *args, **kwargs):
        """``_build_ode_fit_step``'s call, run once: -> the batch's loss before the update."""
        return self._run_keeping("_fit_keep", self._build_ode_fit_step(*args, **kwargs))

    def prepare_ode_fit_step(self, *args, **kwargs):
        """The argument block of ``ode_fit_step(...)`` built and validated ONCE: every ``.run()`` is one more Adam step on the same
        batch and buffers (a benchmark loop, a capture - after ``ode_fit_reserve``)."""
        return self._build_ode_fit_step(*args, **kwargs)

    def ode_fit_get(self):
        """cpmppi_ode_fit_get: -> (the fit's parameters p [8], theta [8]), float32 numpy in the order of ``_lib.ODE_FIT_NAMES``.
        Synchronous."""
        p, theta = np.empty(_L.ODE_FIT_PARAMS, np.float32), np.empty(_L.ODE_FIT_PARAMS, np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.cpmppi_ode_fit_get(self._h, p.ctypes.data_as(fp), theta.ctypes.data_as(fp)))
        return p, theta

    # ------------------------------------------------------------------ the neural imitator (Dense-7IN-32H1-32H2-1OUT)
    def set_dense(self, model):
        """cpmppi_set_dense: ``model`` = {w1 [32,7], b1 [32], w2 [32,32], b2 [32], w3 [1,32], b3 [1]} in the torch.nn.Linear layout
        with the input columns in the order of ``model_folder.DENSE_INPUTS``, and optionally in_scale / in_shift [7], out_scale /
        out_shift [1] (x_n = in_scale x + in_shift, Q = out_scale y + out_shift; identity when absent) - what
        ``model_folder.load_dense_model`` returns.  The library refuses a non-finite value by name; a refused call changes nothing -
        ``has_dense`` stays as it was and a training run goes on; a successful one ends a training run."""
        shapes = dict(zip(DENSE_KEYS, DENSE_SHAPES), in_scale=(7,), in_shift=(7,), out_scale=(1,), out_shift=(1,))
        keep = {}
        for k, shp in shapes.items():
            if model.get(k) is not None:
                a = np.ascontiguousarray(np.asarray(model[k].detach().cpu() if torch.is_tensor(model[k]) else model[k], dtype=np.float32))
                if a.shape != shp:
                    raise ValueError(f"Dense weight {k} must have shape {shp}, got {a.shape}")
                keep[k] = a
            elif k in DENSE_KEYS:
                raise ValueError(f"Dense weight {k} missing")
        m = _L.cpmppi_dense_model()
        for k in shapes:
            setattr(m, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)) if k in keep else None)
        self._check(self.lib.cpmppi_set_dense(self._h, C.byref(m)))
        self.has_dense = True

    def _need_dense(self):
        if not self.has_dense:
            raise ValueError("no model set: call set_dense first")

    def _build_dense_control(self, s, target_position, target_equilibrium, *, Q_out=None, y_out=None, count_dev=None):
        """cpmppi_dense_control: the imitator's control of every env, ``Q_out`` [E] = clip(out_scale y + out_shift, -1, 1), from the
        states ``s`` [E,6] and the targets [E] (device tensors; one launch, nothing allocated by the library).  ``y_out`` [E]: the
        head's normalised output.  ``count_dev``: an int64 device counter advanced by one behind the step (a captured loop).
        -> (Q_out, y_out)."""
        self._need_dense()
        E = device_tensor("s", s, tail=(6,)).shape[0]
        if E == 0:
            raise ValueError("s must be [E,6] with E >= 1")
        for name, t in (("target_position", target_position), ("target_equilibrium", target_equilibrium)):
            if device_tensor(name, t).shape != (E,):
                raise ValueError(f"{name} must be [{E}] for s [{E},6]")
        if Q_out is None:
            Q_out = self.empty(E)
        for name, t in (("Q_out", Q_out), ("y_out", y_out)):
            if t is not None and device_tensor(name, t).shape != (E,):
                raise ValueError(f"{name} must be [{E}]")
        a = _L.cpmppi_dense_control_args()
        a.E, a.s, a.target_position, a.target_equilibrium = E, s.data_ptr(), target_position.data_ptr(), target_equilibrium.data_ptr()
        a.Q_out, a.y_out, a.count_dev = Q_out.data_ptr(), _addr(y_out), _counter("count_dev", count_dev)
        return PreparedCall(self, self.lib.cpmppi_dense_control, a, (s, target_position, target_equilibrium, Q_out, y_out, count_dev),
                            (Q_out, y_out), ())

    dense_control = _run_once(_build_dense_control)

    def prepare_dense_control(self, *args, **kwargs):
        """The argument block of ``dense_control(...)`` built and validated ONCE: ``.run()`` enqueues the launch again on the same
        buffers (the device loop, a capture)."""
        return self._build_dense_control(*args, **kwargs)

    def _build_dagger_step(self, s, target_position, target_equilibrium, Q_expert, beta, Q_out, states, rec_target_position,
                           rec_target_equilibrium, labels, *, r0=0, seed=0, env_offset=0, period=0, period_dev=None,
                           imitator_out=None, gate_out=None, sq_err=None):
        """cpmppi_dagger_step: one DAgger control period for every env (include/cpmppi.h states it) - the imitator's control of
        ``s`` [E,6] and the targets [E], the coin of ``beta`` [E] (Philox: ``seed``, ``env_offset``, the period), ``Q_out`` [E] =
        ``Q_expert`` where the expert drives and the imitator's control elsewhere, and the sample into row (``r0`` + e, period) of
        the dataset ``states`` [R,T,6], ``rec_target_position``, ``rec_target_equilibrium``, ``labels`` [R,T] (``labels`` <-
        ``Q_expert``).  Optional: ``imitator_out`` [R,T], ``gate_out`` [R,T] uint8, ``sq_err`` [E] float64 (accumulated).  The
        period is ``period``, or ``period_dev`` - 1: an int64 device counter the expert's step has advanced already.  Every tensor
        on the device; one launch, nothing allocated.  -> Q_out."""
        self._need_dense()
        E = device_tensor("s", s, tail=(6,)).shape[0]
        if E == 0:
            raise ValueError("s must be [E,6] with E >= 1")
        for name, t in (("target_position", target_position), ("target_equilibrium", target_equilibrium), ("Q_expert", Q_expert),
                        ("beta", beta), ("Q_out", Q_out)):
            if device_tensor(name, t).shape != (E,):
                raise ValueError(f"{name} must be [{E}] for s [{E},6]")
        if device_tensor("states", states).dim() != 3 or states.shape[2] != 6:
            raise ValueError("states must be [R,T,6]")
        R, T = states.shape[:2]
        for name, t, dtype in (("rec_target_position", rec_target_position, torch.float32),
                               ("rec_target_equilibrium", rec_target_equilibrium, torch.float32), ("labels", labels, torch.float32),
                               ("imitator_out", imitator_out, torch.float32), ("gate_out", gate_out, torch.uint8)):
            optional = name in ("imitator_out", "gate_out")
            if not (optional and t is None) and device_tensor(name, t, dtype).shape != (R, T):
                raise ValueError(f"{name} must be [{R},{T}] for states [{R},{T},6]")
        if sq_err is not None and device_tensor("sq_err", sq_err, torch.float64).shape != (E,):
            raise ValueError(f"sq_err must be [{E}] float64")
        r0, period = int(r0), int(period)
        if r0 < 0 or period < 0:
            raise ValueError("r0 and period must not be negative")
        a = _L.cpmppi_dagger_args()
        a.E, a.s, a.target_position, a.target_equilibrium = E, s.data_ptr(), target_position.data_ptr(), target_equilibrium.data_ptr()
        a.Q_expert, a.beta, a.Q_out = Q_expert.data_ptr(), beta.data_ptr(), Q_out.data_ptr()
        a.seed, a.env_offset, a.period, a.period_dev = int(seed), int(env_offset), period, _counter("period_dev", period_dev)
        a.R, a.T, a.r0 = R, T, r0
        a.states, a.rec_target_position, a.rec_target_equilibrium = states.data_ptr(), rec_target_position.data_ptr(), rec_target_equilibrium.data_ptr()
        a.labels, a.imitator_out, a.gate_out, a.sq_err = labels.data_ptr(), _addr(imitator_out), _addr(gate_out), _addr(sq_err)
        keep = (s, target_position, target_equilibrium, Q_expert, beta, Q_out, period_dev, states, rec_target_position,
                rec_target_equilibrium, labels, imitator_out, gate_out, sq_err)
        return PreparedCall(self, self.lib.cpmppi_dagger_step, a, keep, Q_out, ("period",))

    dagger_step = _run_once(_build_dagger_step)

    def prepare_dagger_step(self, *args, **kwargs):
        """The argument block of ``dagger_step(...)`` built and validated ONCE: ``.run(period=c)`` names the period and enqueues the
        launch again on the same buffers (the device loop; a capture, with ``period_dev``)."""
        return self._build_dagger_step(*args, **kwargs)

    def _dense_loss_args(self, states, target_position, target_equilibrium, labels, windows, post_wash_out, shift_labels,
                         loss_out=None, grad_out=None, grad=True):
        """The argument block of cpmppi_dense_loss_grad / cpmppi_dense_train_step, checked: -> (block, what it points into, loss_out,
        grad_out).  ``windows`` [B,2] integers (r, t0) on the HOST: uploaded here, and handed to the library as its host copy."""
        self._need_dense()
        states, labels, R, T = self._recordings(states, labels)
        tp, te = self.tensor(target_position), self.tensor(target_equilibrium)
        if tp.shape != (R, T) or te.shape != (R, T):
            raise ValueError(f"target_position and target_equilibrium must be [{R},{T}] for states [{R},{T},6]")
        P, shift = int(post_wash_out), int(shift_labels)
        if P < 1 or shift < 0:
            raise ValueError(f"post_wash_out >= 1 and shift_labels >= 0, got {P}, {shift}")
        w_host, w_dev, B = self._window_batch(windows, R, T, P - 1 + shift, f"{P} - 1 + {shift}")
        loss_out, grad_out = self._loss_outputs(loss_out, grad_out, grad, _L.DENSE_PARAMS, torch.float32)
        a = _L.cpmppi_dense_loss_args()
        a.B, a.R, a.T, a.post_wash_out, a.shift_labels = B, R, T, P, shift
        a.states, a.target_position, a.target_equilibrium, a.labels = states.data_ptr(), tp.data_ptr(), te.data_ptr(), labels.data_ptr()
        a.windows, a.windows_host = w_dev.data_ptr(), w_host.ctypes.data
        a.loss_out, a.grad_out = loss_out.data_ptr(), _addr(grad_out)
        return a, (states, tp, te, labels, w_dev, w_host, loss_out, grad_out), loss_out, grad_out

    def dense_train_reserve(self, samples):
        """cpmppi_dense_train_reserve: the partial rows of ``dense_loss_grad`` / ``dense_train_step`` for up to ``samples`` = windows x
        post_wash_out samples, so that a later call can be captured."""
        self._check(self.lib.cpmppi_dense_train_reserve(self._h, int(samples)))

    def _build_dense_loss_grad(self, states, target_position, target_equilibrium, labels, windows, post_wash_out=1, shift_labels=0,
                               grad=True, *, loss_out=None, grad_out=None):
        """cpmppi_dense_loss_grad: the imitator's mean squared error over ``windows`` [B,2] = (recording, first row) of
        ``post_wash_out`` rows of ``states`` [R,T,6], ``target_position``, ``target_equilibrium``, ``labels`` [R,T] - every row one
        sample, scored against the normalised label ``shift_labels`` rows on (include/cpmppi.h states it).
        -> (loss [1] float64 on the device, gradient [1345] in the flat order of ``DENSE_KEYS`` - None with ``grad=False``, the loss
        alone, bit for bit the loss of the gradient call)."""
        a, keep, loss_out, grad_out = self._dense_loss_args(states, target_position, target_equilibrium, labels, windows,
                                                            post_wash_out, shift_labels, loss_out, grad_out, grad)
        return PreparedCall(self, self.lib.cpmppi_dense_loss_grad, a, keep, (loss_out, grad_out), ())

    dense_loss_grad = _run_once(_build_dense_loss_grad)

    def prepare_dense_loss_grad(self, *args, **kwargs):
        """The argument block of ``dense_loss_grad(...)`` built and validated ONCE (a capture - after ``dense_train_reserve``)."""
        return self._build_dense_loss_grad(*args, **kwargs)

    def dense_train_begin(self):
        """cpmppi_dense_train_begin: training starts from the model of the last ``set_dense`` - Adam's moments and step counter zero.
        The run lasts until the next ``set_dense``, which ends it."""
        self._need_dense()
        self._check(self.lib.cpmppi_dense_train_begin(self._h))

    def _build_dense_train_step(self, states, target_position, target_equilibrium, labels, windows, post_wash_out=1, shift_labels=0, *,
                                lr, beta1=0.9, beta2=0.999, eps=1e-8, loss_out=None):
        """cpmppi_dense_train_step: the loss and gradient of ``dense_loss_grad`` over this batch of ``windows`` and one Adam update of
        the parameter vector in place, two launches.  -> the batch's loss BEFORE the update, [1] float64 on the device."""
        a, keep, loss_out, _ = self._dense_loss_args(states, target_position, target_equilibrium, labels, windows, post_wash_out,
                                                     shift_labels, loss_out, None, False)
        lib, hyper = self.lib, (float(lr), float(beta1), float(beta2), float(eps))
        return PreparedCall(self, lambda h, ref, stream: lib.cpmppi_dense_train_step(h, ref, *hyper, stream), a, keep, loss_out, ())

    def dense_train_step(self, *args, **kwargs):
        """``_build_dense_train_step``'s call, run once: -> the batch's loss before the update."""
        return self._run_keeping("_dense_keep", self._build_dense_train_step(*args, **kwargs))

    def prepare_dense_train_step(self, *args, **kwargs):
        """The argument block of ``dense_train_step(...)`` built and validated ONCE: every ``.run()`` is one more Adam step on the same
        batch and buffers (a benchmark loop, a capture - after ``dense_train_reserve``)."""
        return self._build_dense_train_step(*args, **kwargs)

    # ------------------------------------------------------------------ fine-tuning the imitator on the task cost through the ODE plant
    def _dense_policy_args(self, states, target_position, target_equilibrium, windows, horizon, pole_lengths=None, loss_out=None,
                           grad_out=None, grad=True, cost_out=None, Q_out=None):
        """The argument block of cpmppi_dense_policy_loss_grad / cpmppi_dense_policy_train_step, checked: -> (block, what it points
        into, loss_out, grad_out).  ``windows`` [B,2] integers (r, t0) on the HOST - a window is ONE row, the start state: uploaded
        here, and handed to the library as its host copy."""
        self._need_dense()
        if self.has_gru:
            raise ValueError("the engine holds a GRU predictor (set_gru): the GRU as the differentiated plant is not built - the cost "
                             "is differentiated through ODE_v0 or ODE")
        states = self.tensor(states)
        if states.dim() != 3 or states.shape[2] != 6 or states.shape[0] == 0 or states.shape[1] == 0:
            raise ValueError(f"states must be [R,T,6] with R, T >= 1, got {tuple(states.shape)}")
        R, T = states.shape[0], states.shape[1]
        tp, te = self.tensor(target_position), self.tensor(target_equilibrium)
        if tp.shape != (R, T) or te.shape != (R, T):
            raise ValueError(f"target_position and target_equilibrium must be [{R},{T}] for states [{R},{T},6]")
        horizon = int(horizon)
        if not 1 <= horizon <= 1024:
            raise ValueError(f"horizon must be in 1..1024, got {horizon}")
        w_host, w_dev, B = self._window_batch(windows, R, T, 0, "0")
        L = self.tensor(pole_lengths, (R,)) if pole_lengths is not None else None
        loss_out, grad_out = self._loss_outputs(loss_out, grad_out, grad, _L.DENSE_PARAMS, torch.float32)
        for name, t, shape in (("cost_out", cost_out, (B,)), ("Q_out", Q_out, (B, horizon))):
            if t is not None and device_tensor(name, t).shape != shape:
                raise ValueError(f"{name} must be {list(shape)}")
        a = _L.cpmppi_dense_policy_args()
        a.B, a.R, a.T, a.horizon = B, R, T, horizon
        a.states, a.target_position, a.target_equilibrium, a.L = states.data_ptr(), tp.data_ptr(), te.data_ptr(), _addr(L)
        a.windows, a.windows_host = w_dev.data_ptr(), w_host.ctypes.data
        a.loss_out, a.grad_out, a.cost_out, a.Q_out = loss_out.data_ptr(), _addr(grad_out), _addr(cost_out), _addr(Q_out)
        return a, (states, tp, te, L, w_dev, w_host, loss_out, grad_out, cost_out, Q_out), loss_out, grad_out

    def dense_policy_reserve(self, B, horizon):
        """cpmppi_dense_policy_reserve: check-points and partial rows of ``dense_policy_loss_grad`` / ``dense_policy_train_step`` for
        up to ``B`` start states and that ``horizon``, so that a later call can be captured."""
        self._check(self.lib.cpmppi_dense_policy_reserve(self._h, int(B), int(horizon)))

    def dense_policy_ckpt(self, fill=None):
        """Test aid (cpmppi_dense_policy_ckpt_floats / _ckpt_copy): the reserved check-point workspace of the cost steps, which is
        the handle's own -> its floats as a host array (synchronous); ``fill``: first every one of them is set to that value."""
        n = int(self.lib.cpmppi_dense_policy_ckpt_floats(self._h))
        host = np.empty(n, np.float32)
        if fill is not None:
            host[:] = fill
        if n:
            self._check(self.lib.cpmppi_dense_policy_ckpt_copy(self._h, host.ctypes.data_as(C.POINTER(C.c_float)), n, int(fill is not None)))
        return host

    def _build_dense_policy_loss_grad(self, states, target_position, target_equilibrium, windows, horizon, pole_lengths=None, grad=True, *,
                                      loss_out=None, grad_out=None, cost_out=None, Q_out=None):
        """cpmppi_dense_policy_loss_grad: the mean over ``windows`` [B,2] = (recording, row) of the closed-loop trajectory cost - from
        the state ``states`` [R,T,6] at that row the imitator drives the engine's ODE predictor for ``horizon`` control steps under
        the row's targets, scored by the engine's cost (include/cpmppi.h states it) - and its derivative with respect to the 1345
        parameters.  ``pole_lengths`` [R]: the pole length per recording.  ``cost_out`` [B]: every start state's cost; ``Q_out``
        [B,horizon]: the controls.
        -> (loss [1] float64 on the device, gradient [1345] in the flat order of ``DENSE_KEYS`` - None with ``grad=False``, the loss
        alone, bit for bit the loss of the gradient call)."""
        a, keep, loss_out, grad_out = self._dense_policy_args(states, target_position, target_equilibrium, windows, horizon, pole_lengths,
                                                              loss_out, grad_out, grad, cost_out, Q_out)
        return PreparedCall(self, self.lib.cpmppi_dense_policy_loss_grad, a, keep, (loss_out, grad_out), ())

    dense_policy_loss_grad = _run_once(_build_dense_policy_loss_grad)

    def prepare_dense_policy_loss_grad(self, *args, **kwargs):
        """The argument block of ``dense_policy_loss_grad(...)`` built and validated ONCE (a capture - after ``dense_policy_reserve``)."""
        return self._build_dense_policy_loss_grad(*args, **kwargs)

    def _build_dense_policy_train_step(self, states, target_position, target_equilibrium, windows, horizon, pole_lengths=None, *, lr,
                                       beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=0.0, loss_out=None):
        """cpmppi_dense_policy_train_step: the loss and gradient of ``dense_policy_loss_grad`` over this batch, the gradient scaled to
        the global norm ``clip_norm`` (<= 0: off) and one Adam update of the parameter vector in place - in the run of
        ``dense_train_begin``, whose moments and counter ``dense_train_step`` shares.  A non-finite loss or norm leaves the
        parameters, the moments and the counter alone.  -> the batch's loss BEFORE the update, [1] float64 on the device."""
        a, keep, loss_out, _ = self._dense_policy_args(states, target_position, target_equilibrium, windows, horizon, pole_lengths, loss_out,
                                                       None, False)
        lib, hyper = self.lib, (float(lr), float(beta1), float(beta2), float(eps), float(clip_norm))
        return PreparedCall(self, lambda h, ref, stream: lib.cpmppi_dense_policy_train_step(h, ref, *hyper, stream), a, keep, loss_out, ())

    def dense_policy_train_step(self, *args, **kwargs):
        """``_build_dense_policy_train_step``'s call, run once: -> the batch's loss before the update."""
        return self._run_keeping("_dense_keep", self._build_dense_policy_train_step(*args, **kwargs))

    def prepare_dense_policy_train_step(self, *args, **kwargs):
        """The argument block of ``dense_policy_train_step(...)`` built and validated ONCE: every ``.run()`` is one more step on the
        same batch and buffers (a benchmark loop, a capture - after ``dense_policy_reserve``)."""
        return self._build_dense_policy_train_step(*args, **kwargs)

    def dense_train_get(self):
        """cpmppi_dense_train_get: the trained weights as the dict ``set_dense`` takes (weights only; the normalisation is the
        caller's).  Synchronous."""
        flat = np.empty(_L.DENSE_PARAMS, np.float32)
        self._check(self.lib.cpmppi_dense_train_get(self._h, flat.ctypes.data_as(C.POINTER(C.c_float))))
        return self.dense_unflatten(flat)

    @staticmethod
    def dense_unflatten(flat):
        """The flat parameter vector [1345] -> {key: array} in the order and shapes of ``DENSE_KEYS``."""
        flat = np.asarray(flat)
        if flat.shape != (_L.DENSE_PARAMS,):
            raise ValueError(f"the flat parameter vector has {_L.DENSE_PARAMS} entries, got {flat.shape}")
        out, at = {}, 0
        for k, shp in zip(DENSE_KEYS, DENSE_SHAPES):
            n = int(np.prod(shp))
            out[k] = flat[at:at + n].reshape(shp).copy()
            at += n
        return out

    @staticmethod
    def dense_flatten(model):
        """{key: array} -> the flat float32 parameter vector [1345]."""
        return np.concatenate([np.asarray(model[k], np.float32).reshape(-1) for k in DENSE_KEYS])

    # ------------------------------------------------------------------ training the GRU predictor on recordings
    def _gru_loss_args(self, states, Q, windows, wash_out, post_wash_out, shift_labels, loss_out=None, grad_out=None, grad=True,
                       rollout=False):
        """The argument block of cpmppi_gru_loss_grad / cpmppi_gru_train_step and their ``rollout`` siblings, checked: -> (block,
        what it points into, loss_out, grad_out).  ``windows`` [B,2] integers (r, t0) on the HOST: uploaded here, and handed to the
        library as its host copy."""
        if not self.has_gru:
            raise ValueError("no model set: call set_gru first")
        states, Q, R, T = self._recordings(states, Q)
        W, P, shift = int(wash_out), int(post_wash_out), int(shift_labels)
        if W < 0 or P < 1 or shift < 0:
            raise ValueError(f"wash_out >= 0, post_wash_out >= 1 and shift_labels >= 0, got {W}, {P}, {shift}")
        if rollout and shift != 1:
            raise ValueError(f"rollout: shift_labels must be 1 (the output of a row is the input of the next), got {shift}")
        w_host, w_dev, B = self._window_batch(windows, R, T, W + P - 1 + shift, f"{W} + {P} - 1 + {shift}")
        loss_out, grad_out = self._loss_outputs(loss_out, grad_out, grad, _L.GRU_PARAMS, torch.float32)
        a = _L.cpmppi_gru_loss_args()
        a.B, a.R, a.T, a.wash_out, a.post_wash_out, a.shift_labels = B, R, T, W, P, shift
        a.states, a.Q, a.windows, a.windows_host = states.data_ptr(), Q.data_ptr(), w_dev.data_ptr(), w_host.ctypes.data
        a.loss_out, a.grad_out = loss_out.data_ptr(), _addr(grad_out)
        return a, (states, Q, w_dev, w_host, loss_out, grad_out), loss_out, grad_out

    def gru_train_reserve(self, B, rows):
        """cpmppi_gru_train_reserve: the workspace of ``gru_loss_grad`` / ``gru_train_step`` for ``B`` windows of ``rows`` = wash_out +
        post_wash_out rows, so that a later call can be captured."""
        self._check(self.lib.cpmppi_gru_train_reserve(self._h, int(B), int(rows)))

    def _build_gru_loss_grad(self, states, Q, windows, wash_out, post_wash_out, shift_labels=1, grad=True, *, loss_out=None,
                             grad_out=None, rollout=False):
        """cpmppi_gru_loss_grad: the teacher-forced loss of the model of ``set_gru`` over ``windows`` [B,2] = (recording, first row)
        of ``states`` [R,T,6], ``Q`` [R,T] (include/cpmppi.h states it): the memory starts at zero, ``wash_out`` rows build it,
        ``post_wash_out`` rows are scored against the normalised features ``shift_labels`` rows on.  ``rollout``:
        cpmppi_gru_rollout_loss_grad - behind the first scored row the model's own normalised outputs are fed back with the recorded
        controls, as ``gru_predict`` runs it (``shift_labels`` must be 1), and the gradient runs through the feedback.
        -> (loss [1] float64 on the device, gradient [10341] in the flat order of ``GRU_KEYS`` - None with ``grad=False``, the
        loss alone, bit for bit the loss of the gradient call)."""
        a, keep, loss_out, grad_out = self._gru_loss_args(states, Q, windows, wash_out, post_wash_out, shift_labels, loss_out,
                                                          grad_out, grad, rollout)
        fn = self.lib.cpmppi_gru_rollout_loss_grad if rollout else self.lib.cpmppi_gru_loss_grad
        return PreparedCall(self, fn, a, keep, (loss_out, grad_out), ())

    gru_loss_grad = _run_once(_build_gru_loss_grad)

    def prepare_gru_loss_grad(self, *args, **kwargs):
        """The argument block of ``gru_loss_grad(...)`` built and validated ONCE: ``.run()`` enqueues the launches again on the same
        buffers (a capture - after one plain run or ``gru_train_reserve``, which allocate the workspace)."""
        return self._build_gru_loss_grad(*args, **kwargs)

    def gru_train_begin(self):
        """cpmppi_gru_train_begin: training starts from the model of the last ``set_gru`` - a master copy on the device, Adam's
        moments and step counter zero.  The run lasts until the next ``set_gru``, which ends it: call this again to train the
        model set then."""
        if not self.has_gru:
            raise ValueError("no model set: call set_gru first")
        self._check(self.lib.cpmppi_gru_train_begin(self._h))

    def _build_gru_train_step(self, states, Q, windows, wash_out, post_wash_out, shift_labels=1, *, lr, beta1=0.9, beta2=0.999,
                              eps=1e-8, loss_out=None, rollout=False):
        """cpmppi_gru_train_step (``rollout``: cpmppi_gru_rollout_train_step): the loss and gradient of ``gru_loss_grad`` over this
        batch of ``windows``, one Adam update of the master copy and the rebuild of the exact-f32 weight images, all on the device.
        Steps of both kinds may alternate.  -> the batch's loss BEFORE the update, [1] float64 on the device."""
        a, keep, loss_out, _ = self._gru_loss_args(states, Q, windows, wash_out, post_wash_out, shift_labels, loss_out, None, False,
                                                   rollout)
        fn = self.lib.cpmppi_gru_rollout_train_step if rollout else self.lib.cpmppi_gru_train_step
        hyper = (float(lr), float(beta1), float(beta2), float(eps))
        return PreparedCall(self, lambda h, ref, stream: fn(h, ref, *hyper, stream), a, keep, loss_out, ())

    def gru_train_step(self, *args, **kwargs):
        """``_build_gru_train_step``'s call, run once: -> the batch's loss before the update."""
        return self._run_keeping("_train_keep", self._build_gru_train_step(*args, **kwargs))

    def gru_train_get(self):
        """cpmppi_gru_train_get: the trained weights as the dict ``set_gru`` takes (weights only; the normalisation is the
        caller's).  Synchronous."""
        flat = np.empty(_L.GRU_PARAMS, np.float32)
        self._check(self.lib.cpmppi_gru_train_get(self._h, flat.ctypes.data_as(C.POINTER(C.c_float))))
        return self.gru_unflatten(flat)

    @classmethod
    def gru_unflatten(cls, flat):
        """The flat parameter vector [10341] of the training entry points -> {key: array} in the order and shapes of ``GRU_KEYS``."""
        flat = np.asarray(flat)
        if flat.shape != (_L.GRU_PARAMS,):
            raise ValueError(f"the flat parameter vector has {_L.GRU_PARAMS} entries, got {flat.shape}")
        out, at = {}, 0
        for k, shp in zip(cls.GRU_KEYS, cls.GRU_SHAPES):
            n = int(np.prod(shp))
            out[k] = flat[at:at + n].reshape(shp).copy()
            at += n
        return out

    @classmethod
    def gru_flatten(cls, model):
        """{key: array} -> the flat float32 parameter vector [10341]."""
        return np.concatenate([np.asarray(model[k], np.float32).reshape(-1) for k in cls.GRU_KEYS])

    # ------------------------------------------------------------------ score of a recording, per env
    def _build_score_runs(self, states, Q=None, *, target_position=0.0, target_position_table=None, save_every=1, sched_stride=1,
                          period_steps=None, first_row=0, last_row=None, out=None):
        """cpmppi_score_runs: the device loop's logs ``states`` [R,E,6] (and ``Q`` [calls,E]) scored per env where they lie
        (include/cpmppi.h states the five numbers; ``_lib.SCORE_COLUMNS`` names them) -> ``out`` [E,5] on the device.
        The target of saved row r: ``target_position_table`` [rows,E] (row r * save_every // sched_stride, the last one beyond the
        end: a schedule run's table), else ``target_position``, a scalar or one value per env.  ``first_row`` / ``last_row``
        restrict the rows scored (to drop the swing-up); the mean of Q^2 then runs over the controller calls made at those rows'
        simulation steps, call c at step c * ``period_steps`` (None: ``save_every`` - one saved row per call, as ``run`` records)."""
        states = self.tensor(states)
        if states.dim() != 3 or states.shape[2] != 6 or states.shape[0] == 0 or states.shape[1] == 0:
            raise ValueError(f"states must be [R,E,6] with R, E >= 1, got {tuple(states.shape)}")
        R, E = states.shape[0], states.shape[1]
        first_row, last_row = int(first_row), R if last_row is None else int(last_row)
        if not 0 <= first_row < last_row <= R:
            raise ValueError(f"first_row {first_row}, last_row {last_row}: a non-empty window inside the recording's {R} rows")
        save_every, sched_stride = int(save_every), int(sched_stride)
        period_steps = save_every if period_steps is None else int(period_steps)
        if min(save_every, sched_stride, period_steps) < 1:
            raise ValueError("save_every, sched_stride and period_steps are numbers of simulation steps: at least 1")
        a = _L.cpmppi_score_args()
        a.E, a.row_envs, a.rows, a.first_row, a.last_row = E, E, R, first_row, last_row
        a.save_every, a.sched_stride = save_every, sched_stride
        a.states = states.data_ptr()
        tp = None
        if target_position_table is not None:
            tp = self.tensor(target_position_table)
            if tp.dim() != 2 or tp.shape[0] == 0 or tp.shape[1] != E:
                raise ValueError(f"target_position_table must be [rows,{E}], got {tuple(tp.shape)}")
            a.target_position_table, a.sched_rows = tp.data_ptr(), tp.shape[0]
        elif np.ndim(target_position) == 0 and not torch.is_tensor(target_position):
            a.target_position_value = float(target_position)
        else:
            tp = self.tensor(target_position, (E,))
            a.target_position = tp.data_ptr()
        if Q is not None:
            Q = self.tensor(Q)
            if Q.dim() != 2 or Q.shape[0] == 0 or Q.shape[1] != E:
                raise ValueError(f"Q must be [calls,{E}], got {tuple(Q.shape)}")
            calls = Q.shape[0]
            q_first = -(-first_row * save_every // period_steps)             # the first call at or after the window's first step
            q_last = min(-(-last_row * save_every // period_steps), calls)
            if q_first >= q_last:
                raise ValueError(f"no controller call of Q's {calls} falls into rows {first_row}..{last_row - 1}")
            a.Q, a.q_rows, a.q_first, a.q_last = Q.data_ptr(), calls, q_first, q_last
        if out is None:
            out = self.empty(E, _L.SCORE_FLOATS)
        elif device_tensor("out", out, tail=(_L.SCORE_FLOATS,)).shape[0] != E:
            raise ValueError(f"out must be [{E},{_L.SCORE_FLOATS}]")
        a.score_out = out.data_ptr()
        return PreparedCall(self, self.lib.cpmppi_score_runs, a, (states, Q, tp, out), out, ())

    score_runs = _run_once(_build_score_runs)

    def prepare_score_runs(self, *args, **kwargs):
        """The argument block of ``score_runs(...)`` built and validated ONCE: ``.run()`` enqueues the launch again on the same
        buffers (a captured loop that ends with its own score)."""
        return self._build_score_runs(*args, **kwargs)

    # ------------------------------------------------------------------ control along recorded trajectories
    _REPLAY_COLUMNS = ("target_position", "target_equilibrium", "L", "previous_input")

    def _build_replay_step(self, states, rows, Q, K, *, period=0, period_dev=None, prime=False, rows_dev=None, target_position=None,
                           target_equilibrium=None, L=None, previous_input=None, Q_mean_out=None, Q_std_out=None, Q_all_out=None,
                           s_out=None, target_position_out=None, target_equilibrium_out=None, L_out=None, previous_input_out=None,
                           u_nom_reset=None):
        """cpmppi_replay_step: one control period ``period`` along recordings, in the plant's place (include/cpmppi.h states the
        call).  ``states`` [R,T,6] and the optional columns [R,T] on the device; ``rows`` [R] the recordings' true lengths on the
        HOST (``rows_dev``: the same as an int32 device tensor, else uploaded here); ``Q`` [R*K] the controls of the ``K`` copies of
        every recording, env r*K + k.  Collected at row ``period``: ``Q_mean_out`` / ``Q_std_out`` [R,T], ``Q_all_out`` [T,R*K];
        published from the next row: ``s_out`` [R*K,6] and the ``*_out`` [R*K]; ``u_nom_reset`` [R*K,H] is zero-filled.
        ``prime``: publish row 0 and collect nothing.  ``period_dev``: the step's int64 device counter, already advanced.
        -> (Q_mean_out, Q_std_out) as given."""
        states = device_tensor("states", states, tail=None)
        if states.dim() != 3 or states.shape[2] != 6 or states.shape[0] == 0 or states.shape[1] == 0:
            raise ValueError(f"states must be [R,T,6] with R, T >= 1, got {tuple(states.shape)}")
        R, T, K = states.shape[0], states.shape[1], int(K)
        E = R * K
        if K < 1 or E > self.E:
            raise ValueError(f"{R} recordings x {K} evaluations: between 1 and the engine's {self.E} envs")
        rows_host = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint32)
        if rows_host.shape != (R,):
            raise ValueError(f"rows must hold one length per recording ({R}), got {rows_host.size}")
        if rows_dev is None:
            rows_dev = torch.as_tensor(rows_host.astype(np.int32)).to(self.device)
        elif device_tensor("rows_dev", rows_dev, torch.int32).shape != (R,):
            raise ValueError(f"rows_dev must be [{R}]")
        a = _L.cpmppi_replay_args()
        a.R, a.T, a.K, a.prime, a.period = R, T, K, int(bool(prime)), int(period)
        a.period_dev = _counter("period_dev", period_dev)
        a.rows, a.rows_host, a.states = rows_dev.data_ptr(), rows_host.ctypes.data, states.data_ptr()
        keep = [states, rows_host, rows_dev, period_dev]

        def point(name, t, shape):
            if t is not None:
                if not (is_dense(t) and t.is_cuda and tuple(t.shape) == shape):
                    raise ValueError(f"{name} must be a contiguous float32 ROCm tensor {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
                keep.append(t)
                setattr(a, name, t.data_ptr())

        columns = dict(target_position=target_position, target_equilibrium=target_equilibrium, L=L, previous_input=previous_input)
        outs = dict(target_position_out=target_position_out, target_equilibrium_out=target_equilibrium_out, L_out=L_out,
                    previous_input_out=previous_input_out)
        for name in self._REPLAY_COLUMNS:
            point(name, columns[name], (R, T))
            if outs[name + "_out"] is not None and columns[name] is None:
                raise ValueError(f"{name}_out needs the recorded column {name}")
            point(name + "_out", outs[name + "_out"], (E,))
        point("Q", Q, (E,))
        point("Q_mean_out", Q_mean_out, (R, T))
        point("Q_std_out", Q_std_out, (R, T))
        point("Q_all_out", Q_all_out, (T, E))
        point("s_out", s_out, (E, 6))
        if u_nom_reset is not None:
            a.H = u_nom_reset.shape[1] if torch.is_tensor(u_nom_reset) and u_nom_reset.dim() == 2 else 0
            point("u_nom_reset", u_nom_reset, (E, a.H))
        return PreparedCall(self, self.lib.cpmppi_replay_step, a, keep, (Q_mean_out, Q_std_out), ("period", "prime"))

    replay_step = _run_once(_build_replay_step)

    def prepare_replay_step(self, *args, **kwargs):
        """The argument block of ``replay_step(...)`` built and validated ONCE: ``.run(period=, prime=)`` updates those two fields and
        enqueues the launch; with ``period_dev`` nothing changes between periods."""
        return self._build_replay_step(*args, **kwargs)

    # ------------------------------------------------------------------ cost-only launch and CEM
    def _per_env(self, x, E):
        x = self.tensor(x)
        if x.dim() != 1:
            x = x.reshape(-1)
        return x.expand(E).contiguous() if x.numel() == 1 else x

    def _control_inputs(self, E, s0, target_position, target_equilibrium, L, previous_input, block=None):
        """The per-env inputs of a control step, from whatever the caller gave: -> (s0 [E,6], target position [E], target
        equilibrium [E], L [E] or None, previous input [E] or None); their addresses and E go into the fields of those names of
        ``block``, the argument block of a fused step."""
        s0, tp, te = self.tensor(s0, (E, 6)), self._per_env(target_position, E), self._per_env(target_equilibrium, E)
        Lt = None if L is None else self._per_env(L, E)
        prev = None if previous_input is None else self._per_env(previous_input, E)
        if block is not None:
            block.E, block.s0, block.target_position, block.target_equilibrium = E, s0.data_ptr(), tp.data_ptr(), te.data_ptr()
            block.L, block.previous_input = _addr(Lt), _addr(prev)
        return s0, tp, te, Lt, prev

    def _outputs(self, block, E, Q_out, **optional):
        """The per-env outputs of a fused rpgd / cem step: ``Q_out`` [E] (None: allocated here) and the optional ones by field
        name, each one given [E, *tail] of its dtype; their addresses go into ``block``.  -> them all, in the order given."""
        table = {"Q_out": (torch.float32, ()), "S_out": (torch.float32, (self.N,)), "plan_out": (torch.float32, (self.H,)),
                 "samples_out": (torch.float32, (self.N, self.H)), "order_out": (torch.int32, (self.N,))}
        out = dict(Q_out=self.empty(E) if Q_out is None else Q_out, **optional)
        for name, t in out.items():
            if t is not None and device_tensor(name, t, *table[name]).shape[0] != E:
                raise ValueError(f"{name} must have {E} rows")
            setattr(block, name, _addr(t))
        return tuple(out.values())

    def _rollout_inputs(self, s0, inputs, target_position, target_equilibrium, L, previous_input=None):
        """rollout_cost / rollout_cost_grad: -> (E, inputs [E,N,H], then what _control_inputs gives)."""
        inputs = self.tensor(inputs)
        E = inputs.shape[0]
        if inputs.shape != (E, self.N, self.H):
            raise ValueError(f"inputs must be [E,{self.N},{self.H}]")
        return (E, inputs) + self._control_inputs(E, s0, target_position, target_equilibrium, L, previous_input)

    def rollout_cost(self, s0, inputs, target_position, target_equilibrium, L=None, predictor="ODE_v0", h0=None):
        """inputs[E,N,H] -> S[E,N]: trajectory cost of given control sequences (no update).  ``predictor="GRU"`` rolls them out
        with the network of ``set_gru`` (cpmppi_rollout_cost_gru): ``h0`` [E,2,32] is each env's memory, shared by its rollouts
        (None: zeros); the network knows no pole length, so ``L`` is refused."""
        gru = _rollout_is_gru(predictor, h0, L)
        E, inputs, s0, tp, te, Lt, _ = self._rollout_inputs(s0, inputs, target_position, target_equilibrium, L)
        S = self.empty(E, self.N)
        if gru:
            h0 = self.tensor(h0, (E, 2, 32))
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
        gru = _rollout_is_gru(predictor, h0, L, previous_input)
        E, inputs, s0, tp, te, Lt, pi = self._rollout_inputs(s0, inputs, target_position, target_equilibrium, L, previous_input)
        S, grad = self.empty(E, self.N), self.empty(E, self.N, self.H)
        if gru:
            h0 = self.tensor(h0, (E, 2, 32))
            self._check(self.lib.cpmppi_rollout_cost_grad_gru(self._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(h0),
                                                              _ptr(S), _ptr(grad), self._stream()))
            return S, grad
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
        # (predictor "ODE" with a per-env pole mass registered runs the kernel's second compilation, rollout_cost_rows_kernel; with
        # tuning rows registered either predictor runs the third, rollout_cost_tuned_kernel)
        rows = d["ode_predictor"] and self._m_rows is not None
        d["kernel"] = ("rollout_cost%s_kernel<%d, %s, %d, %d, %d%s>" % (
            "_rows" if rows else ("_tuned" if self._tuning is not None else ""), d["cost_id"], "true" if d["math_mode"] == _L.MATH_FAST else "false", (0, 1, 2, 3)[d["noise_kind"]],
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

    def _build_rpgd_step(self, s0, Q, m, v, target_position, target_equilibrium, L=None, previous_input=None, *, iterations,
                         learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0, keep_k=None, resamp_per=0, shift=1,
                         distribution="normal", sample_mean=0.0, uniform_lo=0.0, uniform_hi=0.0, seed=0, draw_offset=0,
                         env_offset=0, count=0, adam_iteration=0, count_dev=None, Q_out=None, S_out=None, plan_out=None,
                         order_out=None, rows=None):
        """cpmppi_rpgd_step: one whole rpgd / gradient-tf control step on the plans ``Q`` and the Adam moments ``m``, ``v``
        [E,N,H], all three updated IN PLACE (include/cpmppi.h states the step).  ``count_dev``: int64 device scalar, the control
        steps taken so far - read by the kernel in place of ``count`` / ``adam_iteration`` / ``draw_offset`` and incremented
        after the step (graph replay).  ``rows``: cpmppi_rpgd_step_rows instead - a contiguous float32 device tensor [>= E, 16]
        (``configs.rpgd_rows``) with each env's cost weights, learning rate and gradient clip, taken AS IT IS: every launch and
        replay reads its values when it runs, and ``learning_rate`` / ``gradmax_clip`` go unread.
        -> (Q_out[E], S_out, plan_out, order_out), the last three as given (or None)."""
        E = device_tensor("Q", Q, tail=(self.N, self.H), note=_IN_PLACE).shape[0]
        if E > self.E:
            raise ValueError(f"Q must be [E<={self.E},{self.N},{self.H}], got {tuple(Q.shape)}")
        for name, t in (("m", m), ("v", v)):
            if device_tensor(name, t, tail=(self.N, self.H), note=_IN_PLACE).shape[0] != E:
                raise ValueError(f"{name} must have Q's shape")
        if distribution not in ("normal", "uniform"):
            raise ValueError(f"distribution={distribution!r}; expected 'normal' or 'uniform'")
        a = _L.cpmppi_rpgd_args()
        inputs = self._control_inputs(E, s0, target_position, target_equilibrium, L, previous_input, a)
        out = self._outputs(a, E, Q_out, S_out=S_out, plan_out=plan_out, order_out=order_out)
        a.Q, a.m, a.v = Q.data_ptr(), m.data_ptr(), v.data_ptr()
        a.iterations, a.adam_iteration = int(iterations), int(adam_iteration)
        _set_adam(a, learning_rate, beta1, beta2, epsilon, gradmax_clip)
        a.keep_k, a.resamp_per, a.shift = int(self.N if keep_k is None else keep_k), int(resamp_per), int(shift)
        a.distribution = _L.RPGD_UNIFORM if distribution == "uniform" else _L.RPGD_NORMAL
        a.sample_mean, a.uniform_lo, a.uniform_hi = float(sample_mean), float(uniform_lo), float(uniform_hi)
        a.seed, a.draw_offset, a.env_offset, a.count = int(seed), int(draw_offset), int(env_offset), int(count)
        a.count_dev = _counter("count_dev", count_dev)
        enqueue = self.lib.cpmppi_rpgd_step
        if rows is not None:
            if device_tensor("rows", rows, tail=(_L.TUNING_ROW_FLOATS,)).shape[0] < E:
                raise ValueError(f"rows must hold a row per env ({E}), got {rows.shape[0]}")
            step_rows, rows_at, n_rows = self.lib.cpmppi_rpgd_step_rows, C.c_void_p(rows.data_ptr()), rows.shape[0]

            def enqueue(handle, ref, stream):        # (the block goes first, as in every entry point a PreparedCall enqueues)
                return step_rows(handle, ref, rows_at, n_rows, stream)
        return PreparedCall(self, enqueue, a, inputs + (Q, m, v, count_dev, rows) + out, out,
                            ("count", "adam_iteration", "draw_offset", "iterations"))

    rpgd_step = _run_once(_build_rpgd_step)

    def prepare_rpgd_step(self, *args, **kwargs):
        """The argument block of ``rpgd_step(...)`` built and validated ONCE: ``.run(count=, adam_iteration=, draw_offset=,
        iterations=)`` updates the host counters and enqueues the launch; with ``count_dev`` nothing changes between steps."""
        return self._build_rpgd_step(*args, **kwargs)

    def rpgd_gru_reserve(self, E=None):
        """cpmppi_rpgd_gru_reserve: the workspace of ``rpgd_step_gru`` (check-points and gradient of the handle's largest launch;
        E, default all envs, is checked).  After it the step never allocates - required before a step is captured into a graph."""
        self._check(self.lib.cpmppi_rpgd_gru_reserve(self._h, self.E if E is None else int(E)))

    def _build_rpgd_step_gru(self, s0, Q, m, v, target_position, target_equilibrium, h0=None, *, iterations, learning_rate,
                             beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0, keep_k=None, resamp_per=0, shift=1,
                             distribution="normal", sample_mean=0.0, uniform_lo=0.0, uniform_hi=0.0, seed=0, draw_offset=0,
                             env_offset=0, count=0, adam_iteration=0, count_dev=None, Q_out=None, S_out=None, plan_out=None,
                             order_out=None):
        """cpmppi_rpgd_step_gru: one whole rpgd / gradient-tf control step with the network of ``set_gru`` in the rollout loop and
        its adjoint in the gradient, on the plans ``Q`` and the Adam moments ``m``, ``v`` [E,N,H], all three updated IN PLACE
        (include/cpmppi.h states the step; N <= 128).  ``h0`` [E,2,32]: each env's memory, shared by its plans (None: zeros) -
        read, not advanced: ``gru_advance`` hands it on.  ``count_dev`` and the host counters as ``rpgd_step``'s.
        -> (Q_out[E], S_out, plan_out, order_out), the last three as given (or None)."""
        E = device_tensor("Q", Q, tail=(self.N, self.H), note=_IN_PLACE).shape[0]
        if E > self.E:
            raise ValueError(f"Q must be [E<={self.E},{self.N},{self.H}], got {tuple(Q.shape)}")
        for name, t in (("m", m), ("v", v)):
            if device_tensor(name, t, tail=(self.N, self.H), note=_IN_PLACE).shape[0] != E:
                raise ValueError(f"{name} must have Q's shape")
        if distribution not in ("normal", "uniform"):
            raise ValueError(f"distribution={distribution!r}; expected 'normal' or 'uniform'")
        a = _L.cpmppi_rpgd_gru_args()
        inputs = self._control_inputs(E, s0, target_position, target_equilibrium, None, None)[:3]
        a.E, a.s0, a.target_position, a.target_equilibrium = (E,) + tuple(t.data_ptr() for t in inputs)
        h0 = self.tensor(h0, (E, 2, 32))
        a.h0 = _addr(h0)
        out = self._outputs(a, E, Q_out, S_out=S_out, plan_out=plan_out, order_out=order_out)
        a.Q, a.m, a.v = Q.data_ptr(), m.data_ptr(), v.data_ptr()
        a.iterations, a.adam_iteration = int(iterations), int(adam_iteration)
        _set_adam(a, learning_rate, beta1, beta2, epsilon, gradmax_clip)
        a.keep_k, a.resamp_per, a.shift = int(self.N if keep_k is None else keep_k), int(resamp_per), int(shift)
        a.distribution = _L.RPGD_UNIFORM if distribution == "uniform" else _L.RPGD_NORMAL
        a.sample_mean, a.uniform_lo, a.uniform_hi = float(sample_mean), float(uniform_lo), float(uniform_hi)
        a.seed, a.draw_offset, a.env_offset, a.count = int(seed), int(draw_offset), int(env_offset), int(count)
        a.count_dev = _counter("count_dev", count_dev)
        return PreparedCall(self, self.lib.cpmppi_rpgd_step_gru, a, inputs + (h0, Q, m, v, count_dev) + out, out,
                            ("count", "adam_iteration", "draw_offset", "iterations"))

    rpgd_step_gru = _run_once(_build_rpgd_step_gru)

    def prepare_rpgd_step_gru(self, *args, **kwargs):
        """The argument block of ``rpgd_step_gru(...)`` built and validated ONCE, as ``prepare_rpgd_step``'s."""
        return self._build_rpgd_step_gru(*args, **kwargs)

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

    def _build_cem_step(self, s0, mean, stdev, target_position, target_equilibrium, L=None, previous_input=None, *, iterations,
                        best_k, stdev_min, refine=None, learning_rate=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=0.0,
                        shift=1, mean_fill=0.0, stdev_fill=0.0, seed=0, offset=0, env_offset=0, count_dev=None, Q_out=None,
                        S_out=None, plan_out=None, samples_out=None, order_out=None):
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
        a = _L.cpmppi_cem_args()
        inputs = self._control_inputs(E, s0, target_position, target_equilibrium, L, previous_input, a)
        out = self._outputs(a, E, Q_out, S_out=S_out, plan_out=plan_out, samples_out=samples_out, order_out=order_out)
        a.mean, a.stdev = mean.data_ptr(), stdev.data_ptr()
        a.iterations, a.best_k, a.stdev_min, a.refine = int(iterations), int(best_k), float(stdev_min), self._cem_refine(refine)
        _set_adam(a, learning_rate, beta1, beta2, epsilon, gradmax_clip)
        a.shift, a.mean_fill, a.stdev_fill = int(shift), float(mean_fill), float(stdev_fill)
        a.seed, a.offset, a.env_offset = int(seed), int(offset), int(env_offset)
        a.count_dev = _counter("count_dev", count_dev)
        return PreparedCall(self, self.lib.cpmppi_cem_step, a, inputs + (mean, stdev, count_dev) + out, out, ("offset", "iterations"))

    cem_step = _run_once(_build_cem_step)

    def prepare_cem_step(self, *args, **kwargs):
        """The argument block of ``cem_step(...)`` built and validated ONCE: ``.run(offset=, iterations=)`` updates the host's
        Philox offset and iteration count and enqueues the launch; with ``count_dev`` nothing changes between steps."""
        return self._build_cem_step(*args, **kwargs)

    def _build_cem_step_gru(self, s0, mean, stdev, target_position, target_equilibrium, h0=None, *, iterations, best_k, stdev_min,
                            shift=1, mean_fill=0.0, stdev_fill=0.0, seed=0, offset=0, env_offset=0, count_dev=None, Q_out=None,
                            S_out=None, plan_out=None, samples_out=None, order_out=None):
        """cpmppi_cem_step_gru: one whole cem control step with the network of ``set_gru`` in the rollout loop, on the sampling
        distribution ``mean``, ``stdev`` [E,H], both updated IN PLACE (include/cpmppi.h states the step).  ``h0`` [E,2,32]: each
        env's memory, shared by its samples (None: zeros) - read, not advanced: ``gru_advance`` hands it on.  ``count_dev`` as
        ``cem_step``'s.  -> (Q_out[E], S_out, plan_out, samples_out, order_out), the last four as given (or None)."""
        E = device_tensor("mean", mean, tail=(self.H,), note=_IN_PLACE).shape[0]
        if E > self.E:
            raise ValueError(f"mean must be [E<={self.E},{self.H}], got {tuple(mean.shape)}")
        if device_tensor("stdev", stdev, tail=(self.H,), note=_IN_PLACE).shape[0] != E:
            raise ValueError("stdev must have mean's shape")
        a = _L.cpmppi_cem_gru_args()
        inputs = self._control_inputs(E, s0, target_position, target_equilibrium, None, None)[:3]
        a.E, a.s0, a.target_position, a.target_equilibrium = (E,) + tuple(t.data_ptr() for t in inputs)
        h0 = self.tensor(h0, (E, 2, 32))
        a.h0 = _addr(h0)
        out = self._outputs(a, E, Q_out, S_out=S_out, plan_out=plan_out, samples_out=samples_out, order_out=order_out)
        a.mean, a.stdev = mean.data_ptr(), stdev.data_ptr()
        a.iterations, a.best_k, a.stdev_min = int(iterations), int(best_k), float(stdev_min)
        a.shift, a.mean_fill, a.stdev_fill = int(shift), float(mean_fill), float(stdev_fill)
        a.seed, a.offset, a.env_offset = int(seed), int(offset), int(env_offset)
        a.count_dev = _counter("count_dev", count_dev)
        return PreparedCall(self, self.lib.cpmppi_cem_step_gru, a, inputs + (h0, mean, stdev, count_dev) + out, out,
                            ("offset", "iterations"))

    cem_step_gru = _run_once(_build_cem_step_gru)

    def prepare_cem_step_gru(self, *args, **kwargs):
        """The argument block of ``cem_step_gru(...)`` built and validated ONCE, as ``prepare_cem_step``'s."""
        return self._build_cem_step_gru(*args, **kwargs)

    # ------------------------------------------------------------------ the fused hot path
    def step(self, s0, u_nom, target_position, target_equilibrium, L=None, delta_u=None, knots=None, seed=None,
             offset=0, env_offset=0, u_prev=None, Q_out=None, S_out=None, predictor="ODE_v0", h0=None,
             previous_input=None, offset_dev=None, delta_u_tiled=None, u_nom_out=None, gather_into=None):
        """One MPPI optimizer step for E envs.  ``u_nom`` [E,H] is updated IN PLACE, or — with ``u_nom_out`` [E,H] — only
        read, the updated sequence going to ``u_nom_out`` (two buffers used alternately: shard.NativeGather).

        Exactly one noise source: ``delta_u`` [E,N,H], ``knots`` [E,N,P], ``seed`` (in-kernel Philox) or
        ``delta_u_tiled`` (a buffer from sample_tiled / tile_delta_u).
        ``gather_into`` [world, E*H] (needs a communicator, shard.NativeGather): cpmppi_step_gather — the step plus the
        all-gather of the sequences it writes, ordered on the device, nothing but the kernel on the launch stream.
        Returns (Q_out[E], S_out or None).
        """
        return self._build_step(s0, u_nom, target_position, target_equilibrium, L, delta_u, knots, seed, offset, env_offset, u_prev,
                                Q_out, S_out, predictor, h0, previous_input, offset_dev, delta_u_tiled,
                                u_nom_out).run(gather_into=gather_into)

    def _build_step(self, s0, u_nom, target_position, target_equilibrium, L=None, delta_u=None, knots=None, seed=None, offset=0,
                    env_offset=0, u_prev=None, Q_out=None, S_out=None, predictor="ODE_v0", h0=None, previous_input=None,
                    offset_dev=None, delta_u_tiled=None, u_nom_out=None):
        """step's arguments (all but ``gather_into``, which is ``run``'s), validated, as the prepared call that runs them."""
        E = device_tensor("u_nom", u_nom, note=_IN_PLACE).shape[0]
        if u_nom.shape != (E, self.H) or E > self.E:
            raise ValueError(f"u_nom must be [E<={self.E},{self.H}], got {tuple(u_nom.shape)}")
        given = [x is not None for x in (delta_u, knots, seed, delta_u_tiled)]
        if sum(given) != 1:
            raise ValueError("give exactly one of delta_u, knots, seed, delta_u_tiled")
        a = _L.cpmppi_step_args()
        inputs = self._control_inputs(E, s0, target_position, target_equilibrium, L, previous_input, a)
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
        u_prev = self.tensor(u_prev, (E, self.H))
        if Q_out is None:
            Q_out = self.empty(E)
        a.u_nom, a.u_prev, a.noise = u_nom.data_ptr(), _addr(u_prev), _addr(noise)
        a.Q_out, a.S_out = Q_out.data_ptr(), _addr(S_out)
        a.predictor = _L.PREDICTOR_GRU if _is_gru(predictor) else _L.PREDICTOR_ODE_V0
        h0 = self.tensor(h0, (E, 2, 32))
        a.h0 = _addr(h0)
        if u_nom_out is not None:
            if device_tensor("u_nom_out", u_nom_out).shape != u_nom.shape:
                raise ValueError("u_nom_out must have u_nom's shape")
            a.u_nom_out = u_nom_out.data_ptr()
        a.offset_dev = _counter("offset_dev", offset_dev)         # the Philox step counter kept on the device
        return PreparedCall(self, self.lib.cpmppi_step, a, inputs + (u_nom, noise, u_prev, Q_out, S_out, h0, offset_dev, u_nom_out),
                            (Q_out, S_out), ("offset",), gather=self.lib.cpmppi_step_gather)

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
        return self._build_step(*args, **kwargs)


class PreparedCall:
    """One entry point of the library that takes an argument block, ready to be enqueued any number of times
    (MPPIEngine.prepare_step / prepare_plant_step / prepare_rpgd_step / prepare_rpgd_step_gru / prepare_cem_step / prepare_cem_step_gru / prepare_brunton / prepare_gru_loss_grad / prepare_ode_fit_loss_grad / prepare_ode_fit_step / prepare_dense_control / prepare_dagger_step / prepare_dense_loss_grad / prepare_dense_train_step / prepare_dense_policy_loss_grad / prepare_dense_policy_train_step).  ``args`` is the live
    ctypes block, validated when it was built, and ``ref`` the reference to it that the library is handed; ``keep`` holds the
    tensors it points into; ``enqueue`` is the entry point, ``enqueue(handle, ref, stream)``.  ``result`` is what the call returns:
    the outputs of a control step - ``out``, whose first two are ``Q_out`` and ``S_out`` -, the plant's state, or the Brunton
    test's (statistics, predictions)."""

    def __init__(self, engine, enqueue, args, keep, result, fields, gather=None):
        self.engine, self.enqueue, self.args, self.keep, self.result = engine, enqueue, args, keep, result
        self.fields, self._gather = fields, gather
        self.ref = C.byref(args)

    out = property(lambda self: self.result)
    Q_out = property(lambda self: self.result[0])
    S_out = property(lambda self: self.result[1])

    def set(self, **fields):
        """The counters of the block that change from call to call, by field name: each one given (not None) is set, as an int."""
        for name in fields:
            if name not in self.fields:
                raise TypeError(f"{name!r}: only {', '.join(self.fields)} can be set on this call")
        for name, value in fields.items():
            if value is not None:
                setattr(self.args, name, int(value))

    def run(self, gather_into=None, **fields):
        """`set(**fields)`, enqueue on the engine's stream, -> ``result``.  ``gather_into`` (the MPPI step alone): through
        cpmppi_step_gather, which takes that tensor's address after the block."""
        if fields:                                   # (`set` once more, in line: a call less on the path of every control step)
            for name in fields:
                if name not in self.fields:
                    raise TypeError(f"{name!r}: only {', '.join(self.fields)} can be set on this call")
            for name, value in fields.items():
                if value is not None:
                    setattr(self.args, name, int(value))
        e = self.engine
        if gather_into is None:
            e._check(self.enqueue(e._h, self.ref, e._stream()))
        elif self._gather is None:
            raise TypeError("gather_into: only the MPPI step has a gathering entry point")
        else:
            e._check(self._gather(e._h, self.ref, gather_into.data_ptr(), e._stream()))
        return self.result
