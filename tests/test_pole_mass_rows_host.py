"""Per-row pole mass of predictor_type "ODE" (cpmppi_set_pole_mass_rows), the parts that need no GPU: the reference-generated fixture
tests/golden/ode_pole_mass.npz against the numpy oracle, MPPIEngine.apply_pole_mass_of's routing and set_pole_mass_rows' validation
on a handle-less engine, and the controller-mass table the device loop builds from a batch's `m_pole:` schedule and informer."""
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402

f32 = np.float32


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "ode_pole_mass.npz"))


def test_oracle_reproduces_the_reference_with_a_mass_per_row(g):
    """next_state_predictor_ODE broadcasts variable_parameters.L and .m_pole per row (predictors_customization.py:51-64): the numpy
    oracle with the arrays - and row by row with scalars - gives the reference's float32 values bit for bit."""
    s, Q, L, m = g["kat/s"], g["kat/Q"], g["kat/L"], g["kat/m_pole"]
    assert s.shape == (64, 6) and L.shape == m.shape == (64,) and 0.015 <= m.min() and m.max() <= 0.15 and len(np.unique(m)) == 64
    assert np.array_equal(O.ode_step(s, Q, L=L, m_pole=m), g["kat/s_next"])
    rows = np.stack([O.ode_step(s[i:i + 1], Q[i], L=L[i], m_pole=m[i])[0] for i in range(len(m))])
    assert np.array_equal(rows, g["kat/s_next"])
    assert np.abs(O.ode_step(s, Q, L=L) - g["kat/s_next"]).max() > 9e-2          # the default mass is another trajectory
    s0, Qr, Lr, mr, traj = (g[f"roll/{k}"] for k in ("s0", "Q", "L", "m_pole", "traj"))
    assert traj.shape == (32, 21, 6) and np.array_equal(traj[:, 0], s0)
    assert (np.abs(s0[:16, O.ANGLE_IDX]) < 0.31).all() and (np.abs(s0[16:, O.ANGLE_IDX]) > 2.8).all()      # upright | hanging
    t = s0
    for k in range(Qr.shape[1]):
        t = O.ode_step(t, Qr[:, k], L=Lr, m_pole=mr)
        assert np.array_equal(t, traj[:, k + 1]), k


def test_per_env_mass_kernels_have_no_scratch_and_no_vgpr_spills():
    """The gate of tests/test_abi_and_host.py for the kernels it does not list: rollout_cost_rows_kernel, the rollout kernel's
    definition compiled a second time for predictor_ODE with the pole mass per env - one for every predictor_ODE instantiation
    (4 costs x 4 noise sources x (latency R1, throughput R1 fast + precise, throughput R2, its lone-wave form))."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = [k for k in code_objects.kernels(_lib.LIB_PATH) if "24rollout_cost_rows_kernel" in k["name"]]
    assert len(ks) == 4 * 4 * 5, len(ks)
    bad = [(k["name"], k["private_segment_fixed_size"], k["vgpr_spill_count"]) for k in ks
           if k["private_segment_fixed_size"] != 0 or k["vgpr_spill_count"] != 0]
    assert not bad, bad
    for k in ks:                                  # the headline form keeps four waves per SIMD, like its scalar-mass twin
        if "kernelILi0ELb1ELi2ELi2ELi1ELi" in k["name"]:
            assert k["vgpr_count"] + k["agpr_count"] <= 128, (k["name"], k["vgpr_count"])


class _Lib:
    """Stands in for libcpmppi.so: records the calls."""

    def __init__(self):
        self.calls = []

    def cpmppi_set_pole_mass_rows(self, h, ptr, n):
        self.calls.append(("rows", None if ptr is None or not getattr(ptr, "value", ptr) else "ptr", n))
        return 0

    def cpmppi_set_pole_mass(self, h, m):
        self.calls.append(("scalar", m))
        return 0


def _engine(**cfg):
    """The real MPPIEngine methods over a handle-less engine whose library is _Lib and whose buffers are host tensors."""
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine

    class Engine(MPPIEngine):
        def __init__(self):
            self.mppi, self.lib, self._h = MPPIConfig(**cfg), _Lib(), None
            self._m_pole, self._m_rows, self._m_rows_own = float(f32(0.087)), None, None
            self.device = torch.device("cpu")

        def empty(self, *shape):
            return torch.empty(*shape, dtype=torch.float32)

        def close(self):
            pass

    return Engine()


def test_config_field_and_controller_key():
    from cartpolesimulation_amd.configs import MPPIConfig
    assert MPPIConfig().per_env_pole_mass is False and MPPIConfig(per_env_pole_mass=True).per_env_pole_mass is True
    from cartpolesimulation_amd import _lib
    assert "cpmppi_set_pole_mass_rows" in _lib.EXPORTS and _lib.ABI_VERSION == 5


def test_routing_by_the_shape_of_m_pole():
    """Flag off: exactly today's behaviour (a non-uniform m_pole is refused, the text now names the flag).  Flag on: scalar / uniform
    host array -> the handle's scalar, and the rows are cleared; non-uniform -> the rows; a wrong row count is refused."""
    off = _engine(predictor_type="ODE")
    off.apply_pole_mass_of(SimpleNamespace(m_pole=np.array([0.125, 0.125], f32)))
    assert off.lib.calls == [("scalar", 0.125)]
    with pytest.raises(NotImplementedError, match="m_pole must be the same for every env of a handle.*per_env_pole_mass"):
        off.apply_pole_mass_of(SimpleNamespace(m_pole=np.array([0.1, 0.2], f32)))
    assert off.lib.calls == [("scalar", 0.125)]
    on = _engine(predictor_type="ODE", per_env_pole_mass=True)
    vp = SimpleNamespace(m_pole=0.1)
    on.apply_pole_mass_of(vp, rows=3)
    assert on.lib.calls == [("scalar", float(f32(0.1)))]                       # (no rows registered: nothing to clear)
    vp.m_pole = np.array([0.05, 0.1, 0.15], f32)
    on.apply_pole_mass_of(vp, rows=3)
    assert on.lib.calls[-1] == ("rows", "ptr", 3) and np.array_equal(on._m_rows.numpy(), vp.m_pole)
    n = len(on.lib.calls)
    vp.m_pole[:] = (0.06, 0.11, 0.16)                                           # assigned in place: uploaded again, same buffer - no new registration
    on.apply_pole_mass_of(vp, rows=3)
    assert len(on.lib.calls) == n and np.array_equal(on._m_rows.numpy(), vp.m_pole)
    vp.m_pole = np.full(3, 0.1, f32)                                            # a uniform array after a non-uniform one clears the rows
    on.apply_pole_mass_of(vp, rows=3)
    assert on.lib.calls[n:] == [("rows", None, 0)] and on._m_rows is None       # (0.1 is the scalar already in force)
    vp.m_pole = np.array([0.05, 0.1, 0.15], f32)
    on.apply_pole_mass_of(vp, rows=3)
    same = 0.2
    vp.m_pole = same
    on.apply_pole_mass_of(vp, rows=3)
    assert on.lib.calls[-2:] == [("rows", None, 0), ("scalar", float(f32(0.2)))]
    vp.m_pole = np.array([0.05, 0.1, 0.15], f32)
    on.apply_pole_mass_of(vp, rows=3)
    vp.m_pole = same                                                            # the same float object as before the rows: still applied
    on.apply_pole_mass_of(vp, rows=3)
    assert on.lib.calls[-1] == ("rows", None, 0) and on._m_rows is None
    with pytest.raises(ValueError, match="2 entries, the call has 3 rows"):
        on.apply_pole_mass_of(SimpleNamespace(m_pole=np.array([0.1, 0.2], f32)), rows=3)
    v0 = _engine(per_env_pole_mass=True)                                        # predictor_ODE_v0 never reads the attribute
    v0.apply_pole_mass_of(SimpleNamespace(m_pole=np.array([0.1, 0.2], f32)))
    assert v0.lib.calls == []


def test_set_pole_mass_rows_validates_before_any_library_call():
    eng = _engine(predictor_type="ODE", per_env_pole_mass=True)
    for bad, rows in (([0.1, 0.0, 0.2], None), ([0.1, -0.05], None), ([0.1, np.nan], None), ([0.1, np.inf], None), ([], None),
                      ([[0.1, 0.2]], None), ([0.1, 0.2], 3)):
        with pytest.raises(ValueError):
            eng.set_pole_mass_rows(np.array(bad, f32), rows)
    assert eng.lib.calls == [] and eng._m_rows is None
    eng.set_pole_mass_rows(None)                                                # nothing registered: no call either
    assert eng.lib.calls == []
    v0 = _engine(predictor_type="ODE_v0")
    with pytest.raises(ValueError, match="predictor_type 'ODE' only"):
        v0.set_pole_mass_rows(np.array([0.1, 0.2], f32))
    assert v0.lib.calls == []
    eng.set_pole_mass_rows([0.1, 0.2])
    eng.set_pole_mass_rows(None)
    assert eng.lib.calls == [("rows", "ptr", 2), ("rows", None, 0)]


def test_optimizers_and_predictors_carry_the_flag(monkeypatch):
    """controller_mpc's config key reaches the MPPIConfig of every optimizer and of the predictor seam; the optimizers hand
    num_envs as the row count, the predictors the batch of s."""
    from cartpolesimulation_amd import predictors as P
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem, optimizer_cem_gmm, optimizer_cem_grad_bharadhwaj, \
        optimizer_cem_naive_grad, optimizer_random_action
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    from cartpolesimulation_amd.optimizer_mppi import optimizer_mppi
    for cls in (optimizer_mppi, optimizer_cem, optimizer_cem_gmm, optimizer_cem_naive_grad, optimizer_cem_grad_bharadhwaj,
                optimizer_random_action, optimizer_gradient, optimizer_rpgd):
        assert cls(num_envs=3, per_env_pole_mass=True).cfg.per_env_pole_mass is True, cls.__name__
        o = cls(num_envs=3)
        assert o.cfg.per_env_pole_mass is False and o._mass_rows == {}, cls.__name__
    assert optimizer_rpgd(num_envs=3, per_env_pole_mass=True)._mass_rows == {"rows": 3}

    class Reached(Exception):
        pass

    def reached(*a, **kw):
        raise Reached

    # ... and through the engine: with the flag, rows of num_envs entries are registered and another count is refused; without it
    # the scalar route is what it was
    for flag, m, calls in ((True, [0.05, 0.1, 0.15], [("rows", "ptr", 3)]), (False, [0.125] * 3, [("scalar", 0.125)])):
        for cls in (optimizer_mppi, optimizer_cem, optimizer_rpgd):
            o = cls(num_envs=3, per_env_pole_mass=flag, variable_parameters=SimpleNamespace(m_pole=np.array(m, f32)))
            o.cfg.predictor_type = "ODE"
            o.engine = _engine(predictor_type="ODE", per_env_pole_mass=flag)
            o.engine.tensor = reached
            with pytest.raises(Reached):
                o.step(torch.zeros(3, 6))
            assert o.engine.lib.calls == calls, (cls.__name__, flag)
            if flag:
                o.variable_parameters.m_pole = np.array([0.1, 0.2], f32)
                with pytest.raises(ValueError, match="2 entries, the call has 3 rows"):
                    o.step(torch.zeros(3, 6))

    made = []

    def fake_engine(horizon, dt, n, phys, math_mode, device, ptype="ODE_v0", **flags):
        eng = _engine(mpc_horizon=horizon, predictor_type=ptype, **flags)
        eng.tensor = lambda x, shape=None: torch.as_tensor(np.asarray(x, dtype=f32))
        eng.predict = lambda *a, **kw: (_ for _ in ()).throw(Reached(kw.get("L")))
        made.append(eng)
        return eng

    monkeypatch.setattr(P, "_engine", fake_engine)
    s, Q = np.zeros((2, 6), f32), np.zeros((2, 3, 1), f32)
    vp = SimpleNamespace(m_pole=np.array([0.1, 0.2], f32), L=np.array([0.3, 0.4], f32))
    for make, call in ((lambda: P.next_state_predictor_ODE(0.02, 2, variable_parameters=vp, per_env_pole_mass=True), lambda p: p.step(s, Q[:, 0])),
                       (lambda: P.predictor_ODE(3, 0.02, 2, variable_parameters=vp, per_env_pole_mass=True), lambda p: p.predict_core(s, Q))):
        p = make()
        with pytest.raises(Reached) as ei:
            call(p)
        assert made[-1].mppi.per_env_pole_mass and made[-1].lib.calls == [("rows", "ptr", 2)]
        assert np.array_equal(np.asarray(ei.value.args[0]), vp.L)               # L per row too, as the reference broadcasts it
    w = P.PredictorWrapper(per_env_pole_mass=True)
    w.configure(batch_size=2, horizon=3, dt=0.02, predictor_specification="ODE", variable_parameters=vp)
    assert made[-1].mppi.per_env_pole_mass and isinstance(w.predictor, P.predictor_ODE)
    v0 = P.predictor_ODE_v0(3, 0.02, 2, variable_parameters=vp, per_env_pole_mass=True)   # ODE_v0: the flag has nothing to switch
    assert not made[-1].mppi.per_env_pole_mass and v0._per_row is False


def _batch(E, prm, seed=79):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=35, length_of_experiment=0.3, keep_target_equilibrium_x_seconds_up=0.1, turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 20.0], angleD=40.0, position=0.4, positionD=0.2)))
    return SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(E, seed, stride=1), prm, seed=5)


RANDOM_M = dict(init_value="random", change_every_x_seconds=0.04, mode="random", range_random=[0.015, 0.15], range_clip=None,
                increment=0.002, reset_every_x_seconds="inf")
SWITCHING_RANDOM = dict(mode="switching_random", change_to_on_after_x_seconds_off=0.06, change_to_off_after_x_seconds_on=0.08)


def test_controller_mass_table_per_experiment():
    """`m_pole: mode random, init_value random` with a 'switching_random' informer: at controller call c experiment e is handed its
    true mass where ITS informer says told, its own initial mass otherwise - restated experiment by experiment."""
    from cartpolesimulation_amd.harness import controller_pole_mass
    E = 4
    b = _batch(E, dict(m_pole=RANDOM_M, inform_controller_about_parameters_change=SWITCHING_RANDOM))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # the one-mass warning is not for this path
        m_ctrl, m_env = controller_pole_mass(b, per_env=True)
    assert m_ctrl is None and m_env.shape == (b.n_periods + 1, E) and m_env.dtype == f32
    told_any = untold_any = False
    for e in range(E):
        for c in range(b.n_periods + 1):
            step = min(c * b.n_ctrl, b.m_pole_table.shape[0] - 1)
            told = bool(b.informed[step, e])
            assert m_env[c, e] == (b.m_pole_table[step, e] if told else b.m_pole_table[0, e]), (c, e)
            told_any |= told and b.m_pole_table[step, e] != b.m_pole_table[0, e]
            untold_any |= not told
    assert told_any and untold_any and not (m_env == m_env[:, :1]).all() and not (m_env == m_env[:1]).all()
    assert controller_pole_mass(b, per_env=False) == (None, None)               # without the flag: the handle's mass, as before
    # constant in time, different between experiments (`init_value: random`, `mode: constant`)
    const = _batch(E, dict(m_pole=dict(RANDOM_M, mode="constant")))
    _, m_const = controller_pole_mass(const, per_env=True)
    assert (m_const == m_const[:1]).all() and len(np.unique(m_const[0])) == E and np.array_equal(m_const[0], const.m_pole_table[0])


def test_uniform_schedule_keeps_the_scalar_path():
    """A deterministic updater gives every experiment the same schedule: one value per call with or without the flag (the path
    test_controller_pole_mass_follows_a_uniform_schedule_with_predictor_ODE pins on the GPU); only where the INFORMER differs between
    experiments does the flag change the outcome - a table per experiment instead of the warning."""
    from cartpolesimulation_amd.harness import controller_pole_mass
    E = 3
    inc = dict(init_value=0.087, change_every_x_seconds=0.02, mode="increase", range_random=[0.015, 0.3], range_clip=[0.015, 0.3],
               increment=0.02, reset_every_x_seconds="inf")
    regular = dict(mode="switching_regular", change_to_on_after_x_seconds_off=0.04, change_to_off_after_x_seconds_on=0.1)
    b = _batch(E, dict(m_pole=inc, inform_controller_about_parameters_change=regular))
    calls = np.arange(b.n_periods + 1) * b.n_ctrl
    want = np.where(b.informed[calls, 0], b.m_pole_table[calls, 0], f32(0.087)).astype(f32)
    for per_env in (False, True):
        m_ctrl, m_env = controller_pole_mass(b, per_env=per_env)
        assert m_env is None and m_ctrl.ndim == 1 and np.array_equal(m_ctrl, want) and len(np.unique(want)) > 4
    b2 = _batch(E, dict(m_pole=inc, inform_controller_about_parameters_change=SWITCHING_RANDOM))
    with pytest.warns(UserWarning, match="informer differs between experiments"):
        assert controller_pole_mass(b2, per_env=False) == (None, None)
    m_ctrl, m_env = controller_pole_mass(b2, per_env=True)
    assert m_ctrl is None and np.array_equal(m_env, np.where(b2.informed[calls], b2.m_pole_table[calls], f32(0.087)))


def test_controller_mass_is_decided_on_the_host():
    """harness.ControllerMass, built from the batch and the engine's MPPIConfig alone (nothing is bound, no device is touched): which
    of the two ways the controller is told its pole mass, and whether the mass changes between calls - the one rule behind "no
    captured graph" and "one cpmppi_groups_run per period"."""
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.harness import ControllerMass, controller_pole_mass
    E = 3
    ode, rows = MPPIConfig(predictor_type="ODE"), MPPIConfig(predictor_type="ODE", per_env_pole_mass=True)
    inc = dict(init_value=0.087, change_every_x_seconds=0.02, mode="increase", range_random=[0.015, 0.3], range_clip=[0.015, 0.3],
               increment=0.02, reset_every_x_seconds="inf")
    regular = dict(mode="switching_regular", change_to_on_after_x_seconds_off=0.04, change_to_off_after_x_seconds_on=0.1)

    def facts(m):
        assert (m.values is None) == (m.kind != "value") and (m.table is None) == (m.kind != "rows")
        assert m.engines == [] and m.rows is None and m.rows_table is None and not m.registered
        return m.kind, m.varies

    plain = _batch(E, {})
    assert plain.m_pole_table is None
    for cfg in (MPPIConfig(), ode, rows):
        assert facts(ControllerMass(plain, cfg)) == ("none", False)
    uniform = _batch(E, dict(m_pole=inc, inform_controller_about_parameters_change=regular))
    for cfg in (ode, rows):
        m = ControllerMass(uniform, cfg)
        assert facts(m) == ("value", True) and np.array_equal(m.values, controller_pole_mass(uniform)[0])
    assert facts(ControllerMass(uniform, MPPIConfig())) == ("none", False)      # predictor_ODE_v0 never reads the attribute
    differing = _batch(E, dict(m_pole=RANDOM_M, inform_controller_about_parameters_change=SWITCHING_RANDOM))
    m = ControllerMass(differing, rows)
    assert facts(m) == ("rows", True) and np.array_equal(m.table, controller_pole_mass(differing, per_env=True)[1])
    assert facts(ControllerMass(differing, ode)) == ("none", False)
    constant = _batch(E, dict(m_pole=dict(RANDOM_M, mode="constant")))
    m = ControllerMass(constant, rows)
    assert facts(m) == ("rows", False) and len(np.unique(m.table[0])) == E
    informers = _batch(E, dict(m_pole=inc, inform_controller_about_parameters_change=SWITCHING_RANDOM))
    with pytest.warns(UserWarning, match="informer differs between experiments"):
        assert facts(ControllerMass(informers, ode)) == ("none", False)
    assert facts(ControllerMass(informers, rows)) == ("rows", True)
    # a schedule that never changes the one mass: a value per call that does not vary (a graph may replay it)
    still = ControllerMass(_batch(E, dict(m_pole=dict(inc, mode="constant"))), ode)
    assert facts(still) == ("value", False) and (still.values == f32(0.087)).all()
    # nothing bound: nothing to apply to and nothing to release
    still.apply(0)
    still.release()


def test_controller_mass_gives_every_engine_its_slice():
    """bind / apply / release over stand-in engines (host tensors, recorded library calls): env groups register their OWN slices -
    no handle is ever handed the full vector -, row c is what the vector holds after apply(c), release unregisters once, and a
    binding with register=False (a run paced by an optimizer object) keeps the vector filled without touching any handle."""
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.harness import ControllerMass
    E, slices = 5, [(0, 3), (3, 5)]
    cfg = MPPIConfig(predictor_type="ODE", per_env_pole_mass=True)

    def engines(n):
        out = [_engine(predictor_type="ODE", per_env_pole_mass=True) for _ in range(n)]
        for e in out:
            e.launch_stream = lambda: None                                       # (torch.cuda.stream(None) is no context at all)
        return out

    b = _batch(E, dict(m_pole=RANDOM_M, inform_controller_about_parameters_change=SWITCHING_RANDOM))
    m, engs = ControllerMass(b, cfg), engines(2)
    m.bind(engs, slices)
    assert [e.lib.calls for e in engs] == [[("rows", "ptr", 3)], [("rows", "ptr", 2)]] and m.registered
    for c in (0, 3, b.n_periods):
        m.apply(c)
        assert np.array_equal(m.rows.numpy(), m.table[c]) and [len(e.lib.calls) for e in engs] == [1, 1], c
    m.release()
    m.release()
    assert [e.lib.calls[1:] for e in engs] == [[("rows", None, 0)]] * 2 and not m.registered
    # constant in time: filled at call 0 only
    m, (one,) = ControllerMass(_batch(E, dict(m_pole=dict(RANDOM_M, mode="constant"))), cfg), engines(1)
    m.bind([one])
    assert one.lib.calls == [("rows", "ptr", E)] and m.slices == [(0, E)]
    m.apply(0)
    m.rows.zero_()
    m.apply(1)
    assert not m.rows.any()
    # an optimizer object's run: the vector is kept filled, the handle is left alone; the optimizer is handed the vector itself
    m, (one,) = ControllerMass(b, cfg), engines(1)
    m.bind([one], register=False)
    assert m.for_optimizer(2) is m.rows and np.array_equal(m.rows.numpy(), m.table[2])
    m.release()
    assert one.lib.calls == []
    # one value per call: the scalar goes to every engine, no rows anywhere
    inc = dict(init_value=0.087, change_every_x_seconds=0.02, mode="increase", range_random=[0.015, 0.3], range_clip=[0.015, 0.3],
               increment=0.02, reset_every_x_seconds="inf")
    m, engs = ControllerMass(_batch(E, dict(m_pole=inc)), cfg), engines(2)
    m.bind(engs, slices)
    m.apply(2)
    m.release()
    assert m.kind == "value" and m.rows is None and [e.lib.calls for e in engs] == [[("scalar", float(m.values[2]))]] * 2
    assert m.for_optimizer(3) == float(m.values[3]) and [len(e.lib.calls) for e in engs] == [1, 1]
