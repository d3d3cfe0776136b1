"""CPU: the host side of the per-env rows of the fused rpgd / gradient step (cpmppi_rpgd_step_rows) - the export and the row
indices against the header text, configs.rpgd_rows (packing, defaults, its three errors), the sweep's grid per controller, what the
optimizers' constructors refuse, the rows' way from the optimizer into the prepared call, and the argument block such a call is
built with (the stand-in engines of test_rpgd_fused_host.py and test_engine_calls_host.py: no device, no library call)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_engine_calls_host import Engine, fields_of  # noqa: E402
from test_optimizers_host_logic import _states  # noqa: E402
from test_rpgd_fused_host import RPGD, FusedFake, fused_engine  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_export_row_indices_and_abi_history():
    from cartpolesimulation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    assert "cpmppi_rpgd_step_rows" in _lib.EXPORTS and hasattr(lib, "cpmppi_rpgd_step_rows")
    assert re.search(r"int cpmppi_rpgd_step_rows\(cpmppi_handle\* h, const cpmppi_rpgd_args\* args,\s*const float\* rows, uint32_t n_rows, "
                     r"void\* stream\);", text)
    assert f"#define CPMPPI_RPGD_ROW_LR {_lib.RPGD_ROW_LR}\n" in text and f"#define CPMPPI_RPGD_ROW_GRADMAX_CLIP {_lib.RPGD_ROW_GRADMAX_CLIP}\n" in text
    assert (_lib.RPGD_ROW_LR, _lib.RPGD_ROW_GRADMAX_CLIP) == (7, 8) and _lib.RPGD_ROW_GRADMAX_CLIP < _lib.TUNING_ROW_FLOATS
    params = open(os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_params.hpp")).read()
    assert f"RPGD_ROW_LR = {_lib.RPGD_ROW_LR}, RPGD_ROW_GRADMAX_CLIP = {_lib.RPGD_ROW_GRADMAX_CLIP};" in params
    # a new entry point: no layout changes, recorded in the history of ABI 5
    assert _lib.ABI_VERSION == 5 and "#define CPMPPI_ABI_VERSION 5u" in text
    history = raw[raw.index("#define CPMPPI_ABI_VERSION"):raw.index("#define CPMPPI_STATE_DIM")]
    assert "cpmppi_rpgd_step_rows (a new entry point, likewise)" in history
    assert lib.cpmppi_rpgd_step_rows.argtypes == [C.c_void_p, C.POINTER(_lib.cpmppi_rpgd_args), C.c_void_p, C.c_uint32, C.c_void_p]
    # every function the header declares is exported by the binding, and the other way round
    assert set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text)) == set(_lib.EXPORTS)


def test_row_packing_order_defaults_and_the_three_errors():
    from cartpolesimulation_amd import _lib
    from cartpolesimulation_amd.configs import COST_WEIGHTS, RPGD_ROW_COLUMNS, MPPIConfig, build_c_config, rpgd_rows
    assert RPGD_ROW_COLUMNS == tuple(COST_WEIGHTS["quadratic_boundary_grad_minimal"][1]) + ("learning_rate", "gradmax_clip")
    assert RPGD_ROW_COLUMNS.index("learning_rate") == _lib.RPGD_ROW_LR and RPGD_ROW_COLUMNS.index("gradmax_clip") == _lib.RPGD_ROW_GRADMAX_CLIP
    m = MPPIConfig(cost_weights=dict(ep_weight_up=55.0))
    c = build_c_config(4, m)
    rows = rpgd_rows(m, 4, 0.05, 5)
    assert rows.shape == (4, _lib.TUNING_ROW_FLOATS) and rows.dtype == f32
    for e in range(4):          # defaults: exactly the floats the handle is created with, in cpmppi_set_cost_weights order
        assert list(rows[e, :7]) == [f32(x) for x in list(c.cost_w)[:7]] and rows[e, 2] == f32(55.0)
        assert rows[e, 7] == f32(0.05) and rows[e, 8] == f32(5.0) and not rows[e, 9:].any()
    # columns per env and scalars for all; a clip <= 0 (off) is a value like any other
    rows = rpgd_rows(m, 3, [0.02, 0.05, 0.1], [0, 2, 5], permissible_track_fraction=0.5, R=[1, 2, 3])
    assert list(rows[:, 7]) == [f32(0.02), f32(0.05), f32(0.1)] and list(rows[:, 8]) == [0, 2, 5]
    assert list(rows[:, 6]) == [0.5] * 3 and list(rows[:, 5]) == [1, 2, 3] and list(rows[:, 2]) == [55.0] * 3
    for bad in ("LBD", "SQRTRHOINV", "ep_weight", "sample_stdev"):
        with pytest.raises(ValueError, match=f"'{bad}'.*available: dd_quadratic_weight_up.*learning_rate, gradmax_clip"):
            rpgd_rows(m, 3, 0.05, 5, **{bad: 1.0})
    with pytest.raises(ValueError, match="one value per env"):
        rpgd_rows(m, 3, [0.1, 0.2], 5)
    with pytest.raises(ValueError, match="'ep_weight_up' must be a scalar or one value per env"):
        rpgd_rows(m, 3, 0.05, 5, ep_weight_up=[[1, 2, 3]])
    with pytest.raises(ValueError, match="quadratic_boundary_grad_minimal, not 'default'"):
        rpgd_rows(MPPIConfig(cost_function_specification="default"), 3, 0.05, 5)


def test_grid_columns_per_controller():
    from cartpolesimulation_amd.configs import RPGD_ROW_COLUMNS, TUNING_COLUMNS
    from cartpolesimulation_amd.sweep import expand_grid, grid_columns
    assert grid_columns() == grid_columns("mppi") == TUNING_COLUMNS
    assert grid_columns("rpgd") == grid_columns("gradient") == RPGD_ROW_COLUMNS
    for name in ("rpgd", "gradient"):
        names, settings = expand_grid(dict(ep_weight_up=[20, 40], learning_rate=[0.02, 0.1]), name)
        assert names == ["ep_weight_up", "learning_rate"]
        assert [(s["ep_weight_up"], s["learning_rate"]) for s in settings] == [(20, 0.02), (20, 0.1), (40, 0.02), (40, 0.1)]
        assert expand_grid(dict(gradmax_clip=[0, 5]), name)[1] == [dict(gradmax_clip=0.0), dict(gradmax_clip=5.0)]
        for bad in ("LBD", "SQRTRHOINV"):
            with pytest.raises(ValueError, match=f"'{bad}'; available: {', '.join(RPGD_ROW_COLUMNS)}$"):
                expand_grid({bad: [1.0]}, name)
    # the MPPI step's grid is what it was, under both of its names
    for name in (None, "mppi"):
        assert expand_grid(dict(LBD=[50, 100]), name)[1] == [dict(LBD=50.0), dict(LBD=100.0)]
        with pytest.raises(ValueError, match=f"'learning_rate'; available: {', '.join(TUNING_COLUMNS)}$"):
            expand_grid(dict(learning_rate=[0.1]), name)
    with pytest.raises(ValueError, match="optimizer='cem'"):
        expand_grid(dict(LBD=[1]), "cem")


@pytest.mark.parametrize("name", ["rpgd", "gradient"])
def test_the_constructors_four_refusals(name):
    from cartpolesimulation_amd import optimizer_gradient as OG
    from cartpolesimulation_amd.configs import MPPIConfig, rpgd_rows
    cls = {"rpgd": OG.optimizer_rpgd, "gradient": OG.optimizer_gradient}[name]
    rows = rpgd_rows(MPPIConfig(), 2, 0.05, 5)
    kw = dict(seed=1, mpc_horizon=8, num_rollouts=8, num_envs=2)
    with pytest.raises(ValueError, match=r"rows= needs fused=True.*cpmppi_rpgd_step_rows"):
        cls(rows=rows, **kw)
    model = {"w": np.zeros(1)}
    with pytest.raises(ValueError, match=r"rows= with gru_model / gru_fused"):
        cls(rows=rows, fused=True, gru_model=model, gru_adjoint=True, **kw)
    with pytest.raises(ValueError, match=r"rows= with gru_model / gru_fused"):
        cls(rows=rows, gru_fused=True, gru_model=model, **kw)
    for bad in (rows[:1], rows[:, :9], np.zeros((3, 16), f32), np.zeros(16, f32)):
        with pytest.raises(ValueError, match=r"rows must be \[num_envs=2, 16\]"):
            cls(rows=bad, fused=True, **kw)
    for cost in ("default", "quadratic_boundary_grad"):
        with pytest.raises(ValueError, match=f"rows= holds the cost vector of quadratic_boundary_grad_minimal, not '{cost}'"):
            cls(rows=rows, fused=True, cost_function_specification=cost, **kw)
    opt = cls(rows=rows, fused=True, **kw)                          # ... and the constructor takes what it should
    assert opt.fused and opt.rows is rows
    with pytest.raises(ValueError, match=r"rows= with gru_model / gru_fused"):
        opt.configure(predictor_specification="GRU-6IN-32H1-32H2-5OUT-0")
    assert cls(fused=True, **kw).rows is None and cls(**kw).rows is None


def test_the_rows_travel_inside_the_optimizer_into_the_prepared_call(fused_engine):
    from cartpolesimulation_amd.configs import MPPIConfig, rpgd_rows
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    s = _states(2)
    rows = rpgd_rows(MPPIConfig(), 2, [0.02, 0.1], 5)
    r = optimizer_rpgd(fused=True, rows=rows, **RPGD)
    r.configure()
    assert torch.is_tensor(r.rows) and r.rows.dtype == torch.float32 and np.array_equal(r.rows.numpy(), rows)
    kept = r.rows
    for _ in range(3):
        r.step(s)
    assert all(launch["rows"] is kept for launch in r.engine.fused_launches) and len(r.engine.fused_launches) == 3
    counter = torch.zeros(1, dtype=torch.int64)
    tp, te = torch.zeros(2), torch.ones(2)
    r.step_device(torch.as_tensor(s, dtype=torch.float32), tp, te, count_dev=counter)
    assert r.engine.fused_launches[-1]["rows"] is kept and r.engine.fused_launches[-1]["count_dev"] is counter
    r.optimizer_reset()                                              # a reset keeps the tensor (a caller may hold it to rewrite it)
    r.step(s)
    assert r.rows is kept and r.engine.fused_launches[-1]["rows"] is kept
    g = optimizer_gradient(seed=1, mpc_horizon=8, num_rollouts=6, gradient_steps=3, num_envs=2, fused=True, rows=rows)
    g.configure()
    g.step(s)
    assert np.array_equal(g.engine.fused_launches[-1]["rows"].numpy(), rows)
    # without rows the prepared call is asked for none: the plain entry point
    p = optimizer_rpgd(fused=True, **RPGD)
    p.configure()
    p.step(s)
    assert "rows" not in p.engine.fused_launches[-1]
    # an env count given to configure() is checked against the rows as the constructor's is
    with pytest.raises(ValueError, match=r"rows must be \[num_envs=3, 16\]"):
        optimizer_rpgd(fused=True, rows=rows, **RPGD).configure(num_envs=3)


class BlockEngine(Engine):
    """test_engine_calls_host's stand-in plus what MPPIEngine._build_rpgd_step reads: the shape, host tensors, entry points that
    record their arguments."""
    E, N, H = 4, 8, 5

    def __init__(self):
        from cartpolesimulation_amd.engine import MPPIEngine
        super().__init__()
        self.device = torch.device("cpu")
        self.lib = types.SimpleNamespace(cpmppi_rpgd_step=self.entry("plain"), cpmppi_rpgd_step_rows=self.entry("rows", rc=23))
        for name in ("tensor", "empty", "_per_env", "_control_inputs", "_outputs", "_build_rpgd_step"):
            setattr(self, name, types.MethodType(getattr(MPPIEngine, name), self))


def test_the_argument_block_of_a_rows_call(monkeypatch):
    """The one builder, the one prepared-call type: with rows the block is field for field the plain call's, and `run` hands
    (handle, block, rows' address, rows' count, stream) to cpmppi_rpgd_step_rows; the rows tensor lives as long as the call."""
    import cartpolesimulation_amd.engine as EN
    # (host tensors stand in for device tensors: the dense half of the check stays)
    monkeypatch.setattr(EN, "device_tensor", lambda name, t, dtype=torch.float32, tail=None, note="":
                        t if EN.is_dense(t, dtype, tail) else (_ for _ in ()).throw(ValueError(f"{name} must be a contiguous tensor")))
    eng = BlockEngine()
    E, N, H = 3, eng.N, eng.H
    Q, m, v = (torch.zeros(E, N, H) for _ in range(3))
    s0, tp, te, Lv = torch.zeros(E, 6), torch.zeros(E), torch.ones(E), torch.full((E,), 0.4)
    u = torch.zeros(E)
    rows = torch.zeros(eng.E, 16)
    kw = dict(iterations=4, learning_rate=0.05, gradmax_clip=5.0, keep_k=6, resamp_per=2, seed=9, draw_offset=3, Q_out=u)
    plain = eng._build_rpgd_step(s0, Q, m, v, tp, te, Lv, **kw)
    call = eng._build_rpgd_step(s0, Q, m, v, tp, te, Lv, rows=rows, **kw)
    assert type(call) is EN.PreparedCall and call.fields == plain.fields == ("count", "adam_iteration", "draw_offset", "iterations")
    assert fields_of(call.args) == fields_of(plain.args) and call.args.E == E and call.args.keep_k == 6
    assert any(t is rows for t in call.keep) and not any(t is rows for t in plain.keep)
    assert call.run(count=2, adam_iteration=8) is call.result and call.result[0] is u
    plain.run()
    (name, handle, ref, address, n_rows, stream), (pname, phandle, pref, pstream) = eng.enqueued
    assert (name, handle, stream) == ("rows", eng._h, "the stream") and ref is call.ref and ref._obj is call.args
    assert address.value == rows.data_ptr() and n_rows == eng.E                   # every row of the tensor, more than the call's envs
    assert (pname, phandle, pstream) == ("plain", eng._h, "the stream") and pref is plain.ref
    assert eng.checked == [23, 0] and call.args.count == 2 and call.args.adam_iteration == 8
    # fewer rows than envs, another width, another dtype: refused by the builder
    for bad in (rows[:2], torch.zeros(eng.E, 9), rows.double(), rows.numpy()):
        with pytest.raises(ValueError, match="rows"):
            eng._build_rpgd_step(s0, Q, m, v, tp, te, Lv, rows=bad, **kw)
