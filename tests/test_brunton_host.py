"""CPU-only: the Brunton test's surface that needs no GPU - the two exports, the recording reader, the reference statistics
(tests/brunton_ref.py) and the refusals of brunton_test that precede any engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import brunton_ref as BR
from oracle import oracle_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_exports_and_abi():
    from cartpolesimulation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpmppi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text))
    lib = _lib.load()
    for name in ("cpmppi_brunton", "cpmppi_gru_washout"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.cpmppi_abi_version() == 5 and "#define CPMPPI_ABI_VERSION 5u" in text
    assert lib.cpmppi_gru_washout.argtypes is not None and len(lib.cpmppi_gru_washout.argtypes) == 8
    assert len(lib.cpmppi_brunton.argtypes) == 3
    # the ctypes mirror has the header's fields, in its order
    body = text[text.index("uint32_t R, T;"):text.index("} cpmppi_brunton_args;")]
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            names = decl.rsplit("*", 1)[1] if "*" in decl else decl.split(None, 1)[1]
            fields += [x.strip() for x in names.split(",")]
    assert fields == [f[0] for f in _lib.cpmppi_brunton_args._fields_]
    assert C.sizeof(_lib.cpmppi_brunton_args) == 6 * 4 + 6 * 8


def test_struct_layout_as_a_c_compiler_sees_it(tmp_path):
    import shutil
    import subprocess
    from cartpolesimulation_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cpmppi.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(cpmppi_brunton_args), offsetof(cpmppi_brunton_args, predictor), '
                   'offsetof(cpmppi_brunton_args, states), offsetof(cpmppi_brunton_args, pred_out)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.cpmppi_brunton_args
    assert got == [C.sizeof(A), A.predictor.offset, A.states.offset, A.pred_out.offset]


def test_load_recording_reads_what_write_recording_wrote(tmp_path):
    from cartpolesimulation_amd import recording as R
    from cartpolesimulation_amd.brunton import FEATURES, load_recording
    from cartpolesimulation_amd.configs import PhysicalParameters
    from test_recording import random_block
    rng = np.random.Generator(np.random.SFC64(11))
    T, E, env = 9, 3, 2
    phys = PhysicalParameters()
    block = random_block(rng, T, E)
    header = R.create_csv_header(0.18, 0.002, 0.02, 0.02, "mpc", "mppi", phys)
    path = R.write_recording(str(tmp_path / "rec.csv"), R.typed_columns(block, env, phys, q_update_time=0.25), header=header)
    rec = load_recording(path)
    assert set(rec) == {"time", "Q", "L", *FEATURES}
    for i, name in enumerate(FEATURES):
        assert rec[name].dtype == f32 and np.array_equal(rec[name].view(np.uint32), block["states"][:, env, i].view(np.uint32)), name
    assert np.array_equal(rec["Q"], block["Q"][:, env]) and np.array_equal(rec["L"], block["L"][:, env])       # Q_applied = Q here
    assert rec["time"].dtype == np.float64 and np.array_equal(rec["time"], block["time"])
    # the native writer's bytes are the csv module's (tests/test_recording.py), so one reader serves both; a file without the
    # columns is refused by name
    bad = tmp_path / "bad.csv"
    bad.write_text("# x\r\ntime,angle\r\n0.0,1.0\r\n")
    with pytest.raises(ValueError, match="angleD"):
        load_recording(str(bad))


def test_load_recording_reads_the_reference_written_rows(tmp_path, golden_dir):
    """tests/golden/schedule.npz "csv_rows": the rows of a file the reference's own CartPole class wrote - into the columns
    pandas.read_csv(comment='#'), the reader of the existing recording tests, gives."""
    pd = pytest.importorskip("pandas")
    from cartpolesimulation_amd.brunton import FEATURES, load_recording
    g = np.load(os.path.join(golden_dir, "schedule.npz"), allow_pickle=True)
    for key in ("exp_fine/0", "exp_varL/0"):
        path = tmp_path / (key.replace("/", "_") + ".csv")
        with open(path, "w", newline="") as f:
            f.write("# a recording\r\n#\r\n# Data:\r\n" + g[f"{key}/csv_rows"].item() + "\r\n")
        rec = load_recording(str(path))
        df = pd.read_csv(path, comment="#", float_precision="round_trip")
        assert len(df) > 10 and len(rec["Q"]) == len(df)
        for name in FEATURES:
            assert np.array_equal(rec[name], df[name].to_numpy().astype(f32)), (key, name)
        assert np.array_equal(rec["Q"], df["Q_applied"].to_numpy().astype(f32))
        assert np.array_equal(rec["L"], df["L"].to_numpy().astype(f32)) and np.array_equal(rec["time"], df["time"].to_numpy())


def small_case():
    """2 recordings x 30 rows made BY the oracle's ODE predictor from random controls, horizon 5."""
    rng = np.random.Generator(np.random.SFC64(41))
    R, T = 2, 30
    s0 = np.stack([O.create_cartpole_state(0.4, -1.0, 0.02, 0.1), O.create_cartpole_state(2.9, 3.0, -0.05, -0.2)])
    Q = rng.uniform(-1, 1, (R, T)).astype(f32)
    states = O.predict_core(s0, Q[:, :T - 1], integrator="ODE")
    return states, Q


def test_reference_statistics_against_the_oracle_predictor():
    """A recording the predictor itself produced has step-1 error exactly 0 under that predictor (which pins the alignment of start
    state, control and compared row: one row off in any of them and the error is of the size of a control step), later steps too
    (the same float32 chain); with other controls the vectorised statistics equal the start-by-start loops."""
    states, Q = small_case()
    start, count, H = 2, 20, 5
    s0, Qw, rec, _ = BR.windows(states, Q, start, count, H)
    assert s0.shape == (40, 6) and Qw.shape == (40, 5) and rec.shape == (40, 5, 6)
    assert np.array_equal(s0[20 + 3], states[1, 5]) and np.array_equal(Qw[20 + 3, 2], Q[1, 7]) and np.array_equal(rec[3, 4], states[0, 10])
    pred = O.predict_core(s0, Qw, integrator="ODE")
    st, a = BR.stats(pred, rec)
    assert st.shape == (5, 6, 3) and np.all(st == 0.0)
    off = O.predict_core(s0, np.roll(Qw, 1, axis=1), integrator="ODE")             # the controls one step late
    st, a = BR.stats(off, rec)
    assert st[0, 1, 2] > 1e-2                                                         # angleD after one step under another control
    loops = BR.by_loops(off, rec)
    np.testing.assert_allclose(st[:, :, :2], loops[:, :, :2], rtol=1e-12)
    assert np.array_equal(st[:, :, 2], loops[:, :, 2])
    # the wrap: a prediction 2 pi - 0.01 away from the recorded angle is 0.01 away
    wrapped = pred.copy()
    wrapped[:, 1:, 0] += f32(2 * np.pi - 0.01)
    st, a = BR.stats(wrapped, rec)
    assert abs(st[0, 0, 2] - 0.01) < 1e-6 and a[:, :, 0].max() < np.pi


def test_refusals_before_any_engine(monkeypatch):
    from cartpolesimulation_amd import brunton as B
    from cartpolesimulation_amd import engine as EN

    def no_engine(*a, **k):
        raise AssertionError("an engine was built before the arguments were checked")
    monkeypatch.setattr(EN, "MPPIEngine", no_engine)
    states, Q = small_case()
    with pytest.raises(NotImplementedError, match="'SGP_10'"):
        B.brunton_test((states, Q), predictors=("ODE", "SGP_10"), horizon=5)
    cols = [{**{n: states[r, :30 - 3 * r, i] for i, n in enumerate(B.FEATURES)}, "Q": Q[r, :30 - 3 * r], "time": None} for r in range(2)]
    with pytest.raises(ValueError, match="unequal lengths"):
        B.brunton_test(cols, horizon=5)
    with pytest.raises(ValueError, match="equal length"):
        B.brunton_test((states, Q[:, :-1]), horizon=5)
    with pytest.raises(ValueError, match="after decimation by 3"):
        B.brunton_test((states, Q), horizon=10, decimation=3)                       # 10 rows left, horizon 10
    with pytest.raises(ValueError, match="needs its weights"):
        B.brunton_test((states, Q), predictors=("GRU-6IN-32H1-32H2-5OUT-0",), horizon=5)
    with pytest.raises(ValueError, match="test_len"):
        B.brunton_test((states, Q), horizon=5, test_len=26)                         # 25 starts fit
