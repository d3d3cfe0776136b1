"""CPU-only: what training the GRU predictor needs off the GPU - the reference of the GPU tests against itself, the windows, the
normalisation vectors, the model-folder writer, the exports and argument block, and the refusals that precede any engine.

The reference against itself (tests/gru_train_ref.py): float32 autograd within 5e-6 of float64 autograd, per parameter tensor
relative to the tensor's max |g|, for (B, W, P) = (1,0,1), (33,3,4), (70,5,20), (64,10,50) and the weights of the random model
scaled x1 and x3.  Measured here: 6.9e-7 worst (loss 2.3e-7 relative) - the reference is conditioned three orders of magnitude
better than the 5e-4 the kernels are held to (tests/test_gpu_gru_train.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKOUT = os.path.join(ROOT, "tests", "golden", "reference_checkout")
f32 = np.float32
NEW = ("cpmppi_gru_train_reserve", "cpmppi_gru_loss_grad", "cpmppi_gru_train_begin", "cpmppi_gru_train_step", "cpmppi_gru_train_get")


def random_model(scale=1.0):
    from test_gpu_gru_edges import model_of
    m = dict(model_of("random"))
    return {k: (m[k] * f32(scale) if k in TR.GRU_KEYS else m[k]) for k in m}


# ---------------------------------------------------------------------------------------------- 1. the reference against itself
@pytest.mark.parametrize("B,W,P", [(1, 0, 1), (33, 3, 4), (70, 5, 20), (64, 10, 50)])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_reference_float32_against_float64(B, W, P, scale, capsys):
    from cartpolesimulation_amd.train_gru import make_windows
    states, Q = TR.random_recordings(3, 80)
    legal = make_windows([80] * 3, W, P, 1)
    windows = legal[np.random.Generator(np.random.SFC64(B + W + P)).integers(0, len(legal), B)]
    model = random_model(scale)
    l64, g64 = TR.loss_and_grad(model, states, Q, windows, W, P)
    l32, g32 = TR.loss_and_grad(model, states, Q, windows, W, P, dtype=torch.float32)
    worst = TR.worst_relative(g32, g64)
    with capsys.disabled():
        print(f"\n[train-ref] B {B} W {W} P {P} x{scale}: gradient {worst:.2e}, loss {abs(l32 - l64) / l64:.2e}")
    assert all(np.abs(g64[k]).max() > 0 for k in g64 if W + P > 1 or not k.startswith("w_hh"))
    assert worst < 5e-6
    assert abs(l32 - l64) <= 5e-6 * l64


def test_reference_loss_is_the_stated_mean():
    """One window by hand: numpy cell by cell (oracle_np.gru_cell) against the torch.nn.GRU restatement."""
    from oracle import oracle_np as O
    states, Q = TR.random_recordings(3, 40)
    m, (r, t0, W, P) = random_model(), (1, 7, 2, 3)
    h1, h2, err = np.zeros((1, 32)), np.zeros((1, 32)), []
    for j in range(W + P):
        raw = np.concatenate([[Q[r, t0 + j]], states[r, t0 + j, 1:]]).astype(np.float64)
        x = (raw * m["in_scale"] + m["in_shift"])[None]
        h1 = O.gru_cell(x, h1, m["w_ih0"], m["w_hh0"], m["b_ih0"], m["b_hh0"], dtype=np.float64)
        h2 = O.gru_cell(h1, h2, m["w_ih1"], m["w_hh1"], m["b_ih1"], m["b_hh1"], dtype=np.float64)
        y = h2 @ m["w_out"].astype(np.float64).T + m["b_out"]
        if j >= W:
            err.append(y[0] - (states[r, t0 + j + 1, 1:].astype(np.float64) - m["out_shift"]) / m["out_scale"])
    loss, _ = TR.loss_and_grad(m, states, Q, np.array([[r, t0]]), W, P)
    assert loss == pytest.approx(float(np.mean(np.square(err))), rel=1e-12)


# ---------------------------------------------------------------------------------------------- 2. windows
def test_make_windows_at_recording_ends_and_ragged_lengths():
    from cartpolesimulation_amd.train_gru import make_windows
    w = make_windows([10], 3, 4, 1)                         # last label row t0 + 3 + 4 - 1 + 1 <= 9: t0 <= 2
    assert w.tolist() == [[0, 0], [0, 1], [0, 2]]
    assert make_windows([10], 3, 4, 0).tolist() == [[0, 0], [0, 1], [0, 2], [0, 3]]
    assert make_windows([8], 3, 4, 1).tolist() == [[0, 0]]  # exactly one window fits
    assert make_windows([7], 3, 4, 1).shape == (0, 2)       # one row short
    w = make_windows([9, 3, 8, 0], 0, 6, 1)                 # ragged: the short recordings have none
    assert w.tolist() == [[0, 0], [0, 1], [0, 2], [2, 0], [2, 1]]
    assert make_windows([5], 0, 1, 1).tolist() == [[0, t] for t in range(4)]
    for bad in ((-1, 1, 1), (0, 0, 1), (0, 1, -1)):
        with pytest.raises(ValueError, match="wash_out >= 0, post_wash_out >= 1"):
            make_windows([10], *bad)


# ---------------------------------------------------------------------------------------------- 3. normalisation
def test_normalization_vectors_on_a_constructed_table():
    from cartpolesimulation_amd.train_gru import normalization_from_recordings
    T = 5
    states = np.zeros((2, T, 6), f32)
    lo = np.array([-2.0, -1.0, -0.5, 0.0, 1.0])            # angleD, cos, sin, position, positionD
    hi = np.array([6.0, 1.0, 0.5, 4.0, 3.0])
    states[0, :, 1:] = lo
    states[1, :, 1:] = hi
    states[:, :, 0] = 99.0                                   # the angle itself is no feature
    Q = np.array([[-0.5] * T, [0.25] * T], f32)
    n = normalization_from_recordings(states, Q)
    lo6, hi6 = np.concatenate([[-0.5], lo]), np.concatenate([[0.25], hi])
    assert n["in_scale"].dtype == f32 and n["out_shift"].shape == (5,)
    np.testing.assert_array_equal(n["in_scale"], (2 / (hi6 - lo6)).astype(f32))
    np.testing.assert_array_equal(n["in_shift"], (-(hi6 + lo6) / (hi6 - lo6)).astype(f32))
    np.testing.assert_array_equal(n["out_scale"], ((hi - lo) / 2).astype(f32))
    np.testing.assert_array_equal(n["out_shift"], ((hi + lo) / 2).astype(f32))
    np.testing.assert_allclose(lo6 * n["in_scale"] + n["in_shift"], -1.0, atol=1e-6)
    np.testing.assert_allclose(hi6 * n["in_scale"] + n["in_shift"], 1.0, atol=1e-6)
    np.testing.assert_allclose(n["out_scale"] * 1.0 + n["out_shift"], hi, atol=1e-6)     # the inverse
    # rows past a recording's length do not count
    states2 = states.copy()
    states2[1, 3:, 1] = 1000.0
    n2 = normalization_from_recordings(states2, Q, lengths=[T, 3])
    np.testing.assert_array_equal(n2["in_scale"], n["in_scale"])
    states3 = states.copy()
    states3[:, :, 4] = 0.3
    with pytest.raises(ValueError, match="position.*never vary"):
        normalization_from_recordings(states3, Q)


# ---------------------------------------------------------------------------------------------- 4. model folder
@pytest.mark.parametrize("with_norm", [True, False])
def test_write_model_folder_round_trip(tmp_path, with_norm):
    from cartpolesimulation_amd.model_folder import load_gru_model, read_net_info
    from cartpolesimulation_amd.train_gru import write_model_folder
    model = random_model()
    if not with_norm:
        model = {k: model[k] for k in TR.GRU_KEYS}
    folder = write_model_folder(tmp_path / "GRU-6IN-32H1-32H2-5OUT-0", model, info={"WASH OUT LENGTH": 5})
    back = load_gru_model(folder)
    assert set(back) == set(model)
    for k in model:
        assert back[k].dtype == f32
        np.testing.assert_array_equal(back[k], model[k], err_msg=k)
    info = read_net_info(folder)
    assert info["net_name"] == "GRU-32H1-32H2" and info["net_full_name"] == "GRU-6IN-32H1-32H2-5OUT-0"
    assert info["wash_out_length"] == "5" and info["inputs"][0] == "Q"
    with pytest.raises(ValueError, match="w_hh1 must have shape"):
        write_model_folder(tmp_path / "x", {**model, "w_hh1": np.zeros((96, 16), f32)})


# ---------------------------------------------------------------------------------------------- exports and argument block
def test_exports_and_argument_block(tmp_path):
    import shutil
    import subprocess
    from cartpolesimulation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpmppi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "#define CPMPPI_GRU_PARAMS 10341u" in text and _lib.GRU_PARAMS == 10341
    assert 2 * (96 * 6 + 96 * 32 + 96 + 96) + (96 * 32 - 96 * 6) + 5 * 32 + 5 == 10341
    body = text[text.index("uint32_t B;"):text.index("} cpmppi_gru_loss_args;")]
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            names = decl.rsplit("*", 1)[1] if "*" in decl else decl.split(None, 1)[1]
            fields += [x.strip() for x in names.split(",")]
    A = _lib.cpmppi_gru_loss_args
    assert fields == [f[0] for f in A._fields_]
    assert C.sizeof(A) == 6 * 4 + 6 * 8
    gcc = shutil.which("gcc")
    if gcc is not None:
        src = tmp_path / "sz.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cpmppi.h"\n'
                       'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(cpmppi_gru_loss_args), offsetof(cpmppi_gru_loss_args, '
                       'shift_labels), offsetof(cpmppi_gru_loss_args, states), offsetof(cpmppi_gru_loss_args, grad_out)); return 0; }\n')
        exe = tmp_path / "sz"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [C.sizeof(A), A.shift_labels.offset, A.states.offset, A.grad_out.offset]
    import __graft_entry__
    assert "cpmppi_gru_train.hip" in __graft_entry__.HIP_UNITS


def test_flat_parameter_order():
    from cartpolesimulation_amd.engine import MPPIEngine
    model = random_model()
    flat = MPPIEngine.gru_flatten(model)
    assert flat.shape == (10341,) and flat.dtype == f32
    np.testing.assert_array_equal(flat, TR.flatten(model))
    back = MPPIEngine.gru_unflatten(flat)
    assert list(back) == list(MPPIEngine.GRU_KEYS)
    for k in back:
        np.testing.assert_array_equal(back[k], model[k])
    with pytest.raises(ValueError, match="10341"):
        MPPIEngine.gru_unflatten(flat[:-1])


# ---------------------------------------------------------------------------------------------- 5. refusals before any engine
def test_train_gru_refusals_before_any_engine():
    from cartpolesimulation_amd.train_gru import train_gru
    states, Q = TR.random_recordings(3, 40)
    kw = dict(epochs=1, batch_size=4, lr=1e-3, seed=0, wash_out=2, post_wash_out=3)
    with pytest.raises(ValueError, match=r"states must be \[R,T,6\]"):
        train_gru(None, states[:, :, :5], Q, **kw)
    with pytest.raises(ValueError, match="no recording holds a window of 30 \\+ 20 rows"):
        train_gru(None, states, Q, **{**kw, "wash_out": 30, "post_wash_out": 20})
    with pytest.raises(ValueError, match="epochs and batch_size"):
        train_gru(None, states, Q, **{**kw, "epochs": 0})
    with pytest.raises(ValueError, match="lengths must hold one length"):
        train_gru(None, states, Q, [40, 40], **kw)
    with pytest.raises(ValueError, match="weight w_ih0 must have shape \\(96, 6\\)"):
        train_gru(None, states, Q, init={**random_model(), "w_ih0": np.zeros((96, 7), f32)}, **kw)


def _config():
    import yaml
    with open(os.path.join(CHECKOUT, "SI_Toolkit_ASF", "config_training.yml")) as fh:
        return yaml.safe_load(fh)


def test_training_settings_from_the_shipped_file():
    from cartpolesimulation_amd.train_gru import training_settings
    s, normalize = training_settings(_config(), net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1, wash_out=10, post_wash_out=50)
    assert normalize is True
    assert s == dict(epochs=30, batch_size=64, seed=1873, lr=2.0e-3, reduce_lr_on_plateau=True, patience=2, decrease_factor=0.5,
                     minimal_lr=1.0e-7, min_delta=1.0e-6, wash_out=10, post_wash_out=50, shift_labels=1)


@pytest.mark.parametrize("change,kwargs,message", [
    ({}, dict(dynamics_model=True), "net 'Dense-32H1-32H2'.*built for GRU-32H1-32H2"),
    ({}, dict(net="LSTM-32H1-32H2", dynamics_model=True), "net 'LSTM-32H1-32H2'"),
    ({}, dict(net="GRU-64H1-64H2", dynamics_model=True), "net 'GRU-64H1-64H2'"),
    ({}, dict(net="GRU-32H1-32H2"), "Q_calculated.*pass --dynamics-model"),
    ({}, dict(net="GRU-32H1-32H2", dynamics_model=True), "SHIFT_LABELS 0.*--shift-labels 1"),
    ({"REGULARIZATION": {"ACTIVATED": True}}, dict(net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1), "REGULARIZATION.ACTIVATED"),
    ({"PRUNING": {"ACTIVATED": True}}, dict(net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1), "PRUNING.ACTIVATED"),
    ({"QUANTIZATION": {"ACTIVATED": True}}, dict(net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1), "QUANTIZATION.ACTIVATED"),
    ({"CONFIG_SERIES_MODIFICATION": {"MODE": "train_for_random_vertical_angle_shift"}},
     dict(net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1), "CONFIG_SERIES_MODIFICATION"),
    ({"FILTERS": [{"column": "angleD", "condition": "< 20.0"}]}, dict(net="GRU-32H1-32H2", dynamics_model=True, shift_labels=1), "FILTERS"),
])
def test_training_settings_refuse_by_name(change, kwargs, message):
    from cartpolesimulation_amd.train_gru import training_settings
    config = _config()
    config.update(change)
    with pytest.raises(ValueError, match=message):
        training_settings(config, **kwargs)


def test_command_line_refuses_by_name_before_any_engine(tmp_path):
    from cartpolesimulation_amd.train_gru import main
    base = ["--recordings", str(tmp_path), "--out", str(tmp_path / "model"), "--config-root", CHECKOUT]
    with pytest.raises(SystemExit, match="net 'Dense-32H1-32H2'.*pass --net GRU-32H1-32H2"):
        main(base)
    with pytest.raises(SystemExit, match="pass --dynamics-model"):
        main(base + ["--net", "GRU-32H1-32H2"])
    with pytest.raises(SystemExit, match="--shift-labels 1"):
        main(base + ["--net", "GRU-32H1-32H2", "--dynamics-model"])
    with pytest.raises(ValueError, match="no recording"):                # everything named; the folder is empty
        main(base + ["--net", "GRU-32H1-32H2", "--dynamics-model", "--shift-labels", "1"])
    assert not (tmp_path / "model").exists()
