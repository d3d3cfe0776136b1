"""CPU-only: what training the GRU predictor through the open-loop rollout needs off the GPU - the exports, the reference of the GPU
tests against itself at every shape those tests use, its degenerate case, and what train_gru and its command line decide before
any engine.

The reference against itself (tests/gru_train_rollout_ref.py): at every (model, B, W, P) of tests/test_gpu_gru_train_rollout.py the
float32 realisation's gradient lies within a QUARTER of the project's bound (5e-4 of each tensor's max |g|) of the float64 one.
Measured here: 8.6e-7 worst - the feedback over at most 12 rows does not spoil the conditioning."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402
import gru_train_rollout_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("cpmppi_gru_rollout_loss_grad", "cpmppi_gru_rollout_train_step")
GRAD_TOL = 5e-4


# ---------------------------------------------------------------------------------------------- exports and header
def test_exports_header_and_argument_block():
    from cartpolesimulation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+CPMPPI_ABI_VERSION\s+5u?\b", raw) and lib.cpmppi_abi_version() == 5
    A = _lib.cpmppi_gru_loss_args
    assert [f[0] for f in A._fields_] == ["B", "R", "T", "wash_out", "post_wash_out", "shift_labels", "states", "Q", "windows",
                                          "windows_host", "loss_out", "grad_out"]
    assert C.sizeof(A) == 6 * 4 + 6 * 8 and A.shift_labels.offset == 20 and A.states.offset == 24 and A.grad_out.offset == 64
    assert lib.cpmppi_gru_rollout_loss_grad.argtypes == lib.cpmppi_gru_loss_grad.argtypes
    assert lib.cpmppi_gru_rollout_train_step.argtypes == lib.cpmppi_gru_train_step.argtypes
    # the semantics are stated where the teacher-forced ones are
    assert "cpmppi_gru_rollout_loss_grad: the same loss THROUGH THE OPEN-LOOP ROLLOUT" in raw and "shift_labels must be 1" in raw


# ---------------------------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("name,norm", RR.MODELS, ids=[f"{n}-{'norm' if k else 'identity'}" for n, k in RR.MODELS])
def test_reference_is_conditioned_at_every_shape_of_the_gpu_test(name, norm, capsys):
    states, Q = TR.random_recordings(RR.R, RR.T)
    model = RR.case_model(name, norm)
    worst = 0.0
    for B in RR.BATCHES:
        for W, P in RR.ROWS:
            w = RR.case_windows(B, W, P)
            l64, g64 = RR.loss_and_grad(model, states, Q, w, W, P)
            l32, g32 = RR.loss_and_grad(model, states, Q, w, W, P, dtype=torch.float32)
            rel = TR.worst_relative(g32, g64)
            worst = max(worst, rel)
            assert rel < GRAD_TOL / 4, (B, W, P, rel)
            assert abs(l32 - l64) <= GRAD_TOL / 4 * l64, (B, W, P)
    with capsys.disabled():
        print(f"\n[train-rollout-ref] {name} norm={norm}: float32 against float64, worst gradient {worst:.2e}")


@pytest.mark.parametrize("B,W", [(1, 0), (33, 3), (129, 0)])
def test_one_scored_row_is_the_teacher_forced_reference_exactly(B, W):
    states, Q = TR.random_recordings(RR.R, RR.T)
    model = RR.case_model("random", True)
    w = RR.case_windows(B, W, 1)
    for dtype in (torch.float64, torch.float32):
        l_r, g_r = RR.loss_and_grad(model, states, Q, w, W, 1, dtype=dtype)
        l_t, g_t = TR.loss_and_grad(model, states, Q, w, W, 1, dtype=dtype)
        assert l_r == l_t
        for k in TR.GRU_KEYS:
            assert np.array_equal(g_r[k], g_t[k]), k


def test_the_feedback_changes_the_loss_and_reads_only_the_controls_behind_the_start_row():
    """The reference's own rule, by hand: numpy cell by cell (oracle_np.gru_cell) with the outputs fed back unchanged; and rows
    behind row W matter through Q and the labels alone."""
    from oracle import oracle_np as O
    states, Q = TR.random_recordings(RR.R, RR.T)
    m, (r, t0, W, P) = RR.case_model("random", True), (1, 7, 2, 4)
    h1, h2, err, y = np.zeros((1, 32)), np.zeros((1, 32)), [], None
    for j in range(W + P):
        q = np.float64(Q[r, t0 + j]) * m["in_scale"][0] + m["in_shift"][0]
        if j <= W:
            feats = states[r, t0 + j, 1:].astype(np.float64) * m["in_scale"][1:] + m["in_shift"][1:]
        else:
            feats = y[0]
        x = np.concatenate([[q], feats])[None]
        h1 = O.gru_cell(x, h1, m["w_ih0"], m["w_hh0"], m["b_ih0"], m["b_hh0"], dtype=np.float64)
        h2 = O.gru_cell(h1, h2, m["w_ih1"], m["w_hh1"], m["b_ih1"], m["b_hh1"], dtype=np.float64)
        y = h2 @ m["w_out"].astype(np.float64).T + m["b_out"]
        if j >= W:
            err.append(y[0] - (states[r, t0 + j + 1, 1:].astype(np.float64) - m["out_shift"]) / m["out_scale"])
    w = np.array([[r, t0]])
    loss = RR.loss_only(m, states, Q, w, W, P)
    assert loss == pytest.approx(float(np.mean(np.square(err))), rel=1e-12)
    assert abs(loss - TR.loss_and_grad(m, states, Q, w, W, P)[0]) > 1e-3 * loss


# ---------------------------------------------------------------------------------------------- train_gru and the command line
def test_rollout_refuses_other_label_shifts_before_any_engine():
    from cartpolesimulation_amd.train_gru import run_settings, train_gru
    states, Q = TR.random_recordings(RR.R, RR.T)
    kw = dict(epochs=1, batch_size=4, lr=1e-3, seed=0, wash_out=2, post_wash_out=3)
    for shift in (0, 2):
        with pytest.raises(ValueError, match="shift_labels must be 1"):
            train_gru(None, states, Q, rollout=True, shift_labels=shift, **kw)
        with pytest.raises(ValueError, match="shift_labels must be 1"):
            run_settings(dict(kw, shift_labels=shift), True, rollout=True)
    with pytest.raises(ValueError, match="no recording holds a window of 2 \\+ 60 rows"):      # (every entry of a schedule is checked)
        train_gru(None, states, Q, rollout=True, **{**kw, "epochs": 2, "post_wash_out": (3, 60)})
    with pytest.raises(ValueError, match="post_wash_out must be at least 1"):
        train_gru(None, states, Q, rollout=True, **{**kw, "post_wash_out": (3, 0)})


def test_horizon_schedule_parsing_and_its_repeated_last_entry():
    from cartpolesimulation_amd.train_gru import horizon_of_epoch, horizon_schedule
    assert horizon_schedule(7) == (7,) and horizon_schedule("7") == (7,)
    assert horizon_schedule("5,10,20") == (5, 10, 20) == horizon_schedule([5, 10, 20]) == horizon_schedule(" 5, 10 ,20")
    assert horizon_schedule("5,10,10") == (5, 10, 10)
    s = horizon_schedule("5,10,20")
    assert [horizon_of_epoch(s, e) for e in range(6)] == [5, 10, 20, 20, 20, 20]
    assert [horizon_of_epoch((4,), e) for e in range(3)] == [4, 4, 4]
    for bad in ("", "5,,10", "5,x", "5,-1", "0", "2.5"):
        with pytest.raises(ValueError, match="post_wash_out"):
            horizon_schedule(bad)
    with pytest.raises(ValueError, match="at least 1"):
        horizon_schedule([5, 0])


def test_init_folder_and_net_info_entries(tmp_path):
    from cartpolesimulation_amd.model_folder import read_net_info
    from cartpolesimulation_amd.train_gru import run_settings, write_model_folder
    model = RR.case_model("random", True)
    parent = write_model_folder(tmp_path / "GRU-6IN-32H1-32H2-5OUT-0", model)
    base = dict(epochs=2, batch_size=4, lr=1e-3, seed=3, wash_out=5, post_wash_out=10, shift_labels=1)
    settings, init, info = run_settings(base, True, rollout=True, schedule="5,10,20", init_folder=parent)
    assert settings["rollout"] is True and settings["post_wash_out"] == (5, 10, 20) and settings["wash_out"] == 5
    assert set(init) == set(model)
    for k in model:                                          # the folder's weights AND its normalisation
        assert np.array_equal(np.asarray(init[k], f32).view(np.uint32), np.asarray(model[k], f32).view(np.uint32)), k
    assert info["TRAINING MODE"] == "open-loop rollout" and info["POST WASH OUT SCHEDULE"] == "5, 10, 20"
    assert info["POST WASH OUT LENGTH"] == 20 and info["PARENT NET"] == parent
    child = write_model_folder(tmp_path / "GRU-6IN-32H1-32H2-5OUT-1", init, info=info)
    back = read_net_info(child)
    assert back["training_mode"] == "open-loop rollout" and back["post_wash_out_schedule"] == "5, 10, 20"
    assert back["parent_net"] == parent
    # a folder without a normalisation keeps the identity, not the recordings' min-max
    bare = write_model_folder(tmp_path / "GRU-6IN-32H1-32H2-5OUT-2", {k: model[k] for k in TR.GRU_KEYS})
    _, init2, _ = run_settings(base, True, init_folder=bare)
    assert np.array_equal(init2["in_scale"], np.ones(6, f32)) and np.array_equal(init2["out_shift"], np.zeros(5, f32))
    # the teacher-forced default, fresh weights
    settings, init3, info = run_settings(base, True)
    assert settings["rollout"] is False and settings["post_wash_out"] == 10 and set(init3) == set(TR.GRU_KEYS)
    assert info["TRAINING MODE"] == "teacher forced" and info["POST WASH OUT SCHEDULE"] == "10" and "PARENT NET" not in info
    _, init4, _ = run_settings(base, False)
    assert np.array_equal(init4["in_scale"], np.ones(6, f32))


def test_command_line_refuses_rollout_with_another_shift_before_any_engine(tmp_path):
    from cartpolesimulation_amd.train_gru import main
    base = ["--recordings", str(tmp_path), "--out", str(tmp_path / "model"), "--net", "GRU-32H1-32H2", "--dynamics-model", "--rollout"]
    with pytest.raises(SystemExit, match="shift_labels must be 1"):
        main(base + ["--shift-labels", "2"])
    with pytest.raises(SystemExit, match="post_wash_out schedule"):
        main(base + ["--shift-labels", "1", "--post-wash-out-schedule", "5;10"])
    assert not (tmp_path / "model").exists()
