"""GPU: the neural imitator in the device loop (harness.ImitatorController: run_schedule(imitator=...), generate_dataset(imitator=...),
recording --imitator) and the whole chain once: generate_dataset -> control_along_trajectories -> train_imitator ->
write_model_folder -> load_dense_model -> run_schedule(imitator=...).

Whether the shipped weights balance this plant is NOT claimed anywhere here: nobody has run them on it.  What is pinned: every logged
control is cpmppi_dense_control of the inputs the controller was shown, bit for bit, and the float64 reference (tests/dense_ref.py)
within the bound of tests/test_gpu_imitator.py (8 times what a float32 evaluation of the reference loses, floor 1e-6); the captured
loop equals the launched one in every bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402
from test_gpu_imitator import bits, bound, np_, report  # noqa: E402

f32 = np.float32
E = 4
CFG = dict(seed=51, length_of_experiment=0.8, dt=dict(saving=0.02), keep_target_equilibrium_x_seconds_up=0.3,
           turning_points=dict(track_relative_complexity=12),
           random_initial_state=dict(init_limits=dict(angle=[0.0, 20.0], angleD=40.0, position=0.4, positionD=0.2)))
CHAIN = dict(latency=0.005, seed=14, noise=dict(noise_mode="ON", sigma_angle=0.01, sigma_position=0.002, sigma_angleD=0.2,
                                                 sigma_positionD=0.02))


def engine(n_envs=E):
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine
    return MPPIEngine(n_envs, MPPIConfig(num_rollouts=128, mpc_horizon=8))


def drawn(chain):
    from cartpolesimulation_amd import schedule as SC
    b = SC.RandomExperimentSetter(CFG).draw(E, 93)
    return SC.apply_parameter_schedule(b, CHAIN, seed=94) if chain else b


@pytest.mark.parametrize("chain", [False, True], ids=["true_state", "measurement_chain"])
def test_every_logged_control_is_dense_control_of_the_logged_inputs(chain, capsys):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment, ScheduleBuffers
    b = drawn(chain)
    assert b.n_periods == 40 and (b.measurement_noise is not None) == chain
    model = D.golden_model()
    eng = engine()
    exp = BatchedCartPoleExperiment(eng, seed=9)
    keys = ("states", "dd", "Q", "final_state")
    launched = {k: np_(v).copy() for k, v in exp.run_schedule(b, imitator=D.GOLDEN_FOLDER).items() if k in keys}
    captured = {k: np_(v).copy() for k, v in exp.run_schedule(b, imitator=model, graph=True, steps_per_graph=10).items() if k in keys}
    for k in keys:
        assert np.array_equal(bits(launched[k]), bits(captured[k])), k
    assert launched["Q"].shape == (41, E) and np.isfinite(launched["Q"]).all() and np.isfinite(launched["states"]).all()
    # the loop composed by hand, logging what the controller is shown at every call
    run = ScheduleBuffers(eng, b)
    seen = []
    for c in range(b.n_periods + 1):
        seen.append([np_(x).copy() for x in (run.s_ctrl, run.cur_tp, run.cur_te)])
        eng.dense_control(run.s_ctrl, run.cur_tp, run.cur_te, Q_out=run.Q)
        eng.plant_step(run.s, run.Q, b.n_ctrl if c < b.n_periods else run.tail, period=c, **run.plant)
    by_hand = {k: np_(v) for k, v in run.result().items() if k in keys}
    for k in keys:
        assert np.array_equal(bits(launched[k]), bits(by_hand[k])), k
    s_all, tp_all, te_all = (np.concatenate([x[i] for x in seen]) for i in range(3))
    if chain:
        assert not np.array_equal(s_all[E:2 * E], launched["states"][1])      # (the controller was not shown the true state)
    else:
        assert np.array_equal(s_all[E:2 * E], launched["states"][1])
    # all calls at once, other lanes: the same bits; and the float64 reference
    Q_again, _ = eng.dense_control(eng.tensor(s_all), eng.tensor(tp_all), eng.tensor(te_all))
    assert np.array_equal(bits(np_(Q_again).reshape(41, E)), bits(launched["Q"]))
    q64, _, raw = D.control(model, s_all, tp_all, te_all)
    _, _, raw32 = D.control(model, s_all, tp_all, te_all, torch.float32)
    bq = bound(np.abs(raw32 - raw).max())
    err = np.abs(launched["Q"].reshape(-1) - q64)
    away = np.abs(np.abs(raw) - 1.0) > bq                            # (within the bound of a limit the clip may fall either way)
    report(capsys, f"loop ({'measurement chain' if chain else 'true state'}): control err {err[away].max():.3e}, bound {bq:.3e}; "
                   f"{int((np.abs(raw) > 1).sum())} of {raw.size} controls clipped")
    assert err[away].max() <= bq and err.max() <= 2 * bq
    eng.close()


def test_each_exclusive_combination_is_refused_by_name():
    from cartpolesimulation_amd import recording as REC
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    b, model = drawn(False), D.golden_model()
    eng = engine()
    exp = BatchedCartPoleExperiment(eng, seed=9)
    for text, kw in (("imitator= and optimizer=", dict(optimizer=object())),
                     ("imitator= and predictor='GRU'", dict(predictor="GRU")),
                     ("imitator= and h0", dict(h0=np.zeros((E, 2, 32), f32))),
                     ("imitator= and knots_fn", dict(knots_fn=lambda c: None)),
                     ("imitator= and tuning=", dict(tuning=np.zeros((E, 16), f32)))):
        with pytest.raises(ValueError, match=text):
            exp.run_schedule(b, imitator=model, **kw)
    for text, kw in (("imitator= and gru_model=", dict(gru_model={})), ("imitator= and optimizer=", dict(optimizer=object())),
                     ("groups=1, world=1", dict(groups=2)), ("groups=1, world=1", dict(world=2))):
        with pytest.raises(ValueError, match=text):
            REC.generate_dataset(eng, 2, "unused", config=CFG, imitator=model, **kw)
    for flags in (["--optimizer", "rpgd"], ["--fused"], ["--gru-model", "x"], ["--gru-fused"], ["--groups", "2"]):
        with pytest.raises(SystemExit, match="--imitator and " + flags[0]):
            REC.main(["--imitator", D.GOLDEN_FOLDER, "--experiments", "2", "--out", "unused"] + flags)
    assert not eng.has_dense                                        # nothing was set on the way
    eng.close()


def test_the_controller_stand_in_is_dense_control_with_one_env():
    from cartpolesimulation_amd.controller_neural_imitator import controller_neural_imitator
    s, tp, te, _ = D.recordings(101, R=1, T=5)
    ctrl = controller_neural_imitator("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0}).configure(D.GOLDEN_FOLDER)
    eng = ctrl.engine
    for i in range(5):
        q = ctrl.step(s[0, i], time=0.02 * i, updated_attributes={"target_position": float(tp[0, i]), "target_equilibrium": float(te[0, i])})
        want = eng.dense_control(eng.tensor(s[0, i:i + 1]), eng.tensor(tp[0, i:i + 1]), eng.tensor(te[0, i:i + 1]))[0]
        assert isinstance(q, float) and f32(q) == np_(want)[0]
    eng.close()


def test_the_whole_chain_once(tmp_path, capsys):
    from cartpolesimulation_amd import recording as REC
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.along_trajectories import control_along_trajectories, stack_recordings
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    from cartpolesimulation_amd.model_folder import load_dense_model
    from cartpolesimulation_amd.train_imitator import train_imitator, write_model_folder
    eng = engine()
    cfg = dict(CFG, length_of_experiment=2.0)
    paths = REC.generate_dataset(eng, E, str(tmp_path / "recordings"), config=cfg, seed=3)
    assert len(paths) == E
    relabelled = control_along_trajectories(paths, config=MPPIConfig(num_rollouts=128, mpc_horizon=8), num_evals=2, seed=5)
    states, rows, attrs = stack_recordings(paths)
    labels = relabelled["Q"]
    assert labels.shape == states.shape[:2] == (E, int(rows.max())) and np.isfinite(labels).all() and (rows == rows[0]).all()
    trained, history = train_imitator(eng, states, attrs["target_position"], attrs["target_equilibrium"], labels, rows,
                                      epochs=2, batch_size=64, lr=2e-3, seed=1873)
    assert len(history["loss"]) == 2 and np.isfinite(history["batch_loss"]).all() and history["loss"][0] > 0
    assert all(np.isfinite(v).all() for v in trained.values()) and trained["w2"].shape == (32, 32)
    folder = write_model_folder(tmp_path / "Dense-7IN-32H1-32H2-1OUT-0", trained)
    back = load_dense_model(folder)
    assert set(back) == set(trained) and all(np.array_equal(bits(back[k]), bits(trained[k])) for k in trained)
    b = SC.RandomExperimentSetter(CFG).draw(E, 93)
    exp = BatchedCartPoleExperiment(eng, seed=9)
    before = exp.run_schedule(b, imitator=trained)
    before = {k: np_(before[k]).copy() for k in ("states", "Q")}
    after = exp.run_schedule(b, imitator=folder)
    assert before["Q"].shape == (41, E) and before["states"].shape[1:] == (E, 6)
    assert np.isfinite(before["Q"]).all() and np.isfinite(before["states"]).all() and np.abs(before["Q"]).max() <= 1.0
    assert np.array_equal(bits(before["Q"]), bits(np_(after["Q"]))) and np.array_equal(bits(before["states"]), bits(np_(after["states"])))
    # the data generator with the imitator as its controller: launched and captured write the same rows
    files = {}
    for graph in (False, True):
        out = REC.generate_dataset(eng, 2, str(tmp_path / f"imitator_{graph}"), config=dict(CFG, length_of_experiment=0.2), seed=3,
                                   imitator=folder, graph=graph)
        files[graph] = [[ln if ln.startswith(b"#") else ln.rsplit(b",", 1)[0] for ln in open(p, "rb").read().splitlines()] for p in out]
    assert files[False] == files[True] and b"neural-imitator" in b"\n".join(files[False][0][:40])
    report(capsys, f"chain: {E} recordings x {int(rows[0])} rows, loss {history['loss'][0]:.3e} -> {history['loss'][1]:.3e}")
    eng.close()
