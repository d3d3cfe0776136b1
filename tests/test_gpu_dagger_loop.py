"""GPU: DAgger in the device loop (harness.DaggerController, run_schedule(dagger=...), harness.DaggerDataset) and the driver
train_imitator.dagger, on the 40-period schedule of tests/test_gpu_imitator_loop.py with MPPI 128 x 8 as the expert.

Every comparison is bit for bit: beta = 1 against the plain fused-MPPI run, beta = 0 against run_schedule(imitator=...), beta = 0.5
against the loop composed by hand from the entry points the step fuses (the expert's step into a private buffer, cpmppi_dense_control,
a host `where` with tests/dagger_ref.py's gate, the plant), captured against launched.  Whether DAgger makes this net balance the pole
is NOT asserted anywhere: at these sizes nothing guarantees it; the figures are printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dagger_ref as G  # noqa: E402
import dense_ref as D  # noqa: E402
from test_gpu_imitator_loop import CFG, E, drawn, engine  # noqa: E402

f32 = np.float32
KEYS = ("states", "dd", "Q", "final_state")
DATA = ("states", "target_position", "target_equilibrium", "labels", "imitator", "gate", "sq_err")
MPPI_SEED, GATE_SEED = 9, 0xDA66E5


def report(capsys, text):
    with capsys.disabled():
        print("\n[dagger] " + text)


def raw(x):
    """The bytes of a tensor or array (a NaN equals itself)."""
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(raw(a), raw(b))


def logs(res):
    return {k: res[k].cpu().numpy().copy() for k in KEYS}


def image(ds, rows=slice(None)):
    return {k: getattr(ds, k)[rows].cpu().numpy().copy() for k in DATA}


def dagger_run(eng, b, beta, model=None, recordings=E, dataset=None, **kw):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment, DaggerDataset
    ds = dataset if dataset is not None else DaggerDataset(eng, recordings, b.n_periods + 1)
    exp = BatchedCartPoleExperiment(eng, seed=MPPI_SEED)
    res = exp.run_schedule(b, imitator=model if model is not None else D.golden_model(),
                           dagger=dict(dataset=ds, beta=beta, seed=GATE_SEED), **kw)
    return res, ds


def by_hand(eng, b, beta, expert_call, counter_of=None):
    """The loop composed by hand.  ``expert_call(run, Q_expert, c)`` enqueues the expert's step of call c into ``Q_expert``.
    ``counter_of()``: the device counter of an expert that counts its own calls, which the plant launch then reads as its period.
    -> (the logs, the dataset's tensors as host arrays [E,T,..])."""
    from cartpolesimulation_amd.harness import ScheduleBuffers
    run = ScheduleBuffers(eng, b)
    T = b.n_periods + 1
    Qe = eng.empty(E)
    run.Q.zero_()
    beta = np.broadcast_to(np.asarray(beta, f32), (E,))
    out = dict(states=np.zeros((E, T, 6), f32), target_position=np.zeros((E, T), f32), target_equilibrium=np.zeros((E, T), f32),
               labels=np.zeros((E, T), f32), imitator=np.zeros((E, T), f32), gate=np.zeros((E, T), np.uint8))
    qi_calls, qe_calls = [], []
    for c in range(T):
        out["states"][:, c], out["target_position"][:, c] = run.s_ctrl.cpu().numpy(), run.cur_tp.cpu().numpy()
        out["target_equilibrium"][:, c] = run.cur_te.cpu().numpy()
        expert_call(run, Qe, c)
        qi = eng.dense_control(run.s_ctrl, run.cur_tp, run.cur_te)[0]
        g = G.gate(GATE_SEED, 0, E, c, beta)
        out["labels"][:, c], out["imitator"][:, c], out["gate"][:, c] = Qe.cpu().numpy(), qi.cpu().numpy(), g
        qi_calls.append(out["imitator"][:, c].copy())
        qe_calls.append(out["labels"][:, c].copy())
        run.Q.copy_(torch.where(torch.as_tensor(g, device=eng.device), Qe, qi))
        steps = b.n_ctrl if c < b.n_periods else run.tail
        if counter_of is None:
            eng.plant_step(run.s, run.Q, steps, period=c, **run.plant)
        else:
            eng.plant_step(run.s, run.Q, steps, period_dev=counter_of(), **run.plant)
    out["sq_err"] = G.sq_err(np.zeros(E), qi_calls, qe_calls)
    return logs(run.result()), out


def mppi_expert(eng):
    def call(run, Qe, c):
        eng.step(run.s_ctrl, run.u_nom, run.cur_tp, run.cur_te, L=run.cur_L, seed=MPPI_SEED, offset=c, env_offset=0, Q_out=Qe,
                 **run.previous_input)
    return call


# ---------------------------------------------------------------------------------------------- the loop against its parts
@pytest.mark.parametrize("chain", [False, True], ids=["true_state", "measurement_chain"])
def test_beta_one_is_the_plain_mppi_run_and_beta_zero_the_imitator_run(chain):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    b, model = drawn(chain), D.golden_model()
    assert b.n_periods == 40
    eng = engine()
    exp = BatchedCartPoleExperiment(eng, seed=MPPI_SEED)
    plain = logs(exp.run_schedule(b))
    res, ds = dagger_run(eng, b, 1.0)
    one = logs(res)
    for k in KEYS:
        assert same(plain[k], one[k]), k
    assert res["recordings"] == (0, E) and ds.filled == E
    assert same(ds.labels.cpu().numpy(), plain["Q"].T.copy()) and (ds.gate.cpu().numpy() == 1).all()
    assert same(res["Q_expert"], plain["Q"][-1])
    imitated = logs(exp.run_schedule(b, imitator=model))
    res0, ds0 = dagger_run(eng, b, 0.0)
    zero = logs(res0)
    for k in KEYS:
        assert same(imitated[k], zero[k]), k
    assert np.isfinite(ds0.labels.cpu().numpy()).all() and (ds0.gate.cpu().numpy() == 0).all()
    assert same(ds0.imitator.cpu().numpy(), imitated["Q"].T.copy())
    assert not same(plain["Q"], imitated["Q"])                      # (the two controllers differ: the comparisons above tell them apart)
    assert (ds0.sq_err.cpu().numpy() > 0).all() and np.isfinite(ds0.sq_err.cpu().numpy()).all()
    eng.close()


@pytest.mark.parametrize("chain", [False, True], ids=["true_state", "measurement_chain"])
def test_the_mixture_is_the_loop_composed_by_hand_launched_and_captured(chain):
    b = drawn(chain)
    beta = 0.5
    gates = np.stack([G.gate(GATE_SEED, 0, E, c, beta) for c in range(b.n_periods + 1)])
    assert all(0 < gates[:, e].sum() < len(gates) for e in range(E))         # the seed: every env sees both drivers (judged on the host)
    eng = engine()
    res, ds = dagger_run(eng, b, beta)
    launched, data = logs(res), image(ds)
    want_logs, want = by_hand(eng, b, beta, mppi_expert(eng))
    for k in KEYS:
        assert same(launched[k], want_logs[k]), k
    for k in DATA:
        assert same(data[k], want[k]), k
    assert same(data["gate"], gates.T.astype(np.uint8))
    # the applied control is what the plant logged, and the row recorded is the state SHOWN
    applied = np.where(data["gate"] == 1, data["labels"], data["imitator"])
    assert same(applied, launched["Q"].T.copy())
    assert same(data["states"][:, 0], launched["states"][0])        # (the first call sees the true state either way)
    if chain:
        assert not same(data["states"][:, 1], launched["states"][1])
    else:
        assert same(data["states"][:, 1], launched["states"][1])
    res_c, ds_c = dagger_run(eng, b, beta, graph=True, steps_per_graph=10)
    captured, data_c = logs(res_c), image(ds_c)
    for k in KEYS:
        assert same(launched[k], captured[k]), k
    for k in DATA:
        assert same(data[k], data_c[k]), k
    eng.close()


def rpgd(seed=5):
    from cartpolesimulation_amd.optimizer_gradient import optimizer_rpgd
    opt = optimizer_rpgd(seed=seed, num_envs=E, fused=True, mpc_horizon=8, num_rollouts=32, outer_its=2)
    opt.configure(predictor_specification="ODE")
    return opt


def test_fused_rpgd_as_the_expert():
    from cartpolesimulation_amd.harness import ControllerMass, ExpertBuffers, FusedOptimizer
    b, model = drawn(False), D.golden_model()
    opt = rpgd()
    res, ds = dagger_run(opt.engine, b, 0.5, model=model, optimizer=opt)
    got, data = logs(res), image(ds)
    assert 0 < data["gate"].sum() < data["gate"].size
    # by hand: the same controller kind writing a private controls buffer, then dense_control, a host `where` and the plant
    other = rpgd()
    eng = other.engine
    eng.set_dense(model)
    if getattr(other, "variable_parameters", None) is None:         # (as ScheduleRun hands an optimizer that has none)
        from types import SimpleNamespace
        other.variable_parameters = SimpleNamespace()
    state = {}

    def expert_call(run, Qe, c):
        if not state:
            view = ExpertBuffers(run)
            mass = ControllerMass(b, eng.mppi)
            mass.bind([eng], register=False)
            state.update(ctrl=FusedOptimizer(other, view, mass, previous_input=run.Q), view=view)
        state["ctrl"].control(c)
        Qe.copy_(state["view"].Q)

    want_logs, want = by_hand(eng, b, 0.5, expert_call, counter_of=lambda: state["ctrl"].counter)
    assert state["ctrl"].counter is not None and int(state["ctrl"].counter.item()) == b.n_periods + 1
    for k in KEYS:
        assert same(got[k], want_logs[k]), k
    for k in DATA:
        assert same(data[k], want[k]), k
    assert not same(got["Q"], data["labels"].T.copy())              # (the imitator drove somewhere)
    eng.close()
    opt.engine.close()


# ---------------------------------------------------------------------------------------------- the aggregate
def test_a_second_run_fills_the_next_recordings_and_the_aggregate_is_trained_where_it_lies():
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment, DaggerDataset
    b1, b2 = drawn(False), SC.RandomExperimentSetter(CFG).draw(E, 94)
    model = D.golden_model()
    eng = engine()
    ds = DaggerDataset(eng, 2 * E, b1.n_periods + 1)
    res1, _ = dagger_run(eng, b1, 1.0, dataset=ds)
    first = image(ds, slice(0, E))
    assert res1["recordings"] == (0, E) and ds.filled == E and (image(ds, slice(E, None))["states"] == 0).all()
    res2, _ = dagger_run(eng, b2, 0.5, dataset=ds)
    assert res2["recordings"] == (E, 2 * E) and ds.filled == 2 * E
    again, second = image(ds, slice(0, E)), image(ds, slice(E, None))
    for k in DATA:
        assert same(first[k], again[k]), k
    alone, ds_alone = dagger_run(eng, b2, 0.5)
    for k in DATA:
        assert same(second[k], image(ds_alone)[k]), k               # (a recording does not depend on where it lies)
    assert not same(first["states"], second["states"])
    # a full dataset, and everything that cannot stand beside dagger=, by name; nothing is written on the way
    exp = BatchedCartPoleExperiment(eng, seed=MPPI_SEED)
    with pytest.raises(ValueError, match=f"DaggerDataset is full: {2 * E} of its {2 * E} recordings are written, {E} more"):
        exp.run_schedule(b1, imitator=model, dagger=dict(dataset=ds, beta=1.0))
    from types import SimpleNamespace
    fresh = DaggerDataset(eng, E, b1.n_periods + 1)
    ok = dict(dataset=fresh, beta=0.5, seed=1)
    for text, kw in (("dagger= needs imitator=", dict(dagger=ok)),
                     ("dagger= and predictor='GRU'", dict(dagger=ok, imitator=model, predictor="GRU")),
                     ("dagger= and h0", dict(dagger=ok, imitator=model, h0=np.zeros((E, 2, 32), f32))),
                     ("dagger= and knots_fn", dict(dagger=ok, imitator=model, knots_fn=lambda c: None)),
                     ("dagger= and tuning=", dict(dagger=ok, imitator=model, tuning=np.zeros((E, 16), f32))),
                     ("dagger= and an optimizer with gru_model=", dict(dagger=ok, imitator=model, optimizer=SimpleNamespace(fused=True, gru_model={}))),
                     ("dagger= and a host-paced optimizer=", dict(dagger=ok, imitator=model, optimizer=SimpleNamespace(fused=False))),
                     ("the dataset has 40 rows per recording, the batch makes 41",
                      dict(dagger=dict(ok, dataset=DaggerDataset(eng, E, b1.n_periods)), imitator=model)),
                     (r"beta must be a scalar or \[4\]", dict(dagger=dict(ok, beta=np.ones(3)), imitator=model))):
        with pytest.raises(ValueError, match=text):
            exp.run_schedule(b1, **kw)
    assert fresh.filled == 0 and (fresh.states == 0).all()
    with pytest.raises(ValueError, match="imitator= and optimizer="):          # without dagger= the old refusal stands
        exp.run_schedule(b1, imitator=model, optimizer=SimpleNamespace(fused=True))
    for k in DATA:
        assert same(image(ds, slice(0, E))[k], first[k]), k
    # trained where it lies: windows over both runs' recordings, against host copies uploaded into fresh tensors
    T = ds.T
    windows = np.array([[0, 0], [E - 1, T - 8], [E, 0], [2 * E - 1, T - 8], [1, 7], [E + 2, 20]])
    loss, grad = eng.dense_loss_grad(*ds.tensors, windows, 8, 0)
    copies = [eng.tensor(t.cpu().numpy().copy()) for t in ds.tensors]
    assert all(c.data_ptr() != t.data_ptr() for c, t in zip(copies, ds.tensors))
    loss2, grad2 = eng.dense_loss_grad(*copies, windows, 8, 0)
    assert same(loss, loss2) and same(grad, grad2) and float(loss) > 0 and np.isfinite(grad.cpu().numpy()).all()
    eng.close()


# ---------------------------------------------------------------------------------------------- the driver
def test_the_driver(tmp_path, capsys):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    from cartpolesimulation_amd.model_folder import load_dense_model
    from cartpolesimulation_amd.train_imitator import NORM_KEYS, dagger, normalization_from_recordings, write_model_folder
    kw = dict(experiments=E, iterations=3, beta=(1, 0.5, 0), steps_per_iteration=8, batch_size=64, lr=2e-3, seed=1873)
    eng = engine()
    lines = []
    trained, history = dagger(eng, CFG, log=lines.append, **kw)
    ds = history["dataset"]
    T = ds.T
    assert ds.filled == 3 * E == ds.R and T == 41 and len(lines) == 3
    assert history["beta"] == [1.0, 0.5, 0.0]
    assert [len(history[k]) for k in ("disagreement", "expert_share", "batch_loss", "scores")] == [3] * 4
    assert all(len(x) == 8 for x in history["batch_loss"]) and all(s.shape == (E, 5) for s in history["scores"])
    assert np.isfinite(history["disagreement"]).all() and np.isfinite(history["batch_loss"]).all()
    assert all(np.isfinite(s).all() for s in history["scores"])
    assert history["expert_share"][0] == 1.0 and history["expert_share"][2] == 0.0 and 0 < history["expert_share"][1] < 1
    gate = ds.gate.cpu().numpy()
    assert (gate[:E] == 1).all() and (gate[2 * E:] == 0).all()
    # the normalisation: iteration 0's recordings, fixed
    it0 = [t[:E].cpu().numpy() for t in ds.tensors]
    norm0 = normalization_from_recordings(*it0)
    for k in NORM_KEYS:
        assert same(trained[k], norm0[k]) and same(history["normalization"][k], norm0[k]), k
    # the disagreement reported is the dataset's: sum(sq_err) / samples, per iteration
    sq = ds.sq_err.cpu().numpy()
    for i in range(3):
        assert history["disagreement"][i] == pytest.approx(sq[i * E:(i + 1) * E].sum() / (E * T), rel=1e-12)
    d = ds.imitator.cpu().numpy().astype(np.float64) - ds.labels.cpu().numpy().astype(np.float64)
    assert np.allclose((d * d).sum(axis=1), sq, rtol=1e-12, atol=0)
    # the same seeds: the same bits; captured runs: the same bits
    eng2 = engine()
    again, _ = dagger(eng2, CFG, **kw)
    assert set(again) == set(trained) and all(same(again[k], trained[k]) for k in trained)
    captured, _ = dagger(eng2, CFG, graph=True, **kw)
    assert all(same(captured[k], trained[k]) for k in trained)
    eng2.close()
    # the model folder round trip, and the trained imitator in the loop
    folder = write_model_folder(tmp_path / "Dense-7IN-32H1-32H2-1OUT-0", trained)
    back = load_dense_model(folder)
    assert set(back) == set(trained) and all(same(back[k], trained[k]) for k in trained)
    res = BatchedCartPoleExperiment(eng, seed=MPPI_SEED).run_schedule(drawn(False), imitator=folder)
    assert res["Q"].shape == (41, E) and np.isfinite(res["Q"].cpu().numpy()).all() and np.isfinite(res["states"].cpu().numpy()).all()
    report(capsys, "driver, 3 iterations x 4 experiments x 41 rows, 8 steps of 64: disagreement "
                   + ", ".join(f"{x:.3e}" for x in history["disagreement"]) + "; loss "
                   + ", ".join(f"{x[0]:.3e}->{x[-1]:.3e}" for x in history["batch_loss"]) + " (no improvement is asserted)")
    eng.close()


