"""Host: tests/policy_ref.py, the float64 reference of the cost fine-tuning tests, on its own - its autograd gradient against
central finite differences of itself, its per-start-state targets against oracle_torch's scalar-target cost, both integrators - and
what the Python layer decides without a GPU: the refusals of the --finetune-cost command line, the recordings loader without a label
column, the refusals of finetune_on_cost before it touches the engine.  (finetune_command itself builds an engine: it runs on the
GPU through tools/policy_bench.py and the learning test's finetune_on_cost only.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402
import policy_ref as P  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from oracle import oracle_torch as OT  # noqa: E402

f32 = np.float32


def directional(model, direction, eps, s0, tp, te, H, **kw):
    flat = D.flatten(model).astype(np.float64)
    out = []
    for sign in (1.0, -1.0):
        w = {k: torch.as_tensor(v.astype(np.float64)) for k, v in unflatten64(flat + sign * eps * direction).items()}
        J, _, _ = P.closed_loop(w, D._norm(model, torch.float64), P.t64(s0), P.t64(tp), P.t64(te), H, **kw)
        out.append(float(J.mean()))
    return (out[0] - out[1]) / (2 * eps)


def unflatten64(flat):
    out, at = {}, 0
    for k, shp in zip(D.KEYS, D.SHAPES):
        n = int(np.prod(shp))
        out[k] = np.asarray(flat[at:at + n], np.float64).reshape(shp)
        at += n
    return out


@pytest.mark.parametrize("integrator", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("cost_id,reduce", [(O.COST_QBGM, "sum"), (O.COST_DEFAULT, "mean")])
def test_gradient_against_central_differences(integrator, cost_id, reduce):
    """Along one random direction per weight tensor and two over all 1345 parameters; the weights in float64 exactly as autograd
    holds them.  (default's indicators are piecewise constant: a direction that crosses one would show as a large error.)"""
    model = D.random_model(4, norm=True)
    s0, tp, te = P.start_states(11, 9)
    kw = dict(cost_id=cost_id, integrator=integrator, S=4, horizon_reduce=reduce)
    _, g, _, _, q = P.loss_and_grad(model, s0, tp, te, 3, **kw)
    assert (np.abs(q) < 1).any()
    rng = np.random.default_rng(0)
    at = 0
    directions = []
    for shp in D.SHAPES:
        n = int(np.prod(shp))
        d = np.zeros(D.NPAR)
        d[at:at + n] = rng.standard_normal(n)
        directions.append(d)
        at += n
    directions += [rng.standard_normal(D.NPAR), rng.standard_normal(D.NPAR)]
    for d in directions:
        d /= np.linalg.norm(d)
        fd = directional(model, d, 1e-6, s0, tp, te, 3, **kw)
        assert abs(fd - g @ d) <= 1e-6 * max(abs(g @ d), np.abs(g).max()), (fd, g @ d)


def test_a_clipped_step_passes_nothing_back_through_the_net():
    """out_scale = 50: every control clips, every stage's d u / d parameters is 0 - the whole gradient is exactly 0."""
    model = {**D.random_model(4, norm=True), "out_scale": np.array([50.0], f32)}
    s0, tp, te = P.start_states(11, 5)
    _, g, _, u, q = P.loss_and_grad(model, s0, tp, te, 3, S=2)
    assert (np.abs(q) > 1).all() and (np.abs(u) == 1).all() and not g.any()


@pytest.mark.parametrize("integrator", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("cost_id,reduce", [(O.COST_QBGM, "mean"), (O.COST_DEFAULT, "sum")])
def test_per_state_targets_equal_the_oracle_state_by_state(integrator, cost_id, reduce):
    """J_b of the batch = oracle_torch's trajectory cost of the plan u_b from s0_b under that state's own targets and length."""
    model = D.random_model(9, norm=True)
    s0, tp, te = P.start_states(3, 6)
    s0[0, 4], s0[0, 5] = 0.19, 0.5                                 # one state that reaches the edge inside the horizon
    L = np.random.default_rng(1).uniform(0.3, 0.45, 6).astype(f32)
    H = 4
    _, _, J, u, _ = P.loss_and_grad(model, s0, tp, te, H, grad=False, cost_id=cost_id, integrator=integrator, L=L, horizon_reduce=reduce)
    assert len(set(tp.tolist())) == 6 and {-1.0, 1.0} <= set(te.tolist())
    for b in range(6):
        traj = OT.predict_core(s0[b], P.t64(u[b:b + 1]), L=float(L[b]), integrator=integrator)
        want = OT.trajectory_cost(cost_id, traj, P.t64(u[b:b + 1]), float(tp[b]), float(te[b]), reduce)
        assert abs(J[b] - float(want[0])) <= 1e-12 * abs(float(want[0])), (b, J[b], float(want[0]))


def test_clip_and_adam_is_the_header_s_update():
    opt, ref = D.Adam(np.ones(D.NPAR, f32), 1e-2), D.Adam(np.ones(D.NPAR, f32), 1e-2)
    g = np.random.default_rng(0).standard_normal(D.NPAR)
    norm = np.sqrt((g * g).sum())
    assert np.array_equal(P.clip_and_adam(opt, g, 0.0), ref.step(g))                     # off
    assert np.array_equal(P.clip_and_adam(opt, g, norm), ref.step(g))                    # exactly at the norm: scale 1
    assert np.array_equal(P.clip_and_adam(opt, g, 0.5 * norm), ref.step(0.5 * g))        # on
    before = (opt.p.copy(), opt.m.copy(), opt.v.copy(), opt.t)
    bad = g.copy()
    bad[7] = np.nan
    P.clip_and_adam(opt, bad, 1.0)
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], (opt.p, opt.m, opt.v))) and opt.t == before[3]


# ---------------------------------------------------------------------------------------------- the command line (no GPU is reached)
FINETUNE = ["--finetune-cost", "--init", "I", "--recordings", "R", "--horizon", "8", "--config-root", "C", "--out", "O"]


def without(argv, flag):
    i = argv.index(flag)
    return argv[:i] + argv[i + 2:]


@pytest.mark.parametrize("argv,text", [
    (without(FINETUNE, "--init"), "--finetune-cost needs --init FOLDER"),
    (without(FINETUNE, "--recordings"), "--finetune-cost needs --recordings DIR"),
    (without(FINETUNE, "--horizon"), "--finetune-cost needs --horizon H"),
    (without(FINETUNE, "--config-root"), "--finetune-cost needs --config-root CHECKOUT"),
    (FINETUNE + ["--dagger", "2"], "--finetune-cost and --dagger are two runs"),
    (FINETUNE + ["--label-column", "Q"], "--finetune-cost reads no label: --label-column belongs to the training on recordings"),
    (FINETUNE + ["--shift-labels", "1"], "--finetune-cost reads no label: --shift-labels"),
    (FINETUNE + ["--post-wash-out", "2"], "--finetune-cost reads no label: --post-wash-out"),
    (FINETUNE + ["--graph"], "--graph belongs to --dagger"),
    (["--recordings", "R", "--out", "O", "--horizon", "8"], "--horizon and --clip-norm belong to --finetune-cost"),
    (["--recordings", "R", "--out", "O", "--clip-norm", "1"], "--horizon and --clip-norm belong to --finetune-cost"),
    (["--dagger", "2", "--config-root", "C", "--out", "O", "--clip-norm", "1"], "--horizon and --clip-norm belong to --finetune-cost"),
])
def test_the_command_line_refuses_by_name_before_anything_is_read(argv, text):
    """None of the folders exists: the refusal comes first."""
    from cartpolesimulation_amd.train_imitator import main
    with pytest.raises(SystemExit, match=text):
        main(argv)


def test_fine_tuning_reads_recordings_without_a_control_or_label_column(tmp_path):
    """A start state needs the six features and the two targets; the lengths are the files' own."""
    from cartpolesimulation_amd.along_trajectories import FEATURES
    from cartpolesimulation_amd.train_imitator import LABEL_COLUMN, load_recordings_folder
    rng = np.random.default_rng(0)
    cols = list(FEATURES) + ["target_position", "target_equilibrium"]
    tables = {"a.csv": rng.normal(size=(5, len(cols))), "b.csv": rng.normal(size=(3, len(cols)))}
    for name, t in tables.items():
        with open(tmp_path / name, "w") as fh:
            fh.write("# a preamble line\n" + ",".join(cols) + "\n" + "\n".join(",".join(repr(float(v)) for v in row) for row in t) + "\n")
    states, tp, te, labels, lengths, names = load_recordings_folder(tmp_path, None)
    assert names == ["a.csv", "b.csv"] and lengths.tolist() == [5, 3] and states.shape == (2, 5, 6) and not labels.any()
    assert np.array_equal(states[1, :3], tables["b.csv"][:, :6].astype(f32)) and not states[1, 3:].any()
    assert np.array_equal(tp[0], tables["a.csv"][:, 6].astype(f32)) and np.array_equal(te[1, :3], tables["b.csv"][:, 7].astype(f32))
    with pytest.raises(ValueError, match=LABEL_COLUMN):             # the training on recordings still asks for its label
        load_recordings_folder(tmp_path, LABEL_COLUMN)


def test_finetune_on_cost_refuses_before_the_engine_is_touched():
    from cartpolesimulation_amd.train_imitator import finetune_on_cost
    m = D.random_model(1)                                           # no normalisation
    s0, tp, te = P.start_states(1, 4)
    kw = dict(horizon=3, epochs=1, batch_size=4, lr=1e-3, clip_norm=1.0, seed=0)
    with pytest.raises(ValueError, match="init must carry its normalisation"):
        finetune_on_cost(None, s0[None], tp[None], te[None], init=m, **kw)
    with pytest.raises(ValueError, match="epochs and batch_size must be at least 1"):
        finetune_on_cost(None, s0[None], tp[None], te[None], init=D.random_model(1, norm=True), **{**kw, "epochs": 0})
    with pytest.raises(ValueError, match=r"weight w1 must have shape \(32, 7\)"):
        finetune_on_cost(None, s0[None], tp[None], te[None], init={"w1": np.zeros((3, 3), f32)}, **kw)
