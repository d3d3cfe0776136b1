"""GPU: cpmppi_dense_policy_train_step - the cost step's finalize launch (norm clip, finite guard, Adam in the run it shares with
cpmppi_dense_train_step) - and train_imitator.finetune_on_cost on top.

Reference: tests/policy_ref.py (float64 autograd of the closed loop) and tests/dense_ref.py (the MSE loss, Adam as the header
states it).  The update is pinned the way tests/test_gpu_imitator.py pins the MSE step's, with the device's OWN float32 gradient
(cpmppi_dense_policy_loss_grad on a twin handle holding the same parameters) put through the host's float64 clip and Adam.  What is
left between the two, with e = 2^-24 one float32 rounding: the gradient the host is handed is rounded once (e; the device's Adam
takes it unrounded), the clip's scale inherits that (e), and both sides store their moments rounded, from inputs that differ by
that much (m: 2 e more per step, sqrt(v) likewise) - at most 4 e per step on the quantities the update is formed from, 16 e over
the at most four steps of a test, whose moments are carried on the host.  The update is lr m^ / (sqrt(v^) + eps) and |m^| / sqrt(v^)
<= (1 - beta1) / sqrt(1 - beta2) = 3.2, so the two updates differ by at most 3.2 lr 16 e - an ABSOLUTE figure: a parameter may be
far smaller than its update.  Each side then rounds its parameter once: one more unit in the last place of the larger of the
parameter before and after.  BOUND: |got - want| <= 3.2 lr 16 e + ulp(max(|before|, |want|)) for every parameter."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402
import policy_ref as P  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from test_gpu_policy import LOSS_RTOL, bits, model, new_engine, np_, problem, report  # noqa: E402

f32 = np.float32
B, H = 65, 3
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def tensors(eng, s0, tp, te):
    return eng.tensor(s0[None]), eng.tensor(tp[None]), eng.tensor(te[None])


def params(eng):
    return eng.dense_flatten(eng.dense_train_get())


def update_error(got, want, before):
    """|got - want| per parameter as a share of the module's BOUND (<= 1 passes)."""
    ulp = np.spacing(np.maximum(np.abs(before), np.abs(want)).astype(f32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / (3.2 * ADAM["lr"] * 16 * 2.0 ** -24 + ulp)


def twin_gradient(twin, m, flat, batch, windows, kind):
    """The device's own gradient at the parameters ``flat``: the loss_grad call of ``kind`` on the twin handle."""
    twin.set_dense({**m, **D.unflatten(flat)})
    if kind == "cost":
        loss, g = twin.dense_policy_loss_grad(*batch, windows, H)
    else:
        loss, g = twin.dense_loss_grad(*batch, windows, 1, 0)
    return float(np_(loss)[0]), np_(g).astype(np.float64)


def test_steps_equal_loss_grad_then_the_host_s_clip_and_adam(capsys):
    """Three steps: clip on (half the norm), off, and exactly at the norm - each equal to loss_grad followed by the host's float64
    clip and Adam; and the clip is seen: the same steps unclipped end elsewhere."""
    m = model("random")
    s0, tp, te, windows, order = problem(B)
    eng, twin = new_engine(m, H), new_engine(m, H)
    batch, tbatch = tensors(eng, s0, tp, te), tensors(twin, s0, tp, te)
    eng.dense_train_begin()
    opt, plain = D.Adam(D.flatten(m), **ADAM), D.Adam(D.flatten(m), **ADAM)
    for step, factor in enumerate((0.5, 0.0, 1.0)):
        loss_t, g = twin_gradient(twin, m, opt.p, tbatch, windows, "cost")
        clip = float(f32(factor * np.sqrt((g * g).sum())))
        before = opt.p.copy()
        want = P.clip_and_adam(opt, g, clip).copy()
        plain.step(g)
        loss = float(eng.dense_policy_train_step(*batch, windows, H, clip_norm=clip, **ADAM).item())
        got = params(eng)
        worst = update_error(got, want, before).max()
        report(capsys, f"cost step {step + 1} (clip_norm {clip:.4g} = {factor} x norm): loss {loss:.6e}, worst parameter at {worst:.3f} of the "
                       f"bound, {np.abs(got.astype(np.float64) - want).max():.2e} absolute")
        assert loss == loss_t                                       # the loss before the update: the loss_grad call's bits
        assert worst <= 1.0
        opt.p = got.copy()                                          # the next step is compared from the device's own parameters
    assert np.abs(got - plain.p).max() > 1e-5                       # (unclipped, the second step's moments are others: a part of lr)
    eng.close()
    twin.close()


def test_a_nan_start_state_changes_nothing():
    """One NaN among the start states: loss_out is not finite; parameters keep their bits, and - seen through the next step, which
    equals the step of a handle that never saw the NaN - so do the moments and the counter."""
    m = model("random")
    s0, tp, te, windows, _ = problem(B)
    bad = s0.copy()
    bad[7, 1] = np.nan
    eng, clean = new_engine(m, H), new_engine(m, H)
    good, goodc, poisoned = tensors(eng, s0, tp, te), tensors(clean, s0, tp, te), tensors(eng, bad, tp, te)
    for e in (eng, clean):
        e.dense_train_begin()
    eng.dense_policy_train_step(*good, windows, H, clip_norm=1.0, **ADAM)
    clean.dense_policy_train_step(*goodc, windows, H, clip_norm=1.0, **ADAM)
    before = params(eng)
    loss = float(eng.dense_policy_train_step(*poisoned, windows, H, clip_norm=1.0, **ADAM).item())
    assert not np.isfinite(loss)
    assert np.array_equal(bits(params(eng)), bits(before))
    a = float(eng.dense_policy_train_step(*good, windows, H, clip_norm=1.0, **ADAM).item())
    b = float(clean.dense_policy_train_step(*goodc, windows, H, clip_norm=1.0, **ADAM).item())
    assert a == b and np.array_equal(bits(params(eng)), bits(params(clean)))
    assert not np.array_equal(bits(params(eng)), bits(before))
    eng.close()
    clean.close()


def test_mse_steps_and_cost_steps_alternate_in_one_run(capsys):
    """MSE, cost, MSE, cost on one handle: one set of moments, one counter.  Every step equals the twin's loss_grad of its kind
    followed by the host's Adam with the SHARED moments and step count (separate ones would miss by a large part of lr from the
    second step on), and every loss follows the float64 reference of its kind."""
    m = model("random")
    s0, tp, te, windows, order = problem(B)
    labels = np.random.default_rng(2).uniform(-1, 1, (1, B)).astype(f32)
    eng, twin = new_engine(m, H), new_engine(m, H)
    batch, tbatch = tensors(eng, s0, tp, te), tensors(twin, s0, tp, te)
    lab, tlab = eng.tensor(labels), twin.tensor(labels)
    eng.dense_train_begin()
    opt = D.Adam(D.flatten(m), **ADAM)
    for step, kind in enumerate(("mse", "cost", "mse", "cost")):
        cur, before = {**m, **D.unflatten(opt.p)}, opt.p.copy()
        if kind == "cost":
            loss_t, g = twin_gradient(twin, m, opt.p, tbatch, windows, kind)
            loss64 = P.loss_and_grad(cur, s0[order], tp[order], te[order], H, grad=False)[0]
            want = P.clip_and_adam(opt, g, 0.0).copy()
            loss = float(eng.dense_policy_train_step(*batch, windows, H, **ADAM).item())
            rtol = LOSS_RTOL
        else:
            loss_t, g = twin_gradient(twin, m, opt.p, (*tbatch, tlab), windows, kind)
            loss64 = D.loss_and_grad(cur, *D.samples(s0[None], tp[None], te[None], labels, windows, 1, 0))[0]
            want = opt.step(g).copy()
            loss = float(eng.dense_train_step(*batch, lab, windows, 1, 0, **ADAM).item())
            rtol = 1e-5                                             # (float32 forward of 65 samples; test_gpu_imitator.py's bound is tighter)
        got = params(eng)
        worst = update_error(got, want, before).max()
        report(capsys, f"alternating step {step + 1} ({kind}): loss rel {abs(loss - loss64) / abs(loss64):.2e}, worst parameter at {worst:.3f} of the bound")
        assert loss == loss_t and abs(loss - loss64) <= rtol * abs(loss64)
        assert worst <= 1.0
        opt.p = got.copy()
    eng.close()
    twin.close()


def test_captured_steps_equal_launched_steps():
    from test_gpu_policy import capture
    m = model("random")
    s0, tp, te, windows, _ = problem(130)
    results = []
    for captured in (False, True):
        eng = new_engine(m, 8, "ODE")
        eng.dense_train_begin()
        eng.dense_policy_reserve(130, 8)
        call = eng.prepare_dense_policy_train_step(*tensors(eng, s0, tp, te), windows, 8, clip_norm=5.0, **ADAM)
        if captured:
            graph = capture(eng, call)
            graph.replay()
            l1 = np_(call.result).copy()
            graph.replay()
        else:
            call.run()
            l1 = np_(call.result).copy()
            call.run()
        results.append((l1, np_(call.result).copy(), params(eng)))
        eng.close()
    (a1, a2, pa), (b1, b2, pb) = results
    assert a1[0] != a2[0]                                           # (the second step saw the first one's update)
    assert np.array_equal(bits(a1, np.float64), bits(b1, np.float64)) and np.array_equal(bits(a2, np.float64), bits(b2, np.float64))
    assert np.array_equal(bits(pa), bits(pb))


# ---------------------------------------------------------------------------------------------- learning
LEARN = dict(B=128, H=8, steps=30, lr=2e-3, clip_norm=10.0, seed=12)


@functools.lru_cache(maxsize=None)
def learning_problem():
    """128 start states within 0.3 rad of upright (target_equilibrium 1), a fixed validation batch of 128 others, and the model to
    fine-tune: the golden imitator.  Seed, rate and clip were chosen on the CPU so that the float64 reference's own run (below)
    lowers its validation loss by more than a tenth."""
    def states(seed):
        s0, tp, _ = P.start_states(seed, LEARN["B"], angle=0.3, angleD=1.0, position=0.1, positionD=0.3, target=0.05)
        return s0, tp, np.ones(LEARN["B"], f32)
    return states(LEARN["seed"]), states(LEARN["seed"] + 1), D.golden_model()


@functools.lru_cache(maxsize=None)
def reference_run():
    """-> (every step's training loss before its update of the float64 reference, what the same run with float32 losses and
    gradients - clip and Adam stay the header's - deviates from them by, the float64 validation loss before and after)."""
    (s0, tp, te), val, m = learning_problem()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        opt, cur, losses = D.Adam(D.flatten(m), LEARN["lr"], eps=1e-7), dict(m), []
        for _ in range(LEARN["steps"]):
            loss, g, _, _, _ = P.loss_and_grad(cur, s0, tp, te, LEARN["H"], dtype=dtype)
            losses.append(loss)
            cur = {**cur, **D.unflatten(P.clip_and_adam(opt, g, LEARN["clip_norm"]))}
        runs[dtype] = (np.array(losses), cur)
    ref, trained = runs[torch.float64]
    return (ref, np.abs(runs[torch.float32][0] / ref - 1.0), P.loss_and_grad(m, *val, LEARN["H"], grad=False)[0],
            P.loss_and_grad(trained, *val, LEARN["H"], grad=False)[0])


def test_fine_tuning_follows_the_float64_trajectory_and_lowers_the_cost(capsys):
    """The rule of test_twenty_steps_follow_the_float64_trajectory (tests/test_gpu_imitator.py), with its MARGIN and FLOOR: step 1
    within MARGIN times what the reference's own float32 evaluation loses at step 1, every step within the run's bound - MARGIN
    times the worst deviation of the reference's float32 trajectory -, which itself must not exceed 1e-2; and the validation loss
    falls, as the reference's does."""
    from cartpolesimulation_amd.train_imitator import finetune_on_cost
    from test_gpu_imitator import bound
    ref, dev32, v0, v1 = reference_run()
    assert v1 < 0.9 * v0, f"the reference itself must learn: {v1 / v0:.4f}"
    (s0, tp, te), (vs, vtp, vte), m = learning_problem()
    eng = new_engine(None, LEARN["H"])
    trained, history = finetune_on_cost(eng, s0[None], tp[None], te[None], horizon=LEARN["H"], epochs=LEARN["steps"],
                                        batch_size=LEARN["B"], lr=LEARN["lr"], clip_norm=LEARN["clip_norm"], seed=0, init=m,
                                        validation=(vs[None], vtp[None], vte[None]))
    # (a batch is all 128 states in the epoch's order: the mean cost does not depend on the order beyond float32 summation)
    got = np.abs(np.array(history["loss"]) / ref - 1.0)
    run_bound = bound(dev32.max())
    report(capsys, f"fine-tuning: worst deviation from the float64 trajectory {got.max():.2e} (step {int(got.argmax()) + 1}); float32 reference "
                   f"{dev32.max():.2e}, bound {run_bound:.2e}; step 1 {got[0]:.2e} (float32 reference {dev32[0]:.2e}); "
                   f"validation {history['val_loss'][0]:.5e} -> {history['val_loss'][-1]:.5e} (reference {v0:.5e} -> {v1:.5e})")
    assert got[0] <= bound(dev32[0])
    assert got.max() <= run_bound <= 1e-2
    first = float(eng.dense_policy_loss_grad(eng.tensor(vs[None]), eng.tensor(vtp[None]), eng.tensor(vte[None]),
                                            np.stack([np.zeros(LEARN["B"], np.int64), np.arange(LEARN["B"])], axis=1), LEARN["H"],
                                            grad=False)[0].item())
    assert abs(history["val_loss"][-1] - first) <= 1e-6 * first     # the engine holds the trained model
    assert history["val_loss"][-1] < 0.9 * v0 * (1 + LOSS_RTOL) and abs(history["val_loss"][-1] - v1) <= 1e-2 * v1
    assert set(trained) == set(m) and all(np.isfinite(trained[k]).all() for k in D.KEYS)
    eng.close()
