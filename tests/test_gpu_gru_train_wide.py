"""GPU: GRU training beyond one slice plan - cpmppi_gru_loss_grad / cpmppi_gru_rollout_loss_grad and the training steps at the shapes
of tests/gru_train_wide_cases.py (its docstring has the table: the 64-slice cap, per_slice > 8, a short last slice, slice boundaries
inside rows, slices that lie wholly in row 0, tpr > per_slice, 65 loss partials), and what cpmppi_set_gru does to a training run.

Reference: float64 autograd of tests/gru_train_ref.py (teacher-forced) and tests/gru_train_rollout_ref.py (rollout), whose float32
realisation lies within share_min / 16 at every case (tests/test_gru_train_wide_host.py).

Bounds.  Cases A, B, C: every parameter tensor within share_min / 4 of its max |g| - share_min (gru_train_wide_cases.share_min) is
the least that ONE lost or doubled (row, window tile) moves w_out's gradient by, between 5.6e-4 and 1.7e-3 here, so the project's
5e-4 (GRAD_TOL, also asserted) has no room to see such a tile at these sizes.  Cases D, E: GRAD_TOL and four times the worst deviation
measured (MEASURED, below), the project's rule for a measured bound.  Loss: rtol 5e-4 (LOSS_RTOL); at D the loss-only call equals
the gradient call bit for bit - gru_loss_finalize_kernel's loop over 65 partials, both launches.  Bit for bit: two runs; a handle
whose workspace served other shapes against a fresh one; two replays of a captured step against two launched steps; a handle after
cpmppi_set_gru against a fresh handle of that model.

Measured on the MI355X (this module's first run): gradient, worst tensor, of its max |g| (loss, relative)
  case   golden with normalisation             random without normalisation          asserted (the smaller of the two)
         teacher-forced     rollout            teacher-forced     rollout
  A      2.92e-07 (8.2e-09) 3.82e-07 (4.4e-09) 4.54e-07 (7.2e-09) 3.66e-07 (4.2e-09) share_min / 4 = 2.85e-04
  B      3.12e-07 (1.2e-08) 3.09e-07 (2.3e-10) 2.62e-07 (1.4e-10) 4.28e-07 (8.0e-09) share_min / 4 = 1.41e-04
  C      8.78e-07 (6.4e-09) 7.20e-07 (2.3e-09) 5.85e-07 (7.9e-09) 5.65e-07 (2.1e-09) share_min / 4 = 2.92e-04
  D      2.83e-07 (3.8e-09) 4.85e-07 (4.9e-09) 3.51e-07 (1.1e-08) 5.52e-07 (7.3e-09) 4 x 5.52e-07
  E      5.77e-07 (1.0e-09) 6.07e-07 (8.5e-11) 4.09e-07 (1.2e-08) 3.75e-07 (1.0e-09) 4 x 6.07e-07
The kernels sit a factor 330 (case C, golden, teacher-forced) or more inside share_min / 4.
Training at width (8 recordings x 120 rows of the oracle's plant, W = 5, P = 10, B = 1030 drawn with repetition, lr = 2e-3, 10
steps, against float64 Adam; the loss falls from 0.3759 to 0.2564): step 1 9.6e-09, worst step 1.20e-08 (step 9) - a tenth of the
1.19e-07 behind TRAIN_LOSS_RTOL of test_gpu_gru_train.py, which is asserted unchanged.
What the bound is for, measured once with two one-line changes of the source built outside the tree: gru_wgrad_kernel handed
tiles - 1 moves the gradient by 2.4e-03 .. 6.5e-03 at A, 9.1e-04 .. 1.4e-03 at B and 1.3e-03 .. 1.8e-03 at C - 4.6 to 23 times
share_min / 4, and at B as little as 1.8 times 5e-4; gru_loss_finalize_kernel striding by 65 moves case D's loss by 1.0e-02 and
nothing else.  (With case C at (W, P) = (10, 30), where it stood first, the lost tile moved three of its four runs by 2.8e-04 ..
3.8e-04, below 5e-4; gru_train_wide_cases says why C scores 6 rows.)"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402
import gru_train_rollout_ref as RR  # noqa: E402
import gru_train_wide_cases as WC  # noqa: E402
from test_gpu_gru_train import GRAD_TOL, LOSS_RTOL, P_TOTAL, TRAIN_LOSS_RTOL, bits, new_engine, np_, unflat  # noqa: E402

f32 = np.float32
MODELS = (("golden", True), ("random", False))
MEASURED = {"D": 5.52e-7, "E": 6.07e-7}                     # worst deviation of the gradient over MODELS and both modes (module docstring)
HYPER = (2e-3, 0.9, 0.999, 1e-8)


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-train-wide] " + text)


def recordings():
    return TR.random_recordings(WC.R, WC.T)


def run_case(eng, states, Q, key, rollout, **kw):
    B, W, P = WC.CASES[key]
    return eng.gru_loss_grad(states, Q, WC.case_windows(key), W, P, rollout=rollout, **kw)


def copies(pair):
    return np_(pair[0]).copy(), np_(pair[1]).copy()


def same_bits(a, b):
    return np.array_equal(bits(a[0], np.float64), bits(b[0], np.float64)) and np.array_equal(bits(a[1]), bits(b[1]))


def test_the_cases_windows_are_the_packages_legal_ones():
    from cartpolesimulation_amd.train_gru import make_windows
    for B, W, P in WC.CASES.values():
        assert np.array_equal(WC.legal_windows(W, P), make_windows([WC.T] * WC.R, W, P, 1))


# ---------------------------------------------------------------------------------------------- 1. gradient against float64 autograd
@pytest.mark.parametrize("rollout", [False, True], ids=["teacher-forced", "rollout"])
@pytest.mark.parametrize("name,norm", MODELS, ids=["golden-norm", "random-identity"])
def test_loss_and_gradient_against_float64_autograd(name, norm, rollout, capsys):
    eng = new_engine(RR.case_model(name, norm))
    states, Q = (eng.tensor(x) for x in recordings())
    plan = {key: WC.slice_plan(*WC.CASES[key], *WC.source_constants()) for key in WC.CASES}
    for key, (B, W, P) in WC.CASES.items():
        loss, grad = run_case(eng, states, Q, key, rollout)
        l_ref, g_ref = WC.reference(key, name, norm, rollout)
        g, l = unflat(np_(grad)), float(np_(loss)[0])
        rel_g, rel_l = TR.worst_relative(g, g_ref), abs(l - l_ref) / l_ref
        if key in WC.SHARE_CASES:
            bound, why = WC.share_bound(key, name, norm) / 4, "share_min / 4"
        else:
            bound, why = min(4 * MEASURED[key], GRAD_TOL), "4 x measured"
        report(capsys, f"{name} norm={norm} {'rollout' if rollout else 'teacher-forced'} case {key} (B {B} W {W} P {P}; per_slice "
                       f"{plan[key]['per_slice']}, slices {plan[key]['slices']}): gradient {rel_g:.3e} (bound {bound:.3e}, {why}), loss {rel_l:.3e}")
        assert np.isfinite(np_(grad)).all()
        assert rel_g < bound, (key, rel_g, bound)
        assert rel_g < GRAD_TOL, key
        assert rel_l < LOSS_RTOL, key
        for l_ in range(2):                                  # the r and z gates see b_ih + b_hh: the same sum, bit for bit
            assert np.array_equal(bits(g[f"b_ih{l_}"][:64]), bits(g[f"b_hh{l_}"][:64]))
            assert not np.array_equal(bits(g[f"b_ih{l_}"][64:]), bits(g[f"b_hh{l_}"][64:]))
        if key == "D":                                       # 65 partial losses: the finalize loop, once per launch sequence
            only, none = run_case(eng, states, Q, key, rollout, grad=False)
            assert none is None and np.array_equal(bits(np_(only), np.float64), bits(np_(loss), np.float64))
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("rollout", [False, True], ids=["teacher-forced", "rollout"])
def test_two_runs_same_bits_and_sentinels(rollout):
    eng = new_engine(RR.case_model("golden", True))
    states, Q = (eng.tensor(x) for x in recordings())
    for key in ("C", "D"):
        gbuf = torch.full((P_TOTAL + 8,), -7.0, dtype=torch.float32, device=eng.device)
        lbuf = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
        run_case(eng, states, Q, key, rollout, loss_out=lbuf[1:2], grad_out=gbuf[:P_TOTAL])
        first_g, first_l = np_(gbuf).copy(), np_(lbuf).copy()
        assert (first_g[P_TOTAL:] == -7.0).all() and first_l[0] == -7.0 and first_l[2] == -7.0 and first_l[1] > 0
        assert (first_g[:P_TOTAL] != -7.0).all()
        gbuf.fill_(-7.0)
        lbuf.fill_(-7.0)
        run_case(eng, states, Q, key, rollout, loss_out=lbuf[1:2], grad_out=gbuf[:P_TOTAL])
        assert np.array_equal(bits(np_(gbuf)), bits(first_g)) and np.array_equal(bits(np_(lbuf), np.float64), bits(first_l, np.float64))
    eng.close()


@pytest.mark.parametrize("rollout", [False, True], ids=["teacher-forced", "rollout"])
def test_workspace_handed_between_shapes(rollout):
    """C, E, B, C on one handle: Bp moves the check-point base, and the cells of the lanes beyond B were written by a larger call.
    Each result equals that of a fresh handle that ran only that shape."""
    m = RR.case_model("random", True)
    alone = {}
    for key in ("C", "E", "B"):
        fresh = new_engine(m)
        alone[key] = copies(run_case(fresh, *recordings(), key, rollout))
        fresh.close()
    eng = new_engine(m)
    states, Q = (eng.tensor(x) for x in recordings())
    for key in ("C", "E", "B", "C"):
        assert same_bits(copies(run_case(eng, states, Q, key, rollout)), alone[key]), key
    assert not same_bits(alone["C"], alone["B"])
    eng.close()


def test_a_captured_step_at_the_cap_equals_the_launched_one():
    """gru_train_reserve(1030, 40), then cpmppi_gru_train_step at case C captured on a side stream: two replays leave the master copy
    and the losses of two launched steps on a second handle."""
    m = RR.case_model("golden", True)
    B, W, P = WC.CASES["C"]
    w = WC.case_windows("C")
    states, Q = recordings()
    eng = new_engine(m)
    eng.gru_train_begin()
    eager_l = [np_(eng.gru_train_step(states, Q, w, W, P, lr=HYPER[0], beta1=HYPER[1], beta2=HYPER[2], eps=HYPER[3])).copy() for _ in range(2)]
    eager_p = eng.gru_flatten(eng.gru_train_get())
    eng.close()
    assert eager_l[0][0] != eager_l[1][0]
    eng = new_engine(m)
    eng.gru_train_begin()
    eng.gru_train_reserve(B, W + P)
    s_dev, q_dev = eng.tensor(states), eng.tensor(Q)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    a, keep, _, _ = eng._gru_loss_args(s_dev, q_dev, w, W, P, 1, lbuf, None, False)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng._check(eng.lib.cpmppi_gru_train_step(eng._h, C.byref(a), *HYPER, eng._stream()))
    torch.cuda.current_stream(eng.device).wait_stream(side)
    torch.cuda.synchronize()
    assert bool((lbuf == -7.0).all()), "a capture ran the kernels"
    assert np.array_equal(bits(eng.gru_flatten(eng.gru_train_get())), bits(eng.gru_flatten(m)))
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(np_(lbuf), np.float64), bits(eager_l[i], np.float64)), i
    assert np.array_equal(bits(eng.gru_flatten(eng.gru_train_get())), bits(eager_p))
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. training at width
@functools.lru_cache(maxsize=None)
def training_case():
    from cartpolesimulation_amd.train_gru import initial_weights, make_windows, normalization_from_recordings
    states, Q = TR.oracle_recordings()
    init = {**initial_weights(1873), **normalization_from_recordings(states, Q)}
    legal = make_windows([states.shape[1]] * states.shape[0], 5, 10, 1)
    rng = np.random.default_rng(1030)
    batches = [legal[rng.integers(0, len(legal), 1030)] for _ in range(10)]
    losses, _ = TR.adam_training(init, states, Q, batches, 5, 10, lr=HYPER[0], eps=HYPER[3])
    return states, Q, init, batches, losses


def test_training_at_width_against_float64_adam(capsys):
    states, Q, init, batches, ref = training_case()
    assert ref[-1] < ref[0], "the reference itself must learn"
    eng = new_engine(init)
    s_dev, q_dev = eng.tensor(states), eng.tensor(Q)
    eng.gru_train_begin()
    out = torch.empty(len(batches), dtype=torch.float64, device=eng.device)
    for i, w in enumerate(batches):
        eng.gru_train_step(s_dev, q_dev, w, 5, 10, lr=HYPER[0], eps=HYPER[3], loss_out=out[i:i + 1])
    losses = np_(out)
    dev = np.abs(losses / ref - 1.0)
    report(capsys, f"training at width: reference loss {ref[0]:.5f} -> {ref[-1]:.5f}, device {losses[0]:.5f} -> {losses[-1]:.5f}; step 1 "
                   f"{dev[0]:.3e}, worst step {dev.max():.3e} (step {int(dev.argmax()) + 1}); TRAIN_LOSS_RTOL {TRAIN_LOSS_RTOL:.3e}")
    assert dev[0] < LOSS_RTOL
    assert dev.max() < TRAIN_LOSS_RTOL
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. cpmppi_set_gru ends a training run
def small_batch():
    states, Q = TR.random_recordings(RR.R, RR.T)
    return states, Q, RR.case_windows(33, 3, 4), 3, 4


def test_set_gru_ends_a_training_run():
    """set_gru(A), begin, two steps, set_gru(B): a step and a get are refused by name and launch nothing, the images are B's; begin
    then starts from B with zero moments and a zero counter."""
    model_a, model_b = RR.case_model("golden", True), RR.case_model("random", True)
    states, Q, w, W, P = small_batch()
    kw = dict(lr=HYPER[0], beta1=HYPER[1], beta2=HYPER[2], eps=HYPER[3])
    eng, fresh = new_engine(model_a), new_engine(model_b)
    s_dev, q_dev = eng.tensor(states), eng.tensor(Q)
    eng.gru_train_begin()
    for _ in range(2):
        eng.gru_train_step(s_dev, q_dev, w, W, P, **kw)
    assert not np.array_equal(bits(eng.gru_flatten(eng.gru_train_get())), bits(eng.gru_flatten(model_a)))
    eng.set_gru(model_b)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    for rollout, fn in ((False, "cpmppi_gru_train_step"), (True, "cpmppi_gru_rollout_train_step")):
        a, keep, _, _ = eng._gru_loss_args(s_dev, q_dev, w, W, P, 1, lbuf, None, False, rollout)
        assert getattr(eng.lib, fn)(eng._h, C.byref(a), *HYPER, eng._stream()) == -1
        assert fn + ": call cpmppi_gru_train_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    flat = np.full(P_TOTAL, -7.0, f32)
    assert eng.lib.cpmppi_gru_train_get(eng._h, flat.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert "cpmppi_gru_train_get: call cpmppi_gru_train_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert bool((lbuf == -7.0).all()) and (flat == -7.0).all()
    # nothing rebuilt the images from the old master copy: they are model B's
    mine = copies(eng.gru_loss_grad(s_dev, q_dev, w, W, P))
    theirs = copies(fresh.gru_loss_grad(states, Q, w, W, P))
    assert same_bits(mine, theirs)
    mine = copies(eng.gru_loss_grad(s_dev, q_dev, w, W, P, rollout=True))
    assert same_bits(mine, copies(fresh.gru_loss_grad(states, Q, w, W, P, rollout=True)))
    # a new run starts from B: the moments and the counter of the run before are gone
    eng.gru_train_begin()
    fresh.gru_train_begin()
    assert np.array_equal(bits(eng.gru_flatten(eng.gru_train_get())), bits(eng.gru_flatten(model_b)))
    l_mine = np_(eng.gru_train_step(s_dev, q_dev, w, W, P, **kw)).copy()
    l_theirs = np_(fresh.gru_train_step(states, Q, w, W, P, **kw)).copy()
    assert np.array_equal(bits(l_mine, np.float64), bits(l_theirs, np.float64))
    p_mine, p_theirs = eng.gru_flatten(eng.gru_train_get()), fresh.gru_flatten(fresh.gru_train_get())
    assert np.array_equal(bits(p_mine), bits(p_theirs)) and not np.array_equal(bits(p_mine), bits(eng.gru_flatten(model_b)))
    eng.close()
    fresh.close()


def test_the_exact_f32_consumers_see_the_trained_weights():
    """k steps and no set_gru: gru_predict on the training handle equals, bit for bit, a fresh handle given gru_train_get()'s weights
    with the same normalisation."""
    m = RR.case_model("random", True)
    states, Q, w, W, P = small_batch()
    eng = new_engine(m)
    before = np_(eng.gru_predict(states[:, 0], Q[:, :8])).copy()
    eng.gru_train_begin()
    for _ in range(3):
        eng.gru_train_step(states, Q, w, W, P, lr=HYPER[0], eps=HYPER[3])
    mine = np_(eng.gru_predict(states[:, 0], Q[:, :8])).copy()
    fresh = new_engine({**eng.gru_train_get(), **{k: m[k] for k in TR.NORM_KEYS}})
    theirs = np_(fresh.gru_predict(states[:, 0], Q[:, :8])).copy()
    assert np.array_equal(bits(mine), bits(theirs)) and not np.array_equal(bits(mine), bits(before))
    eng.close()
    fresh.close()
