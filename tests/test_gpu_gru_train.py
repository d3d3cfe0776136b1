"""GPU: training the GRU predictor on recordings - cpmppi_gru_loss_grad (gru_train_forward_kernel, gru_loss_finalize_kernel,
gru_train_reverse_kernel, gru_wgrad_kernel, gru_wgrad_reduce_kernel) and cpmppi_gru_train_begin / _step / _get
(gru_adam_repack_kernel), the Python on top (train_gru) and its command line.

Reference: tests/gru_train_ref.py - torch.nn.GRU + Linear, float64 autograd and float64 torch.optim.Adam on the CPU; pinned against
its own float32 realisation at 6.9e-7 (tests/test_train_gru_host.py).

Bounds, the project's own from tests/test_gpu_grad.py: every parameter tensor within 5e-4 of its max |g| (a tensor the reference
has exactly zero - the recurrent matrices of a one-row window - must be exactly zero), the loss within rtol 5e-4.  There is no
flagged class: the function has no clip and no bounce.  Bit for bit: two runs; loss-only against the gradient call; the b_ih / b_hh
rows of the r and z gates; rows after the windows; a capture's replay; a handle whose images the device rebuilt against one whose
images the host packed.  One Adam step: the closed form in float64, rounded to the float32 the master copy is stored as, within
4 float32 epsilons of lr (measured: equal in every bit).

Shapes: R = 3, T = 40; B in {1, 31, 33, 129} (one lane, a ragged wave, two waves, beyond one workgroup) x (W, P) in {(0,1), (3,4),
(0,6)}, every batch with a window repeated, two that overlap, and one that ends at the recording's last legal row.

Measured on the MI355X (this module's first run; worst over the 12 shapes):
  model    normalisation   gradient (of max |g|)   loss (relative)
  golden   with            1.09e-06                2.9e-08
  golden   without         8.00e-07                7.0e-08
  random   with            6.82e-07                1.6e-07
  random   without         7.51e-07                1.5e-07
Training run (8 recordings x 120 rows of the oracle's plant, W = 5, P = 10, B = 64, lr = 2e-3, 50 steps, against float64 Adam): the
reference's mean loss of steps 40-50 is 0.0815 of step 1's; worst relative deviation of a step's loss 1.19e-07 (step 44; step 1:
1.9e-08), asserted at four times that (TRAIN_LOSS_RTOL) and never beyond 1e-2."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402
from test_gpu_gru_edges import model_of  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKOUT = os.path.join(ROOT, "tests", "golden", "reference_checkout")
R, T = 3, 40
BATCHES = (1, 31, 33, 129)
ROWS = ((0, 1), (3, 4), (0, 6))
GRAD_TOL, LOSS_RTOL = 5e-4, 5e-4
TRAIN_LOSS_RTOL = 4 * 1.19e-7   # four times the measured deviation (module docstring), never beyond 1e-2
P_TOTAL = 10341


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-train] " + text)


def bits(x, dtype=f32):
    return np.ascontiguousarray(np.asarray(x, dtype)).view(np.uint32 if dtype == f32 else np.uint64)


def np_(t):
    return t.cpu().numpy()


def model(name, norm=True):
    m = dict(model_of(name))
    return m if norm else {k: m[k] for k in TR.GRU_KEYS}


def new_engine(m=None):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(1, MPPIConfig(num_rollouts=32, mpc_horizon=8))
    if m is not None:
        eng.set_gru(m)
    return eng


@functools.lru_cache(maxsize=None)
def windows_of(B, W, P, shift=1):
    """B windows of the R x T recordings: drawn from the legal ones, then [1] = [0] (a window twice), [2] = one row on from [0]
    (overlapping), [-1] = the last recording's last legal window."""
    from cartpolesimulation_amd.train_gru import make_windows
    legal = make_windows([T] * R, W, P, shift)
    w = legal[np.random.Generator(np.random.SFC64([B, W, P])).integers(0, len(legal) - 1, B)].copy()
    if B >= 3:
        w[0] = (0, 4)
        w[1] = w[0]
        w[2] = (0, 5)
    w[-1] = legal[-1]
    assert w[-1, 0] == R - 1 and w[-1, 1] + W + P - 1 + shift == T - 1
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(name, norm, B, W, P):
    states, Q = TR.random_recordings(R, T)
    return TR.loss_and_grad(model(name, norm), states, Q, windows_of(B, W, P), W, P)


def unflat(g):
    from cartpolesimulation_amd.engine import MPPIEngine
    return MPPIEngine.gru_unflatten(np.asarray(g))


# ---------------------------------------------------------------------------------------------- 1. gradient against float64 autograd
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "identity"])
@pytest.mark.parametrize("name", ["golden", "random"])
def test_loss_and_gradient_against_float64_autograd(name, norm, capsys):
    eng = new_engine(model(name, norm))
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    worst_g = worst_l = 0.0
    for B in BATCHES:
        for W, P in ROWS:
            loss, grad = eng.gru_loss_grad(states, Q, windows_of(B, W, P), W, P)
            l_ref, g_ref = reference(name, norm, B, W, P)
            g, l = unflat(np_(grad)), float(np_(loss)[0])
            rel_g, rel_l = TR.worst_relative(g, g_ref), abs(l - l_ref) / l_ref
            report(capsys, f"{name} norm={norm} B {B} W {W} P {P}: gradient {rel_g:.3e}, loss {rel_l:.3e}")
            worst_g, worst_l = max(worst_g, rel_g), max(worst_l, rel_l)
            assert np.isfinite(np_(grad)).all()
            assert rel_g < GRAD_TOL, (B, W, P)
            assert rel_l < LOSS_RTOL, (B, W, P)
            # the r and z gates see b_ih + b_hh: both rows receive the same sum, bit for bit
            for l_ in range(2):
                assert np.array_equal(bits(g[f"b_ih{l_}"][:64]), bits(g[f"b_hh{l_}"][:64]))
                assert not np.array_equal(bits(g[f"b_ih{l_}"][64:]), bits(g[f"b_hh{l_}"][64:]))
            if W + P == 1:                                   # a single row from a zero memory has no recurrence
                assert not g["w_hh0"].any() and not g["w_hh1"].any()
    report(capsys, f"{name} norm={norm}: WORST gradient {worst_g:.3e}, loss {worst_l:.3e}")
    eng.close()


def test_wash_out_rows_and_rows_after_the_window():
    """The same windows with another wash-out length give another gradient; rows of the recordings that no window reaches give the
    same bits."""
    eng = new_engine(model("random"))
    states, Q = TR.random_recordings(R, T)
    w = np.array([[0, 0], [1, 3], [2, 10], [1, 9]])          # last label row at most 10 + 3 + 4 - 1 + 1 = 17
    loss_a, grad_a = (np_(x).copy() for x in eng.gru_loss_grad(states, Q, w, 3, 4))
    loss_b, grad_b = (np_(x).copy() for x in eng.gru_loss_grad(states, Q, w, 2, 4))
    assert loss_a[0] != loss_b[0] and (bits(grad_a) != bits(grad_b)).mean() > 0.9
    s2, q2 = states.copy(), Q.copy()
    s2[:, 18:] = -s2[:, 18:] + f32(0.5)
    q2[:, 18:] = f32(0.77)
    loss_c, grad_c = (np_(x).copy() for x in eng.gru_loss_grad(s2, q2, w, 3, 4))
    assert np.array_equal(bits(loss_a, np.float64), bits(loss_c, np.float64)) and np.array_equal(bits(grad_a), bits(grad_c))
    s2[:, 17] += f32(0.25)                                  # the last label row does count
    loss_d, _ = eng.gru_loss_grad(s2, q2, w, 3, 4)
    assert np_(loss_d)[0] != loss_a[0]
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. determinism and bounds
def test_two_runs_loss_only_and_sentinels():
    eng = new_engine(model("golden"))
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    for B, (W, P) in ((129, (3, 4)), (33, (0, 6))):
        w = windows_of(B, W, P)
        gbuf = torch.full((P_TOTAL + 8,), -7.0, dtype=torch.float32, device=eng.device)
        lbuf = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
        eng.gru_loss_grad(states, Q, w, W, P, loss_out=lbuf[1:2], grad_out=gbuf[:P_TOTAL])
        first_g, first_l = np_(gbuf).copy(), np_(lbuf).copy()
        assert (first_g[P_TOTAL:] == -7.0).all() and first_l[0] == -7.0 and first_l[2] == -7.0 and first_l[1] > 0
        assert (first_g[:P_TOTAL] != -7.0).all()
        gbuf.fill_(-7.0)
        lbuf.fill_(-7.0)
        eng.gru_loss_grad(states, Q, w, W, P, loss_out=lbuf[1:2], grad_out=gbuf[:P_TOTAL])
        assert np.array_equal(bits(np_(gbuf)), bits(first_g)) and np.array_equal(bits(np_(lbuf), np.float64), bits(first_l, np.float64))
        lbuf.fill_(-7.0)
        loss, none = eng.gru_loss_grad(states, Q, w, W, P, grad=False, loss_out=lbuf[1:2])
        assert none is None and np.array_equal(bits(np_(lbuf), np.float64), bits(first_l, np.float64))
    eng.close()


def test_refusals_launch_nothing():
    from cartpolesimulation_amd import _lib as L
    eng, bare = new_engine(model("golden")), new_engine()
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    W, P = 3, 4
    gbuf = torch.full((P_TOTAL,), -7.0, dtype=torch.float32, device=eng.device)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    stream = eng._stream()

    def block():
        return eng._gru_loss_args(states, Q, windows_of(33, W, P), W, P, 1, lbuf, gbuf, True)

    def refused(handle, a, code, text, keep=None):
        rc = eng.lib.cpmppi_gru_loss_grad(handle, C.byref(a), stream)
        assert rc == code, (rc, text)
        assert text in eng.lib.cpmppi_last_error(handle).decode(), eng.lib.cpmppi_last_error(handle).decode()
        torch.cuda.synchronize()
        assert bool((gbuf == -7.0).all()) and bool((lbuf == -7.0).all()), text

    a, keep, _, _ = block()
    refused(bare._h, a, -1, "cpmppi_gru_loss_grad: no model set")
    for field in ("states", "Q", "windows", "windows_host", "loss_out"):
        a, keep, _, _ = block()
        setattr(a, field, None)
        refused(eng._h, a, -1, "cpmppi_gru_loss_grad: states, Q, windows, windows_host and loss_out are required")
    for field in ("B", "R", "T", "post_wash_out"):
        a, keep, _, _ = block()
        setattr(a, field, 0)
        refused(eng._h, a, -1, "cpmppi_gru_loss_grad: B, R, T and post_wash_out must be at least 1")
    for r, t0 in ((R, 0), (0, T - (W + P - 1 + 1)), (0, 2 ** 32 - 1)):
        a, keep, _, _ = block()
        keep[3][5] = (r, t0)                                 # the HOST copy is what is checked
        refused(eng._h, a, -1, "cpmppi_gru_loss_grad: window 5 = (%d, %d) lies outside" % (r, t0))
    a, keep, _, _ = block()
    a.shift_labels = 30                                      # the labels would lie past the recording
    refused(eng._h, a, -1, "lies outside")
    for field in ("states", "grad_out", "loss_out"):
        a, keep, _, _ = block()
        setattr(a, field, getattr(a, field) + (4 if field == "loss_out" else 2))
        refused(eng._h, a, -5, "cpmppi_gru_loss_grad: misaligned pointer")
    # the last legal row is accepted
    a, keep, _, _ = block()
    keep[3][5] = (0, T - 1 - (W + P - 1 + 1))
    assert eng.lib.cpmppi_gru_loss_grad(eng._h, C.byref(a), stream) == 0
    torch.cuda.synchronize()
    # training entry points without their start
    assert eng.lib.cpmppi_gru_train_step(eng._h, C.byref(a), 1e-3, 0.9, 0.999, 1e-8, stream) == -1
    assert "cpmppi_gru_train_step: call cpmppi_gru_train_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    flat = np.zeros(P_TOTAL, f32)
    assert eng.lib.cpmppi_gru_train_get(eng._h, flat.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert eng.lib.cpmppi_gru_train_begin(bare._h) == -1 and "no model set" in eng.lib.cpmppi_last_error(bare._h).decode()
    assert eng.lib.cpmppi_gru_train_reserve(eng._h, 0, 4) == -1
    # the engine's own checks word the refusals before the library is asked
    with pytest.raises(ValueError, match="every window"):
        eng.gru_loss_grad(states, Q, [[0, T - 7]], W, P)
    with pytest.raises(ValueError, match="every window"):
        eng.gru_loss_grad(states, Q, [[R, 0]], W, P)
    with pytest.raises(ValueError, match="windows must be integers"):
        eng.gru_loss_grad(states, Q, np.zeros((4, 2), f32), W, P)
    with pytest.raises(ValueError, match="post_wash_out >= 1"):
        eng.gru_loss_grad(states, Q, [[0, 0]], W, 0)
    with pytest.raises(ValueError, match="no model set"):
        bare.gru_loss_grad(states, Q, [[0, 0]], W, P)
    with pytest.raises(ValueError, match="no model set"):
        bare.gru_train_begin()
    eng.close()
    bare.close()


def test_capture_is_refused_cold_and_replays_warm():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = new_engine(model("golden"))
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    W, P = 3, 4
    gbuf = torch.full((P_TOTAL,), -7.0, dtype=torch.float32, device=eng.device)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    call = eng.prepare_gru_loss_grad(states, Q, windows_of(129, W, P), W, P, loss_out=lbuf, grad_out=gbuf)
    marker = eng.zeros(4)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g0, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_gru_loss_grad: the stream is being captured"):
                call.run()
            marker.add_(1.0)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    g0.replay()
    torch.cuda.synchronize()
    assert np_(marker).tolist() == [1.0] * 4 and bool((gbuf == -7.0).all()) and bool((lbuf == -7.0).all())
    eng.gru_train_reserve(129, W + P)                       # the reserving call
    call.run()
    eager_l, eager_g = np_(lbuf).copy(), np_(gbuf).copy()
    gbuf.fill_(-7.0)
    lbuf.fill_(-7.0)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call.run()
    torch.cuda.current_stream(eng.device).wait_stream(side)
    torch.cuda.synchronize()
    assert bool((gbuf == -7.0).all()), "a capture ran the kernels"
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(np_(gbuf)), bits(eager_g)) and np.array_equal(bits(np_(lbuf), np.float64), bits(eager_l, np.float64))
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. image rebuild, Adam
def test_device_built_images_equal_host_built_ones():
    """After 5 training steps the weights, downloaded and packed on the host of a FRESH handle, give bit for bit the loss and
    gradient of the training handle, whose images the device rebuilt; likewise right after gru_train_begin."""
    from cartpolesimulation_amd.engine import MPPIEngine
    m = model("random")
    norm = {k: m[k] for k in TR.NORM_KEYS}
    eng = new_engine(m)
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    W, P = 3, 4
    probe = windows_of(129, W, P)
    host = [np_(x).copy() for x in eng.gru_loss_grad(states, Q, probe, W, P)]
    eng.gru_train_begin()
    begun = [np_(x).copy() for x in eng.gru_loss_grad(states, Q, probe, W, P)]
    assert np.array_equal(bits(host[0], np.float64), bits(begun[0], np.float64)) and np.array_equal(bits(host[1]), bits(begun[1]))
    for i, B in enumerate((33, 31, 129, 1, 33)):
        eng.gru_train_step(states, Q, windows_of(B, W, P), W, P, lr=2e-3 * (i + 1))
    trained = eng.gru_train_get()
    assert (MPPIEngine.gru_flatten(trained) != MPPIEngine.gru_flatten(m)).mean() > 0.99
    mine = [np_(x).copy() for x in eng.gru_loss_grad(states, Q, probe, W, P)]
    assert mine[0][0] != host[0][0]
    fresh = new_engine({**trained, **norm})
    theirs = [np_(x).copy() for x in fresh.gru_loss_grad(states, Q, probe, W, P)]
    assert np.array_equal(bits(mine[0], np.float64), bits(theirs[0], np.float64))
    assert np.array_equal(bits(mine[1]), bits(theirs[1]))
    eng.close()
    fresh.close()


def test_one_adam_step_is_the_closed_form(capsys):
    from cartpolesimulation_amd.engine import MPPIEngine
    m = model("golden")
    eng = new_engine(m)
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    W, P, w = 3, 4, windows_of(33, 3, 4)
    lr, b1, b2, eps = f32(2e-3), f32(0.9), f32(0.999), f32(1e-7)
    loss0, grad = eng.gru_loss_grad(states, Q, w, W, P)
    g, p0 = np_(grad).astype(np.float64), MPPIEngine.gru_flatten(m).astype(np.float64)
    eng.gru_train_begin()
    loss = eng.gru_train_step(states, Q, w, W, P, lr=lr, beta1=b1, beta2=b2, eps=eps)
    assert np.array_equal(bits(np_(loss), np.float64), bits(np_(loss0), np.float64))       # the loss BEFORE the update
    p1 = MPPIEngine.gru_flatten(eng.gru_train_get())
    B1, B2 = float(b1), float(b2)
    mom1, mom2 = B1 * 0.0 + (1.0 - B1) * g, B2 * 0.0 + (1.0 - B2) * g * g
    closed = p0 - float(lr) * (mom1 / (1.0 - B1 ** 1)) / (np.sqrt(mom2 / (1.0 - B2 ** 1)) + float(eps))
    dev = np.abs(p1.astype(np.float64) - closed.astype(f32).astype(np.float64)).max()
    moved = np.abs(p1.astype(np.float64) - p0)
    report(capsys, f"one Adam step: |device - closed form| {dev:.3e} (4 eps lr = {4 * np.finfo(f32).eps * float(lr):.3e}); "
                   f"steps between {moved.min():.3e} and {moved.max():.3e}")
    assert dev <= 4 * np.finfo(f32).eps * float(lr)
    assert moved.max() <= float(lr) * 1.001 and np.median(moved) > 0.9 * float(lr)
    # a second step: bias correction with t = 2, the moments carried
    g2 = np_(eng.gru_loss_grad(states, Q, w, W, P)[1]).astype(np.float64)
    eng.gru_train_step(states, Q, w, W, P, lr=lr, beta1=b1, beta2=b2, eps=eps)
    p2 = MPPIEngine.gru_flatten(eng.gru_train_get()).astype(np.float64)
    m1, m2 = mom1.astype(f32).astype(np.float64), mom2.astype(f32).astype(np.float64)        # (stored as float32)
    m1, m2 = B1 * m1 + (1.0 - B1) * g2, B2 * m2 + (1.0 - B2) * g2 * g2
    closed2 = p1.astype(np.float64) - float(lr) * (m1 / (1.0 - B1 ** 2)) / (np.sqrt(m2 / (1.0 - B2 ** 2)) + float(eps))
    assert np.abs(p2 - closed2.astype(f32).astype(np.float64)).max() <= 4 * np.finfo(f32).eps * float(lr)
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. training run against float64 Adam
@functools.lru_cache(maxsize=None)
def training_case():
    from cartpolesimulation_amd.train_gru import initial_weights, make_windows, normalization_from_recordings
    states, Q = TR.oracle_recordings()
    init = {**initial_weights(1873), **normalization_from_recordings(states, Q)}
    legal = make_windows([states.shape[1]] * states.shape[0], 5, 10, 1)
    rng = np.random.default_rng(1873)
    batches = [legal[rng.permutation(len(legal))[:64]] for _ in range(50)]
    losses, weights = TR.adam_training(init, states, Q, batches, 5, 10, lr=2e-3, eps=1e-8)
    return states, Q, init, batches, losses, weights


def test_training_run_against_float64_adam(capsys):
    from cartpolesimulation_amd.brunton import brunton_test
    states, Q, init, batches, ref, _ = training_case()
    ratio = ref[40:].mean() / ref[0]
    assert ratio < 0.15, f"the reference itself must learn: {ratio:.3f}"
    eng = new_engine(init)
    s_dev, q_dev = eng.tensor(states), eng.tensor(Q)
    eng.gru_train_begin()
    out = torch.empty(len(batches), dtype=torch.float64, device=eng.device)
    for i, w in enumerate(batches):
        eng.gru_train_step(s_dev, q_dev, w, 5, 10, lr=2e-3, eps=1e-8, loss_out=out[i:i + 1])
    losses = np_(out)
    dev = np.abs(losses / ref - 1.0)
    report(capsys, f"training run: reference ratio {ratio:.4f}, device ratio {losses[40:].mean() / losses[0]:.4f}; step 1 {dev[0]:.3e}, "
                   f"worst step {dev.max():.3e} (step {int(dev.argmax()) + 1})")
    assert dev[0] < LOSS_RTOL
    assert dev.max() < TRAIN_LOSS_RTOL <= 1e-2
    trained = {**eng.gru_train_get(), **{k: init[k] for k in TR.NORM_KEYS}}
    eng.close()
    spec = "GRU-6IN-32H1-32H2-5OUT-0"
    before = brunton_test((states, Q), predictors=(spec,), horizon=1, gru_model=init)[spec]["rmse"][0, 1:]
    after = brunton_test((states, Q), predictors=(spec,), horizon=1, gru_model=trained)[spec]["rmse"][0, 1:]
    report(capsys, f"one-step Brunton rmse (angleD, cos, sin, position, positionD): before {before}, after {after}")
    # in units of each feature's range (the loss the training minimises is in those units)
    scale = init["out_scale"].astype(np.float64)
    assert np.sum((after / scale) ** 2) < np.sum((before / scale) ** 2)


def test_train_gru_schedule_and_validation(capsys):
    """train_gru end to end on the same data: batches from default_rng(seed), the plateau rule on the validation loss, the model
    left in the engine."""
    from cartpolesimulation_amd.train_gru import train_gru
    states, Q, init, _, _, _ = training_case()
    eng = new_engine()
    lines = []
    trained, hist = train_gru(eng, states[:6], Q[:6], epochs=3, batch_size=64, lr=2e-3, seed=3, wash_out=5, post_wash_out=10,
                              validation=(states[6:], Q[6:], None), init={k: init[k] for k in TR.GRU_KEYS}, patience=1,
                              min_delta=10.0, log=lines.append)
    assert len(hist["loss"]) == 3 and len(hist["val_loss"]) == 3 and len(lines) == 3
    assert len(hist["batch_loss"]) == 3 * -(-6 * 105 // 64)
    assert hist["lr"] == [2e-3, 2e-3, 1e-3]                  # min_delta 10: only the first epoch improves on infinity
    assert hist["loss"][-1] < hist["loss"][0] and hist["val_loss"][-1] < hist["val_loss"][0]
    assert set(trained) == set(TR.GRU_KEYS) | set(TR.NORM_KEYS)
    # the engine holds the trained model: its validation loss is the last one reported
    from cartpolesimulation_amd.train_gru import make_windows
    vw = make_windows([120, 120], 5, 10, 1)
    loss, _ = eng.gru_loss_grad(states[6:], Q[6:], vw, 5, 10, grad=False)
    assert float(np_(loss)[0]) == pytest.approx(hist["val_loss"][-1], rel=1e-12)
    eng.close()


# ---------------------------------------------------------------------------------------------- 5. command line
def test_command_line_writes_a_folder_the_tools_accept(tmp_path, capsys):
    from cartpolesimulation_amd import brunton as B
    from cartpolesimulation_amd import recording as RC
    from cartpolesimulation_amd import train_gru as TG
    from cartpolesimulation_amd.model_folder import load_gru_model
    states, Q = TR.oracle_recordings()
    rec = tmp_path / "Recordings"
    rec.mkdir()
    for r in range(4):
        cols = {"time": 0.02 * np.arange(states.shape[1])}
        cols.update({name: states[r, :, i] for i, name in enumerate(B.FEATURES)})
        cols.update({"Q_applied": Q[r], "L": np.full(states.shape[1], f32(0.395))})
        RC.write_recording(str(rec / f"Experiment-{r}.csv"), cols, header=["Data:"])
    out = tmp_path / "Models" / "GRU-6IN-32H1-32H2-5OUT-0"
    model_, hist = TG.main(["--recordings", str(rec), "--out", str(out), "--config-root", CHECKOUT, "--net", "GRU-32H1-32H2",
                            "--dynamics-model", "--shift-labels", "1", "--wash-out", "5", "--post-wash-out", "10", "--epochs", "2"])
    text = capsys.readouterr().out
    assert "epoch 2/2" in text and "model folder" in text and len(hist["loss"]) == 2 and hist["loss"][1] < hist["loss"][0]
    back = load_gru_model(str(out))
    assert set(back) == set(model_)
    for k in back:
        assert np.array_equal(bits(back[k]), bits(model_[k])), k
    cfg = tmp_path / "config_testing.yml"
    cfg.write_text("predictors_specifications_testing: ['GRU-6IN-32H1-32H2-5OUT-0']\ntest_file: 'x.csv'\ntest_len: 'max'\n"
                   "test_max_horizon: 5\ntest_start_idx: 0\ndecimation: 1\n")
    res = B.main(["--config-root", CHECKOUT, "--config-testing", str(cfg), "--test-file", str(rec), "--gru-model", str(out)])
    r = res["GRU-6IN-32H1-32H2-5OUT-0"]
    assert r["n_starts"] == 4 * (120 - 5) and np.isfinite(r["rmse"]).all()
