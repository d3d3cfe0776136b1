"""GPU: the neural imitator - cpmppi_dense_control (dense_control_kernel), cpmppi_dense_loss_grad and cpmppi_dense_train_*
(dense_grad_kernel, dense_finalize_kernel), the refusals of the C ABI and train_imitator on top.

Reference: tests/dense_ref.py, float64 torch on the CPU (pinned in tests/test_imitator_host.py).

Bounds.  No constant: for every compared tensor the test evaluates dense_ref in FLOAT32 on the CPU at the case's own shape and takes
what that plain evaluation of the same formulas loses against float64 - per gradient tensor relative to max |g|, for the loss
relative to the loss, for controls absolute.  The device must stay within MARGIN = 8 times that, with a floor of 1e-6: room for
another summation order (MFMA tiles, per-workgroup partial rows), not for a missing term (profiles/r28/mutants.txt).

Sample counts N = B P, derived from the unit's constants (read from cpmppi_dense.hip: TILE, WG_TILES, FIN_CHUNK): 1; 63 and 65 (one
lane short of a tile, one beyond); WG_SAMPLES + 1; 2 WG_SAMPLES + 44 (three workgroups, the last with one ragged tile);
FIN_CHUNK WG_SAMPLES + 1 (one partial row more than one pass of the finalize kernel's chunked loop)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, FLOOR = 8.0, 1e-6
R, T = 4, 200


def unit_constant(name):
    with open(os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_dense.hip")) as fh:
        return int(re.search(r"constexpr int " + name + r" = (\d+);", fh.read()).group(1))


TILE, WG_TILES, FIN_CHUNK = unit_constant("TILE"), unit_constant("WG_TILES"), unit_constant("FIN_CHUNK")
WG = TILE * WG_TILES
# (B, P, shift_labels): N = B P
CASES = ((1, 1, 0), (63, 1, 0), (13, 5, 1), (WG + 1, 1, 1), ((2 * WG + 44) // 50, 50, 0), ((FIN_CHUNK * WG + 1) // 5, 5, 1))
assert TILE == 64 and [b * p for b, p, _ in CASES] == [1, 63, 65, WG + 1, 2 * WG + 44, FIN_CHUNK * WG + 1]


def report(capsys, text):
    with capsys.disabled():
        print("\n[imitator] " + text)


def bits(x, dtype=f32):
    return np.ascontiguousarray(np.asarray(x, dtype)).view(np.uint32 if dtype == f32 else np.uint64)


def np_(t):
    return t.cpu().numpy()


def bound(err32):
    return max(MARGIN * float(err32), FLOOR)


@functools.lru_cache(maxsize=None)
def model(name):
    return D.golden_model() if name == "golden" else D.random_model(21)


@functools.lru_cache(maxsize=None)
def data():
    return D.recordings(7, R, T)


def new_engine(m=None):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(1, MPPIConfig(num_rollouts=32, mpc_horizon=8))
    if m is not None:
        eng.set_dense(m)
    return eng


@functools.lru_cache(maxsize=None)
def windows_of(B, P, shift):
    """B windows drawn (with repeats) from the legal ones; [0] ends on its recording's last legal row."""
    from cartpolesimulation_amd._training import make_windows
    legal = make_windows([T] * R, 0, P, shift)
    w = legal[np.random.default_rng(B * 1000 + P).integers(0, len(legal), B)]
    w[0] = (R - 1, T - P - shift)
    return w


@functools.lru_cache(maxsize=None)
def reference(name, B, P, shift):
    """-> (loss64, grad64, relative float32 loss error, float32 gradient error per tensor relative to max |g|)."""
    x, lab = D.samples(*data(), windows_of(B, P, shift), P, shift)
    loss, g = D.loss_and_grad(model(name), x, lab)
    loss32, g32 = D.loss_and_grad(model(name), x, lab, torch.float32)
    return loss, g, abs(loss32 - loss) / loss, per_tensor(g32, g)


def per_tensor(got, want):
    out, at = [], 0
    for shp in D.SHAPES:
        n = int(np.prod(shp))
        out.append(float(np.abs(got[at:at + n] - want[at:at + n]).max() / np.abs(want[at:at + n]).max()))
        at += n
    return np.array(out)


# ---------------------------------------------------------------------------------------------- dense_control
@pytest.mark.parametrize("E", [1, 65, 300])
def test_control_against_float64(E, capsys):
    m = model("golden")
    s, tp, te, _ = D.recordings(101, R=1, T=300)
    s, tp, te = s[0, :E].copy(), tp[0, :E].copy(), te[0, :E].copy()
    q64, y64, raw = D.control(m, s, tp, te)
    _, y32, raw32 = D.control(m, s, tp, te, torch.float32)
    if E > 1:                                                       # the draw, judged on the CPU alone
        assert (raw > 1).any() and (raw < -1).any() and (np.abs(raw) < 1).sum() >= E / 2
    eng = new_engine(m)
    y_out, count = eng.empty(E), torch.full((1,), 41, dtype=torch.int64, device=eng.device)
    Q, y = eng.dense_control(eng.tensor(s), eng.tensor(tp), eng.tensor(te), y_out=y_out, count_dev=count)
    Q2, _ = eng.dense_control(eng.tensor(s), eng.tensor(tp), eng.tensor(te), count_dev=count)
    Q, y, Q2 = np_(Q), np_(y), np_(Q2)
    assert y is not None and int(count.item()) == 43                # one per call
    assert np.array_equal(bits(Q), bits(Q2))
    by, bq = bound(np.abs(y32 - y64).max()), bound(np.abs(raw32 - raw).max())
    # an env the float64 reference has within the bound of a limit may land on either side of it
    inside, above, below = np.abs(raw) < 1 - bq, raw > 1 + bq, raw < -1 - bq
    report(capsys, f"control E={E}: y err {np.abs(y - y64).max():.3e} (float32 ref {np.abs(y32 - y64).max():.3e}, bound {by:.3e}), "
                   f"Q err {np.abs(Q - q64)[inside].max() if inside.any() else 0:.3e} (bound {bq:.3e})")
    assert np.abs(y - y64).max() <= by
    assert np.abs(Q - q64)[inside].max(initial=0.0) <= bq
    assert (Q[above] == 1.0).all() and (Q[below] == -1.0).all() and (np.abs(Q) <= 1.0).all()
    eng.close()


def test_control_passes_a_nan_on_in_its_env_only():
    m = model("golden")
    s, tp, te, _ = D.recordings(101, R=1, T=70)
    s, tp, te = s[0].copy(), tp[0].copy(), te[0].copy()
    eng = new_engine(m)
    clean, _ = eng.dense_control(eng.tensor(s), eng.tensor(tp), eng.tensor(te))
    clean = np_(clean).copy()
    s[3, 4], tp[66] = np.nan, np.nan
    Q, y = eng.dense_control(eng.tensor(s), eng.tensor(tp), eng.tensor(te), y_out=eng.empty(70))
    Q, y = np_(Q), np_(y)
    bad = np.zeros(70, bool)
    bad[[3, 66]] = True
    assert np.isnan(Q[bad]).all() and np.isnan(y[bad]).all()
    assert np.array_equal(bits(Q[~bad]), bits(clean[~bad]))
    eng.close()


# ---------------------------------------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("name", ["golden", "random"])
@pytest.mark.parametrize("B,P,shift", CASES)
def test_loss_and_gradient_against_float64_autograd(name, B, P, shift, capsys):
    loss64, g64, loss_err32, g_err32 = reference(name, B, P, shift)
    eng = new_engine(model(name))
    dev = [eng.tensor(x) for x in data()]
    w = windows_of(B, P, shift)
    loss, grad = eng.dense_loss_grad(*dev, w, P, shift)
    loss, grad = np_(loss).copy(), np_(grad).copy()
    err = per_tensor(grad.astype(np.float64), g64)
    ratio = err / np.maximum(g_err32, FLOOR / MARGIN)
    report(capsys, f"{name} N={B * P} (B={B}, P={P}, shift={shift}): gradient err per tensor {np.array2string(err, precision=2)} = "
                   f"{np.array2string(ratio, precision=2)} x float32 ref; loss rel {abs(loss[0] - loss64) / loss64:.2e} "
                   f"(float32 ref {loss_err32:.2e})")
    for k, e, e32 in zip(D.KEYS, err, g_err32):
        assert e <= bound(e32), (k, e, e32)
    assert abs(loss[0] - loss64) / loss64 <= bound(loss_err32)
    # the loss alone: the bits of the gradient call's; a second run: the same bits
    only, none = eng.dense_loss_grad(*dev, w, P, shift, grad=False)
    assert none is None and np.array_equal(bits(np_(only), np.float64), bits(loss, np.float64))
    loss2, grad2 = eng.dense_loss_grad(*dev, w, P, shift)
    assert np.array_equal(bits(np_(loss2), np.float64), bits(loss, np.float64)) and np.array_equal(bits(np_(grad2)), bits(grad))
    eng.close()


def test_a_small_call_after_a_larger_one_equals_a_fresh_handle():
    m = model("random")
    big, small = CASES[-1], CASES[2]
    eng, fresh = new_engine(m), new_engine(m)
    dev = [eng.tensor(x) for x in data()]
    eng.dense_loss_grad(*dev, windows_of(*big), big[1], big[2])
    a = eng.dense_loss_grad(*dev, windows_of(*small), small[1], small[2])
    b = fresh.dense_loss_grad(*dev, windows_of(*small), small[1], small[2])
    assert np.array_equal(bits(np_(a[0]), np.float64), bits(np_(b[0]), np.float64)) and np.array_equal(bits(np_(a[1])), bits(np_(b[1])))
    eng.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------- Adam
def test_two_adam_steps_match_the_closed_form(capsys):
    m, (B, P, shift) = model("random"), CASES[3]
    w = windows_of(B, P, shift)
    x, lab = D.samples(*data(), w, P, shift)
    eng = new_engine(m)
    dev = [eng.tensor(x_) for x_ in data()]
    eng.dense_train_begin()
    assert np.array_equal(bits(eng.dense_flatten(eng.dense_train_get())), bits(D.flatten(m)))
    opt, cur = D.Adam(D.flatten(m), 1e-3), dict(m)
    for step in range(2):
        loss64, g64 = D.loss_and_grad(cur, x, lab)
        before = opt.p.copy()
        want = opt.step(g64).copy()
        loss = float(eng.dense_train_step(*dev, w, P, shift, lr=1e-3).item())
        got = eng.dense_flatten(eng.dense_train_get())
        # the update of a parameter is lr m^ / (sqrt(v^) + eps): it follows the gradient's error where |g| >> eps; compared on the
        # update itself, relative to lr
        d = np.abs((got.astype(np.float64) - before) - (want.astype(np.float64) - before)) / 1e-3
        big = np.abs(g64) > 1e-3 * np.abs(g64).max()
        report(capsys, f"Adam step {step + 1}: loss rel {abs(loss - loss64) / loss64:.2e}; update error / lr: {d[big].max():.2e} where |g| > "
                       f"1e-3 max|g| ({big.sum()} of {D.NPAR}), {d.max():.2e} overall")
        assert abs(loss - loss64) / loss64 <= bound(reference("random", B, P, shift)[2])
        # step 1 is lr g / (|g| + eps), insensitive to g; at step 2 an error dg moves the update by about lr dg / |g|: with the
        # gradient bound b of max |g| that is b / 1e-3 of lr where |g| > 1e-3 max |g|, taken twice (both steps' gradients enter);
        # everywhere an update is at most about lr in size
        b = bound(reference("random", B, P, shift)[3].max())
        assert d[big].max() <= 2 * b / 1e-3 and d.max() < 2.0
        cur = {**cur, **D.unflatten(got)}                           # the next step is compared from the device's own parameters
        opt.p = got.copy()
    eng.close()


@functools.lru_cache(maxsize=None)
def trajectory():
    """Twenty steps at B = 64 from the random model: the float64 trajectory's losses, and the float32 one's deviation from them."""
    from cartpolesimulation_amd._training import make_windows
    legal = make_windows([T] * R, 0, 1, 0)
    rng = np.random.default_rng(5)
    batches = [legal[rng.choice(len(legal), 64, replace=False)] for _ in range(20)]
    xs = [D.samples(*data(), w, 1, 0) for w in batches]
    _, ref = D.train(model("random"), xs, 2e-3)
    # the same run with float32 gradients (Adam stays the header's)
    opt, cur, l32 = D.Adam(D.flatten(model("random")), 2e-3), dict(model("random")), []
    for x, lab in xs:
        loss, g = D.loss_and_grad(cur, x, lab, torch.float32)
        l32.append(loss)
        cur = {**cur, **D.unflatten(opt.step(g))}
    return batches, np.array(ref), np.abs(np.array(l32) / np.array(ref) - 1.0)


def test_twenty_steps_follow_the_float64_trajectory(capsys):
    """The rule of tests/test_gpu_gru_train.py: step 1 within the loss bound, every step within the run's bound, never beyond 1e-2 -
    the run's bound here being MARGIN times what the float32 trajectory of the reference itself deviates by."""
    batches, ref, dev32 = trajectory()
    eng = new_engine(model("random"))
    dev = [eng.tensor(x) for x in data()]
    eng.dense_train_begin()
    out = torch.empty(20, dtype=torch.float64, device=eng.device)
    for i, w in enumerate(batches):
        eng.dense_train_step(*dev, w, 1, 0, lr=2e-3, loss_out=out[i:i + 1])
    got = np.abs(np_(out) / ref - 1.0)
    run_bound = bound(dev32.max())
    report(capsys, f"20 steps: worst deviation {got.max():.2e} (step {int(got.argmax()) + 1}); float32 reference {dev32.max():.2e}, "
                   f"bound {run_bound:.2e}; step 1 {got[0]:.2e}")
    assert got[0] <= bound(dev32[0])
    assert got.max() <= run_bound <= 1e-2
    eng.close()


def test_a_parameter_with_zero_gradient_keeps_its_bits():
    """Hidden unit 5 of layer 2 with w3[5], its incoming row of w2 and its bias zero: h2[5] is exactly 0, so the gradients of all
    three are exactly 0 in dense_ref (checked first) and stay so from step to step - Adam leaves their bits alone.  Unit 9 of
    layer 1 with column 9 of w2 zero: its row of w1 and its bias have the gradient exactly 0 at the FIRST step (w2's column then
    moves), and keep their bits through it."""
    m = {k: v.copy() for k, v in model("random").items()}
    m["w3"][0, 5], m["w2"][5, :], m["b2"][5] = 0.0, 0.0, 0.0
    m["w2"][:, 9] = 0.0
    B, P, shift = CASES[2]
    w = windows_of(B, P, shift)
    x, lab = D.samples(*data(), w, P, shift)
    g = D.unflatten(D.loss_and_grad(m, x, lab)[1])
    zero = lambda g: not (g["w2"][5].any() or g["b2"][5] or g["w3"][0, 5] or g["w1"][9].any() or g["b1"][9])  # noqa: E731
    assert zero(g) and g["w2"][4].all() and g["w2"][:, 9].any()     # exact zeros on the CPU, and only there
    eng = new_engine(m)
    dev = [eng.tensor(x_) for x_ in data()]
    assert zero(D.unflatten(np_(eng.dense_loss_grad(*dev, w, P, shift)[1])))
    eng.dense_train_begin()
    for step in range(3):
        eng.dense_train_step(*dev, w, P, shift, lr=1e-2)
        got = eng.dense_train_get()
        for k, i in (("w2", 5), ("b2", 5), ("w3", (0, 5))) + ((("w1", 9), ("b1", 9)) if step == 0 else ()):
            assert np.array_equal(bits(got[k][i]), bits(m[k][i])), (k, step)
    assert not np.array_equal(got["w2"][4], m["w2"][4]) and got["w2"][:, 9].any()
    eng.close()


def test_captured_steps_equal_launched_steps():
    m, (B, P, shift) = model("random"), CASES[4]
    w = windows_of(B, P, shift)
    results = []
    for captured in (False, True):
        eng = new_engine(m)
        dev = [eng.tensor(x) for x in data()]
        eng.dense_train_begin()
        eng.dense_train_reserve(B * P)
        call = eng.prepare_dense_train_step(*dev, w, P, shift, lr=1e-3)
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            fixed = eng.use_stream(side)
            try:
                with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                    call.run()
            finally:
                eng.use_stream(fixed)
            torch.cuda.current_stream().wait_stream(side)
            graph.replay()
            l1 = np_(call.result).copy()
            graph.replay()
        else:
            call.run()
            l1 = np_(call.result).copy()
            call.run()
        l2 = np_(call.result).copy()
        results.append((l1, l2, eng.dense_flatten(eng.dense_train_get())))
        eng.close()
    (a1, a2, pa), (b1, b2, pb) = results
    assert a1[0] != a2[0]                                           # (the second step saw the first one's update)
    assert np.array_equal(bits(a1, np.float64), bits(b1, np.float64)) and np.array_equal(bits(a2, np.float64), bits(b2, np.float64))
    assert np.array_equal(bits(pa), bits(pb))


def test_a_capture_that_would_allocate_is_refused():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = new_engine(model("random"))
    dev = [eng.tensor(x) for x in data()]
    call = eng.prepare_dense_loss_grad(*dev, windows_of(*CASES[4]), CASES[4][1], CASES[4][2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    fixed = eng.use_stream(side)
    try:
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_dense_loss_grad: the stream is being captured.*cpmppi_dense_train_reserve"):
                call.run()
    finally:
        eng.use_stream(fixed)
    eng.close()


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_refusals_by_name_launch_nothing_and_change_nothing():
    from cartpolesimulation_amd import _lib as L
    from cartpolesimulation_amd._lib import CpmppiError
    m = model("random")
    eng = new_engine()
    lib, h = eng.lib, eng._h
    s, tp, te, lab = (eng.tensor(x) for x in data())
    w = windows_of(*CASES[2])
    w_host = np.ascontiguousarray(w, np.uint32)
    w_dev = torch.as_tensor(w_host.astype(np.int32)).to(eng.device)
    loss, grad = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device), torch.full((D.NPAR,), -7.0, device=eng.device)

    def loss_args(**kw):
        a = L.cpmppi_dense_loss_args()
        a.B, a.R, a.T, a.post_wash_out, a.shift_labels = len(w), R, T, CASES[2][1], CASES[2][2]
        a.states, a.target_position, a.target_equilibrium, a.labels = s.data_ptr(), tp.data_ptr(), te.data_ptr(), lab.data_ptr()
        a.windows, a.windows_host, a.loss_out, a.grad_out = w_dev.data_ptr(), w_host.ctypes.data, loss.data_ptr(), grad.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(text, fn, *args):
        assert fn(h, *args) != 0
        err = lib.cpmppi_last_error(h).decode()
        assert re.search(text, err), err

    Q = torch.full((R * T,), -7.0, device=eng.device)

    def control_args(**kw):
        a = L.cpmppi_dense_control_args()
        a.E, a.s, a.target_position, a.target_equilibrium, a.Q_out = R * T, s.data_ptr(), tp.data_ptr(), te.data_ptr(), Q.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    # no model yet
    refused("cpmppi_dense_loss_grad: no model set", lib.cpmppi_dense_loss_grad, C.byref(loss_args()), None)
    refused("cpmppi_dense_control: no model set", lib.cpmppi_dense_control, C.byref(control_args()), None)
    refused("cpmppi_dense_train_begin: no model set", lib.cpmppi_dense_train_begin)
    refused("cpmppi_dense_train_step: call cpmppi_dense_train_begin first", lib.cpmppi_dense_train_step, C.byref(loss_args()), 1e-3, 0.9,
            0.999, 1e-8, None)
    with pytest.raises(ValueError, match="no model set: call set_dense first"):
        eng.dense_control(s[0], tp[0], te[0])
    eng.set_dense(m)
    for text, kw in (("states, target_position, target_equilibrium, labels, windows, windows_host and loss_out are required", dict(states=None)),
                     (".*are required", dict(labels=None)), (".*are required", dict(windows_host=None)),
                     (".*are required", dict(loss_out=None)),
                     ("B, R, T and post_wash_out must be at least 1", dict(B=0)), (".*at least 1", dict(post_wash_out=0)),
                     (".*at least 1", dict(R=0)),
                     (r"window 0 = \(3, 194\) lies outside r < R, t0 \+ post_wash_out - 1 \+ shift_labels <= T - 1", dict(shift_labels=2)),
                     ("window .* lies outside", dict(R=3)),
                     ("misaligned pointer", dict(states=s.data_ptr() + 2)), ("misaligned pointer", dict(loss_out=loss.data_ptr() + 4))):
        refused("cpmppi_dense_loss_grad: " + text, lib.cpmppi_dense_loss_grad, C.byref(loss_args(**kw)), None)
    for text, kw in (("E must be at least 1", dict(E=0)), ("s, target_position, target_equilibrium and Q_out are required", dict(Q_out=None)),
                     ("misaligned pointer", dict(y_out=Q.data_ptr() + 1)), ("misaligned pointer", dict(count_dev=Q.data_ptr() + 4))):
        refused("cpmppi_dense_control: " + text, lib.cpmppi_dense_control, C.byref(control_args(**kw)), None)
    refused("cpmppi_dense_train_reserve: samples must be at least 1", lib.cpmppi_dense_train_reserve, 0)
    refused("cpmppi_dense_train_get: call cpmppi_dense_train_begin first", lib.cpmppi_dense_train_get,
            np.empty(D.NPAR, f32).ctypes.data_as(C.POINTER(C.c_float)))
    torch.cuda.synchronize()
    assert (np_(loss) == -7.0).all() and (np_(grad) == -7.0).all() and (np_(Q) == -7.0).all()      # nothing was launched
    # a refused set_dense (one NaN bias) leaves the control's bits and a live training run as they were
    ctl = lambda: np_(eng.dense_control(s[0], tp[0], te[0])[0]).copy()  # noqa: E731
    eng.dense_train_begin()
    eng.dense_train_step(s, tp, te, lab, w, CASES[2][1], CASES[2][2], lr=1e-3)
    before, params = ctl(), eng.dense_flatten(eng.dense_train_get())
    bad = {k: v.copy() for k, v in m.items()}
    bad["b2"][7] = np.nan
    with pytest.raises(CpmppiError, match=r"cpmppi_set_dense: b2\[7\] is not finite"):
        eng.set_dense(bad)
    with pytest.raises(CpmppiError, match="cpmppi_set_dense: out_scale is 0"):
        eng.set_dense({**m, "out_scale": np.zeros(1, f32)})
    fp = C.POINTER(C.c_float)
    half = L.cpmppi_dense_model()
    half.w1 = m["w1"].ctypes.data_as(fp)
    refused("cpmppi_set_dense: b1 is NULL", lib.cpmppi_set_dense, C.byref(half))
    assert np.array_equal(bits(ctl()), bits(before)) and np.array_equal(bits(eng.dense_flatten(eng.dense_train_get())), bits(params))
    eng.dense_train_step(s, tp, te, lab, w, CASES[2][1], CASES[2][2], lr=1e-3)      # the run is alive
    assert not np.array_equal(bits(eng.dense_flatten(eng.dense_train_get())), bits(params))
    # a successful set_dense ends the run
    eng.set_dense(m)
    with pytest.raises(CpmppiError, match="cpmppi_dense_train_step: call cpmppi_dense_train_begin first"):
        eng.dense_train_step(s, tp, te, lab, w, CASES[2][1], CASES[2][2], lr=1e-3)
    with pytest.raises(CpmppiError, match="cpmppi_dense_train_get: call cpmppi_dense_train_begin first"):
        eng.dense_train_get()
    fresh = new_engine(m)
    assert np.array_equal(bits(ctl()), bits(np_(fresh.dense_control(s[0], tp[0], te[0])[0])))        # the model just set, untouched
    fresh.close()
    eng.close()


# ---------------------------------------------------------------------------------------------- learning
LEARN = dict(epochs=60, batch_size=64, lr=1e-2, seed=3)


@functools.lru_cache(maxsize=None)
def learning_problem():
    """A teacher - a random Dense net at weight scale 0.5 - labels 4 recordings x 200 rows of random states; the student starts from
    another seed.  Epochs and rate were chosen on the CPU so that dense_ref's own float64 training (the batches of
    _training.run_epochs) ends below 1/20 of its first-epoch loss."""
    from cartpolesimulation_amd.train_imitator import initial_weights, normalization_from_recordings
    s, tp, te, _ = data()
    teacher = D.random_model(77, scale=0.5)
    x = D.features(s, tp, te).reshape(-1, 7).astype(f32)
    with torch.no_grad():
        lab = D.forward(D._tensors(teacher, torch.float64), torch.as_tensor(x).double()).numpy().reshape(R, T).astype(f32)
    init = {**initial_weights(LEARN["seed"]), **normalization_from_recordings(s, tp, te, lab)}
    return s, tp, te, lab, init


def reference_training():
    from cartpolesimulation_amd._training import make_windows
    s, tp, te, lab, init = learning_problem()
    windows, rng = make_windows([T] * R, 0, 1, 0), np.random.default_rng(LEARN["seed"])
    epochs, cur, opt = [], dict(init), D.Adam(D.flatten(init), LEARN["lr"], eps=1e-7)
    for _ in range(LEARN["epochs"]):
        order, losses = rng.permutation(len(windows)), []
        for i in range(0, len(order), LEARN["batch_size"]):
            x, y = D.samples(s, tp, te, lab, windows[order[i:i + LEARN["batch_size"]]], 1, 0)
            loss, g = D.loss_and_grad(cur, x, y)
            losses.append(loss)
            cur = {**cur, **D.unflatten(opt.step(g))}
        epochs.append(float(np.mean(losses)))
    return epochs


def test_the_student_learns_the_teacher(capsys):
    from cartpolesimulation_amd.train_imitator import train_imitator
    ref = reference_training()
    assert ref[-1] < ref[0] / 20, f"the reference itself must learn: {ref[-1] / ref[0]:.4f}"
    s, tp, te, lab, init = learning_problem()
    eng = new_engine()
    trained, history = train_imitator(eng, s, tp, te, lab, init=init, reduce_lr_on_plateau=False, **LEARN)
    report(capsys, f"learning: reference {ref[-1] / ref[0]:.4f} of its first epoch, device {history['loss'][-1] / history['loss'][0]:.4f}; "
                   f"first epoch {history['loss'][0]:.4e} (reference {ref[0]:.4e})")
    assert history["loss"][-1] < history["loss"][0] / 10
    assert set(trained) == set(init) and all(np.isfinite(trained[k]).all() for k in trained)
    # the engine holds the trained model, and the run is over
    q = eng.dense_control(eng.tensor(s[0]), eng.tensor(tp[0]), eng.tensor(te[0]))[0]
    fresh = new_engine(trained)
    assert np.array_equal(bits(np_(q)), bits(np_(fresh.dense_control(fresh.tensor(s[0]), fresh.tensor(tp[0]), fresh.tensor(te[0]))[0])))
    fresh.close()
    eng.close()
