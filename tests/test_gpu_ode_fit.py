"""GPU: fitting the ODE predictor's physical parameters - cpmppi_ode_fit_loss_grad (ode_fit_kernel, ode_fit_finalize_kernel),
cpmppi_ode_fit_begin / _set_theta / _step / _get, the Python on top (fit_ode) and its command line.

Reference: tests/ode_fit_ref.py - both integrators in float64 torch with the eight parameters as tensors, autograd for d loss /
d theta and every window's own d term / d p; pinned by tests/test_ode_fit_host.py.

Bounds, the project's own GRAD_TOL from tests/test_gpu_grad.py: EVERY component of d loss / d theta within 5e-4 of ITSELF (J_fric's
gradient is a thousandth of the largest: a wrong term there must not hide under the maximum), the loss within rtol 5e-4.  The
condition under which a component can be held to itself is asserted from the reference alone: no component is a near-cancellation
over the windows, |sum| >= 0.05 sum |term|; the window seeds (SEEDS) are the first for which the float64 reference says so, with a
margin (0.07).  A window's own row (per_window_out) is held to 5e-4 of max(|its own component|, 0.05 x the median window's |component|):
below 5 % of the typical window the component is itself a cancellation over the window's steps, and the float32 error is that of
the terms it is the sum of.

Shapes: TR.random_recordings(3, 40); B in {1, 31, 33, 129, 257} (one lane, a ragged wave, two waves, past one workgroup of 256) x
horizon in {1, 3, 12}; every batch of three or more has a window repeated, two that overlap, and one that ends at the recording's
last legal row.  Both predictors, both math modes, all eight parameters trainable, at set_theta(THETA_PROBE).

Bounce: an ODE_v0 set whose every window bounces (starts 1 - 4 mm inside the edge moving outward); a window is flagged when any
substep's bounce test of the reference lies within 1e-5 of TrackHalfLength, at most 10 % may be, the others are held to the bound.

Measured on the MI355X (this module's first run; worst over the 15 shapes):
  predictor  math     gradient (of the component itself)   loss (relative)   per-window row (of its bound's scale)
  ODE_v0     fast     1.61e-05                             2.9e-07           3.1e-05
  ODE_v0     precise  8.81e-06                             2.9e-07           3.3e-05
  ODE        fast     2.62e-06                             1.8e-07           4.3e-05
  ODE        precise  2.25e-06                             2.9e-07           6.6e-05
Bounce set: 30 windows, 1 flagged, worst unflagged 7.8e-06 (fast), 5.9e-06 (precise).  One Adam step: theta and p equal the closed
form in every bit.
Fit (8 recordings x 120 rows of the oracle at the true parameters, horizon 10, B = 64, lr = 0.02, 150 steps, against float64 Adam):
the reference brings every trained theta within 7.2e-5 of the truth and the loss to 1.3e-7 of its start; over the steps where the
reference's loss is above 1e-3 of step 1's (51 for ODE, 58 for ODE_v0) the worst relative deviation of a step's loss is 2.26e-05 (ODE,
step 49; ODE_v0: 1.89e-05, step 48), asserted at four times that (FIT_LOSS_RTOL) and never beyond 1e-2; the device's theta ends within
7.2e-5 of the truth, and the scaled Brunton rmse at step 10 falls from 1.7e-1 to 6.5e-5."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402
import ode_fit_ref as F  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKOUT = os.path.join(ROOT, "tests", "golden", "reference_checkout")
R, T = 3, 40
BATCHES = (1, 31, 33, 129, 257)
HORIZONS = (1, 3, 12)
H_MAX = 12
GRAD_TOL, LOSS_RTOL = 5e-4, 5e-4
# the first seed per (B, horizon) for which the float64 reference has no near-cancellation (>= 0.07) with either predictor
SEEDS = {(1, 1): 0, (1, 3): 0, (1, 12): 0, (31, 1): 4, (31, 3): 1, (31, 12): 1, (33, 1): 0, (33, 3): 4, (33, 12): 2,
         (129, 1): 1, (129, 3): 0, (129, 12): 7, (257, 1): 2, (257, 3): 0, (257, 12): 7}
ALL = F.NAMES
FIT_LOSS_RTOL = 4 * 2.26e-5     # four times the measured worst deviation of a step's loss (module docstring), never beyond 1e-2
MODES = [("ODE_v0", "fast"), ("ODE_v0", "precise"), ("ODE", "fast"), ("ODE", "precise")]


def report(capsys, text):
    with capsys.disabled():
        print("\n[ode-fit] " + text)


def bits(x, dtype=f32):
    return np.ascontiguousarray(np.asarray(x, dtype)).view(np.uint32 if dtype == f32 else np.uint64)


def np_(t):
    return t.cpu().numpy()


def new_engine(predictor="ODE_v0", math_mode="fast", phys=None, H=H_MAX):
    from cartpolesimulation_amd.configs import MPPIConfig, PhysicalParameters
    from cartpolesimulation_amd.engine import MPPIEngine
    return MPPIEngine(1, MPPIConfig(num_rollouts=32, mpc_horizon=H, math_mode=math_mode, predictor_type=predictor),
                      phys or PhysicalParameters())


@functools.lru_cache(maxsize=None)
def scale_of():
    from cartpolesimulation_amd.train_gru import normalization_from_recordings
    s = normalization_from_recordings(*TR.random_recordings(R, T))["in_scale"][1:]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def windows_of(B, h):
    """B windows of the R x T recordings: drawn from the legal ones, then [1] = [0] (a window twice), [2] = one row on from [0]
    (overlapping), [-1] = the last recording's last legal window."""
    from cartpolesimulation_amd.train_gru import make_windows
    legal = make_windows([T] * R, 0, h, 1)
    w = legal[np.random.Generator(np.random.SFC64([SEEDS[B, h], B, h])).integers(0, len(legal) - 1, B)].copy()
    if B >= 3:
        w[0] = (0, 4)
        w[1] = w[0]
        w[2] = (0, 5)
    w[-1] = legal[-1]
    assert w[-1, 0] == R - 1 and w[-1, 1] + h == T - 1
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(predictor, B, h):
    states, Q = TR.random_recordings(R, T)
    return F.loss_and_grad(F.params_at(F.base_of(), F.THETA_PROBE), states, Q, windows_of(B, h), h, scale_of(), predictor)


def window_bound(ref_rows):
    """[B,8]: 5e-4 of max(|the window's own component|, 0.05 x the median window's |component|) (module docstring)."""
    typical = np.median(np.abs(ref_rows), axis=0, keepdims=True)
    return GRAD_TOL * np.maximum(np.abs(ref_rows), 0.05 * typical)


# ---------------------------------------------------------------------------------------------- 1. gradient against float64 autograd
@pytest.mark.parametrize("predictor,math_mode", MODES)
def test_loss_and_gradient_against_float64_autograd(predictor, math_mode, capsys):
    eng = new_engine(predictor, math_mode)
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    eng.ode_fit_begin()
    eng.ode_fit_set_theta(F.THETA_PROBE)
    p, theta = eng.ode_fit_get()
    assert np.array_equal(bits(theta), bits(F.THETA_PROBE))
    assert np.abs(p.astype(np.float64) / F.params_at(F.base_of(), F.THETA_PROBE) - 1.0).max() <= 4 * np.finfo(f32).eps
    worst_g = worst_l = worst_w = 0.0
    for B in BATCHES:
        for h in HORIZONS:
            ref = reference(predictor, B, h)
            terms = ref["term_grads"]
            assert (np.abs(terms.sum(axis=0)) >= 0.05 * np.abs(terms).sum(axis=0)).all(), (B, h)      # from the reference alone
            rows = torch.full((B, 9), -7.0, dtype=torch.float32, device=eng.device)
            loss, grad = eng.ode_fit_loss_grad(states, Q, windows_of(B, h), h, ALL, scale_of(), per_window_out=rows)
            g, l, rows = np_(grad), float(np_(loss)[0]), np_(rows).astype(np.float64)
            rel_g = np.abs(g - ref["grad_theta"]) / np.abs(ref["grad_theta"])
            rel_l = abs(l - ref["loss"]) / ref["loss"]
            ref_rows = np.concatenate([ref["terms"][:, None], terms], axis=1)
            rel_w = (np.abs(rows - ref_rows) / (window_bound(ref_rows) / GRAD_TOL)).max()
            report(capsys, f"{predictor} {math_mode} B {B} h {h}: gradient {rel_g.max():.3e} ({ALL[rel_g.argmax()]}), loss {rel_l:.3e}, "
                           f"per window {rel_w:.3e}")
            worst_g, worst_l, worst_w = max(worst_g, rel_g.max()), max(worst_l, rel_l), max(worst_w, rel_w)
            assert np.isfinite(g).all() and np.isfinite(rows).all()
            assert (rel_g <= GRAD_TOL).all(), (B, h, rel_g)
            assert rel_l <= LOSS_RTOL, (B, h)
            assert (np.abs(rows - ref_rows) <= window_bound(ref_rows)).all(), (B, h)
            if B >= 3:                                       # the repeated window gives the same row, bit for bit
                assert np.array_equal(bits(rows[0]), bits(rows[1])) and not np.array_equal(bits(rows[0]), bits(rows[2]))
    report(capsys, f"{predictor} {math_mode}: WORST gradient {worst_g:.3e}, loss {worst_l:.3e}, per window {worst_w:.3e}")
    eng.close()


# ---------------------------------------------------------------------------------------------- 2. the edge bounce
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_bounce_takes_the_branch(math_mode, capsys):
    from cartpolesimulation_amd.train_gru import make_windows
    states, Q = F.bounce_recordings()
    Rb, Tb, h = states.shape[0], states.shape[1], 2
    w = make_windows([Tb] * Rb, 0, h, 1)
    p32 = F.params_at(F.base_of(), F.THETA_PROBE)
    ref = F.loss_and_grad(p32, states, Q, w, h, scale_of(), "ODE_v0")
    assert ref["bounced"].all()                              # every window of the set bounces
    flagged = ref["margin"] < 1e-5
    assert flagged.mean() <= 0.10, flagged.mean()
    quiet = F.loss_and_grad(p32, states, Q, w, h, scale_of(), "ODE_v0", THL=1e9)           # the same windows without an edge
    eng = new_engine("ODE_v0", math_mode)
    eng.ode_fit_begin()
    eng.ode_fit_set_theta(F.THETA_PROBE)
    rows = torch.zeros(len(w), 9, dtype=torch.float32, device=eng.device)
    eng.ode_fit_loss_grad(states, Q, w, h, ALL, scale_of(), per_window_out=rows)
    rows = np_(rows).astype(np.float64)
    ref_rows = np.concatenate([ref["terms"][:, None], ref["term_grads"]], axis=1)
    ok = ~flagged
    err = np.abs(rows - ref_rows) / (window_bound(ref_rows) / GRAD_TOL)
    report(capsys, f"bounce {math_mode}: {len(w)} windows, {int(flagged.sum())} flagged, worst unflagged {err[ok].max():.3e}")
    assert (np.abs(rows - ref_rows) <= window_bound(ref_rows))[ok].all()
    # the bounce was taken: the rows are nowhere near those of a track without an edge, L's direct term included
    assert (np.abs(rows[ok, 0] - quiet["terms"][ok]) > 1e-2 * np.abs(ref["terms"][ok])).all()
    i = ALL.index("L")
    assert (np.abs(ref["term_grads"][ok, i] - quiet["term_grads"][ok, i]) > 100 * window_bound(ref_rows)[ok, 1 + i]).mean() > 0.9
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. against the Brunton test
@pytest.mark.parametrize("predictor,math_mode", MODES)
def test_loss_is_the_brunton_tests_squared_error(predictor, math_mode):
    """At the handle's own parameters (no fit begun) loss * B * horizon * 5 = sum_f scale_f^2 sum e_f^2 of cpmppi_brunton over the
    same starts, features 1..5."""
    eng = new_engine(predictor, math_mode)
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    h, start, count = 3, 2, 30
    w = np.array([(r, start + i) for r in range(R) for i in range(count)])
    loss, grad = eng.ode_fit_loss_grad(states, Q, w, h, ALL, scale_of())
    stats, _ = eng.brunton(states, Q, horizon=h, start=start, count=count)
    s2 = np_(stats)[:, 1:, 1].sum(axis=0)                    # sum e^2 per feature over the steps
    want = float((scale_of().astype(np.float64) ** 2 * s2).sum())
    got = float(np_(loss)[0]) * len(w) * h * 5
    assert abs(got - want) <= 5e-4 * want, (got, want)
    assert np.isfinite(np_(grad)).all() and np_(grad).all()
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. bit for bit
def test_two_runs_loss_only_untrained_and_sentinels():
    eng = new_engine("ODE", "fast")
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    eng.ode_fit_begin()
    eng.ode_fit_set_theta(F.THETA_PROBE)
    for B, h, names in ((257, 3, ALL), (33, 12, ("u_max", "J_fric", "L")), (129, 1, ("u_max",))):
        w = windows_of(B, h)
        gbuf = torch.full((8 + 2,), -7.0, dtype=torch.float64, device=eng.device)
        lbuf = torch.full((3,), -7.0, dtype=torch.float64, device=eng.device)
        rbuf = torch.full((B + 1, 9), -7.0, dtype=torch.float32, device=eng.device)

        def run(grad=True):
            return eng.ode_fit_loss_grad(states, Q, w, h, names, scale_of(), grad=grad, loss_out=lbuf[1:2],
                                         grad_out=gbuf[1:9] if grad else None, per_window_out=rbuf[:B])
        run()
        first = [np_(x).copy() for x in (gbuf, lbuf, rbuf)]
        assert first[0][0] == -7.0 and first[0][9] == -7.0 and first[1][0] == -7.0 and first[1][2] == -7.0 and first[1][1] > 0
        assert (first[2][B] == -7.0).all() and (first[2][:B] != -7.0).all()
        trained = np.array([n in names for n in ALL])
        assert (first[0][1:9][trained] != 0).all() and (bits(first[0][1:9][~trained], np.float64) == 0).all()      # exactly +0
        assert (first[2][:B, 1:][:, trained] != 0).all() and (bits(first[2][:B, 1:][:, ~trained]) == 0).all()
        for buf in (gbuf, lbuf, rbuf):
            buf.fill_(-7.0)
        run()
        for a, b, dt in zip((gbuf, lbuf, rbuf), first, (np.float64, np.float64, f32)):
            assert np.array_equal(bits(np_(a), dt), bits(b, dt))
        lbuf.fill_(-7.0)
        gbuf.fill_(-7.0)
        loss, none = run(grad=False)
        assert none is None and np.array_equal(bits(np_(lbuf), np.float64), bits(first[1], np.float64)) and bool((gbuf == -7.0).all())
    # a step with one trainable parameter: the others keep theta and p bit for bit, and theirs is the only change
    p0, t0 = eng.ode_fit_get()
    eng.ode_fit_step(states, Q, windows_of(33, 3), 3, ("M_fric",), scale_of(), lr=0.02)
    p1, t1 = eng.ode_fit_get()
    i = ALL.index("M_fric")
    keep = np.arange(8) != i
    assert np.array_equal(bits(p0[keep]), bits(p1[keep])) and np.array_equal(bits(t0[keep]), bits(t1[keep]))
    assert abs(abs(float(t1[i]) - float(t0[i])) - 0.02) < 1e-4 and p1[i] != p0[i]
    eng.close()


def test_capture_is_refused_cold_and_replays_warm():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = new_engine("ODE_v0", "fast")
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    gbuf = torch.full((8,), -7.0, dtype=torch.float64, device=eng.device)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    call = eng.prepare_ode_fit_loss_grad(states, Q, windows_of(257, 3), 3, ALL, scale_of(), loss_out=lbuf, grad_out=gbuf)
    marker = eng.zeros(4)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g0, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_ode_fit_loss_grad: the stream is being captured"):
                call.run()
            marker.add_(1.0)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    g0.replay()
    torch.cuda.synchronize()
    assert np_(marker).tolist() == [1.0] * 4 and bool((gbuf == -7.0).all()) and bool((lbuf == -7.0).all())
    eng.ode_fit_reserve(257)                                 # the reserving call
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
    assert np.array_equal(bits(np_(gbuf), np.float64), bits(eager_g, np.float64))
    assert np.array_equal(bits(np_(lbuf), np.float64), bits(eager_l, np.float64))
    eng.close()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing():
    from cartpolesimulation_amd.configs import PhysicalParameters
    eng = new_engine("ODE", "fast")
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    h = 3
    gbuf = torch.full((8,), -7.0, dtype=torch.float64, device=eng.device)
    lbuf = torch.full((1,), -7.0, dtype=torch.float64, device=eng.device)
    rbuf = torch.full((33, 9), -7.0, dtype=torch.float32, device=eng.device)
    lrows = eng.tensor(np.full((R, T), 0.4, f32))
    stream = eng._stream()

    def block(names=ALL, L=None):
        return eng._ode_fit_args(states, Q, windows_of(33, h), h, names, scale_of(), L, lbuf, gbuf, True, rbuf)

    def refused(handle, a, code, text, fn=None):
        rc = (fn or eng.lib.cpmppi_ode_fit_loss_grad)(handle, C.byref(a), stream) if fn is None else fn(a)
        assert rc == code, (rc, text, eng.lib.cpmppi_last_error(handle).decode())
        assert text in eng.lib.cpmppi_last_error(handle).decode(), eng.lib.cpmppi_last_error(handle).decode()
        torch.cuda.synchronize()
        assert bool((gbuf == -7.0).all()) and bool((lbuf == -7.0).all()) and bool((rbuf == -7.0).all()), text

    def both(change, code, text):
        """cpmppi_ode_fit_loss_grad and, in its own name, cpmppi_ode_fit_step (a fit is begun below)."""
        a, keep = block()[:2]
        change(a, keep)
        refused(eng._h, a, code, "cpmppi_ode_fit_loss_grad: " + text)
        if begun:
            refused(eng._h, a, code, "cpmppi_ode_fit_step: " + text,
                    fn=lambda a: eng.lib.cpmppi_ode_fit_step(eng._h, C.byref(a), 0.02, 0.9, 0.999, 1e-8, stream))

    # before a fit: step, get and set_theta
    begun = False
    a, keep = block()[:2]                                    # (`keep` holds the window arrays the block points into)
    assert eng.lib.cpmppi_ode_fit_step(eng._h, C.byref(a), 0.02, 0.9, 0.999, 1e-8, stream) == -1
    assert "cpmppi_ode_fit_step: call cpmppi_ode_fit_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    eight = (C.c_float * 8)()
    assert eng.lib.cpmppi_ode_fit_get(eng._h, eight, eight) == -1
    assert "cpmppi_ode_fit_get: call cpmppi_ode_fit_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    assert eng.lib.cpmppi_ode_fit_set_theta(eng._h, eight) == -1
    assert "cpmppi_ode_fit_set_theta: call cpmppi_ode_fit_begin first" in eng.lib.cpmppi_last_error(eng._h).decode()
    assert eng.lib.cpmppi_ode_fit_reserve(eng._h, 0) == -1
    assert eng.lib.cpmppi_ode_fit_loss_grad(eng._h, None, stream) == -1
    for begun in (False, True):
        if begun:
            eng.ode_fit_begin()
            eng.ode_fit_set_theta(F.THETA_PROBE)
            state0 = [x.copy() for x in eng.ode_fit_get()]
        for field in ("states", "Q", "windows", "windows_host", "loss_out"):
            both(lambda a, k: setattr(a, field, None), -1, "states, Q, windows, windows_host and loss_out are required")
        for field in ("B", "R", "T", "horizon"):
            both(lambda a, k: setattr(a, field, 0), -1, "B, R, T and horizon must be at least 1")
        both(lambda a, k: setattr(a, "horizon", H_MAX + 1), -1, "horizon 13 is longer than the handle's (12)")
        for r, t0 in ((R, 0), (0, T - h), (0, 2 ** 32 - 1)):
            both(lambda a, k: k[4].__setitem__(5, (r, t0)), -1, "window 5 = (%d, %d) lies outside" % (r, t0))   # the HOST copy is checked
        for mask in (0, 256, 2 ** 31):
            both(lambda a, k: setattr(a, "trainable", mask), -1, "trainable = %d" % mask)
        both(lambda a, k: setattr(a, "L", lrows.data_ptr()), -1, "L is trainable and L rows are given")
        for field in ("states", "Q", "windows", "per_window_out"):
            both(lambda a, k: setattr(a, field, getattr(a, field) + 2), -5, "misaligned pointer")
        for field in ("loss_out", "grad_out"):
            both(lambda a, k: setattr(a, field, getattr(a, field) + 4), -5, "misaligned pointer")
        rows = eng.tensor(np.full(64, 0.087, f32))
        eng._check(eng.lib.cpmppi_set_pole_mass_rows(eng._h, C.c_void_p(rows.data_ptr()), 64))
        both(lambda a, k: None, -1, "per-row pole masses are registered")
        eng._check(eng.lib.cpmppi_set_pole_mass_rows(eng._h, None, 0))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(state0, eng.ode_fit_get()))     # nothing moved theta or p
    # L rows without a trainable L, and the last legal row, are accepted
    a, keep = block(tuple(n for n in ALL if n != "L"), lrows)[:2]
    keep[4][5] = (0, T - 1 - h)
    assert eng.lib.cpmppi_ode_fit_loss_grad(eng._h, C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert bool((gbuf != -7.0).all()) and float(gbuf[ALL.index("L")]) == 0.0
    eng.close()
    # a trainable parameter whose base is not positive
    zero = new_engine("ODE", "fast", PhysicalParameters(J_fric=0.0))
    a, keep = zero._ode_fit_args(states, Q, windows_of(33, h), h, ("J_fric",), scale_of(), None, lbuf, gbuf, True, rbuf)[:2]
    gbuf.fill_(-7.0)
    lbuf.fill_(-7.0)
    rbuf.fill_(-7.0)
    assert zero.lib.cpmppi_ode_fit_loss_grad(zero._h, C.byref(a), stream) == -1
    assert "cpmppi_ode_fit_loss_grad: trainable parameter J_fric has the base value 0" in zero.lib.cpmppi_last_error(zero._h).decode()
    torch.cuda.synchronize()
    assert bool((gbuf == -7.0).all()) and bool((lbuf == -7.0).all()) and bool((rbuf == -7.0).all())
    a.trainable = 1 << ALL.index("u_max")                   # ... is fine to hold fixed
    assert zero.lib.cpmppi_ode_fit_loss_grad(zero._h, C.byref(a), stream) == 0
    torch.cuda.synchronize()
    zero.close()


# ---------------------------------------------------------------------------------------------- 6. Adam
def test_one_adam_step_is_the_closed_form(capsys):
    eng = new_engine("ODE_v0", "fast")
    states, Q = (eng.tensor(x) for x in TR.random_recordings(R, T))
    w, h = windows_of(129, 3), 3
    lr, b1, b2, eps = f32(0.02), f32(0.9), f32(0.999), f32(1e-7)
    B1, B2 = float(b1), float(b2)
    base = F.base_of().astype(np.float64)
    eng.ode_fit_begin()
    eng.ode_fit_set_theta(F.THETA_PROBE)
    loss0, grad = eng.ode_fit_loss_grad(states, Q, w, h, ALL, scale_of())
    g, t0 = np_(grad).copy(), eng.ode_fit_get()[1].astype(np.float64)
    loss = eng.ode_fit_step(states, Q, w, h, ALL, scale_of(), lr=lr, beta1=b1, beta2=b2, eps=eps)
    assert np.array_equal(bits(np_(loss), np.float64), bits(np_(loss0), np.float64))       # the loss BEFORE the update
    p1, t1 = eng.ode_fit_get()
    mom1, mom2 = (1.0 - B1) * g, (1.0 - B2) * g * g
    closed = (t0 - float(lr) * (mom1 / (1.0 - B1)) / (np.sqrt(mom2 / (1.0 - B2)) + float(eps))).astype(f32)
    tol = 4 * np.finfo(f32).eps * float(lr)
    dev = np.abs(t1.astype(np.float64) - closed.astype(np.float64)).max()
    p_closed = (base * np.exp(t1.astype(np.float64))).astype(f32)
    dev_p = np.abs(p1.astype(np.float64) / p_closed.astype(np.float64) - 1.0).max()
    report(capsys, f"one Adam step: |theta - closed form| {dev:.3e} (4 eps lr = {tol:.3e}); p against float32(base exp(theta)): {dev_p:.3e}")
    assert dev <= tol
    assert dev_p <= 4 * np.finfo(f32).eps
    assert np.abs(np.abs(t1.astype(np.float64) - t0) - float(lr)).max() < 1e-4     # Adam's first step is lr in every component
    # a second step: bias correction with t = 2, the moments carried as float32
    g2 = np_(eng.ode_fit_loss_grad(states, Q, w, h, ALL, scale_of())[1]).copy()
    eng.ode_fit_step(states, Q, w, h, ALL, scale_of(), lr=lr, beta1=b1, beta2=b2, eps=eps)
    p2, t2 = eng.ode_fit_get()
    m1, m2 = mom1.astype(f32).astype(np.float64), mom2.astype(f32).astype(np.float64)
    m1, m2 = B1 * m1 + (1.0 - B1) * g2, B2 * m2 + (1.0 - B2) * g2 * g2
    closed2 = (t1.astype(np.float64) - float(lr) * (m1 / (1.0 - B1 ** 2)) / (np.sqrt(m2 / (1.0 - B2 ** 2)) + float(eps))).astype(f32)
    assert np.abs(t2.astype(np.float64) - closed2.astype(np.float64)).max() <= tol
    assert np.abs(p2.astype(np.float64) / (base * np.exp(t2.astype(np.float64))).astype(f32) - 1.0).max() <= 4 * np.finfo(f32).eps
    # begin again: theta, the moments and the counter are zero - the first step is the closed form with t = 1 once more
    eng.ode_fit_begin()
    p, t = eng.ode_fit_get()
    assert not t.any() and np.array_equal(bits(p), bits(F.base_of()))
    eng.close()


# ---------------------------------------------------------------------------------------------- 7. a fit that works
@pytest.mark.parametrize("predictor", ["ODE", "ODE_v0"])
def test_fit_recovers_the_true_parameters(predictor, capsys):
    import dataclasses
    from cartpolesimulation_amd.brunton import brunton_test
    from cartpolesimulation_amd.configs import PhysicalParameters
    from cartpolesimulation_amd.fit_ode import fitted_parameters
    fit = F.reference_fit(predictor)
    idx = [ALL.index(n) for n in fit["trainable"]]
    # the reference itself does it
    assert np.abs(fit["theta"] - fit["theta_true"])[idx].max() < 1e-3 and fit["losses"][-1] < 1e-5 * fit["losses"][0]
    start = fitted_parameters(PhysicalParameters(), fit["start"])
    eng = new_engine(predictor, "fast", start, H=10)
    states, Q = eng.tensor(fit["states"]), eng.tensor(fit["Q"])
    eng.ode_fit_begin()
    losses = torch.empty(len(fit["batches"]), dtype=torch.float64, device=eng.device)
    for i, w in enumerate(fit["batches"]):
        eng.ode_fit_step(states, Q, w, 10, fit["trainable"], fit["scale"], lr=0.02, loss_out=losses[i:i + 1])
    losses = np_(losses)
    p, theta = eng.ode_fit_get()
    eng.close()
    live = fit["losses"] > 1e-3 * fit["losses"][0]           # below that float32 data noise governs
    dev = np.abs(losses - fit["losses"])[live] / fit["losses"][live]
    report(capsys, f"fit {predictor}: {int(live.sum())} steps compared, worst loss deviation {dev.max():.3e} (step {int(dev.argmax()) + 1}); "
                   f"theta error {np.abs(theta - fit['theta_true'])[idx].max():.3e}; final loss ratio {losses[-1] / losses[0]:.3e}")
    assert FIT_LOSS_RTOL <= 1e-2 and dev.max() <= FIT_LOSS_RTOL
    rel = np.abs(p.astype(np.float64) / fit["truth"].astype(np.float64) - 1.0)
    assert rel[idx].max() <= 1e-2, rel
    untrained = [i for i in range(8) if i not in idx]
    assert np.array_equal(bits(p[untrained]), bits(fit["start"][untrained])) and not theta[untrained].any()
    # the Brunton test agrees: the fitted parameters predict the recordings better than the start
    fitted = fitted_parameters(start, p)
    rmse = [brunton_test((fit["states"], fit["Q"]), (predictor,), horizon=10, phys=ph)[predictor]["rmse"][-1, 1:] for ph in (start, fitted)]
    scaled = [float(np.sqrt(((r * fit["scale"]) ** 2).sum())) for r in rmse]
    report(capsys, f"fit {predictor}: scaled Brunton rmse at step 10: start {scaled[0]:.3e}, fitted {scaled[1]:.3e}")
    assert scaled[1] < scaled[0]
    assert dataclasses.asdict(fitted)["TrackHalfLength"] == PhysicalParameters().TrackHalfLength


# ---------------------------------------------------------------------------------------------- 8. fit_ode and the command line
def write_csv(path, states, Q, dt=0.02):
    names = ("time", "angle", "angleD", "angle_cos", "angle_sin", "position", "positionD", "Q")
    with open(path, "w") as fh:
        fh.write("# a recording of the oracle\n" + ",".join(names) + "\n")
        for t in range(len(Q)):
            fh.write(",".join([repr(t * dt)] + [repr(float(x)) for x in states[t]] + [repr(float(Q[t]))]) + "\n")


def test_command_line_writes_parameters(tmp_path, capsys):
    from cartpolesimulation_amd import fit_ode
    from cartpolesimulation_amd.brunton import brunton_test
    from cartpolesimulation_amd.configs import load_reference_yaml
    states, Q = F.oracle_recordings("ODE")
    folder = tmp_path / "Recordings"
    folder.mkdir()
    for r in range(3):
        write_csv(folder / f"rec{r}.csv", states[r], Q[r])
    out = tmp_path / "fitted" / "params.yaml"
    argv = ["--recordings", str(folder), "--out", str(out), "--config-root", CHECKOUT, "--net", "Custom-ODE_module-ODEModel",
            "--predictor", "ODE", "--trainable", "u_max,M_fric", "--horizon", "5", "--epochs", "2", "--lr", "0.02",
            "--validation", str(folder)]
    fitted, history = fit_ode.main(argv)
    text = capsys.readouterr().out
    assert "Brunton rmse at step 5" in text and "before:" in text and "after:" in text and "u_max:" in text
    assert len(history["loss"]) == len(history["val_loss"]) == 2 and len(history["batch_loss"]) == 2 * -(-3 * 115 // 64)
    base = load_reference_yaml(CHECKOUT)[0]
    back = fit_ode.read_parameters(out, base)
    assert back == fitted and back.u_max != base.u_max and back.M_fric != base.M_fric and back.g == base.g and back.L == base.L
    res = brunton_test((states[:3], Q[:3]), ("ODE",), horizon=5, phys=back)["ODE"]
    assert np.isfinite(res["rmse"]).all()
    with pytest.raises(SystemExit, match="fit_ode: net 'GRU-32H1-32H2'"):
        fit_ode.main(argv[:6] + ["--net", "GRU-32H1-32H2"])
    with pytest.raises(SystemExit, match="TrackHalfLength is not offered"):
        fit_ode.main(argv[:6] + ["--trainable", "TrackHalfLength"])
