"""GPU: the seam kernels of cpmppi_seams.hip (the public C ABI of the reference's plugin seams) beyond one wave, one pass and one launch
path - the soft-min update, the cost on materialised trajectories with several rows per wave, the sampler / interpolation / tiling
kernels over several 64-step passes, ragged quads and fewer envs than the handle's, and the sampler's knot limit at its boundary.

Inputs, references and bounds: seam_cases.py (judged on the host by test_seams_host.py).  Every reference is the oracle or float64
numpy of the formula on the same float32 inputs; one launch path is compared with another only bit for bit, and then one side is
also compared with the oracle.  Each test prints `seam-headroom <group> <largest error / bound>` before it asserts (pytest -s)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import seam_cases as SC  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

f32 = np.float32
MATH_MODES = ["precise", "fast"]
BAD_ARG = -1                                                   # CPMPPI_ERR_BAD_ARG
SENTINEL = -777.25


def engine(E, N, H, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig, legacy_mppi_config
    if kw.get("cost_function_specification") == "legacy_mppi_cartpole":
        return MPPIEngine(E, legacy_mppi_config(num_rollouts=N, mpc_horizon=H, **kw))
    return MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, **kw))


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t, f32)
    return np.ascontiguousarray(a).view(np.uint32)


def sentinel_filled(eng, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=eng.device)


def headroom(group, err, bound):
    """Largest error as a fraction of its bound (elements whose bound and error are both zero count as 0)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    frac = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    worst = float(frac.max()) if frac.size else 0.0
    print(f"seam-headroom {group} {worst:.4g}")
    return worst


# ---- 1: the soft-min update seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LBD", SC.RWA_LBDS)
@pytest.mark.parametrize("shape", SC.RWA_SHAPES, ids=str)
def test_reward_weighted_average_beyond_one_wave_and_pass(shape, LBD):
    """cpmppi_reward_weighted_average at the smallest shapes that reach each loop of rwa_kernel (seam_cases.RWA_SHAPES), per-env
    inputs, four cost regimes, against w = exp(-(S - min S) / LBD), (w @ du) / sum w in float64 within (N/4 + 16) 2^-23 max_n |du| per
    column.  Measured on MI355X: at most 0.023 of the bound (profiles/HISTORY.md r11)."""
    E, N, H = shape
    eng = engine(E, N, H, LBD=LBD)
    for regime in SC.RWA_REGIMES:
        S, du = SC.rwa_inputs(shape, LBD, regime)
        out = eng.reward_weighted_average(S, du).cpu().numpy()
        assert out.shape == (E, H)
        ref, bound = SC.rwa_reference(S, du, LBD), SC.rwa_bound(du)
        err = np.abs(out.astype(np.float64) - ref)
        headroom(f"softmin {shape} LBD={LBD:g} {regime}", np.where(np.isfinite(err), err, np.inf), bound)
        assert np.isfinite(out).all(), regime
        assert (err <= bound).all(), (regime, float((err / bound).max()))
        if regime == "dominant":                               # every other weight is exactly 0, this one exactly 1
            assert np.array_equal(out, du[:, N - 1]), regime
    eng.close()


# ---- 2: the cost seam ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=2)
def cost_case_inputs(B, H):
    """Built once per shape, shared by the cases of that shape (which run one after the other), left unchanged."""
    return SC.cost_inputs(B, H)


def _cost_calls(eng, name, c):
    """-> (all three outputs of the one large launch, of launches of at most 8192 rows, the large launch's call arguments)."""
    _, te, with_prev, _, _ = SC.COST_CASES[name]
    B, H = c["inputs"].shape
    traj, inputs = eng.tensor(c["traj"]), eng.tensor(c["inputs"])
    kw = {}
    if name == "legacy":
        kw = dict(u_nom=eng.tensor(c["u_nom"]), u_prev=eng.tensor(c["u_prev"]))
    elif with_prev:
        kw = dict(u_prev=eng.tensor(np.full(H, SC.PREVIOUS_INPUT, f32)))
    big = eng.trajectory_cost(traj, inputs, float(SC.X_T), te, **kw)
    parts = [eng.trajectory_cost(traj[i:i + SC.COST_SMALL_LAUNCH], inputs[i:i + SC.COST_SMALL_LAUNCH], float(SC.X_T), te, **kw)
             for i in range(0, B, SC.COST_SMALL_LAUNCH)]
    small = [torch.cat([p[j] for p in parts]) for j in range(3)]
    return big, small, (traj, inputs, float(SC.X_T), te, kw)


def _assert_cost_seam(name, B, H):
    options, _, _, rtol, atol = SC.COST_CASES[name]
    c = cost_case_inputs(B, H)
    eng = engine(1, 64, H, **options)
    big, small, (traj, inputs, x_t, te, kw) = _cost_calls(eng, name, c)
    # 1: rows per wave > 1 (a row loop, a ragged last wave) computes, bit for bit, what one row per wave computes
    for a, b, what in zip(big, small, ("stage", "terminal", "total")):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (name, what)
    # 3: one output pointer alone: the other two are not there to be written, the one given is the all-three call's
    for j, what in enumerate(("stage", "terminal", "total")):
        one = eng.trajectory_cost(traj, inputs, x_t, te, want=(what,), **kw)
        assert [o is None for o in one] == [i != j for i in range(3)], what
        assert np.array_equal(bits(one[j]), bits(big[j])), (name, what)
    # 2: the oracle
    stage, term, total = (t.cpu().numpy() for t in big)
    stage_ref, term_ref, total_ref = SC.cost_oracle(name, c)
    allow = atol + SC.cos_slack(name, c) + rtol * np.abs(stage_ref.astype(np.float64))
    err = np.abs(stage.astype(np.float64) - stage_ref)
    headroom(f"cost {name} B={B} H={H} stage", err, allow)
    total_err = np.abs(total.astype(np.float64) - total_ref)
    headroom(f"cost {name} B={B} H={H} total", total_err, rtol * np.abs(total_ref.astype(np.float64)))
    assert np.isfinite(stage).all() and (err <= allow).all(), (name, float((err / allow).max()))
    assert np.array_equal(term, term_ref), name
    np.testing.assert_allclose(total, total_ref, rtol=rtol, atol=0)
    if name in SC.LIVE_INDICATOR:                              # rows whose total the 6e9 / 1.2e8 terms do not swamp, on their own
        clear = SC.cost_clear_rows(name, c)
        assert clear.mean() >= 0.25
        big_term = 1e8 / ((H + 1) if options.get("horizon_reduce") == "mean" else 1)
        assert total_ref[clear].max() < big_term < total_ref[~clear].min()
        headroom(f"cost {name} B={B} H={H} total of the rows without a live indicator", total_err[clear],
                 rtol * np.abs(total_ref[clear].astype(np.float64)))
        np.testing.assert_allclose(total[clear], total_ref[clear], rtol=rtol, atol=0)
    eng.close()


@pytest.mark.parametrize("name", list(SC.COST_CASES))
@pytest.mark.parametrize("B,H", SC.COST_SHAPES)
def test_trajectory_cost_with_several_rows_per_wave(B, H, name):
    """cpmppi_trajectory_cost above 8192 rows (rows_per_wave 2 and 3, the last wave holding one row; H = 70: a second lane pass with
    6 live lanes, the legacy cost's u_nom[k] / u_prev[k] beyond k = 64): stage, terminal and total equal, bit for bit, the launches of
    at most 8192 rows over the same rows, and meet the oracle - stages element by element (rtol 1e-4 + the atol the existing seam tests
    hold for the cost), terminals exactly, totals at rtol 1e-4, no row excluded (the inputs keep every indicator argument clear of
    its threshold: test_seams_host.py).  Measured on MI355X: a stage at most 0.34 of its allowance (quadratic_boundary_grad, target
    equilibrium -1), a total 0.005 of its (profiles/HISTORY.md r11)."""
    _assert_cost_seam(name, B, H)


def test_trajectory_cost_rows_per_wave_clamp():
    """B = 524289: ceil((B + 8191) / 8192) = 65 rows per wave, clamped to 64; the last wave holds one row."""
    _assert_cost_seam("qbgm", *SC.COST_CLAMP_SHAPE)


# ---- 4: sampler, interpolation, tiling ----------------------------------------------------------------------------------------------
def _assert_sampler_rule(math_mode, du, kn, H, period, group):
    """The sampler's own delta_u against the oracle's interpolation of the sampler's own knots: PRECISE bit for bit, FAST within the
    derived float32-slope bound per element."""
    ref = SC.oracle_interpolation(kn, H, period)
    if math_mode == "precise":
        assert np.array_equal(bits(du), bits(ref)), group
    else:
        err = np.abs(du.astype(np.float64) - ref)
        bound = SC.fast_interpolation_bound(kn, H, period)
        headroom(f"fast-interpolation {group}", err, bound)
        assert (err <= bound).all(), (group, float((err / np.maximum(bound, 1e-300)).max()))
        assert err.max() > 0 or period == 1 or du.size < 64    # (FAST does take its own path; on a knot both return the knot)


@pytest.mark.parametrize("math_mode", MATH_MODES)
@pytest.mark.parametrize("shape", SC.SAMPLER_SHAPES, ids=str)
def test_sampler_interpolation_and_tiling_shapes(shape, math_mode):
    """sample_kernel, sample_tiled_kernel and tile_kernel at one row, at less than one wave, over three 64-step passes with a ragged
    last quad, a partial knot quad and a half-empty block, and with 67.6 KB of dynamic LDS: caller knots bit for bit against the
    oracle, the sampler's own delta_u by the PRECISE / FAST rule, and the WHOLE tiled buffers - padding included - against the
    index formula of include/cpmppi.h written out in numpy.  Measured on MI355X: FAST at most 0.88 of its bound."""
    E, N, H, period = shape
    eng = engine(E, N, H, period_interpolation_inducing_points=period, math_mode=math_mode)
    assert eng.P == O.knot_count(H, period)
    kn = SC.caller_knots(shape, eng.mppi.sigma)
    du_ref = SC.oracle_interpolation(kn, H, period)
    assert np.array_equal(bits(eng.interpolate(kn)), bits(du_ref))
    kn_s, du_s = eng.sample(seed=4321, offset=7, env_offset=2, knots=True, delta_u=True)
    kn_s, du_s = kn_s.cpu().numpy(), du_s.cpu().numpy()
    assert np.isfinite(kn_s).all() and (E * N * eng.P < 8 or 0.5 < kn_s.std() / eng.mppi.sigma < 1.5)
    _assert_sampler_rule(math_mode, du_s, kn_s, H, period, f"{shape} {math_mode}")
    # the tiled buffers, whole: from the same Philox draws, from caller knots, from a delta_u buffer
    n_tiled = int(eng.lib.cpmppi_tiled_floats(eng._h, E))
    assert n_tiled == E * ((N + 63) // 64) * ((H + 3) // 4) * 256
    assert eng.tiled_empty().numel() == n_tiled
    # (into sentinel-filled buffers: an element a kernel leaves unwritten must not inherit the right value from a freed buffer)
    tiled = eng.sample_tiled(seed=4321, offset=7, env_offset=2, out=sentinel_filled(eng, n_tiled))
    assert np.array_equal(bits(tiled), bits(SC.tiled_reference(du_s)))
    assert np.array_equal(bits(eng.sample_tiled(knots=kn, out=sentinel_filled(eng, n_tiled))), bits(SC.tiled_reference(du_ref)))
    assert np.array_equal(bits(eng.tile_delta_u(du_ref, out=sentinel_filled(eng, n_tiled))), bits(SC.tiled_reference(du_ref)))
    eng.close()


def _raw(eng, fn, *args):
    return getattr(eng.lib, fn)(eng._h, *args, eng._stream())


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("math_mode", MATH_MODES)
def test_sampler_entry_points_with_fewer_envs_than_the_handle(math_mode):
    """E = 2 on a 3-env handle, every sampler entry point: the third env's part of a sentinel-filled output stays untouched, the first
    two envs are the E = 3 call's, and env_offset = 1 reproduces envs 1 and 2 of it.  The E = 3 results are pinned to the oracle."""
    shape = E, N, H, period = SC.SAMPLER_SHAPES[2]
    eng = engine(E, N, H, period_interpolation_inducing_points=period, math_mode=math_mode)
    P = eng.P
    kn = SC.caller_knots(shape, eng.mppi.sigma)
    du_ref = SC.oracle_interpolation(kn, H, period)
    kn3, du3 = (t.cpu().numpy() for t in eng.sample(seed=99, offset=3, env_offset=0, knots=True, delta_u=True))
    _assert_sampler_rule(math_mode, du3, kn3, H, period, f"{shape} {math_mode} E=3")
    tiled3 = SC.tiled_reference(du3)
    assert np.array_equal(bits(eng.sample_tiled(seed=99, offset=3, env_offset=0, out=sentinel_filled(eng, tiled3.size))), bits(tiled3))
    per_env = tiled3.size // E

    def filled(*shape_):
        return sentinel_filled(eng, *shape_)

    def untouched(t):
        return bool((t == SENTINEL).all())

    # cpmppi_sample / cpmppi_interpolate through the C entry points, into buffers of the test's own
    for env_offset, envs in ((0, slice(0, 2)), (1, slice(1, 3))):
        kn_buf, du_buf = filled(E, N, P), filled(E, N, H)
        assert _raw(eng, "cpmppi_sample", 2, 99, 3, env_offset, _ptr(kn_buf), _ptr(du_buf)) == 0
        assert untouched(kn_buf[2]) and untouched(du_buf[2])
        assert np.array_equal(bits(kn_buf[:2]), bits(kn3[envs])) and np.array_equal(bits(du_buf[:2]), bits(du3[envs]))
        out = filled(tiled3.size)
        eng.sample_tiled(seed=99, offset=3, env_offset=env_offset, E=2, out=out)
        assert untouched(out[2 * per_env:])
        assert np.array_equal(bits(out[:2 * per_env]), bits(SC.tiled_reference(du3[envs])))
    du_buf = filled(E, N, H)
    assert _raw(eng, "cpmppi_interpolate", 2, _ptr(eng.tensor(kn)), _ptr(du_buf)) == 0
    assert untouched(du_buf[2]) and np.array_equal(bits(du_buf[:2]), bits(du_ref[:2]))
    out = filled(tiled3.size)
    eng.sample_tiled(knots=kn[:2], out=out)
    assert untouched(out[2 * per_env:]) and np.array_equal(bits(out[:2 * per_env]), bits(SC.tiled_reference(du_ref[:2])))
    out = filled(tiled3.size)
    eng.tile_delta_u(du_ref[:2], out=out)
    assert untouched(out[2 * per_env:]) and np.array_equal(bits(out[:2 * per_env]), bits(SC.tiled_reference(du_ref[:2])))
    eng.close()


# ---- 5: the knot limit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", MATH_MODES)
def test_sampler_knot_limit_boundary(math_mode):
    """The sampler stages [256][P + 1] knots in LDS and admits 159 KB: P = 158 (H = 157, one knot per step) is the largest knot count
    that runs - and meets the oracle's interpolation -, P = 159 is refused by all three sampler entry points with CPMPPI_ERR_BAD_ARG
    before anything is launched, and the message names the limit the check enforces."""
    shape = E, N, H, period = SC.KNOT_LIMIT_SHAPE
    eng = engine(E, N, H, period_interpolation_inducing_points=period, math_mode=math_mode)
    assert eng.P == SC.KNOT_LIMIT
    kn_s, du_s = (t.cpu().numpy() for t in eng.sample(seed=5, offset=1, knots=True, delta_u=True))
    _assert_sampler_rule(math_mode, du_s, kn_s, H, period, f"{shape} {math_mode} at the knot limit")
    n_tiled = eng.tiled_empty().numel()
    assert np.array_equal(bits(eng.sample_tiled(seed=5, offset=1, out=sentinel_filled(eng, n_tiled))), bits(SC.tiled_reference(du_s)))
    kn = SC.caller_knots(shape, eng.mppi.sigma)
    du_ref = SC.oracle_interpolation(kn, H, period)
    assert np.array_equal(bits(eng.interpolate(kn)), bits(du_ref))
    assert np.array_equal(bits(eng.sample_tiled(knots=kn, out=sentinel_filled(eng, n_tiled))), bits(SC.tiled_reference(du_ref)))
    torch.cuda.synchronize()
    eng.close()
    # one knot more
    H1 = H + 1
    over = engine(E, N, H1, period_interpolation_inducing_points=period, math_mode=math_mode)
    assert over.P == SC.KNOT_LIMIT + 1
    kn_buf, du_buf = sentinel_filled(over, E, N, over.P), sentinel_filled(over, E, N, H1)
    tiled = sentinel_filled(over, int(over.lib.cpmppi_tiled_floats(over._h, E)))
    calls = (("cpmppi_sample", (E, 5, 1, 0, _ptr(kn_buf), _ptr(du_buf))),
             ("cpmppi_interpolate", (E, _ptr(kn_buf), _ptr(du_buf))),
             ("cpmppi_sample_tiled", (E, 5, 1, 0, None, _ptr(tiled))),
             ("cpmppi_sample_tiled", (E, 0, 0, 0, _ptr(kn_buf), _ptr(tiled))))
    for fn, args in calls:
        assert _raw(over, fn, *args) == BAD_ARG, fn
        msg = over.lib.cpmppi_last_error(over._h).decode()
        assert fn in msg and f"more than {SC.KNOT_LIMIT} knots per rollout" in msg, msg
    torch.cuda.synchronize()
    for buf in (kn_buf, du_buf, tiled):
        assert bool((buf == SENTINEL).all())
    over.close()
