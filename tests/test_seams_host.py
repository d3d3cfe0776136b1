"""CPU: the inputs and bounds of the seam-kernel tests (seam_cases.py; the GPU side is test_gpu_seams.py) judged on their own - a
bound that a correct float32 evaluation misses, or that a dropped row stays inside, pins nothing; a cost input grazing an indicator
threshold compares roundings, not kernels."""
import numpy as np
import pytest

import seam_cases as SC
from oracle import oracle_np as O

f32 = np.float32


@pytest.mark.parametrize("shape", SC.RWA_SHAPES, ids=str)
@pytest.mark.parametrize("LBD", SC.RWA_LBDS)
def test_softmin_bound_admits_float32_and_catches_a_dropped_row(shape, LBD):
    E, N, H = shape
    for regime in SC.RWA_REGIMES:
        S, du = SC.rwa_inputs(shape, LBD, regime)
        assert S.shape == (E, N) and du.shape == (E, N, H) and S.dtype == du.dtype == f32
        if E > 1:                                               # the envs differ: a wrong env base pointer shows
            assert not np.array_equal(du[0], du[1])
            assert not np.array_equal(S[0], S[1]) or (regime == "dominant" and N == 1)      # (there S is the one row's 5)
        ref, bound = SC.rwa_reference(S, du, LBD), SC.rwa_bound(du)
        assert np.isfinite(ref).all() and bound.shape == ref.shape == (E, H)
        # a float32 evaluation in another summation order stays within the bound
        err = np.abs(SC.rwa_float32_other_order(S, du, LBD).astype(np.float64) - ref)
        assert (err <= bound).all(), (regime, float((err / bound).max()))
        if regime == "offset":                                  # without the subtraction of the minimum: every weight underflows
            with np.errstate(under="ignore"):
                assert not np.exp((f32(-1.0) / f32(LBD)) * S).astype(f32).any()
        if regime == "dominant":                                # every weight but row N-1's is exactly zero, in float64 too
            assert np.array_equal(ref, du[:, N - 1].astype(np.float64))
        if regime == "spread_dupmin":
            assert (S[:, 0] == S.min(axis=1)).all() and (S[:, N - 1] == S.min(axis=1)).all()
        # removing ANY single row (spread regime) lands beyond ten times the bound in at least one column
        if regime == "spread" and N > 1:
            for n in range(N):
                keep = np.arange(N) != n
                dropped = SC.rwa_reference(S[:, keep], du[:, keep], LBD)
                beyond = (np.abs(dropped - ref) > 10.0 * bound).any(axis=1)
                assert beyond.all(), (n, float((np.abs(dropped - ref) / bound).max()))


@pytest.mark.parametrize("B,H", SC.COST_SHAPES + [SC.COST_CLAMP_SHAPE])
def test_cost_inputs_keep_clear_of_every_indicator_threshold(B, H):
    c = SC.cost_inputs(B, H)
    assert c["traj"].shape == (B, H + 1, 6) and c["inputs"].shape == (B, H) and c["traj"].dtype == c["inputs"].dtype == f32
    m = SC.cost_margins(c)
    assert m["stage_x"] >= SC.X_MARGIN and m["terminal_x"] >= SC.X_MARGIN, m
    assert m["stage_angle"] >= SC.ANGLE_MARGIN and m["terminal_angle"] >= SC.ANGLE_MARGIN and m["legacy_u"] >= SC.U_MARGIN, m
    # ... and still reach what they are meant to: angles over the whole circle, positions beyond every track-edge term, both values of
    # the terminal indicator, the legacy input penalty on and off
    traj = c["traj"]
    assert np.abs(traj[..., O.ANGLE_IDX]).max() > 3.1 and np.abs(traj[:, :H, O.POSITION_IDX]).max() > 1.05 * SC.THL
    for thr in SC.STAGE_X_THRESHOLDS:
        over = np.abs(traj[:, :H, O.POSITION_IDX]) > thr
        assert 0.02 < over.mean() < 0.5
    term = O.default_terminal_cost(traj[:, -1], SC.X_T)
    assert 0.02 < (term == 0).mean() < 0.5
    assert 0.02 < (np.abs(c["u_nom"][None, :] + c["inputs"]) > 1.0).mean() < 0.5
    for name in SC.LIVE_INDICATOR:                              # rows whose total a relative comparison sees through: at least a quarter
        clear = SC.cost_clear_rows(name, c)
        assert clear.mean() >= 0.25 and not clear.all()
    # the launch shape is what the case is named for: rows per wave as the host picks them, a ragged last wave
    rpw = min(max((B + 8191) // 8192, 1), 64)
    assert rpw == {8193: 2, 16390: 3, 524289: 64}[B] and (B + 8191) // 8192 == {8193: 2, 16390: 3, 524289: 65}[B]
    assert B % rpw == 1


def test_cost_oracle_sees_the_terms_the_cases_are_there_for():
    """One step off in u_prev[k] / the previous input moves the oracle's stage cost far beyond the case's tolerance (the raised
    control-change-rate weights), and the horizon mean differs from the sum."""
    B, H = 64, 70
    c = SC.cost_inputs(B, H)
    for name, (_, _, _, rtol, atol) in SC.COST_CASES.items():
        stage, term, total = SC.cost_oracle(name, c)
        assert stage.shape == (B, H) and term.shape == total.shape == (B,) and stage.dtype == total.dtype == f32
        assert np.isfinite(stage).all() and (stage >= 0).all()
    stage, _, _ = SC.cost_oracle("legacy", c)
    shifted = dict(c, u_prev=np.roll(c["u_prev"], 1))
    off = np.abs(SC.cost_oracle("legacy", shifted)[0] - stage) > 10 * (1e-4 * np.abs(stage) + SC.cos_slack("legacy", c))
    assert off.mean() > 0.5
    for name in ("qb_prev", "qbg_prev_up", "qbg_prev_down"):
        stage, _, _ = SC.cost_oracle(name, c)
        wrong = dict(c, inputs=np.concatenate([c["inputs"][:, :1], c["inputs"][:, :1], c["inputs"][:, 2:]], axis=1))  # u[1] := u[0]
        d = np.abs(SC.cost_oracle(name, wrong)[0][:, 2] - stage[:, 2])            # stage 2 reads u[1] as its u_before
        assert (d > 10 * (SC.COST_CASES[name][3] * np.abs(stage[:, 2]) + SC.COST_CASES[name][4])).mean() > 0.25, name
    assert np.allclose(SC.cost_oracle("qbgm_mean", c)[2] * (H + 1), SC.cost_oracle("qbgm", c)[2], rtol=1e-5)
    assert float(SC.cos_slack("default", c).max()) <= 20000.0 * 2.0 ** -23 and not SC.cos_slack("qbgm", c).any()


@pytest.mark.parametrize("shape", SC.SAMPLER_SHAPES + [SC.KNOT_LIMIT_SHAPE], ids=str)
def test_sampler_references(shape):
    E, N, H, period = shape
    kn = SC.caller_knots(shape, 0.2)
    P = O.knot_count(H, period)
    assert kn.shape == (E, N, P)
    du = SC.oracle_interpolation(kn, H, period)
    # the FAST bound admits a float32 slope + one FMA (what the FAST sampler forms) and is a few float32 ulp, not a tolerance
    j, i = np.arange(H) // period, (np.arange(H) % period).astype(f32)
    slope = ((kn[:, :, j + 1] - kn[:, :, j]) * (f32(1.0) / f32(period))).astype(f32)
    fast = (slope.astype(np.float64) * i + kn[:, :, j]).astype(f32)               # (float64 product + sum, one rounding: the FMA)
    bound = SC.fast_interpolation_bound(kn, H, period)
    assert (np.abs(fast.astype(np.float64) - du) <= bound).all()
    assert bound.max() <= 5 * 2.0 ** -24 * np.abs(kn).max() * 2
    # the tiled reference: every element where the formula puts it, zeros elsewhere, of the size the library reports
    tiled = SC.tiled_reference(du)
    G, Hq = (N + 63) // 64, (H + 3) // 4
    assert tiled.size == E * G * Hq * 256 and np.count_nonzero(tiled) == np.count_nonzero(du)
    for env, n, k in ((0, 0, 0), (E - 1, N - 1, H - 1), (E - 1, N // 2, H // 2)):
        assert tiled[((((env * G + n // 64) * Hq + k // 4) * 64 + n % 64) * 4 + k % 4)] == du[env, n, k]
    back = tiled.reshape(E, G, Hq, 64, 4).transpose(0, 1, 3, 2, 4).reshape(E, G * 64, Hq * 4)
    assert np.array_equal(back[:, :N, :H], du) and not back[:, N:].any() and not back[:, :, H:].any()


def test_knot_limit_is_the_lds_check():
    """[256][P + 1] floats within 159 KB: P = 158 is the last knot count admitted."""
    fits = lambda P: 256 * (P + 1) * 4 <= 159 * 1024  # noqa: E731
    assert fits(SC.KNOT_LIMIT) and not fits(SC.KNOT_LIMIT + 1)
    E, N, H, period = SC.KNOT_LIMIT_SHAPE
    assert O.knot_count(H, period) == SC.KNOT_LIMIT and O.knot_count(H + 1, period) == SC.KNOT_LIMIT + 1
