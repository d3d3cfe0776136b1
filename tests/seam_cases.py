"""Inputs, references and bounds of the seam-kernel tests (cpmppi_seams.hip beyond one wave, one pass and one launch path): shared by
the GPU tests (test_gpu_seams.py) and the host test that judges the inputs and bounds themselves (test_seams_host.py), so that both
run on the very same numbers.  In the style of rollout_matrix.py / gru_grad_ref.py: plain tables and builders, no GPU.

Every reference here is the oracle (oracle/oracle_np.py) or float64 numpy of the formula in include/cpmppi.h / SURVEY.md evaluated on
the same float32 inputs; every bound is derived from the number formats, never from what a kernel returned."""
from dataclasses import replace

import numpy as np
from numpy.random import SFC64, Generator

from oracle import oracle_np as O

f32 = np.float32
THL = float(O.DEFAULT_PARAMS.TrackHalfLength)

# ---- 1: the soft-min update seam (rwa_kernel: 4 waves, wave w owns rows w, w + 4, ..; lane = column) ---------------------------------
# (E, N, H), each the smallest that first reaches one path of the kernel
RWA_SHAPES = [(3, 1, 1),        # one row: waves 1 - 3 own none
              (2, 2, 1),        # waves 2 and 3 own no row
              (3, 28, 5),       # the largest N with the tail loop only (n + 28 < N never holds)
              (3, 29, 64),      # wave 0 enters the eight-rows-in-flight loop once; exactly one column pass
              (3, 33, 65),      # the second column pass has one live column (kk clamped on the other 63 lanes)
              (2, 300, 130)]    # N > 256: min / sum loops go round twice; three column passes; unrolled loop + tail in every wave
RWA_LBDS = (100.0, 1.0)
RWA_REGIMES = ("spread", "offset", "dominant", "spread_dupmin")


def rwa_inputs(shape, LBD, regime):
    """-> S[E,N], delta_u[E,N,H] float32, drawn per env (a wrong env base pointer shows).
    spread: S ~ U(0, 2 LBD), every row carries weight.  offset: S = 1e6 + U(0, 3 LBD) - without the subtraction of the minimum every
    weight underflows (0 / 0).  dominant: S ~ LBD U(1e3, 2e3) except row N-1 (a tail-loop row) at S = 5: every other weight is exactly
    0 in float32 and in float64, the output is row N-1 of delta_u.  spread_dupmin: spread with its minimum in rows 0 AND N-1."""
    E, N, H = shape
    rng = Generator(SFC64([E, N, H, int(LBD), RWA_REGIMES.index(regime)]))
    if regime in ("spread", "spread_dupmin"):
        S = rng.uniform(0.0, 2.0 * LBD, (E, N))
        if regime == "spread_dupmin":
            S[:, 0] = S[:, N - 1] = 0.5 * S.min(axis=1)
    elif regime == "offset":
        S = 1.0e6 + rng.uniform(0.0, 3.0 * LBD, (E, N))
    elif regime == "dominant":
        S = LBD * rng.uniform(1.0e3, 2.0e3, (E, N))
        S[:, N - 1] = 5.0
    else:
        raise ValueError(regime)
    du = 0.3 * rng.standard_normal((E, N, H))
    return S.astype(f32), du.astype(f32)


def rwa_reference(S, du, LBD):
    """w = exp(-(S - min S) / LBD), out = (w @ du) / sum w per env, float64 (controller_mppi_cartpole.py:306-321)."""
    S, du = np.asarray(S, np.float64), np.asarray(du, np.float64)
    w = np.exp(-(S - S.min(axis=1, keepdims=True)) / np.float64(LBD))
    return np.einsum("en,enk->ek", w, du) / w.sum(axis=1, keepdims=True)


def rwa_bound(du):
    """Per (env, column): (N/4 + 16) 2^-23 max_n |du[env, n, k]| - a wave's sequential float32 accumulation over its ceil(N/4) rows
    (each step rounds a partial sum of at most sum w |du| <= sum w max|du|, and the quotient by sum w takes that back to max|du|), plus
    the cross-wave sums, the normalising sum and a few ulp per weight."""
    N = du.shape[1]
    return (N / 4.0 + 16.0) * 2.0 ** -23 * np.abs(np.asarray(du, np.float64)).max(axis=1)


def rwa_float32_other_order(S, du, LBD):
    """The same update in float32 in ANOTHER summation order than the kernel's (rows last to first, one accumulator, weights
    normalised first): what the bound must admit."""
    E, N, H = du.shape
    out = np.zeros((E, H), f32)
    for e in range(E):
        w = np.exp((f32(-1.0) / f32(LBD)) * (S[e] - S[e].min())).astype(f32)
        a = f32(0.0)
        for n in range(N - 1, -1, -1):
            a = f32(a + w[n])
        acc = np.zeros(H, f32)
        for n in range(N - 1, -1, -1):
            acc = (acc + (w[n] / a).astype(f32) * du[e, n]).astype(f32)
        out[e] = acc
    return out


# ---- 2: the cost seam (trajectory_cost_kernel: lane = time step, a wave walks rows_per_wave rows) ------------------------------------
COST_SHAPES = [(8193, 70),      # rpw = 2, the last wave holds one row, the second lane pass has 6 live lanes
               (16390, 5)]      # rpw = 3, the last wave holds one row
COST_CLAMP_SHAPE = (524289, 3)  # ceil((B + 8191) / 8192) = 65 -> the clamp at 64; quadratic_boundary_grad_minimal only
COST_SMALL_LAUNCH = 8192        # at most this many rows: rows_per_wave == 1
X_T = f32(0.01)
PREVIOUS_INPUT = f32(0.37)
X_MARGIN, ANGLE_MARGIN, U_MARGIN = 1.0e-3 * THL, 1.0e-3, 1.0e-3
STAGE_X_THRESHOLDS = (0.85 * THL, 0.90 * THL, 0.95 * THL)      # ptf THL (qbgm, qbg), default.py's, quadratic_boundary's / legacy's
# name -> (MPPIConfig options, target_equilibrium, previous input given?, rtol, atol of a stage element)
# The control-change-rate weights are raised where the shipped ones leave the term invisible (quadratic_boundary_grad ships 0,
# quadratic_boundary and the legacy cost 1 against 5000 / 12 500 (1 - cos)^2: rollout_matrix.py COST_WEIGHTS), so that the read of
# u_before / u_prev[k] is pinned (test_seams_host.py: one step off lands beyond ten times the tolerance).
# rtol 1e-4 everywhere; atol: what tests/test_gpu_parity.py / test_gpu_boundary.py hold for the same cost.  `default` and the legacy
# cost have no stage atol there; theirs is the float32 cos of the angle term alone, per element (cos_slack below), nothing fixed.
COST_CASES = {
    "qbgm": (dict(cost_function_specification="quadratic_boundary_grad_minimal"), 1.0, False, 1e-4, 1e-5),
    "default": (dict(cost_function_specification="default"), 1.0, False, 1e-4, 0.0),
    "qb_prev": (dict(cost_function_specification="quadratic_boundary", cost_weights=dict(ccrc_weight=1.0e3)), 1.0, True, 1e-4, 1e-2),
    "qbg_prev_up": (dict(cost_function_specification="quadratic_boundary_grad",
                         cost_weights=dict(ccrc_weight_up=50.0, ccrc_weight_down=50.0)), 1.0, True, 1e-4, 1e-3),
    "qbg_prev_down": (dict(cost_function_specification="quadratic_boundary_grad",
                           cost_weights=dict(ccrc_weight_up=50.0, ccrc_weight_down=50.0)), -1.0, True, 1e-4, 1e-3),
    "legacy": (dict(cost_function_specification="legacy_mppi_cartpole", cost_weights=dict(ccrc_weight=1.0e4)), 1.0, False, 1e-4, 0.0),
    "qbgm_mean": (dict(cost_function_specification="quadratic_boundary_grad_minimal", horizon_reduce="mean"), 1.0, False, 1e-4, 1e-5),
    "default_mean": (dict(cost_function_specification="default", horizon_reduce="mean"), 1.0, False, 1e-4, 0.0),
}
LIVE_INDICATOR = {"default": 0.90 * THL, "default_mean": 0.90 * THL, "legacy": 0.95 * THL, "qb_prev": 0.95 * THL}


def _push_abs(v, thr, margin):
    """|v| clear of thr by 1.5 margin wherever it is within that of it (in place; the sign and the side of thr are kept)."""
    a = np.abs(v)
    near = np.abs(a - thr) < 1.5 * margin
    v[near] = np.copysign(np.where(a[near] >= thr, thr + 1.5 * margin, thr - 1.5 * margin), v[near])


def cost_inputs(B, H):
    """-> dict(traj[B,H+1,6], inputs[B,H], u_nom[H], u_prev[H]) float32: synthetic (the seam is a pure function of them).
    Angles uniform in (-pi, pi); even rows keep |x| < 0.84 THL (no track-edge term at all), odd rows reach 1.1 THL (beyond every one);
    every eighth row ends inside the terminal indicator's box.  Every indicator argument is then pushed clear of its threshold: |x|
    of a stage against 0.85 / 0.90 / 0.95 THL, the terminal |angle| against 0.2 and |x - x*| against 0.1 THL, and the two the costs
    hold besides: |u_nom + delta_u| against 1 (legacy) and |angle| of a stage against 0 (quadratic_boundary_grad's
    cos(angle) > cos(admissible_angle) = 1)."""
    rng = Generator(SFC64([B, H, 2]))
    rows = np.arange(B)
    ang = rng.uniform(-np.pi, np.pi, (B, H + 1))
    amp = np.where(rows % 2 == 0, 0.84, 1.10) * THL
    x = rng.uniform(-1.0, 1.0, (B, H + 1)) * amp[:, None]
    inside = rows % 8 == 0
    ang[inside, H] = rng.uniform(-0.15, 0.15, int(inside.sum()))
    x[inside, H] = float(X_T) + rng.uniform(-0.08, 0.08, int(inside.sum())) * THL
    traj = np.zeros((B, H + 1, 6), f32)
    traj[:, :, O.ANGLE_IDX], traj[:, :, O.POSITION_IDX] = ang, x
    traj[:, :, O.ANGLED_IDX] = rng.uniform(-8.0, 8.0, (B, H + 1))
    traj[:, :, O.POSITIOND_IDX] = rng.uniform(-0.6, 0.6, (B, H + 1))
    xs = traj[:, :H, O.POSITION_IDX]
    for thr in STAGE_X_THRESHOLDS:
        _push_abs(xs, thr, X_MARGIN)
    _push_abs(traj[:, :H, O.ANGLE_IDX], 0.0, ANGLE_MARGIN)
    _push_abs(traj[:, H, O.ANGLE_IDX], 0.2, ANGLE_MARGIN)
    d = traj[:, H, O.POSITION_IDX].astype(np.float64) - float(X_T)
    _push_abs(d, 0.1 * THL, X_MARGIN)
    traj[:, H, O.POSITION_IDX] = d + float(X_T)
    traj[:, :, O.ANGLE_COS_IDX], traj[:, :, O.ANGLE_SIN_IDX] = np.cos(traj[:, :, O.ANGLE_IDX]), np.sin(traj[:, :, O.ANGLE_IDX])
    u_nom = rng.uniform(-0.5, 0.5, H).astype(f32)
    u_prev = rng.uniform(-0.5, 0.5, H).astype(f32)
    inputs = rng.uniform(-1.0, 1.0, (B, H)).astype(f32)
    total = (u_nom[None, :] + inputs).astype(np.float64)
    _push_abs(total, 1.0, U_MARGIN)
    inputs = (total - u_nom[None, :]).astype(f32)
    return dict(traj=traj, inputs=inputs, u_nom=u_nom, u_prev=u_prev)


def cost_margins(c):
    """Distance of every indicator argument of `cost_inputs` to its threshold, the smallest over the batch, in float64 on the float32
    inputs: dict(stage_x, stage_angle, terminal_angle, terminal_x, legacy_u)."""
    traj, H = c["traj"].astype(np.float64), c["inputs"].shape[1]
    ax = np.abs(traj[:, :H, O.POSITION_IDX])
    return dict(stage_x=min(float(np.abs(ax - thr).min()) for thr in STAGE_X_THRESHOLDS),
                stage_angle=float(np.abs(traj[:, :H, O.ANGLE_IDX]).min()),
                terminal_angle=float(np.abs(np.abs(traj[:, H, O.ANGLE_IDX]) - 0.2).min()),
                terminal_x=float(np.abs(np.abs(traj[:, H, O.POSITION_IDX] - float(X_T)) - 0.1 * THL).min()),
                legacy_u=float(np.abs(np.abs((c["u_nom"][None, :] + c["inputs"]).astype(np.float64)) - 1.0).min()))


def cost_clear_rows(name, c):
    """Rows none of whose stages carries the cost's big track-edge term (6e9 / 1.2e8 per stage; quadratic_boundary: from 0 up to 2.4e12):
    only there does a relative comparison of the total see the other terms."""
    H = c["inputs"].shape[1]
    return ~(np.abs(c["traj"][:, :H, O.POSITION_IDX]) > LIVE_INDICATOR[name]).any(axis=1)


def cost_oracle(name, c):
    """-> (stage[B,H], terminal[B], total[B]) float32 from the oracle's own cost functions."""
    options, te, with_prev, _, _ = COST_CASES[name]
    traj, inputs = c["traj"], c["inputs"]
    spec, reduce = options["cost_function_specification"], options.get("horizon_reduce", "sum")
    te = f32(te)
    if spec == "legacy_mppi_cartpole":
        cc = replace(O.DEFAULT_COST, leg_ccrc_weight=options["cost_weights"]["ccrc_weight"])
        stage = O.legacy_stage_cost(traj[:, :-1], c["u_nom"][None, :], inputs, c["u_prev"][None, :], X_T, c=cc).astype(f32)
        term = O.legacy_terminal_cost(traj[:, -1], X_T).astype(f32)
        return stage, term, (np.sum(stage, axis=1) + term).astype(f32)
    cc = replace(O.DEFAULT_COST)
    if spec == "quadratic_boundary_grad_minimal":
        cid, stage = O.COST_QBGM, O.qbgm_stage_cost(traj[:, :-1], inputs, X_T, te)
    elif spec == "default":
        cid, stage = O.COST_DEFAULT, O.default_stage_cost(traj[:, :-1], inputs, X_T, te)
    elif spec == "quadratic_boundary":
        cid, cc.qb_weights, cc.qb_previous_input = O.COST_QB, dict(options["cost_weights"]), (PREVIOUS_INPUT if with_prev else None)
        stage = O.qb_stage_cost(traj[:, :-1], inputs, cc.qb_previous_input, X_T, te, cc.qb_weights)
    else:
        cid, cc.qbg_weights, cc.qbg_previous_input = O.COST_QBG, dict(options["cost_weights"]), PREVIOUS_INPUT
        stage = O.qbg_stage_cost(traj[:, :-1], inputs, PREVIOUS_INPUT, X_T, te, cc.qbg_weights)
    term = (O.default_terminal_cost(traj[:, -1], X_T) if cid in (O.COST_DEFAULT, O.COST_QB)
            else np.zeros(traj.shape[0], f32)).astype(f32)
    return stage.astype(f32), term, O.trajectory_cost(cid, traj, inputs, X_T, te, reduce, c=cc)


def cos_slack(name, c):
    """Per stage element: what 2^-23 on cos(angle) (two float32 ulp below 1: the device's cosf and the host's are each within one of
    the true value) moves the angle term of `default` (20000 / 4 (1 - cos)^2) and of the legacy cost (50000 / 4 (1 - cos)^2) by:
    |d/dcos| 2^-23 = w / 2 (1 - cos) 2^-23.  An element at cos ~ 1 whose other terms happen to be small is not pinned to 1e-4 relative
    by any float32 cos.  Zero for the costs whose atol the existing tests fix."""
    w = {"default": 20000.0, "default_mean": 20000.0, "legacy": 50000.0}.get(name)
    H = c["inputs"].shape[1]
    if w is None:
        return np.zeros((c["traj"].shape[0], H))
    return 0.5 * w * (1.0 - np.cos(c["traj"][:, :H, O.ANGLE_IDX].astype(np.float64))) * 2.0 ** -23


# ---- 4: sampler, interpolation, tiling ------------------------------------------------------------------------------------------------
# (E, N, H, period)
SAMPLER_SHAPES = [(1, 1, 1, 10),        # one row, one step, P = 2
                  (2, 5, 7, 3),         # ten rows: less than one wave; P = 4
                  (3, 67, 130, 10),     # P = 14: the last knot quad partial; three 64-step passes, H % 4 == 2; two row groups per env, the
                                        # second with 3 live rows; 6 groups: a half-empty second block
                  (1, 300, 64, 1)]      # P = 65: 67.6 KB of dynamic LDS, beyond the default 64 KB; H exactly one pass
KNOT_LIMIT = 158                        # the largest knot count the sampler's LDS check admits: [256][P + 1] floats <= 159 KB
KNOT_LIMIT_SHAPE = (1, 8, KNOT_LIMIT - 1, 1)


def caller_knots(shape, sigma):
    E, N, H, period = shape
    rng = Generator(SFC64([E, N, H, period, 4]))
    return (sigma * rng.standard_normal((E, N, O.knot_count(H, period)))).astype(f32)


def oracle_interpolation(kn, H, period):
    E, N, P = kn.shape
    return O.interpolate_knots(kn.reshape(E * N, P), H, period).reshape(E, N, H)


def fast_interpolation_bound(kn, H, period):
    """Per element of delta_u[E,N,H]: 3 2^-24 |z_hi - z_lo| + 2^-23 max(|z_lo|, |z_hi|).  The FAST sampler takes the reference's own
    float32 difference, multiplies it by the rounded reciprocal of the period and rounds the product: a float32 slope within 2 2^-24
    (relative, to first order) of the reference's float64 one, times i < period steps, i.e. 2 2^-24 |z_hi - z_lo| - the third
    half-ulp covers the second-order terms and the rounded difference standing for the exact one.  The one FMA then rounds a result of
    at most max(|z_lo|, |z_hi|) once, and so does the reference's float32 store: 2^-24 each."""
    kn = np.asarray(kn, np.float64)
    j = np.arange(H) // period
    zl, zh = kn[:, :, j], kn[:, :, j + 1]
    return 3.0 * 2.0 ** -24 * np.abs(zh - zl) + 2.0 ** -23 * np.maximum(np.abs(zl), np.abs(zh))


def tiled_reference(du):
    """delta_u[E,N,H] -> the whole tiled buffer by the index formula of include/cpmppi.h written out: element (env, n, k) sits at
    ((((env G + n / 64) Hq + k / 4) 64 + n % 64) 4 + k % 4 with G = ceil(N / 64), Hq = ceil(H / 4); everything else is zero."""
    E, N, H = du.shape
    G, Hq = (N + 63) // 64, (H + 3) // 4
    env, n, k = np.meshgrid(np.arange(E), np.arange(N), np.arange(H), indexing="ij")
    idx = ((((env * G + n // 64) * Hq + k // 4) * 64 + n % 64) * 4 + k % 4)
    out = np.zeros(E * G * Hq * 256, f32)
    out[idx.reshape(-1)] = np.asarray(du, f32).reshape(-1)
    return out
