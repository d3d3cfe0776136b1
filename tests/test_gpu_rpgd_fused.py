"""GPU: the fused rpgd / gradient-tf control step (cpmppi_rpgd_step) - against the staged launches it fuses, against a float64
restatement on the CPU, its permutation / redraw / shift, its device step counter, the captured closed loop, the controller
seam and its refusals.

Shapes: N = 16 (a partial wave, the shipped rpgd size), 40 (gradient-tf), 80 (two waves: ranking across waves, surplus lanes in the
barriers); H = 35 with period 4 (no multiple of the period) and H = 7; shift 0, 1, 2; E = 3.

Tolerances.  Against the staged path the bounds are 4 x the worst deviation measured on an MI355X over all parametrised cases
(the figures stand next to the bounds below); against the float64 restatement likewise (RESTATED_*)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from oracle import oracle_torch as OT  # noqa: E402
from oracle import philox_np as PH  # noqa: E402
import parity_util as PU  # noqa: E402

f32 = np.float32
QBG_W = dict(ccrc_weight_up=3.0, ccrc_weight_down=3.0, dd_linear_weight_up=2.0, dd_linear_weight_down=2.0)
COST_IDS = {"quadratic_boundary_grad_minimal": O.COST_QBGM, "default": O.COST_DEFAULT, "quadratic_boundary_grad": 3}
HP = dict(learning_rate=0.05, beta1=0.9, beta2=0.999, epsilon=1e-2, gradmax_clip=5.0)      # adam_epsilon 1e-2: Lipschitz in the gradient
PERIOD, STDEV = 4, 0.5

# ---- fused against staged: measured worst over the 18 cases of test_fused_equals_the_staged_sequence -> bound = 4 x worst
# (controls and plans are O(1) in [-1, 1]; m and v relative to the env's largest entry; S relative)
# Measured: Q, m, v, plan_out and Q_out of the fused step are BITWISE the staged sequence's in all 18 cases (the sweep and the Adam
# update are the staged kernels' statements), so their bound, 4 x 0, is equality.  S differs by the plain against the rotated
# sin / cos of the cost-only launch: worst 1.0e-6 relative (default / ODE / N 80; the existing test bounds that pair at 2e-4);
# under quadratic_boundary_grad, whose staged final cost is the adjoint kernel's own, S is bitwise too.
STAGED_MEASURED = dict(Q=0.0, m=0.0, v=0.0, S=1.0e-6, plan=0.0, Q_out=0.0)
STAGED_TOL = {k: 4.0 * x for k, x in STAGED_MEASURED.items()}
# ---- fused against the float64 restatement, two control steps (test_fused_equals_the_cpu_restatement) -> bound = 4 x worst
# Measured over plans clear of every branch, worst of the two steps (after step 0 / after step 1): Q 5.05e-7 / 1.54e-6 absolute,
# m 1.91e-6 / 1.94e-5 and v 1.34e-5 / 1.50e-5 of the env's largest entry, S 4.16e-6 / 9.35e-6 relative, Q_out 1.35e-7 / 2.76e-7; the
# ranking equal in both steps; flagged plans (6 and 1 of 48) no further off than the clear ones (worst Q 5.95e-7).  The float32
# adjoint sits far inside the 5e-4 of the gradient scale that test_gradient_vs_autograd allows, and 4 x the worst on the controls,
# 6.2e-6, far inside the project's 1e-4 band.
RESTATED_MEASURED = dict(Q=1.55e-6, m=1.95e-5, v=1.51e-5, S=9.4e-6, Q_out=2.8e-7)
RESTATED_TOL = {k: 4.0 * x for k, x in RESTATED_MEASURED.items()}


def report(capsys, text):
    with capsys.disabled():
        print("\n[rpgd] " + text)


def make(E, N, H, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    kw.setdefault("SQRTRHOINV", STDEV * math.sqrt(0.02))         # the sampler's sigma = the optimizer's sample_stdev
    return MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, shift_mode="none", period_interpolation_inducing_points=PERIOD, **kw))


def problem(E, N, H, seed, spread=0.3):
    """States well inside the track, per-env target / L / previous input, start plans with a few controls beyond the limits."""
    rng = np.random.Generator(np.random.SFC64(seed))
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.6, 0.6), rng.uniform(-1.5, 1.5), rng.uniform(-0.04, 0.04),
                                           rng.uniform(-0.1, 0.1)) for _ in range(E)]).astype(f32)
    tp = rng.uniform(-0.03, 0.03, E).astype(f32)
    Lv = rng.uniform(0.3, 0.45, E).astype(f32)
    prev = rng.uniform(-0.3, 0.3, E).astype(f32)
    Q = (spread * rng.standard_normal((E, N, H))).astype(f32)
    Q[:, 0] *= 4.0                                               # one plan per env with controls beyond the limits
    return s0, tp, np.ones(E, f32), Lv, prev, Q


def shifted(x, by, repeat_last):
    if by == 0:
        return x.copy()
    tail = np.repeat(x[..., -1:], by, axis=-1) if repeat_last else np.zeros_like(x[..., :by])
    return np.concatenate([x[..., by:], tail], axis=-1)


def staged(eng, s0, Q0, tp, te, Lv, prev, iterations, shift, qbg, first_iteration=1):
    """The staged control step as optimizer_gradient.py makes it: (rollout_cost_grad, adam_step) x iterations, the final cost,
    argmin, the shift.  -> numpy dict; `Q_final` are the plans before the shift."""
    Q = eng.tensor(Q0.copy())
    m, v = torch.zeros_like(Q), torch.zeros_like(Q)
    for i in range(iterations):
        _, G = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)
        eng.adam_step(Q, G, m, v, first_iteration + i, HP["learning_rate"], HP["beta1"], HP["beta2"], HP["epsilon"], HP["gradmax_clip"])
    S = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)[0] if qbg else eng.rollout_cost(s0, Q, tp, te, L=Lv)
    best = torch.argmin(S, dim=1)
    rows = torch.arange(Q.shape[0], device=Q.device)
    out = dict(S=S.cpu().numpy(), Q_out=Q[rows, best, 0].cpu().numpy(), plan=Q[rows, best].cpu().numpy(), Q_final=Q.cpu().numpy())
    out.update(Q=shifted(out["Q_final"], shift, True), m=shifted(m.cpu().numpy(), shift, False), v=shifted(v.cpu().numpy(), shift, False))
    return out


def fused(eng, s0, Q0, tp, te, Lv, prev, iterations, shift, m0=None, v0=None, **kw):
    E, N, H = Q0.shape
    Q = eng.tensor(Q0.copy())
    m = eng.tensor(m0.copy()) if m0 is not None else torch.zeros_like(Q)
    v = eng.tensor(v0.copy()) if v0 is not None else torch.zeros_like(Q)
    S, plan = eng.empty(E, N), eng.empty(E, H)
    order = torch.empty(E, N, dtype=torch.int32, device=Q.device)
    u, _, _, _ = eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev, iterations=iterations, shift=shift, S_out=S,
                               plan_out=plan, order_out=order, **HP, **kw)
    torch.cuda.synchronize()
    return dict(Q=Q.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), S=S.cpu().numpy(), plan=plan.cpu().numpy(),
                Q_out=u.cpu().numpy(), order=order.cpu().numpy())


def deviations(got, ref):
    """Worst deviation per quantity: Q, plan, Q_out absolute; m, v relative to the env's largest entry; S relative."""
    d = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("Q", "plan")}
    for k in ("m", "v"):
        scale = np.abs(ref[k]).reshape(ref[k].shape[0], -1).max(axis=1)[:, None, None] + 1e-30
        d[k] = float((np.abs(got[k] - ref[k]) / scale).max())
    d["S"] = float((np.abs(got["S"] - ref["S"]) / np.abs(ref["S"])).max())
    d["Q_out"] = float(np.abs(got["Q_out"] - ref["Q_out"]).max())
    return d


STAGED_SHAPES = [(16, 35, 1), (40, 7, 0), (80, 35, 2)]
# (cost, predictor, N) -> seed, where seed 11 leaves the two cheapest staged plans of some env within 100 x the tolerance on S
STAGED_SEEDS = {("default", "ODE_v0", 40): 12, ("default", "ODE", 40): 12, ("quadratic_boundary_grad", "ODE_v0", 16): 12}


def staged_case(cost, predictor, N, H, shift, seed=None):
    """One case of fused-against-staged -> (deviations, best-to-second gap of the staged costs relative to the best, max |x| of the
    oracle's trajectories of the start and the final plans)."""
    E = 3
    seed = STAGED_SEEDS.get((cost, predictor, N), 11) if seed is None else seed
    eng = make(E, N, H, cost_function_specification=cost, predictor_type=predictor, cost_weights=QBG_W if cost.endswith("_grad") else None)
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, seed)
    if predictor == "ODE":                                       # ... and a pole mass per env
        eng.set_pole_mass_rows(np.asarray([0.080, 0.087, 0.095], f32))
    ref = staged(eng, s0, Q0, tp, te, Lv, prev, 4, shift, cost.endswith("_grad"))
    got = fused(eng, s0, Q0, tp, te, Lv, prev, 4, shift)
    eng.close()
    Ss = np.sort(ref["S"], axis=1)
    gap = float(((Ss[:, 1] - Ss[:, 0]) / np.abs(Ss[:, 0])).min())
    reach = max(float(np.abs(O.predict_core(s0[e], np.clip(q[e], -1, 1), L=Lv[e], integrator=predictor)[:, :, O.POSITION_IDX]).max())
                for e in range(E) for q in (Q0, ref["Q_final"]))
    assert np.array_equal(got["order"][:, 0], np.argmin(got["S"], axis=1))
    return deviations(got, ref), gap, reach


@pytest.mark.parametrize("predictor", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("cost", list(COST_IDS))
@pytest.mark.parametrize("N,H,shift", STAGED_SHAPES)
def test_fused_equals_the_staged_sequence(N, H, shift, cost, predictor, capsys):
    """Same start plans, states, per-env L and previous input; 4 iterations, no resampling: Q, m, v, S_out, Q_out and plan_out of
    the one call against rollout_cost_grad / adam_step / final cost / argmin / shift.  Every entry of every plan is compared.  The
    two differ by float contraction and, in S, by the plain against the rotated sin / cos of the cost-only launch."""
    d, gap, reach = staged_case(cost, predictor, N, H, shift)
    report(capsys, f"fused vs staged {cost} / {predictor} N {N} H {H} shift {shift}: " + ", ".join(f"{k} {x:.2e}" for k, x in d.items())
           + f"; best-to-second gap {gap:.2e}, reach {reach:.3f} m")
    # no plan comes near the edge bounce (predictor_ODE_v0's only branch in the adjoint): from the oracle's trajectories
    assert reach < 0.17
    for k in ("Q", "m", "v", "S", "plan"):
        assert d[k] <= STAGED_TOL[k], f"{k}: {d[k]:.3e} > {STAGED_TOL[k]:.3e}"
    # the chosen control: compared where the staged costs name their best plan beyond doubt (a precondition on the inputs)
    assert gap > 100.0 * STAGED_TOL["S"], f"best-to-second gap {gap:.2e} within 100 x the tolerance on S"
    assert d["Q_out"] <= STAGED_TOL["Q_out"]


# ---------------------------------------------------------------------------------------------------------------------------------
# The float64 restatement: oracle_torch's cost and gradient, numpy Adam, numpy ranking, philox_np's knots for the redraw.
RS = dict(E=3, N=16, H=35, keep_k=12, resamp_per=2, shift=1, iterations=4, seed=5, draw_offset=3, problem_seed=23)


def interpolated(knots, H, period):
    """delta_u [.., H] from knots [.., P] as sample_kernel forms it for its own knots: slope in float32, one fma per step."""
    k = np.arange(H)
    j, i = k // period, k % period
    zl, zh = knots[..., j].astype(np.float64), knots[..., j + 1].astype(np.float64)
    slope = ((knots[..., j + 1] - knots[..., j]).astype(f32) * f32(1.0 / period)).astype(np.float64)
    return (slope * i + zl).astype(f32)


def restated():
    """Two consecutive control steps in float64 -> per step dict(Q, m, v, S, Q_out, order, flagged [E,N], min rank gap)."""
    E, N, H, k, rp = RS["E"], RS["N"], RS["H"], RS["keep_k"], RS["resamp_per"]
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, RS["problem_seed"])
    lr, b1, b2, eps, clipn = (HP[x] for x in ("learning_rate", "beta1", "beta2", "epsilon", "gradmax_clip"))
    Q, m, v = Q0.astype(np.float64), np.zeros((E, N, H)), np.zeros((E, N, H))
    P = (H + PERIOD - 1) // PERIOD + 1
    steps, t, prev_in = [], 0, prev.astype(np.float64)
    for c in range(2):
        flagged = np.zeros((E, N), bool)
        for _ in range(RS["iterations"]):
            t += 1
            for e in range(E):
                _, g = OT.cost_and_grad(O.COST_QBGM, s0[e], Q[e], tp[e], 1.0, L=Lv[e], previous_input=prev_in[e], integrator="ODE")
                traj = O.predict_core(s0[e], np.clip(Q[e], -1, 1).astype(f32), L=Lv[e], integrator="ODE")
                flagged[e] |= PU.flag_indicators(traj, "qbgm", tp[e]) | (np.abs(np.abs(Q[e]) - 1.0) < 1e-3).any(axis=1)
                nrm = np.sqrt((g ** 2).sum(-1, keepdims=True))
                gc = g * np.minimum(1.0, clipn / np.maximum(nrm, 1e-300))
                m[e] = b1 * m[e] + (1 - b1) * gc
                v[e] = b2 * v[e] + (1 - b2) * gc * gc
                Q[e] = np.clip(Q[e] - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m[e] / (np.sqrt(v[e]) + eps), -1, 1)
        S = np.stack([OT.cost_and_grad(O.COST_QBGM, s0[e], Q[e], tp[e], 1.0, L=Lv[e], previous_input=prev_in[e], integrator="ODE")[0]
                      for e in range(E)])
        order = np.argsort(S, axis=1, kind="stable")
        Ss = np.sort(S, axis=1)
        u = Q[np.arange(E), order[:, 0], 0].copy()
        if (c + 1) % rp == 0:
            fresh = interpolated(PH.knots(RS["seed"], RS["draw_offset"], 0, E, N, P, STDEV), H, PERIOD)
            fresh = np.clip(fresh + f32(0.1), -1, 1).astype(np.float64)
            idx = order[:, :k, None].repeat(H, axis=2)
            Q = np.concatenate([np.take_along_axis(Q, idx, 1), fresh[:, k:]], axis=1)
            m = np.concatenate([np.take_along_axis(m, idx, 1), np.zeros((E, N - k, H))], axis=1)
            v = np.concatenate([np.take_along_axis(v, idx, 1), np.zeros((E, N - k, H))], axis=1)
            flagged = np.concatenate([np.take_along_axis(flagged, order[:, :k], 1), np.zeros((E, N - k), bool)], axis=1)
        Q, m, v = shifted(Q, RS["shift"], True), shifted(m, RS["shift"], False), shifted(v, RS["shift"], False)
        steps.append(dict(Q=Q.copy(), m=m.copy(), v=v.copy(), S=S, Q_out=u, order=order, flagged=flagged,
                          rank_gap=float((np.diff(Ss, axis=1) / np.abs(Ss[:, :-1])).min())))
        prev_in = u
    return (s0, tp, te, Lv, prev, Q0), steps


_restated = {}


def restated_once():
    if not _restated:
        _restated["x"] = restated()
    return _restated["x"]


def test_restatement_inputs_are_mostly_clear_of_branches():
    """A condition on the inputs, from the oracle alone: at most a quarter of the plans are flagged in either step, and the float64
    costs rank the plans beyond what float32 can reorder (relative gaps above 1e-4)."""
    _, steps = restated_once()
    for st in steps:
        assert st["flagged"].mean() <= 0.25 and st["rank_gap"] > 1e-4


def test_fused_equals_the_cpu_restatement(capsys):
    """Two consecutive control steps of predictor ODE / quadratic_boundary_grad_minimal, the second one resampling (normal, mean
    0.1), against the float64 restatement; the second step starts from the first one's plans, moments and control.  Plans clear of
    every branch within the bound; flagged ones (parity_util.flag_indicators, a control within 1e-3 of a limit) within 4 x the bound
    but for 5 % of them."""
    E, N, H = RS["E"], RS["N"], RS["H"]
    (s0, tp, te, Lv, prev, Q0), steps = restated_once()
    eng = make(E, N, H, predictor_type="ODE")
    Q, m, v = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
    S, u, order = eng.empty(E, N), eng.zeros(E), torch.empty(E, N, dtype=torch.int32, device=Q.device)
    worst, n_fl, n_fl_off = dict.fromkeys(RESTATED_TOL, 0.0), 0, 0
    prev_in = eng.tensor(prev)
    for c, ref in enumerate(steps):
        eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev_in, iterations=RS["iterations"], keep_k=RS["keep_k"],
                      resamp_per=RS["resamp_per"], shift=RS["shift"], sample_mean=0.1, seed=RS["seed"], draw_offset=RS["draw_offset"],
                      count=c, adam_iteration=c * RS["iterations"], Q_out=u, S_out=S, order_out=order, **HP)
        prev_in = u
        torch.cuda.synchronize()
        got = dict(Q=Q.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), S=S.cpu().numpy(), Q_out=u.cpu().numpy())
        fl = ref["flagged"]
        per_plan = {k: np.abs(got[k] - ref[k]).max(axis=2) for k in ("Q", "m", "v")}
        for k in ("m", "v"):
            per_plan[k] = per_plan[k] / (np.abs(ref[k]).reshape(E, -1).max(axis=1)[:, None] + 1e-30)
        for k in ("Q", "m", "v"):
            worst[k] = max(worst[k], float(per_plan[k][~fl].max()))
            n_fl_off += int((per_plan[k][fl] > 4.0 * RESTATED_TOL[k]).sum())
        n_fl += 3 * int(fl.sum())
        worst["S"] = max(worst["S"], float((np.abs(got["S"] - ref["S"]) / np.abs(ref["S"])).max()))
        worst["Q_out"] = max(worst["Q_out"], float(np.abs(got["Q_out"] - ref["Q_out"]).max()))
        report(capsys, f"fused vs float64 restatement, after step {c}: " + ", ".join(f"{k} {x:.2e}" for k, x in worst.items())
               + f"; flagged {int(fl.sum())} of {fl.size}, worst flagged Q {per_plan['Q'][fl].max() if fl.any() else 0.0:.2e}")
        assert np.array_equal(order.cpu().numpy(), ref["order"]), f"step {c}: ranking"
        for k in worst:
            assert worst[k] <= RESTATED_TOL[k], f"step {c} {k}: {worst[k]:.3e} > {RESTATED_TOL[k]:.3e}"
    assert n_fl_off <= int(np.ceil(0.05 * n_fl)), f"{n_fl_off} of {n_fl} flagged plan rows outside 4 x the bound"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distribution", ["normal", "uniform"])
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("N,H,keep_k", [(80, 7, 50), (16, 35, 12)])
def test_resampling_is_a_permutation_plus_the_samplers_rows(N, H, keep_k, shift, distribution):
    """The same call twice from identical buffers at (c + 1) % resamp_per == 0, once with keep_k = N and once with keep_k < N: the
    survivors are BITWISE the no-resample result's rows in rank order (moments included), the other rows are the sampler's rows of the
    same index - shaped, clipped, shifted - with zero moments, and the ranking is cpmppi_cem_update's."""
    E, seed, offset, mean, ulo, uhi = 3, 77, 6, 0.15, -0.6, 0.7
    eng = make(E, N, H, **(dict(SQRTRHOINV=math.sqrt(0.02)) if distribution == "uniform" else {}))
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 41)
    rng = np.random.Generator(np.random.SFC64(42))
    m0 = (0.1 * rng.standard_normal(Q0.shape)).astype(f32)
    v0 = (0.01 * rng.uniform(0.1, 1.0, Q0.shape)).astype(f32)
    kw = dict(resamp_per=2, count=3, adam_iteration=6, seed=seed, draw_offset=offset, distribution=distribution, sample_mean=mean,
              uniform_lo=ulo, uniform_hi=uhi, m0=m0, v0=v0)
    a = fused(eng, s0, Q0, tp, te, Lv, prev, 2, shift, keep_k=N, **kw)
    b = fused(eng, s0, Q0, tp, te, Lv, prev, 2, shift, keep_k=keep_k, **kw)
    assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["order"], b["order"]) and np.array_equal(a["Q_out"], b["Q_out"])
    assert np.array_equal(a["plan"], b["plan"])
    idx = a["order"][:, :keep_k, None].astype(np.int64).repeat(H, axis=2)
    for k in ("Q", "m", "v"):
        assert np.array_equal(b[k][:, :keep_k], np.take_along_axis(a[k], idx, 1)), k
        assert a[k].shape == b[k].shape
    assert not b["m"][:, keep_k:].any() and not b["v"][:, keep_k:].any()
    assert a["m"][:, keep_k:, :H - shift].any()                              # (the no-resample call kept them)
    # the redrawn rows: the engine's own sampler at the same seed and offset, rows of the same index
    z = eng.sample(seed, offset=offset, knots=False, delta_u=True)[1]
    if distribution == "normal":
        fresh = z + mean
    else:
        fresh = ulo + (uhi - ulo) * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))
    fresh = shifted(fresh.clamp(-1.0, 1.0).cpu().numpy(), shift, True)
    np.testing.assert_allclose(b["Q"][:, keep_k:], fresh[:, keep_k:], atol=1e-6, rtol=0)
    assert np.ptp(fresh[:, keep_k:]) > 0.3
    if distribution == "uniform":
        assert fresh.min() >= ulo - 1e-6 and fresh.max() <= uhi + 1e-6
    # the ranking = the stable top-k of cpmppi_cem_update on the same costs; row 0 is torch.argmin's choice
    elites = eng.cem_update(eng.tensor(a["S"]), eng.tensor(Q0), N, 0.0, return_elites=True)[2].cpu().numpy()
    assert np.array_equal(a["order"], elites) and np.array_equal(a["order"][:, 0], np.argmin(a["S"], axis=1))
    # a call off the resampling period with keep_k < N leaves the rows where they are
    c = fused(eng, s0, Q0, tp, te, Lv, prev, 2, shift, keep_k=keep_k, **dict(kw, count=2))
    d = fused(eng, s0, Q0, tp, te, Lv, prev, 2, shift, keep_k=N, **dict(kw, count=2))
    for k in ("Q", "m", "v"):
        assert np.array_equal(c[k], d[k])
    eng.close()


def test_device_counter_equals_the_host_counters():
    """2 resamp_per + 1 steps with the step counter on the device against the same steps with count / adam_iteration / draw_offset
    from the host: Q, m, v and Q_out bitwise equal after every step; the counter ends at the number of steps."""
    E, N, H, rp, iters, keep_k = 3, 16, 35, 2, 3, 12
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 51)
    kw = dict(iterations=iters, keep_k=keep_k, resamp_per=rp, shift=1, seed=13, sample_mean=0.05, **HP)
    bufs = [[eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E)] for _ in range(2)]
    counter = torch.zeros(1, dtype=torch.int64, device=bufs[0][0].device)
    s = eng.tensor(s0)
    draws = 4
    for c in range(2 * rp + 1):
        Qh, mh, vh, uh = bufs[0]
        eng.rpgd_step(s, Qh, mh, vh, tp, te, L=Lv, previous_input=uh, count=c, adam_iteration=c * iters,
                      draw_offset=4 + c // rp, Q_out=uh, **kw)
        Qd, md, vd, ud = bufs[1]
        eng.rpgd_step(s, Qd, md, vd, tp, te, L=Lv, previous_input=ud, count_dev=counter, draw_offset=draws, Q_out=ud, **kw)
        for h, d in zip(bufs[0], bufs[1]):
            assert torch.equal(h, d), f"step {c}"
        assert int(counter.item()) == c + 1
        eng.plant_advance(s, uh, L=Lv, n_substeps=10)                        # the next step sees another state
    assert bufs[0][0][:, keep_k:].abs().max() > 0 and not torch.equal(bufs[0][0], eng.tensor(Q0))
    eng.close()


def _schedule_batch(E):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=31, length_of_experiment=0.5, keep_target_equilibrium_x_seconds_up=0.2, turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    return SC.RandomExperimentSetter(cfg).draw(E, 83, L=np.linspace(0.3, 0.45, E).astype(f32))


def _rpgd(E, fused, **over):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    c = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), config=dict(seed=9, fused=fused, **over), num_envs=E)
    c.configure("rpgd", predictor_specification="ODE")
    return c.optimizer


def test_captured_loop_equals_the_launched_loop():
    """run_schedule(graph=True, steps_per_graph=5) with a fused rpgd optimizer against graph=False with the same configuration: 4 envs,
    25 control periods, resamp_per = 10 - recorded states and controls bitwise equal.  A staged optimizer is still refused."""
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    E, outs = 4, []
    for graph in (False, True):
        b = _schedule_batch(E)
        opt = _rpgd(E, True, resamp_per=10)
        assert opt.fused and opt.resamp_per == 10 and opt.num_rollouts == 16 and opt.mpc_horizon == 35
        res = BatchedCartPoleExperiment(opt.engine, seed=0).run_schedule(b, graph=graph, steps_per_graph=5, optimizer=opt)
        torch.cuda.synchronize()
        outs.append({k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state")})
        opt.engine.close()
    assert b.n_periods == 25 and outs[0]["Q"].shape == (26, E) and np.abs(outs[0]["Q"]).max() > 0.05
    assert np.isfinite(outs[0]["states"]).all()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    staged_opt = _rpgd(E, False)
    with pytest.raises(ValueError, match="paced by the host"):
        BatchedCartPoleExperiment(staged_opt.engine, seed=0).run_schedule(_schedule_batch(E), graph=True, optimizer=staged_opt)
    staged_opt.engine.close()


@pytest.mark.parametrize("spec", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("name", ["gradient", "rpgd"])
def test_fused_optimizers_through_the_controller_seam(name, spec):
    """controller_mpc(config=dict(fused=True)).configure('gradient' | 'rpgd') at the shipped hyper-parameters: shape and limits of the
    control, the best logged cost after one step is below the best cost before, 60 control steps on the device plant keep mildly
    perturbed poles upright (the thresholds of test_gradient_optimizers_through_the_controller_seam)."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    E = 8

    def build(**kw):
        c = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                           control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=3, fused=True))
        c.configure(name, predictor_specification=spec, **kw)
        return c

    ctrl = build()
    opt = ctrl.optimizer
    assert opt.fused and opt.cfg.predictor_type == spec and opt.num_rollouts == (40 if name == "gradient" else 16)
    eng = opt.engine
    rng = np.random.Generator(np.random.SFC64(2))
    s = eng.tensor(np.stack([O.create_cartpole_state(rng.uniform(-0.25, 0.25), rng.uniform(-0.5, 0.5),
                                                     rng.uniform(-0.05, 0.05), 0.0) for _ in range(E)]))
    tp, te, Lv = np.zeros(E, f32), np.ones(E, f32), np.full(E, 0.395, f32)
    S_before = eng.rollout_cost(s, opt.Q, tp, te, L=Lv).min(dim=1).values.cpu()
    Q0 = ctrl.step(s, 0.0, {})
    assert Q0.shape == (E, 1) and np.abs(Q0).max() <= 1.0
    assert opt.count == 1 and opt.adam_it == (5 if name == "gradient" else 4)
    ctrl2 = build(controller_logging=True)
    ctrl2.step(s, 0.0, {})
    log = ctrl2.controller_data_for_csv
    assert log["J_logged"].shape == (E, opt.num_rollouts) and log["u_logged"].shape == (E, 35)
    np.testing.assert_array_equal(log["Q_logged"], log["u_logged"][:, 0])
    assert (torch.as_tensor(log["J_logged"]).min(dim=1).values < S_before).all()
    for _ in range(60):
        Q = opt.step(s, as_tensor=True)
        eng.plant_advance(s, Q, L=Lv, n_substeps=10)
    sh = s.cpu().numpy()
    assert (np.abs(sh[:, O.ANGLE_IDX]) < 0.35).mean() >= 0.75 and np.abs(sh[:, O.POSITION_IDX]).max() < 0.198
    assert opt.count == 61
    eng.close()
    ctrl2.optimizer.engine.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kw", [
    ("legacy cost", dict(cost_function_specification="legacy_mppi_cartpole")),
    ("quadratic_boundary", dict(cost_function_specification="quadratic_boundary")),
    ("PRECISE math", dict(math_mode="precise")),
    ("S beyond the LDS budget", dict(intermediate_steps=101)),
    ("N beyond one workgroup", dict(num_rollouts=320))])
def test_refusals_about_the_handle(what, kw):
    """What cpmppi_rollout_cost_grad refuses, and more plans than a workgroup holds: refused with a text, by the step and by the
    reserve, and the handle goes on serving what it supports."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, H = 2, 5
    N = kw.pop("num_rollouts", 24)
    eng = make(E, N, H, **kw)
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 9)
    Q, m, v = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
    for _ in range(2):
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: "):
            eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, iterations=2, **HP)
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_reserve: "):
            eng.rpgd_reserve()
    assert np.array_equal(Q.cpu().numpy(), Q0)
    if what in ("quadratic_boundary", "PRECISE math", "N beyond one workgroup"):
        assert np.isfinite(eng.rollout_cost(s0, Q, tp, te, L=Lv).cpu().numpy()).all()
    assert np.isfinite(eng.sample(1, knots=False, delta_u=True)[1].cpu().numpy()).all()
    eng.close()


def test_refusals_about_the_arguments_leave_the_handle_usable():
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 3, 16, 7
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 10)
    Q, m, v = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
    ok = dict(iterations=2, keep_k=12, resamp_per=2, shift=1, **HP)

    def call(**over):
        return eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev, **dict(ok, **over))

    for over, text in ((dict(keep_k=0), "keep_k"), (dict(keep_k=N + 1), "keep_k"), (dict(iterations=0), "iterations"),
                       (dict(shift=H + 1), "shift")):
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: .*" + text):
            call(**over)
    assert np.array_equal(Q.cpu().numpy(), Q0)
    # a NULL among the required pointers, a misaligned one: through the argument block itself
    prep = eng.prepare_rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev, **ok)
    for field in ("s0", "target_position", "target_equilibrium", "Q", "m", "v", "Q_out"):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, None)
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: null pointer"):
            prep.run()
        setattr(prep.args, field, keep + 2)
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: misaligned pointer"):
            prep.run()
        setattr(prep.args, field, keep)
    counter = torch.zeros(2, dtype=torch.int64, device=Q.device)
    prep.args.count_dev = counter.data_ptr() + 4
    with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: misaligned pointer"):
        prep.run()
    prep.args.count_dev = None
    assert np.array_equal(Q.cpu().numpy(), Q0)
    # fewer pole masses registered than envs in the call
    eng.set_pole_mass_rows(eng.tensor(np.full(2, 0.09, f32)))
    with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: 3 rows"):
        call()
    eng.set_pole_mass_rows(None)
    # ... and a valid call afterwards succeeds
    u = call()[0]
    torch.cuda.synchronize()
    assert np.isfinite(u.cpu().numpy()).all() and not np.array_equal(Q.cpu().numpy(), Q0)
    eng.close()


def test_capture_without_a_reserved_workspace_is_refused_and_the_capture_survives():
    """On a capturing stream the step must not allocate: without cpmppi_rpgd_reserve it is refused with a text before any HIP call
    that a capture forbids - the capture goes on, ends and replays; after the reserve the same step is captured and replayed."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 16, 7
    eng = make(E, N, H)
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 12)
    s, tpd, ted, Ld = eng.tensor(s0), eng.tensor(tp), eng.tensor(te), eng.tensor(Lv)
    Q, m, v, u = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E)
    counter = torch.zeros(1, dtype=torch.int64, device=Q.device)
    marker = eng.zeros(4)
    prep = eng.prepare_rpgd_step(s, Q, m, v, tpd, ted, L=Ld, iterations=2, count_dev=counter, Q_out=u, **HP)
    side = torch.cuda.Stream(device=Q.device)
    side.wait_stream(torch.cuda.current_stream(Q.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: the stream is being captured"):
                prep.run()
            marker.add_(1.0)
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.array_equal(Q.cpu().numpy(), Q0) and int(counter.item()) == 0
    # reserved: captured, replayed twice = two launched steps
    eng.rpgd_reserve()
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(Q.device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            prep.run()
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g2.replay()
    g2.replay()
    torch.cuda.synchronize()
    ref = fused(eng, s0, Q0, tp, te, Lv, None, 2, 1, count=0, adam_iteration=0)
    ref2 = fused(eng, s0, ref["Q"], tp, te, Lv, None, 2, 1, m0=ref["m"], v0=ref["v"], count=1, adam_iteration=2)
    assert int(counter.item()) == 2 and np.array_equal(Q.cpu().numpy(), ref2["Q"]) and np.array_equal(u.cpu().numpy(), ref2["Q_out"])
    eng.close()
