"""GPU: the GRU predictor path at its edges - gru_predict_kernel across blocks and tails, gru_rollout_cost_kernel with every glue
flag, ragged rollout counts, knot periods other than 10, its step outputs (device step counter, u_nom_out, S_out = NULL), and the
batched optimizer's hidden-state hand-over.  tests/test_gpu_gru.py pins the numerics at friendly shapes and default options; this
module is about the statements around them.

Reference: oracle/oracle_np.py (gru_predict, gru_mppi_step) in float32 and, as the second realisation, in float64.  Perturbations
compared against the oracle come from the host (SFC64) or are read back from the library's own sampler.

Bounds (the project's, none new): costs through parity_util.assert_costs (1e-4 band + the oracle's float32 / float64 gap; rollouts
the float32 oracle cannot pin to a quarter of the band - and, for `default`, rollouts within reach of an indicator threshold - are
flagged); u_nom and Q through assert_controls (1e-4 + soft-min allowance); states and hidden states 1e-4 + |oracle32 - oracle64|,
the angle on the circle; the same statements on the same inputs bit for bit.  Every oracle-compared env has at most 5 % of its
rollouts flagged (asserted), and where the glue flags are the subject (test_glue_flags_vs_oracle) at least 5 % of the oracle's u_run entries sit on a
limit (clip) or beyond +-1 (penalise) (asserted).

The predict seam's h_out is ONE contiguous [2, B, 32] block: what lies behind the first layer's plane is the second layer's first
row.  The sentinel rows of the direct call therefore sit behind traj and behind the second plane; the first plane's far side is
checked by the second plane being bit-identical to the engine call's.

Measured on the MI355X (this module's first run; worst over the cases of a test, clear rollouts):
  test                                         worst assert_costs excess   worst |u_nom - oracle32|
  test_glue_flags_vs_oracle                    0.439 of the allowance      1.69e-05
  test_ragged_rollout_counts_vs_oracle         0.019                       2.98e-08
  test_noise_sources_agree_at_other_periods    0.016                       2.24e-06
  test_batched_optimizer_with_the_gru          -                           2.24e-08 (memory: 1.49e-07)
  test_predict_seam_across_blocks_and_tails    states 1.28e-05 (an angle whose sin / cos pair has radius 0.004), hidden 3.58e-07
One noise source against the delta_u step of the same perturbations (nothing derivable exists, so: measured over the 16 cases,
asserted at four times the measurement and never beyond the 1e-4 band):
  PRECISE   S bit-identical for knots and Philox (asserted so);         u_nom within 1.192e-07
  FAST      S bit-identical for Philox (asserted so), knots 9.636e-07 relative (71 - 82 of 200 costs differ); u_nom 3.874e-07
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import parity_util as PU  # noqa: E402

f32 = np.float32
COSTS = {"quadratic_boundary_grad_minimal": O.COST_QBGM, "default": O.COST_DEFAULT}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_c5.npz")
# one noise source against the delta_u step: (worst relative difference of S, worst absolute difference of u_nom), 4 x the
# measurement of the module docstring; 0.0 = measured bit-identical, asserted so
SOURCE_TOL = {("fast", "knots"): (4 * 9.636e-07, 4 * 3.874e-07), ("fast", "philox"): (0.0, 4 * 3.874e-07),
              ("precise", "knots"): (0.0, 4 * 1.192e-07), ("precise", "philox"): (0.0, 4 * 1.192e-07)}


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-edges] " + text)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model_of(name):
    """"golden": tests/golden/gru_c5.npz.  "random": the weights of test_gru_random_weights_vs_oracle at scale 0.3 (SFC64(30)),
    input and output normalisation included."""
    if name == "golden":
        g = np.load(GOLDEN)
        return {k: g[k] for k in g.files if k not in ("s0", "Q", "h0", "traj", "h_final")}
    scale = 0.3
    rng = np.random.Generator(np.random.SFC64(30))
    u = lambda *s: (scale * rng.uniform(-1, 1, s)).astype(f32)  # noqa: E731
    return dict(w_ih0=u(96, 6), w_hh0=u(96, 32), b_ih0=u(96), b_hh0=u(96), w_ih1=u(96, 32), w_hh1=u(96, 32), b_ih1=u(96),
                b_hh1=u(96), w_out=(0.3 * rng.uniform(-1, 1, (5, 32))).astype(f32), b_out=(0.1 * rng.uniform(-1, 1, 5)).astype(f32),
                in_scale=rng.uniform(0.5, 2.0, 6).astype(f32), in_shift=(0.1 * rng.uniform(-1, 1, 6)).astype(f32),
                out_scale=rng.uniform(0.5, 1.5, 5).astype(f32), out_shift=(0.05 * rng.uniform(-1, 1, 5)).astype(f32))


def engine(E, N, H, model="golden", **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, **kw))
    eng.set_gru(model_of(model))
    return eng


def oracle_cfg(N, H, period=10, cost="quadratic_boundary_grad_minimal", **flags):
    return O.MPPIConfig(N=N, H=H, period=period, cost_id=COSTS[cost], **flags)


def oracle_pair(model, s, u0, du, tp, cfg, h0, low=-1.0, high=1.0, te=1.0):
    """The oracle's GRU MPPI step for one env in float32 and float64 (te: that env's target equilibrium)."""
    a = O.gru_mppi_step(model_of(model), s, u0, du, f32(tp), f32(te), cfg, h0=h0, low=low, high=high)
    b = O.gru_mppi_step(model_of(model), s, u0, du, f32(tp), f32(te), cfg, h0=h0, low=low, high=high, dtype=np.float64)
    return a, b


def cost_flags(ref32, ref64, cost, tp):
    fl = PU.flag_rounding_sensitive(ref32["S"], ref64["S"])
    if cost == "default":
        fl = fl | PU.flag_indicators(ref32["traj"], "default", tp)
    return fl


def hanging_default(cost, te):
    """default.py's cost with the hanging target: its angle term is negative, and rollout_matrix.buckets hands the verdict on
    such costs to tools/dev/hanging_target.py."""
    return cost == "default" and te < 0


def check_env(S, un, Q, ref32, ref64, du, cost, tp, what, te=1.0, horizon_reduce="sum"):
    """One env of a step against the oracle pair under the module's bounds -> (worst excess of a clear rollout, worst |u_nom - u32|).
    `default` with te < 0: the costs' verdict is hanging_default_buckets, as in rollout_matrix.buckets (flags: the indicators)."""
    if hanging_default(cost, te):
        from rollout_matrix import hanging_target
        fl = PU.flag_indicators(ref32["traj"], "default", tp)
        assert fl.mean() <= 0.05, f"{what}: {int(fl.sum())} of {fl.size} rollouts flagged"
        b = hanging_target().assert_hanging_default_costs(S, ref32["S"], ref64["S"], fl, f"{what} costs (hanging target)",
                                                          H=du.shape[1], horizon_reduce=horizon_reduce)
    else:
        fl = cost_flags(ref32, ref64, cost, tp)
        assert fl.mean() <= 0.05, f"{what}: {int(fl.sum())} of {fl.size} rollouts flagged"
        b = PU.assert_costs(S, ref32["S"], ref64["S"], fl, f"{what} costs")
    allow = PU.softmin_allowance(ref32["S"], ref64["S"], du, LBD=100.0)
    PU.assert_controls(un, ref32["u_new"], ref64["u_new"], f"{what} u_nom", allowance=allow)
    PU.assert_controls(Q, ref32["Q"], ref64["Q"], f"{what} Q", allowance=allow[0])
    clear = ~b["flagged"]
    return (float(b["excess"][clear].max()) if clear.any() else 0.0), float(np.abs(un - ref32["u_new"]).max())


def draw_env(rng, H, u_scale, h_scale=0.2):
    """One env's inputs in the order test_glue_flags_vs_oracle fixes: state, target position, nominal sequence, memory."""
    s = O.create_cartpole_state(rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2))
    tp = f32(rng.uniform(-0.05, 0.05))
    u0 = (u_scale * rng.standard_normal(H)).astype(f32)
    h0 = (h_scale * rng.standard_normal((2, 32))).astype(f32)
    return s, tp, u0, h0


def circle(d):
    """|d| for a difference of states [..., 6], the angle's on the circle."""
    d = np.abs(np.array(d, np.float64))
    a = d[..., O.ANGLE_IDX] % (2 * np.pi)
    d[..., O.ANGLE_IDX] = np.minimum(a, 2 * np.pi - a)
    return d


# ---- the predict seam
@functools.lru_cache(maxsize=None)
def predict_case(model, B, H):
    rng = np.random.Generator(np.random.SFC64(100 * B + H))
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-3, 3), rng.uniform(-8, 8), rng.uniform(-0.19, 0.19), rng.uniform(-0.8, 0.8))
                   for _ in range(B)])
    Q = rng.uniform(-1, 1, (B, H)).astype(f32)
    h0 = (0.5 * rng.standard_normal((2, B, 32))).astype(f32)
    refs = {}
    for key, h in (("h0", h0), ("zero", None)):
        refs[key] = (O.gru_predict(model_of(model), s0, Q, h), O.gru_predict(model_of(model), s0, Q, h, dtype=np.float64))
    return s0, Q, h0, refs


@functools.lru_cache(maxsize=None)
def predict_engine(model):
    return engine(1, 64, 8, model)


@pytest.mark.parametrize("H", [1, 2, 7])
@pytest.mark.parametrize("B", [1, 31, 33, 128, 129, 300])
@pytest.mark.parametrize("model", ["golden", "random"])
def test_predict_seam_across_blocks_and_tails(model, B, H, capsys):
    """gru_predict_kernel with rows that all differ: one row, a tile less one, a tile plus one, a full block, a second block with one
    live row, a tail in the third block; H = 1 (no next control to feed), 2 and 7; with a memory [2, B, 32] and without.  Trajectory
    and final hidden state against the oracle; for B = 33 and 129 once more through the C entry point into caller-owned buffers
    with 64 sentinel rows behind traj and behind h_out."""
    from cartpolesimulation_amd.engine import _ptr
    s0, Q, h0, refs = predict_case(model, B, H)
    eng = predict_engine(model)
    worst_s = worst_h = 0.0
    for key, h in (("h0", h0), ("zero", None)):
        traj, hfin = eng.gru_predict(s0, Q, h0=h, return_hidden=True)
        traj, hfin = traj.cpu().numpy(), hfin.cpu().numpy()
        assert traj.shape == (B, H + 1, 6) and hfin.shape == (2, B, 32)
        assert np.array_equal(bits(traj[:, 0]), bits(s0))
        (t32, h32), (t64, h64) = refs[key]
        d, gap = circle(traj - t32), circle(t32 - t64)
        assert np.all(d <= 1e-4 + gap), f"{key}: states off by {np.max(d - gap):.2e} at row {np.argmax((d - gap).max(axis=(1, 2)))}"
        dh, gh = np.abs(hfin - h32), np.abs(h32 - h64)
        assert np.all(dh <= 1e-4 + gh), f"{key}: hidden off by {dh.max():.2e} at row {np.argmax(dh.max(axis=(0, 2)))}"
        worst_s, worst_h = max(worst_s, float(d.max())), max(worst_h, float(dh.max()))
        if B in (33, 129):
            SENT = f32(-7.25)
            traj_buf = torch.full((B + 64, H + 1, 6), float(SENT), dtype=torch.float32, device=eng.device)
            h_buf = torch.full((2 * B + 64, 32), float(SENT), dtype=torch.float32, device=eng.device)
            s_t, Q_t, h_t = eng.tensor(s0), eng.tensor(Q), eng.tensor(h)
            eng._check(eng.lib.cpmppi_gru_predict(eng._h, B, H, _ptr(s_t), _ptr(Q_t), _ptr(h_t), _ptr(traj_buf), _ptr(h_buf),
                                                  eng._stream()))
            tb, hb = traj_buf.cpu().numpy(), h_buf.cpu().numpy()
            assert np.all(tb[B:] == SENT), "rows behind traj were written"
            assert np.all(hb[2 * B:] == SENT), "rows behind h_out were written"
            assert np.array_equal(bits(tb[:B]), bits(traj))
            assert np.array_equal(bits(hb[:2 * B].reshape(2, B, 32)), bits(hfin))
    report(capsys, f"item1 {model} B {B} H {H}: state {worst_s:.2e} hidden {worst_h:.2e}")


# ---- glue flags
GLUE = [dict(control_mode="clip", shift_mode="repeat_last", correction_u="u_run", horizon_reduce="sum"),
        dict(control_mode="penalise", shift_mode="append_zero", correction_u="u_nom", horizon_reduce="sum"),
        dict(control_mode="clip", shift_mode="none", correction_u="u_nom", horizon_reduce="mean"),
        dict(control_mode="penalise", shift_mode="repeat_last", correction_u="u_run", horizon_reduce="mean"),
        dict(control_mode="clip", shift_mode="append_zero", correction_u="u_run", horizon_reduce="mean"),
        dict(control_mode="penalise", shift_mode="none", correction_u="u_nom", horizon_reduce="sum")]
G_E, G_N, G_H, G_PERIOD, G_LOW, G_HIGH = 2, 130, 11, 5, -0.7, 0.9


@functools.lru_cache(maxsize=None)
def glue_inputs(ci):
    rng = np.random.Generator(np.random.SFC64(100 + ci))
    stdev = oracle_cfg(G_N, G_H).stdev
    envs = []
    for _ in range(G_E):
        s, tp, u0, h0 = draw_env(rng, G_H, 0.4)
        envs.append((s, tp, u0, h0, O.sample_delta_u(rng, G_N, G_H, 3 * stdev, G_PERIOD)))
    return [np.stack([e[i] for e in envs]) for i in range(5)]


@functools.lru_cache(maxsize=None)
def glue_reference(model, ci, cost):
    s0, tp, u0, h0, du = glue_inputs(ci)
    cfg = oracle_cfg(G_N, G_H, G_PERIOD, cost, **GLUE[ci])
    return [oracle_pair(model, s0[e], u0[e], du[e], tp[e], cfg, h0[e], G_LOW, G_HIGH) for e in range(G_E)]


def flags_act(ci, u_run):
    """Share of the oracle's u_run entries on which the control_mode of combination ci visibly acts."""
    if GLUE[ci]["control_mode"] == "clip":
        return float(np.mean((u_run == f32(G_LOW)) | (u_run == f32(G_HIGH))))
    return float(np.mean(np.abs(u_run) > 1.0))


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("ci", range(len(GLUE)))
@pytest.mark.parametrize("model", ["golden", "random"])
def test_glue_flags_vs_oracle(model, ci, cost, math_mode, capsys):
    """The GRU kernel's own copies of the control_mode, correction_u, horizon_reduce and shifted_nominal statements, with limits
    other than +-1 and a knot period of 5 at H = 11: 2 envs x 130 rollouts (a second block with two live rows), host perturbations
    of three times the configured spread so that clipping and overshoot are common."""
    s0, tp, u0, h0, du = glue_inputs(ci)
    eng = engine(G_E, G_N, G_H, model, period_interpolation_inducing_points=G_PERIOD, action_low=G_LOW, action_high=G_HIGH,
                 cost_function_specification=cost, math_mode=math_mode, **GLUE[ci])
    un, S = eng.tensor(u0.copy()), eng.empty(G_E, G_N)
    Q, _ = eng.step(s0, un, tp, np.ones(G_E, f32), S_out=S, predictor="GRU", h0=h0, delta_u=du)
    un, S, Q = un.cpu().numpy(), S.cpu().numpy(), Q.cpu().numpy()
    worst = [0.0, 0.0]
    for e, (r32, r64) in enumerate(glue_reference(model, ci, cost)):
        assert flags_act(ci, r32["u_run"]) >= 0.05, f"env {e}: {GLUE[ci]['control_mode']} acts on {flags_act(ci, r32['u_run']):.3f} only"
        x, d = check_env(S[e], un[e], Q[e], r32, r64, du[e], cost, tp[e], f"{model} glue {ci} {cost} {math_mode} env {e}")
        worst = [max(worst[0], x), max(worst[1], d)]
    report(capsys, f"item2 {model} ci {ci} {cost} {math_mode}: excess {worst[0]:.3f} u_nom {worst[1]:.2e}")
    eng.close()


# ---- ragged rollout counts
RAGGED_N = [1, 5, 31, 32, 33, 127, 128, 129, 257]


def step_with_source(eng, source, s0, u0, tp, h0, kn, du, seed, offset, env_offset=0):
    E = s0.shape[0]
    kw = {"delta_u": dict(delta_u=du), "knots": dict(knots=kn), "philox": dict(seed=seed, offset=offset, env_offset=env_offset)}[source]
    un, S = eng.tensor(u0.copy()), eng.empty(E, eng.N)
    Q, _ = eng.step(s0, un, tp, np.ones(E, f32), S_out=S, predictor="GRU", h0=h0, **kw)
    return S.cpu().numpy(), un.cpu().numpy(), Q.cpu().numpy()


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("case", range(len(RAGGED_N)))
def test_ragged_rollout_counts_vs_oracle(case, math_mode, capsys):
    """owner / nn / rows / nb of the rollout kernel: N around the 32-rollout tile and the 128-rollout block, down to one rollout;
    3 envs, H = 3 = the knot period; the noise source rotates over delta_u, knots and Philox with the case."""
    N, E, H = RAGGED_N[case], 3, 3
    source = ("delta_u", "knots", "philox")[case % 3]
    eng = engine(E, N, H, period_interpolation_inducing_points=3, math_mode=math_mode)
    rng = np.random.Generator(np.random.SFC64(300 + N))
    s0, tp, u0, h0 = (np.stack(x) for x in zip(*[draw_env(rng, H, 0.2) for _ in range(E)]))
    kn, du = eng.sample(seed=3, offset=1, knots=True, delta_u=True)
    S, un, Q = step_with_source(eng, source, s0, u0, tp, h0, kn, du, 3, 1)
    du = du.cpu().numpy()
    cfg = oracle_cfg(N, H, 3)
    worst = [0.0, 0.0]
    for e in range(E):
        r32, r64 = oracle_pair("golden", s0[e], u0[e], du[e], tp[e], cfg, h0[e])
        x, d = check_env(S[e], un[e], Q[e], r32, r64, du[e], "quadratic_boundary_grad_minimal", tp[e], f"N {N} {source} {math_mode} env {e}")
        worst = [max(worst[0], x), max(worst[1], d)]
        if N == 1:                                               # one rollout: the update is that rollout's controls
            shifted = np.concatenate([u0[e, 1:], u0[e, -1:]])
            assert np.abs(un[e] - np.clip(shifted + du[e, 0], -1.0, 1.0)).max() <= 1e-6
    report(capsys, f"item3 N {N} {source} {math_mode}: excess {worst[0]:.3f} u_nom {worst[1]:.2e}")
    eng.close()


# ---- noise sources at other periods
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("period,H", [(1, 10), (3, 26), (10, 1), (10, 26)])
def test_noise_sources_agree_at_other_periods(period, H, cost, math_mode, capsys):
    """A knot on every step, a period that does not divide H, a horizon of one step inside one period, and the shipped period at an
    H it does not divide: the sampler's delta_u, its knots and the in-kernel Philox stream of the same seed / offset / env offset
    are the same step - each against the oracle on that delta_u, and against one another."""
    E, N, seed, offset, env_offset = 2, 100, 11, 5, 7
    eng = engine(E, N, H, period_interpolation_inducing_points=period, cost_function_specification=cost, math_mode=math_mode)
    rng = np.random.Generator(np.random.SFC64(400 + 10 * period + H))
    s0, tp, u0, h0 = (np.stack(x) for x in zip(*[draw_env(rng, H, 0.2) for _ in range(E)]))
    kn, du = eng.sample(seed=seed, offset=offset, env_offset=env_offset, knots=True, delta_u=True)
    assert kn.shape == (E, N, -(-H // period) + 1)
    out = {src: step_with_source(eng, src, s0, u0, tp, h0, kn, du, seed, offset, env_offset) for src in ("delta_u", "knots", "philox")}
    du = du.cpu().numpy()
    cfg = oracle_cfg(N, H, period, cost)
    worst = [0.0, 0.0]
    for e in range(E):
        r32, r64 = oracle_pair("golden", s0[e], u0[e], du[e], tp[e], cfg, h0[e])
        for src, (S, un, Q) in out.items():
            x, d = check_env(S[e], un[e], Q[e], r32, r64, du[e], cost, tp[e], f"period {period} H {H} {cost} {math_mode} {src} env {e}")
            worst = [max(worst[0], x), max(worst[1], d)]
    S0, u_0, _ = out["delta_u"]
    dS = {src: float(np.max(np.abs(out[src][0] - S0) / np.abs(S0))) for src in ("knots", "philox")}
    du_nom = {src: float(np.abs(out[src][1] - u_0).max()) for src in ("knots", "philox")}
    words = {src: int((bits(out[src][0]) != bits(S0)).sum()) for src in ("knots", "philox")}
    report(capsys, f"item4 period {period} H {H} {cost} {math_mode}: excess {worst[0]:.3f} u_nom {worst[1]:.2e}; "
                   f"sources: S rel {max(dS.values()):.3e} u_nom {max(du_nom.values()):.3e}, S words differing {words}")
    for src in ("knots", "philox"):
        tol_S, tol_u = SOURCE_TOL[math_mode, src]
        assert tol_S <= 1e-4 and tol_u <= 1e-4
        if tol_S == 0.0:
            assert words[src] == 0, f"{src}: {words[src]} costs differ from the delta_u step's"
        assert dS[src] <= tol_S and du_nom[src] <= tol_u, (src, dS[src], du_nom[src])
    eng.close()


# ---- step counter and output routing
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_device_step_counter_and_output_routing(math_mode):
    """The GRU branch of the step with Philox noise: three steps on the device step counter equal three steps at host offsets
    0, 1, 2 bit for bit (S, u_nom, Q after each) and leave the word at 3; u_nom_out receives what the in-place step writes and
    leaves u_nom alone; S_out = NULL changes neither u_nom nor Q."""
    E, N, H, seed = 2, 130, 11, 21
    eng = engine(E, N, H, math_mode=math_mode)
    rng = np.random.Generator(np.random.SFC64(500))
    s0, tp, u0, h0 = (np.stack(x) for x in zip(*[draw_env(rng, H, 0.2) for _ in range(E)]))
    te = np.ones(E, f32)

    def run(un, **kw):
        S = eng.empty(E, N)
        Q, _ = eng.step(s0, un, tp, te, S_out=S, predictor="GRU", h0=h0, seed=seed, env_offset=3, **kw)
        return S.cpu().numpy(), Q.cpu().numpy()

    counter = torch.zeros(1, dtype=torch.int64, device=eng.device)
    un_dev, un_host = eng.tensor(u0.copy()), eng.tensor(u0.copy())
    seen = []
    for k in range(3):
        S_d, Q_d = run(un_dev, offset_dev=counter)
        S_h, Q_h = run(un_host, offset=k)
        assert np.array_equal(bits(S_d), bits(S_h)), f"step {k}: S"
        assert np.array_equal(bits(Q_d), bits(Q_h)), f"step {k}: Q"
        assert np.array_equal(bits(un_dev.cpu().numpy()), bits(un_host.cpu().numpy())), f"step {k}: u_nom"
        seen.append(S_h)
    assert int(counter.item()) == 3
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])     # the offset reaches the noise
    # u_nom_out
    un_in, un_out = eng.tensor(u0.copy()), eng.empty(E, H).fill_(123.0)
    S_o, Q_o = run(un_in, offset=0, u_nom_out=un_out)
    un_ref = eng.tensor(u0.copy())
    S_r, Q_r = run(un_ref, offset=0)
    assert np.array_equal(bits(un_in.cpu().numpy()), bits(u0))
    assert np.array_equal(bits(un_out.cpu().numpy()), bits(un_ref.cpu().numpy()))
    assert np.array_equal(bits(S_o), bits(S_r)) and np.array_equal(bits(Q_o), bits(Q_r))
    assert not np.array_equal(un_ref.cpu().numpy(), u0)
    # S_out = NULL
    un_n = eng.tensor(u0.copy())
    Q_n, S_none = eng.step(s0, un_n, tp, te, predictor="GRU", h0=h0, seed=seed, env_offset=3, offset=0)
    assert S_none is None
    assert np.array_equal(bits(un_n.cpu().numpy()), bits(un_ref.cpu().numpy())) and np.array_equal(bits(Q_n.cpu().numpy()), bits(Q_r))
    eng.close()


# ---- the batched optimizer
def test_batched_optimizer_with_the_gru(capsys):
    """optimizer_mppi with three envs and the network in the loop: the memory [E, 2, 32] goes through gru_predict as [2, E, 32] and
    back.  Three states, three targets, four steps; after each, every env's u_nom and control against the oracle on the sampler's
    perturbations and the test's own running memory, and the optimizer's memory against the oracle's."""
    from types import SimpleNamespace
    from cartpolesimulation_amd.optimizer_mppi import optimizer_mppi
    E, N, H, seed = 3, 130, 11, 4
    model = model_of("golden")
    vp = SimpleNamespace(target_position=np.array([-0.05, 0.0, 0.04], f32), target_equilibrium=np.ones(E, f32))
    opt = optimizer_mppi(control_limits=(np.array([-1.0]), np.array([1.0])), num_envs=E, gru_model=model, noise="philox",
                         num_rollouts=N, mpc_horizon=H, seed=seed, variable_parameters=vp)
    opt.configure(dt=0.02, predictor_specification="GRU-6IN-32H1-32H2-5OUT-0")
    cfg = oracle_cfg(N, H)
    s = np.stack([O.create_cartpole_state(0.3, -0.5, 0.02, 0.1), O.create_cartpole_state(-0.4, 1.0, -0.05, -0.1),
                  O.create_cartpole_state(0.1, 0.3, 0.08, 0.15)])
    u_ref, h_ref = np.zeros((E, H), f32), np.zeros((E, 2, 32), f32)
    worst_u = worst_h = 0.0
    for it in range(4):
        u = opt.step(s)
        assert u.shape == (E, 1)
        du = opt.engine.sample(seed=seed, offset=it, knots=False, delta_u=True)[1].cpu().numpy()
        un, hd = opt.u_nom.cpu().numpy(), opt.h.cpu().numpy()
        assert hd.shape == (E, 2, 32)
        for e in range(E):
            r32, r64 = oracle_pair("golden", s[e], u_ref[e], du[e], vp.target_position[e], cfg, h_ref[e])
            fl = cost_flags(r32, r64, "quadratic_boundary_grad_minimal", vp.target_position[e])
            assert fl.mean() <= 0.05
            allow = PU.softmin_allowance(r32["S"], r64["S"], du[e], LBD=100.0)
            PU.assert_controls(un[e], r32["u_new"], r64["u_new"], f"step {it} env {e} u_nom", allowance=allow)
            PU.assert_controls(u[e, 0], r32["Q"], r64["Q"], f"step {it} env {e} control", allowance=allow[0])
            worst_u = max(worst_u, float(np.abs(un[e] - r32["u_new"]).max()))
            u_ref[e] = r32["u_new"]
            q = np.array([[u[e, 0]]], f32)                     # the memory advances under the control the optimizer applied
            h32 = O.gru_predict(model, s[e][None], q, h_ref[e][:, None, :])[1][:, 0]
            h64 = O.gru_predict(model, s[e][None], q, h_ref[e][:, None, :], dtype=np.float64)[1][:, 0]
            dh = np.abs(hd[e] - h32)
            assert np.all(dh <= 1e-4 + np.abs(h32 - h64)), f"step {it} env {e}: memory off by {dh.max():.2e}"
            worst_h = max(worst_h, float(dh.max()))
            h_ref[e] = h32
        if it == 0:                                              # envs whose memories agreed would hide a transpose slip
            for a, b in ((0, 1), (0, 2), (1, 2)):
                for layer in range(2):
                    assert np.abs(h_ref[a, layer] - h_ref[b, layer]).max() > 1e-3
        s = np.stack([O.ode_v0_step(s[e][None], u[e].astype(f32))[0] for e in range(E)])
    report(capsys, f"item6: u_nom {worst_u:.2e} memory {worst_h:.2e}")


# ---- a fixed random cut
def test_random_gru_configurations_regression():
    """A fixed cut of tools/dev/gru_shape_fuzz.py (24 random shape / period / cost / glue flag / action limit / noise source / math
    mode / weight configurations, seed 7) stays inside that tool's rules."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "dev", "gru_shape_fuzz.py"), "--n", "24", "--seed", "7"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    summary = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert summary == {"configurations": 24, "passed": 24, "failed": 0, "seed": 7}, r.stdout[-3000:]
