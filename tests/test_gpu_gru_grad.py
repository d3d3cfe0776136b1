"""GPU: cpmppi_rollout_cost_grad_gru - the gradient of the GRU rollout cost with respect to the inputs - against float64 autograd of
the oracle's function (tests/gru_grad_ref.py, pinned on the CPU by tests/test_gru_grad_ref_host.py), with the statements around
it: the last input's closed form, bit identity with the cost-only launch, rows beyond N, refusals, capture, descent, and the four
gradient-family optimizers with ``gru_adjoint=True``.

Bounds of the gradient comparison are tests/test_gpu_grad.py's, the error relative to each rollout's max |g|: every unflagged
rollout < 5e-4, median < 1e-4, flagged rollouts beyond 2e-3 at most 5 % of the flagged, S within rtol 5e-4.  Float32 torch autograd
of the same function sits at worst 3.2e-5 (medians <= 1.3e-6) against float64.

Measured on the MI355X (this module's first run; worst over the shapes of a model / cost pair, sum and mean, with and without a
memory; the forward sweep runs the split-f16 cell under FAST and the exact-f32 chains under PRECISE, the reverse exact f32 in both):
  model / cost                                   unflagged, FAST   PRECISE     median (worst)   flagged    S relative
  golden / quadratic_boundary_grad_minimal       2.28e-05          1.16e-05    1.02e-06         1.45e-06   2.52e-06
  golden / default                               2.17e-05          1.57e-05    1.71e-06         2.29e-06   1.20e-06
  random / quadratic_boundary_grad_minimal       1.41e-04          3.31e-04    3.07e-06         1.94e-06   6.98e-05
(per shape: profiles/r10/gradient_accuracy.txt).  The last input's gradient equals the closed form within 4 float32 epsilons,
S_out equals the cost-only launch bit for bit in both math modes, descent: every plan cheaper, mean cost ratio 0.625
(quadratic_boundary_grad_minimal) and 0.408 (default); the optimizers' memory is within 1.04e-07 of the oracle's.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import gru_grad_ref as R  # noqa: E402
from test_gpu_gru_edges import bits, draw_env, engine, model_of  # noqa: E402

f32 = np.float32
SENT = f32(-7.25)


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-grad] " + text)


def call_grad(eng, E, s0, inputs, tp, te, h0, S, grad):
    """The C entry point itself, on device tensors (None = NULL)."""
    from cartpolesimulation_amd.engine import _ptr
    return eng.lib.cpmppi_rollout_cost_grad_gru(eng._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(h0), _ptr(S), _ptr(grad),
                                                eng._stream())


# ---- 1. the gradient against float64 autograd
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("E,N,H", R.SHAPES)
@pytest.mark.parametrize("model,cost", R.PAIRS)
def test_gradient_vs_float64_autograd(model, cost, E, N, H, math_mode, capsys):
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    te = np.ones(E, f32)
    worst = dict(clear=0.0, flagged=0.0, S=0.0, median=0.0)
    for reduce in ("sum", "mean"):
        eng = engine(E, N, H, model, cost_function_specification=cost, math_mode=math_mode, horizon_reduce=reduce)
        for with_h0 in (True, False):
            S, G = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h0 if with_h0 else None)
            S, G = S.cpu().numpy(), G.cpu().numpy()
            J, g, flagged = R.case_reference(model, cost, E, N, H, with_h0, reduce)
            beyond = np.abs(Q) > 1.0
            assert np.all(G[beyond] == 0.0) and np.all(g[beyond] == 0.0)
            scale = np.abs(g).max(axis=2) + 1e-6
            err = np.abs(G - g).max(axis=2) / scale
            n_fl, n_fl_off = int(flagged.sum()), int(((err >= 2e-3) & flagged).sum())
            worst["clear"] = max(worst["clear"], float(err[~flagged].max()))
            worst["flagged"] = max(worst["flagged"], float(err[flagged].max()) if n_fl else 0.0)
            worst["S"] = max(worst["S"], float((np.abs(S - J) / np.abs(J)).max()))
            worst["median"] = max(worst["median"], float(np.median(err)))
            report(capsys, f"item1 {model} {cost} {(E, N, H)} {math_mode} {reduce} h0 {with_h0}: worst clear {err[~flagged].max():.2e} "
                           f"median {np.median(err):.2e} flagged {n_fl} ({n_fl_off} beyond 2e-3) S rel {(np.abs(S - J) / np.abs(J)).max():.2e}")
            np.testing.assert_allclose(S, J, rtol=5e-4)
            clear_off = int(((err >= 5e-4) & ~flagged).sum())
            assert clear_off == 0, f"{clear_off} of {int((~flagged).sum())} unflagged rollouts differ by more than 5e-4 (worst {err[~flagged].max():.2e})"
            assert np.median(err) < 1e-4
            assert n_fl_off <= int(np.ceil(0.05 * n_fl)), f"{n_fl_off} of {n_fl} flagged rollouts outside 2e-3"
        eng.close()
    report(capsys, f"item1 {model} {cost} {(E, N, H)} {math_mode}: WORST clear {worst['clear']:.2e} median {worst['median']:.2e} "
                   f"flagged {worst['flagged']:.2e} S {worst['S']:.2e}")


# ---- 2. the last input's gradient in closed form
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("N,H", [(33, 7), (300, 1)])
def test_last_input_gradient_is_the_control_term_alone(N, H, reduce, math_mode):
    """The state after the last control step is never costed under quadratic_boundary_grad_minimal, so d S / d Q[H-1] is the direct
    term 2 cc_weight R u (over H + 1 under `mean`), to float32 rounding; H = 1 is the whole gradient."""
    E = 2 if N == 33 else 1
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    eng = engine(E, N, H, "golden", math_mode=math_mode, horizon_reduce=reduce)
    _, G = eng.rollout_cost_grad(s0, Q, tp, np.ones(E, f32), predictor="GRU", h0=h0)
    G = G.cpu().numpy()
    c = O.DEFAULT_COST
    u = Q[:, :, H - 1].astype(np.float64)
    want = 2.0 * float(c.qbgm_cc_weight) * float(c.qbgm_R) * u / ((H + 1) if reduce == "mean" else 1.0)
    want[np.abs(u) > 1.0] = 0.0
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(G[:, :, H - 1], want, rtol=4 * np.finfo(f32).eps, atol=0.0)
    eng.close()


# ---- 3. same statements, same bits
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("cost", list(R.COSTS))
def test_costs_are_the_cost_only_launch_and_S_out_is_optional(cost, math_mode):
    E, N, H = 2, 129, 7
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    eng = engine(E, N, H, cost_function_specification=cost, math_mode=math_mode)
    te = np.ones(E, f32)
    s_t, in_t, tp_t, te_t, h_t = eng.tensor(s0), eng.tensor(Q), eng.tensor(tp), eng.tensor(te), eng.tensor(h0)
    for h, hd in ((h0, h_t), (None, None)):
        S, G = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h)
        S_cost = eng.rollout_cost(s0, Q, tp, te, predictor="GRU", h0=h)
        assert np.isfinite(S.cpu().numpy()).all() and np.array_equal(S.cpu().numpy(), S_cost.cpu().numpy())
        assert np.array_equal(bits(S.cpu().numpy()), bits(S_cost.cpu().numpy()))
        G2 = torch.full((E, N, H), float(SENT), dtype=torch.float32, device=eng.device)
        assert call_grad(eng, E, s_t, in_t, tp_t, te_t, hd, None, G2) == 0, eng.lib.cpmppi_last_error(eng._h)
        assert np.array_equal(bits(G2.cpu().numpy()), bits(G.cpu().numpy()))
    eng.close()


# ---- 4. nothing beyond N or the buffers
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("N", [33, 129])
def test_rows_behind_the_buffers_stay_untouched(N, math_mode):
    """A direct C call of E = 2 envs on a handle built for 3 into caller-owned S [2 N + 64] and grad [2 N + 64, H] of sentinels."""
    E, H = 2, 7
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    eng = engine(E + 1, N, H, math_mode=math_mode)
    s_t, in_t, tp_t, te_t, h_t = eng.tensor(s0), eng.tensor(Q), eng.tensor(tp), eng.tensor(np.ones(E, f32)), eng.tensor(h0)
    S = torch.full((E * N + 64,), float(SENT), dtype=torch.float32, device=eng.device)
    G = torch.full((E * N + 64, H), float(SENT), dtype=torch.float32, device=eng.device)
    assert call_grad(eng, E, s_t, in_t, tp_t, te_t, h_t, S, G) == 0, eng.lib.cpmppi_last_error(eng._h)
    So, Go = S.cpu().numpy(), G.cpu().numpy()
    assert np.all(So[E * N:] == SENT), "rows behind S were written"
    assert np.all(Go[E * N:] == SENT), "rows behind grad were written"
    S2, G2 = eng.rollout_cost_grad(s0, Q, tp, np.ones(E, f32), predictor="GRU", h0=h0)
    assert np.array_equal(bits(So[:E * N].reshape(E, N)), bits(S2.cpu().numpy()))
    assert np.array_equal(bits(Go[:E * N].reshape(E, N, H)), bits(G2.cpu().numpy()))
    assert not np.any(Go[:E * N] == SENT)
    eng.close()


# ---- 5. refusals
@pytest.mark.parametrize("case", ["no model", "E zero", "E beyond cfg.E", "NULL s0", "NULL inputs", "NULL target_position",
                                  "NULL target_equilibrium", "NULL grad_out", "legacy cost", "quadratic_boundary_grad cost",
                                  "quadratic_boundary cost"])
def test_refusals_launch_nothing(case):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 33, 5
    cost = {"legacy cost": "legacy_mppi_cartpole", "quadratic_boundary_grad cost": "quadratic_boundary_grad",
            "quadratic_boundary cost": "quadratic_boundary"}.get(case, "default")
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, cost_function_specification=cost))
    if case != "no model":
        eng.set_gru(model_of("golden"))
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    s_t, in_t, tp_t, te_t = eng.tensor(s0), eng.tensor(Q), eng.tensor(tp), eng.tensor(np.ones(E, f32))
    S = torch.full((E + 1, N), float(SENT), dtype=torch.float32, device=eng.device)
    G = torch.full((E + 1, N, H), float(SENT), dtype=torch.float32, device=eng.device)
    args = dict(E=E, s0=s_t, inputs=in_t, tp=tp_t, te=te_t, h0=None, S=S, grad=G)
    args.update({"E beyond cfg.E": dict(E=E + 1), "E zero": dict(E=0), "NULL s0": dict(s0=None), "NULL inputs": dict(inputs=None),
                 "NULL target_position": dict(tp=None), "NULL target_equilibrium": dict(te=None),
                 "NULL grad_out": dict(grad=None)}.get(case, {}))
    rc = call_grad(eng, *(args[k] for k in ("E", "s0", "inputs", "tp", "te", "h0", "S", "grad")))
    torch.cuda.synchronize()
    assert rc == -1
    msg = eng.lib.cpmppi_last_error(eng._h).decode()
    assert msg.startswith("cpmppi_rollout_cost_grad_gru: "), msg
    want = {"no model": "no model set", "E zero": "E out of range", "E beyond cfg.E": "E out of range"}.get(
        case, "supports quadratic_boundary_grad_minimal and default" if case.endswith("cost") else "are required")
    assert want in msg, msg
    assert np.all(S.cpu().numpy() == SENT) and np.all(G.cpu().numpy() == SENT), "a refused call wrote"
    if case == "no model":                                       # the engine method words its own refusals before any library call
        te = np.ones(E, f32)
        with pytest.raises(ValueError, match="takes no L"):
            eng.rollout_cost_grad(s0, Q, tp, te, L=np.full(E, 0.4, f32), predictor="GRU")
        with pytest.raises(ValueError, match="takes no previous_input"):
            eng.rollout_cost_grad(s0, Q, tp, te, previous_input=np.zeros(E, f32), predictor="GRU")
        with pytest.raises(ValueError, match="memory of the GRU"):
            eng.rollout_cost_grad(s0, Q, tp, te, h0=np.zeros((E, 2, 32), f32))
        with pytest.raises(CpmppiError, match="cpmppi_rollout_cost_grad_gru: no model set"):
            eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU")
    eng.close()


# ---- 6. capture
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_capture_replays_bit_identically_and_a_fresh_handle_is_refused(math_mode):
    """On a fresh handle the call under capture would have to allocate its check-points: refused by name, the capture goes on.  After
    one warm call the two launches are captured and replayed with new values in the same buffers, bit-equal to the eager call."""
    E, N, H = 2, 129, 7
    eng = engine(E, N, H, math_mode=math_mode)
    draws = [R.case_inputs(E, N, H)]
    rng = np.random.Generator(np.random.SFC64(8100))
    envs = []
    for _ in range(E):
        s, tp, _, h0 = draw_env(rng, H, 0.2)
        envs.append((s, tp, h0, rng.uniform(-1.2, 1.2, (N, H)).astype(f32)))
    draws.append(tuple(np.stack([e[i] for e in envs]) for i in range(4)))
    te = np.ones(E, f32)
    s0, tp, h0, Q = draws[0]
    s_t, tp_t, h_t, in_t = (eng.tensor(x.copy()) for x in (s0, tp, h0, Q))
    te_t = eng.tensor(te)
    S = torch.full((E, N), float(SENT), dtype=torch.float32, device=eng.device)
    G = torch.full((E, N, H), float(SENT), dtype=torch.float32, device=eng.device)
    marker = eng.zeros(4)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g0, stream=side):
            assert call_grad(eng, E, s_t, in_t, tp_t, te_t, h_t, S, G) == -1
            msg = eng.lib.cpmppi_last_error(eng._h).decode()
            marker.add_(1.0)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    assert msg.startswith("cpmppi_rollout_cost_grad_gru: the stream is being captured"), msg
    g0.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.all(G.cpu().numpy() == SENT) and np.all(S.cpu().numpy() == SENT)
    # warm: the workspace exists from here on
    eager = [tuple(x.cpu().numpy() for x in eng.rollout_cost_grad(a, d, b, te, predictor="GRU", h0=c)) for a, b, c, d in draws]
    assert not np.array_equal(eager[0][1], eager[1][1])
    g1 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g1, stream=side):
            assert call_grad(eng, E, s_t, in_t, tp_t, te_t, h_t, S, G) == 0, eng.lib.cpmppi_last_error(eng._h)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    torch.cuda.synchronize()
    assert np.all(G.cpu().numpy() == SENT)                       # captured, not run
    for k in (1, 0):
        for dst, src in zip((s_t, tp_t, h_t, in_t), draws[k]):
            dst.copy_(torch.as_tensor(src))
        g1.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(S.cpu().numpy()), bits(eager[k][0])), f"replay with draw {k}: S"
        assert np.array_equal(bits(G.cpu().numpy()), bits(eager[k][1])), f"replay with draw {k}: grad"
    eng.close()


# ---- 7. descent
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("cost", list(R.COSTS))
def test_gradient_descent_lowers_the_costs(cost, math_mode, capsys):
    """tests/test_gpu_grad.py's criterion under the network: 30 x (gradient + Adam, lr 0.02, clip 5) make more than 80 % of the plans
    cheaper and bring the mean cost below 0.9 of the start.  (The float64 reference: every plan cheaper, mean ratios 0.60-0.65 under
    quadratic_boundary_grad_minimal and 0.37-0.46 under default.)"""
    E, N, H = 4, 32, 35
    eng = engine(E, N, H, "golden", cost_function_specification=cost, math_mode=math_mode)
    rng = np.random.Generator(np.random.SFC64(8))
    s0, tp, h0, Q0 = [], [], [], []
    for _ in range(E):
        s, t, _, h = draw_env(rng, 35, 0.3)
        s0.append(s); tp.append(t); h0.append(h); Q0.append((0.3 * rng.standard_normal((N, H))).astype(f32))
    s0, tp, h0 = np.stack(s0), np.stack(tp), np.stack(h0)
    te = np.ones(E, f32)
    Q = eng.tensor(np.stack(Q0))
    m, v = torch.zeros_like(Q), torch.zeros_like(Q)
    S0 = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h0)[0].clone()
    for it in range(1, 31):
        _, G = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h0)
        eng.adam_step(Q, G, m, v, it, 0.02, gradmax_clip=5.0)
    S1 = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h0)[0]
    cheaper, ratio = (S1 < S0).float().mean().item(), (S1.mean() / S0.mean()).item()
    report(capsys, f"item7 {cost} {math_mode}: {cheaper:.3f} of the plans cheaper, mean cost ratio {ratio:.3f}")
    assert cheaper > 0.8 and ratio < 0.9
    eng.close()


# ---- 8. the optimizers on the device
@functools.lru_cache(maxsize=None)
def _ode_controls(name):
    return _run_controller(name, None)[0]


def _run_controller(name, model):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    E = 3
    config = dict(seed=3) if model is None else dict(seed=3, gru_model=model, gru_adjoint=True)
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                          control_limits=([-1.0], [1.0]), num_envs=E, config=config)
    ctrl.configure(name)
    s = np.stack([O.create_cartpole_state(0.3, -0.5, 0.02, 0.1), O.create_cartpole_state(-0.4, 1.0, -0.05, -0.1),
                  O.create_cartpole_state(0.1, 0.3, 0.08, 0.15)])
    controls, states = [], []
    for _ in range(3):
        u = ctrl.step(s, 0.0, {})
        controls.append(np.array(u, f32).reshape(E))
        states.append(s)
        s = np.stack([O.ode_v0_step(s[e][None], np.array(u, f32).reshape(E, 1)[e])[0] for e in range(E)])
    return np.stack(controls), np.stack(states), ctrl.optimizer


@pytest.mark.parametrize("name", ["rpgd", "gradient", "cem-naive-grad", "cem-grad-bharadhwaj"])
def test_gradient_family_over_the_gru_through_the_controller(name, capsys):
    """controller_mpc with config={"gru_model": ..., "gru_adjoint": True} at the shipped sizes, 3 envs, 3 control steps: controls
    finite and inside the limits, other than the ODE run's, and the optimizer's memory is the oracle's after the applied controls."""
    model = model_of("golden")
    u, states, opt = _run_controller(name, model)
    assert opt.optimizer_name == name and opt.gru_adjoint and opt.h is not None
    assert opt.num_rollouts == {"rpgd": 16, "gradient": 40, "cem-naive-grad": 200, "cem-grad-bharadhwaj": 32}[name] and opt.mpc_horizon == 35
    assert np.isfinite(u).all() and np.abs(u).max() <= 1.0
    assert not np.array_equal(u, _ode_controls(name))
    E = u.shape[1]
    h32, h64 = np.zeros((2, E, 32), f32), np.zeros((2, E, 32), np.float64)
    for k in range(3):
        h32 = O.gru_predict(model, states[k], u[k][:, None], h32)[1]
        h64 = O.gru_predict(model, states[k], u[k][:, None], h64, dtype=np.float64)[1]
    hd = opt.h.cpu().numpy()
    assert hd.shape == (E, 2, 32)
    dh = np.abs(hd - h32.transpose(1, 0, 2))
    report(capsys, f"item8 {name}: memory {dh.max():.2e}")
    assert dh.max() <= 1e-4
    opt.optimizer_reset()
    assert not opt.h.any()
