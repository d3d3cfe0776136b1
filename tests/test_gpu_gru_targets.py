"""GPU: the two scalars every GRU rollout kernel reads per env - target position `a.x_t[env]` and target equilibrium `a.te[env]` - in
gru_rollout_cost_kernel, gru_cost_only_kernel, gru_grad_forward_kernel and gru_grad_reverse_kernel, with the hanging target (te = -1)
beside the upright one in every launch, and the gradient launch beyond one block per env, limits other than +-1 and control_mode
"penalise".  Before this module no GPU test passed a target equilibrium other than +1 to a GRU kernel.

Cases and references: tests/gru_target_cases.py; tests/test_gru_target_cases_host.py asserts on the oracle alone that they are
mostly clear of branches and that a kernel which ignored te, read env 0's, took |te|, a neighbour's target position or the limits
+-1 would sit more than ten bounds away.  Bounds (none new): the fused step through test_gpu_gru_edges.check_env (assert_costs,
softmin_allowance, assert_controls; `default` with te = -1: tools/dev/hanging_target.py's verdict, as rollout_matrix.buckets), the
cost-only launch through assert_costs, the gradient under tests/test_gpu_gru_grad.py's: every unflagged rollout < 5e-4 of its
max |g|, median < 1e-4, flagged rollouts beyond 2e-3 at most 5 % of the flagged, S within rtol 5e-4, and G == 0 exactly where the
float64 reference's is.

The gradient's shapes, the smallest that reach its addressing `((env * N + n) * GRU_CKPT_FLOATS) + k * rows * GRU_CKPT_FLOATS`:
  case  E  N    H  what it reaches
  a     3  130  4  two blocks per env, two live columns in the second; the reverse loop runs k = 2, 1, 0: the check-point of k - 1
                   is read twice.  Also under clip with the limits -0.7 / 0.9 and under penalise
  b     2  257  3  three blocks, one live column in the last; one read of the previous check-point
  c     2  129  9  through the C entry point on a handle built for 3 envs: rows = E N of the launch, not of the handle

Measured on the MI355X (this module's first run; worst over the cases of a test, both math modes, sum and mean, with and without a
memory):
  test                                              worst figure
  test_fused_step_with_mixed_targets                excess 0.256 of the allowance, |u_nom - oracle32| 1.28e-05
  test_cost_only_launch_with_mixed_targets          excess 0.224; S bit-equal to the gradient launch's
  test_gradient_with_mixed_targets                  unflagged 7.55e-05, median 2.48e-06, flagged 5.53e-06, S relative 1.71e-06
  test_gradient_under_other_limits_and_penalise     unflagged 3.69e-05, median 2.54e-06, flagged 3.08e-06, S relative 7.12e-06
  test_last_input_closed_form_under_penalise        within 4 float32 epsilons
  test_controller_hands_the_hanging_target_to_the_kernel   bit-equal to eng.step with te = -1, and other than the te = +1 control
The 47 cases take 3.4 s together, 0.27 s the slowest.  Sensitivity to four arithmetic mutants of the kernels: profiles/gru_targets/mutants.txt.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import gru_target_cases as TC  # noqa: E402
import parity_util as PU  # noqa: E402
from test_gpu_gru_edges import bits, check_env, cost_flags, engine, model_of  # noqa: E402
from test_gpu_gru_grad import SENT, call_grad  # noqa: E402

f32 = np.float32


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-targets] " + text)


# ---- the fused step
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("model,cost", TC.PAIRS)
def test_fused_step_with_mixed_targets(model, cost, math_mode, capsys):
    """gru_rollout_cost_kernel: 3 envs x 130 rollouts, H = 11, knot period 5, host perturbations; te = (-1, +1, -1) and three
    target positions in one launch.  S, u_nom and Q of every env against the oracle pair called with that env's te."""
    c, x = TC.STEP, TC.step_inputs()
    E, N, H = c["E"], c["N"], c["H"]
    eng = engine(E, N, H, model, period_interpolation_inducing_points=c["period"], cost_function_specification=cost, math_mode=math_mode)
    un, S = eng.tensor(x["u0"].copy()), eng.empty(E, N)
    Q, _ = eng.step(x["s0"], un, x["tp"], x["te"], S_out=S, predictor="GRU", h0=x["h0"], delta_u=x["du"])
    un, S, Q = un.cpu().numpy(), S.cpu().numpy(), Q.cpu().numpy()
    worst = [0.0, 0.0]
    for e, (r32, r64) in enumerate(TC.step_reference(model, cost)):
        ex, d = check_env(S[e], un[e], Q[e], r32, r64, x["du"][e], cost, x["tp"][e], f"{model} {cost} {math_mode} env {e} (te {x['te'][e]:+.0f})",
                          te=float(x["te"][e]))
        worst = [max(worst[0], ex), max(worst[1], d)]
    report(capsys, f"step {model} {cost} {math_mode}: excess {worst[0]:.3f} u_nom {worst[1]:.2e}")
    eng.close()


# ---- the cost-only launch
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("model,cost", TC.PAIRS)
def test_cost_only_launch_with_mixed_targets(model, cost, math_mode, capsys):
    """gru_cost_only_kernel on the step case's envs with given plans: S against the oracle pair under assert_costs, and bit-equal to
    the S of the gradient launch (gru_grad_forward_kernel) on the same inputs."""
    c, x = TC.STEP, TC.step_inputs()
    E, N, H = c["E"], c["N"], c["H"]
    eng = engine(E, N, H, model, cost_function_specification=cost, math_mode=math_mode)
    S = eng.rollout_cost(x["s0"], x["plans"], x["tp"], x["te"], predictor="GRU", h0=x["h0"]).cpu().numpy()
    worst = 0.0
    for e, (r32, r64) in enumerate(TC.plans_reference(model, cost)):
        fl = cost_flags(r32, r64, cost, x["tp"][e])
        assert fl.mean() <= 0.05
        b = PU.assert_costs(S[e], r32["S"], r64["S"], fl, f"{model} {cost} {math_mode} env {e} (te {x['te'][e]:+.0f}) costs")
        worst = max(worst, float(b["excess"][~b["flagged"]].max()))
    S_grad = eng.rollout_cost_grad(x["s0"], x["plans"], x["tp"], x["te"], predictor="GRU", h0=x["h0"])[0].cpu().numpy()
    assert np.isfinite(S).all() and np.array_equal(bits(S), bits(S_grad))
    report(capsys, f"plans {model} {cost} {math_mode}: excess {worst:.3f}")
    eng.close()


# ---- the gradient
def compare_gradient(S, G, key, model, cost, with_h0, reduce, mode, what, worst):
    """tests/test_gpu_gru_grad.py's comparison of one launch with the float64 reference of case `key`; updates `worst`."""
    J, g, flagged = TC.grad_reference(key, model, cost, with_h0, reduce, mode)
    assert np.array_equal(G == 0.0, g == 0.0), f"{what}: the gradient is zero on {int((G == 0).sum())} inputs, the reference's on {int((g == 0).sum())}"
    err = TC.gradient_errors(G, g)
    n_fl, n_fl_off = int(flagged.sum()), int(((err >= 2e-3) & flagged).sum())
    rel_S = np.abs(S - J) / np.abs(J)
    for k, v in (("clear", err[~flagged].max()), ("flagged", err[flagged].max() if n_fl else 0.0), ("S", rel_S.max()), ("median", np.median(err))):
        worst[k] = max(worst[k], float(v))
    np.testing.assert_allclose(S, J, rtol=5e-4, err_msg=what)
    clear_off = (err >= 5e-4) & ~flagged
    assert not clear_off.any(), (f"{what}: {int(clear_off.sum())} of {int((~flagged).sum())} unflagged rollouts differ by more than 5e-4 "
                                 f"(worst {err[~flagged].max():.2e}), per env {clear_off.sum(axis=1).tolist()}")
    assert np.median(err) < 1e-4, what
    for e in range(err.shape[0]):                                # (an env's own median: one env of three cannot hide behind the others)
        assert np.median(err[e]) < 1e-4, f"{what}: env {e} median {np.median(err[e]):.2e}"
    assert n_fl_off <= int(np.ceil(0.05 * n_fl)), f"{what}: {n_fl_off} of {n_fl} flagged rollouts outside 2e-3"


def run_gradient_case(key, model, cost, math_mode, mode, capsys):
    c, x = TC.GRAD[key], TC.grad_inputs(key)
    E, N, H = c["E"], c["N"], c["H"]
    control_mode, lo, hi, _ = TC.MODES[mode]
    worst = dict(clear=0.0, flagged=0.0, S=0.0, median=0.0)
    for reduce in ("sum", "mean"):
        eng = engine(c["handle_envs"], N, H, model, cost_function_specification=cost, math_mode=math_mode, horizon_reduce=reduce,
                     control_mode=control_mode, action_low=lo, action_high=hi)
        for with_h0 in (True, False):
            h0 = x["h0"] if with_h0 else None
            if c["handle_envs"] == E:
                S, G = eng.rollout_cost_grad(x["s0"], x["Q"], x["tp"], x["te"], predictor="GRU", h0=h0)
                S, G = S.cpu().numpy(), G.cpu().numpy()
            else:                                                # the C entry point: fewer envs than the handle was built for
                S_t = torch.full((E * N + 64,), float(SENT), dtype=torch.float32, device=eng.device)
                G_t = torch.full((E * N + 64, H), float(SENT), dtype=torch.float32, device=eng.device)
                args = [eng.tensor(a) for a in (x["s0"], x["Q"], x["tp"], x["te"])] + [eng.tensor(h0) if with_h0 else None]
                assert call_grad(eng, E, *args, S_t, G_t) == 0, eng.lib.cpmppi_last_error(eng._h)
                S, G = S_t.cpu().numpy(), G_t.cpu().numpy()
                assert np.all(S[E * N:] == SENT) and np.all(G[E * N:] == SENT), "rows behind the buffers were written"
                S, G = S[:E * N].reshape(E, N), G[:E * N].reshape(E, N, H)
            compare_gradient(S, G, key, model, cost, with_h0, reduce, mode, f"{key} {mode} {model} {cost} {math_mode} {reduce} h0 {with_h0}", worst)
        eng.close()
    report(capsys, f"grad {key} {mode} {model} {cost} {math_mode}: WORST clear {worst['clear']:.2e} median {worst['median']:.2e} "
                   f"flagged {worst['flagged']:.2e} S {worst['S']:.2e}")


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("key", list(TC.GRAD))
@pytest.mark.parametrize("model,cost", TC.PAIRS)
def test_gradient_with_mixed_targets(model, cost, key, math_mode, capsys):
    """cpmppi_rollout_cost_grad_gru under clip with the limits +-1 at the three shapes of the module docstring, both signs of te in
    every launch; sum and mean, with and without a memory."""
    run_gradient_case(key, model, cost, math_mode, "clip", capsys)


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("mode", ["limits", "penalise"])
@pytest.mark.parametrize("model,cost", TC.PAIRS)
def test_gradient_under_other_limits_and_penalise(model, cost, mode, math_mode, capsys):
    """Case "a" on the same inputs.  `limits`: clip with action_low = -0.7, action_high = 0.9 - the gradient is exactly zero outside
    [lo, hi], the inputs between a limit and +-1 included, whose gradient under the limits +-1 is not (both through `G == 0
    exactly where the reference's is`; the host test asserts which entries of the references those are).  `penalise`: no input has
    an exactly zero gradient, the cell is fed the raw input and inputs beyond +-1 are compared like any other."""
    Q = TC.grad_inputs("a")["Q"]
    zero = {"limits": (Q < f32(TC.LIMITS[0])) | (Q > f32(TC.LIMITS[1])), "penalise": np.zeros(Q.shape, bool)}[mode]
    ref_zero = TC.grad_reference("a", model, cost, True, "sum", mode)[1] == 0.0
    assert np.array_equal(ref_zero, zero) and (np.abs(Q) > 1.0).mean() > 0.05
    run_gradient_case("a", model, cost, math_mode, mode, capsys)


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_last_input_closed_form_under_penalise(reduce, math_mode):
    """test_last_input_gradient_is_the_control_term_alone without the clamp: under penalise d S / d Q[H-1] = 2 cc_weight R u (over
    H + 1 under `mean`) for |u| > 1 as well, whatever the env's targets."""
    c, x = TC.GRAD["a"], TC.grad_inputs("a")
    E, N, H = c["E"], c["N"], c["H"]
    eng = engine(E, N, H, "golden", math_mode=math_mode, horizon_reduce=reduce, control_mode="penalise")
    _, G = eng.rollout_cost_grad(x["s0"], x["Q"], x["tp"], x["te"], predictor="GRU", h0=x["h0"])
    G = G.cpu().numpy()
    cc = O.DEFAULT_COST
    u = x["Q"][:, :, H - 1].astype(np.float64)
    want = 2.0 * float(cc.qbgm_cc_weight) * float(cc.qbgm_R) * u / ((H + 1) if reduce == "mean" else 1.0)
    assert (np.abs(u) > 1.0).sum() >= 10
    np.testing.assert_allclose(G[:, :, H - 1], want, rtol=4 * np.finfo(f32).eps, atol=0.0)
    eng.close()


# ---- the Python layer
def _controller_first_control(te, model, E, N, H, s):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    ctrl = controller_mpc("CartPole", {"target_position": 0.05, "target_equilibrium": te, "L": 0.395},
                          control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=3, gru_model=model, num_rollouts=N, mpc_horizon=H))
    ctrl.configure("mppi")
    u = np.array(ctrl.step(s, 0.0, {}), f32).reshape(E)
    return u, ctrl.optimizer


def test_controller_hands_the_hanging_target_to_the_kernel():
    """controller_mpc with "target_equilibrium": -1.0 and a GRU model, MPPI, two envs: its first control equals, bit for bit,
    eng.step called with te = -1 on the same seed and inputs, and differs from the control of a te = +1 controller."""
    from cartpolesimulation_amd.engine import MPPIEngine
    E, N, H = 2, 130, 11
    model = model_of("golden")
    s = np.stack([O.create_cartpole_state(np.pi - 0.4, -0.5, 0.02, 0.1), O.create_cartpole_state(-np.pi + 0.7, 1.0, -0.05, -0.1)])
    u_down, opt = _controller_first_control(-1.0, model, E, N, H, s)
    u_up, _ = _controller_first_control(1.0, model, E, N, H, s)
    assert opt.optimizer_name == "mppi" and opt.h is not None and (opt.num_rollouts, opt.mpc_horizon) == (N, H)
    eng = MPPIEngine(E, opt.cfg, opt.phys)
    eng.set_gru(model)
    tp, L = np.full(E, 0.05, f32), np.full(E, 0.395, f32)
    Q = {}
    for te in (-1.0, 1.0):
        Q[te] = eng.step(s, eng.zeros(E, H), tp, np.full(E, te, f32), L=L, predictor="GRU", h0=np.zeros((E, 2, 32), f32), seed=3,
                         offset=0)[0].cpu().numpy()
    assert np.isfinite(u_down).all() and np.abs(u_down).max() <= 1.0
    assert np.array_equal(bits(u_down), bits(Q[-1.0])) and np.array_equal(bits(u_up), bits(Q[1.0]))
    assert np.all(u_down != u_up)
    eng.close()
