"""CPU: the float64 reference of the GRU gradient tests (tests/gru_grad_ref.py) is the oracle's function, and the cases it is
evaluated on are not vacuous.

* Its trajectory equals oracle_np.gru_predict(..., dtype=float64) to 1e-12 and its cost equals oracle_np.trajectory_cost on that
  trajectory, so what torch.autograd differentiates is get_trajectory_cost(predict_core_GRU(s, Q), Q).
* The cases of tests/test_gpu_gru_grad.py are mostly clear of branches.  At the gradient-tf size, 3 x 40 x 35, at most 5 % of an
  env's rollouts are flagged (an indicator threshold of `default` within reach, or an input within 1e-3 of a control limit) for
  every model / cost pair used: 2.5 % measured for the golden model under both costs and for the random model under
  quadratic_boundary_grad_minimal; the random model under `default` reaches 17.5 % (its cart runs to the track's edge) and is
  therefore not a case.  At every shape the flagged rollouts of an env number at most ceil(0.05 N) and never all of them.
* The gradient is not trivially small: every rollout that is not clipped throughout has a gradient scale of its own, and the
  first four rollouts of an env (three times the spread) do have entries beyond the limits, where the gradient is exactly 0.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import gru_grad_ref as R  # noqa: E402
from test_gpu_gru_edges import model_of  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("model,cost", R.PAIRS)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_restatement_is_the_oracle(model, cost, reduce):
    E, N, H = 2, 16, 35
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    for e in range(E):
        for h in (h0[e], None):
            J, g, traj = R.cost_and_grad(model_of(model), cost, s0[e], Q[e], tp[e], 1.0, h, reduce)
            Qc = np.clip(Q[e], -1, 1)
            hb = None if h is None else np.repeat(h[:, None, :], N, axis=1)
            want = O.gru_predict(model_of(model), s0[e], Qc, hb, dtype=np.float64)[0]
            assert np.abs(traj - want).max() <= 1e-12
            # the oracle forms its costs in float32 from the trajectory it is handed
            Jo = O.trajectory_cost(R.COSTS[cost], want.astype(f32), Qc, f32(tp[e]), f32(1.0), reduce)
            np.testing.assert_allclose(J, Jo, rtol=2e-5)
            assert g.shape == (N, H) and np.all(g[np.abs(Q[e]) > 1.0] == 0.0)


@pytest.mark.parametrize("model,cost", R.PAIRS)
def test_at_most_5_percent_of_an_env_is_flagged(model, cost):
    """Every model / cost pair of the GPU comparison at the gradient-tf size, 3 x 40 x 35, with the memory and without: at most
    5 % of an env's rollouts are flagged (an indicator threshold within reach on the oracle's trajectory, or an input within 1e-3
    of a control limit).  Measured: 2.5 % (one rollout of 40 in two of the three envs, from the inputs alone) for all three."""
    E, N, H = R.SHAPES[0]
    assert (E, N, H) == (3, 40, 35)
    worst = 0.0
    for with_h0 in (True, False):
        flagged = R.case_reference(model, cost, E, N, H, with_h0, "sum")[2]
        worst = max(worst, float(flagged.mean(axis=1).max()))
    print(f"{model} {cost}: flagged share per env, worst {worst:.4f}")
    assert worst <= 0.05


@pytest.mark.parametrize("E,N,H", R.SHAPES)
def test_cases_are_mostly_clear_of_branches_and_have_gradients(E, N, H):
    """Every shape, every model / cost pair, with the memory and without.  A share of 5 % is not a count of rollouts below N = 20,
    so per env the flagged rollouts are counted against ceil(0.05 N) - the rounding tests/test_gpu_grad.py gives its 5 % cap - and
    never all of them: 2 of 40, 1 of 16, 31 or 33, 7 of 129, 15 of 300, none of 1.  Measured: 1 of 40 (3 x 40 x 35), 1 of 16 in
    both envs (2 x 16 x 35, SFC64(1051): an input within 1e-3 of a limit, whatever the model and the cost), 1 of 31 under golden /
    default, none elsewhere.  Every rollout that is not clipped throughout has a gradient scale of its own."""
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    assert (np.abs(Q[:, :min(4, N)]) > 1.0).any()
    cap = int(np.ceil(0.05 * N))
    for model, cost in R.PAIRS:
        for with_h0 in (True, False):
            J, g, flagged = R.case_reference(model, cost, E, N, H, with_h0, "sum")
            counts = flagged.sum(axis=1)
            print(f"{model} {cost} h0 {with_h0}: flagged per env {counts.tolist()} of {N} (cap {cap})")
            assert (counts <= cap).all() and (counts < N).all(), (model, cost, with_h0, counts.tolist())
            assert np.isfinite(J).all() and np.isfinite(g).all()
            inside = (np.abs(Q) < 1.0).any(axis=2)
            assert (np.abs(g).max(axis=2)[inside] > 0).all()


def test_random_model_under_default_is_not_a_case():
    """Why PAIRS leaves it out: 7 of 40 rollouts of an env (17.5 %) are flagged at the gradient-tf size - its cart runs to the
    track's edge."""
    import parity_util as PU
    E, N, H = 3, 40, 35
    s0, tp, h0, Q = R.case_inputs(E, N, H)
    worst = 0.0
    for e in range(E):
        traj = O.gru_predict(model_of("random"), s0[e], np.clip(Q[e], -1, 1), np.repeat(h0[e][:, None, :], N, axis=1),
                             dtype=np.float64)[0]
        f = PU.flag_indicators(traj, "default", tp[e]) | (np.abs(np.abs(Q[e]) - 1.0) < 1e-3).any(axis=1)
        worst = max(worst, float(f.mean()))
    assert worst > 0.05
    assert abs(worst - 0.175) < 1e-9                                      # (the figure the case list was decided on)
