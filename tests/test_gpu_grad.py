"""GPU: gradient of rollout + plugin cost w.r.t. the inputs (cpmppi_rollout_cost_grad) against torch.autograd of the
float64 oracle - at the gradient optimizers' own sizes and across blocks, with its refusals -, the Adam and SGD steps
against numpy, and the gradient optimizers on top."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from oracle import oracle_torch as OT  # noqa: E402
import parity_util as PU  # noqa: E402

f32 = np.float32
QBG_W = dict(ccrc_weight_up=3.0, ccrc_weight_down=3.0, dd_linear_weight_up=2.0, dd_linear_weight_down=2.0)


def make(E, N, H, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    return MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, shift_mode="none", **kw))


def envs(E, seed, edge=False):
    rng = np.random.Generator(np.random.SFC64(seed))
    if edge:
        s0 = np.stack([O.create_cartpole_state(0.4, 1.0, sgn * 0.185, sgn * 0.55) for sgn in np.resize([1.0, -1.0], E)])
    else:
        s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.8, 0.8), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1),
                                               rng.uniform(-0.3, 0.3)) for _ in range(E)])
    tp = rng.uniform(-0.05, 0.05, E).astype(f32)
    Lv = rng.uniform(0.3, 0.45, E).astype(f32)
    return s0, tp, Lv, rng


CASES = [("quadratic_boundary_grad_minimal", O.COST_QBGM, 1.0, "sum", False),
         ("quadratic_boundary_grad_minimal", O.COST_QBGM, -1.0, "mean", False),
         ("quadratic_boundary_grad_minimal", O.COST_QBGM, 1.0, "sum", True),
         ("default", O.COST_DEFAULT, 1.0, "sum", False),
         ("quadratic_boundary_grad", 3, 1.0, "sum", False),
         ("quadratic_boundary_grad", 3, -1.0, "sum", True)]


@pytest.mark.parametrize("predictor_type", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("name,cost_id,te,reduce,edge", CASES)
def test_gradient_vs_autograd(name, cost_id, te, reduce, edge, predictor_type):
    """Both in-tree ODE predictors: predictor_ODE_v0 (bounce branch in the adjoint) and predictor_ODE (Euler-Cromer, no bounce -
    what the shipped config_controllers.yml:2-3 pairs with `optimizer: rpgd`)."""
    E, N, H = 3, 40, 35                                          # gradient-tf sizes (config_optimizers.yml:50,60)
    eng = make(E, N, H, cost_function_specification=name, horizon_reduce=reduce,
               cost_weights=QBG_W if cost_id == 3 else None, predictor_type=predictor_type)
    s0, tp, Lv, rng = envs(E, 21, edge)
    Q = (0.5 * rng.standard_normal((E, N, H))).astype(f32)
    Q[:, :4] *= 3.0                                              # some controls beyond the limits: clipped, zero gradient
    prev = np.asarray([0.2, -0.1, 0.0], dtype=f32)
    S, G = eng.rollout_cost_grad(s0, Q, tp, np.full(E, te, f32), L=Lv, previous_input=prev)
    S, G = S.cpu().numpy(), G.cpu().numpy()
    # the forward value is the cost-only launch's
    S2 = eng.rollout_cost(s0, Q, tp, np.full(E, te, f32), L=Lv).cpu().numpy() if cost_id != 3 else None
    if S2 is not None:
        np.testing.assert_allclose(S, S2, rtol=2e-4)
    bounced, n_flagged, n_flagged_off = 0, 0, 0
    for e in range(E):
        J, g = OT.cost_and_grad(cost_id, s0[e], Q[e], tp[e], te, L=Lv[e], horizon_reduce=reduce, previous_input=prev[e],
                                qbg_weights=QBG_W, integrator=predictor_type)
        traj = O.predict_core(s0[e], np.clip(Q[e], -1, 1), L=Lv[e], integrator=predictor_type)
        bounced += int((np.abs(traj[:, :, O.POSITION_IDX]).max(axis=1) >= 0.197).sum())
        np.testing.assert_allclose(S[e], J, rtol=5e-4)
        assert np.all(G[e][np.abs(Q[e]) > 1.0] == 0.0) and np.all(g[np.abs(Q[e]) > 1.0] == 0.0)
        # float32 adjoint through 350 substeps vs float64 autograd, relative to each rollout's gradient scale.  Buckets as
        # in parity_util, from the ORACLE's trajectory: a rollout that comes within float32 reach of a branch
        # (edge bounce, +-pi wrap, a cost indicator threshold, the control limit) may legitimately take the other branch
        # in one of the two evaluations - those are flagged and capped; every other rollout must be inside the bound.
        scale = np.abs(g).max(axis=1, keepdims=True) + 1e-6
        err = (np.abs(G[e] - g) / scale).max(axis=1)
        # (predictor_ODE has no bounce: its only state discontinuity is the +-pi seam of atan2, derivative 1 through it)
        flagged = (PU.flag_discontinuities(traj) if predictor_type == "ODE_v0" else np.zeros(N, bool)) | PU.flag_indicators(traj, {O.COST_QBGM: "qbgm", O.COST_DEFAULT: "default"}.get(cost_id, "qbg"), tp[e])
        flagged |= (np.abs(np.abs(Q[e]) - 1.0) < 1e-3).any(axis=1)
        clear_off = int(((err >= 5e-4) & ~flagged).sum())
        assert clear_off == 0, f"env {e}: {clear_off} of {int((~flagged).sum())} rollouts clear of every branch differ by more than 5e-4 (worst {err[~flagged].max():.2e})"
        assert np.median(err) < 1e-4
        n_flagged += int(flagged.sum()); n_flagged_off += int(((err >= 2e-3) & flagged).sum())
    assert n_flagged_off <= int(np.ceil(0.05 * n_flagged)), f"{n_flagged_off} of {n_flagged} flagged rollouts outside 2e-3"
    if edge:
        assert bounced > 0                                       # the bounce branch of the adjoint was exercised (ODE: rollouts beyond the edge)


def test_adam_step_vs_numpy():
    E, N, H = 2, 40, 35
    eng = make(E, N, H)
    rng = np.random.Generator(np.random.SFC64(3))
    Q = rng.uniform(-0.9, 0.9, (E, N, H)).astype(f32)
    m, v = np.zeros_like(Q), np.zeros_like(Q)
    Qd, md, vd = eng.tensor(Q.copy()), eng.tensor(m.copy()), eng.tensor(v.copy())
    lr, b1, b2, eps, clipn = 0.05, 0.9, 0.999, 1e-8, 5.0
    for it in range(1, 4):
        g = (rng.standard_normal((E, N, H)) * rng.choice([0.1, 1.0, 30.0], (E, N, 1))).astype(f32)
        eng.adam_step(Qd, eng.tensor(g), md, vd, it, lr, b1, b2, eps, clipn)
        nrm = np.sqrt((g.astype(np.float64) ** 2).sum(-1, keepdims=True))
        gc = g * np.minimum(1.0, clipn / np.maximum(nrm, 1e-30))
        m = b1 * m + (1 - b1) * gc
        v = b2 * v + (1 - b2) * gc * gc
        lr_t = lr * np.sqrt(1 - b2 ** it) / (1 - b1 ** it)
        Q = np.clip(Q - lr_t * m / (np.sqrt(v) + eps), -1, 1)
        np.testing.assert_allclose(Qd.cpu().numpy(), Q, atol=2e-6)
    np.testing.assert_allclose(md.cpu().numpy(), m, rtol=1e-5, atol=1e-7)
    with pytest.raises(RuntimeError):
        eng.adam_step(Qd, eng.tensor(g), md, vd, 0, lr)          # iterations count from 1


def test_gradient_descent_lowers_the_costs():
    E, N, H = 4, 32, 35
    eng = make(E, N, H)
    s0, tp, Lv, rng = envs(E, 8)
    te = np.ones(E, f32)
    Q = eng.tensor((0.3 * rng.standard_normal((E, N, H))).astype(f32))
    m, v = torch.zeros_like(Q), torch.zeros_like(Q)
    S0, _ = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv)
    S0 = S0.clone()
    for it in range(1, 31):
        _, G = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv)
        eng.adam_step(Q, G, m, v, it, 0.02, gradmax_clip=5.0)
    S1, _ = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv)
    assert (S1 < S0).float().mean().item() > 0.8 and S1.mean().item() < 0.9 * S0.mean().item()


@pytest.mark.parametrize("spec", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("name", ["gradient", "rpgd"])
def test_gradient_optimizers_through_the_controller_seam(name, spec):
    """controller_mpc.configure('gradient-tf' | 'rpgd'): shipped hyper-parameters (config_optimizers.yml:49-86), the plan
    improves the cost of the best candidate, the loop on the batched plant keeps mildly perturbed poles upright - on
    predictor_ODE_v0 and on the shipped pairing, `optimizer: rpgd` + `predictor_specification: "ODE"` (config_controllers.yml:2-3)."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    E = 8
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                          control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=3))
    ctrl.configure(name, predictor_specification=spec)
    opt = ctrl.optimizer
    assert opt.cfg.predictor_type == spec
    assert opt.optimizer_name == name and opt.num_rollouts == (40 if name == "gradient" else 16) and opt.mpc_horizon == 35
    eng = opt.engine
    rng = np.random.Generator(np.random.SFC64(2))
    s = eng.tensor(np.stack([O.create_cartpole_state(rng.uniform(-0.25, 0.25), rng.uniform(-0.5, 0.5),
                                                     rng.uniform(-0.05, 0.05), 0.0) for _ in range(E)]))
    tp, te, Lv = np.zeros(E, f32), np.ones(E, f32), np.full(E, 0.395, f32)
    S_before = eng.rollout_cost(s, opt.Q, tp, te, L=Lv).min(dim=1).values.clone()
    Q0 = ctrl.step(s, 0.0, {})
    assert Q0.shape == (E, 1) and np.abs(Q0).max() <= 1.0
    # (plans were shifted after the step: compare the best cost reached on the un-shifted problem via the log)
    ctrl2 = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                           control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=3))
    ctrl2.configure(name, controller_logging=True, predictor_specification=spec)
    ctrl2.step(s, 0.0, {})
    S_after = torch.as_tensor(ctrl2.controller_data_for_csv["J_logged"]).min(dim=1).values
    assert (S_after < S_before.cpu()).all()
    # closed loop: 60 control steps on the device plant
    for k in range(60):
        Q = ctrl.optimizer.step(s, as_tensor=True)
        eng.plant_advance(s, Q, L=Lv, n_substeps=10)
    sh = s.cpu().numpy()
    assert (np.abs(sh[:, O.ANGLE_IDX]) < 0.35).mean() >= 0.75 and np.abs(sh[:, O.POSITION_IDX]).max() < 0.198


def test_gradient_with_more_substeps_than_the_default_lds_budget():
    """intermediate_steps = 20 needs 120 KB of LDS for the sub-states: launches (160 KB opt-in) and matches autograd."""
    E, N, H = 1, 8, 6
    eng = make(E, N, H, intermediate_steps=20)
    s0, tp, Lv, rng = envs(E, 5)
    Q = (0.4 * rng.standard_normal((E, N, H))).astype(f32)
    S, G = eng.rollout_cost_grad(s0, Q, tp, np.ones(E, f32), L=Lv)
    J, g = OT.cost_and_grad(O.COST_QBGM, s0[0], Q[0], tp[0], 1.0, L=Lv[0], S=20)
    np.testing.assert_allclose(S.cpu().numpy()[0], J, rtol=5e-4)
    scale = np.abs(g).max(axis=1, keepdims=True) + 1e-6
    assert (np.abs(G.cpu().numpy()[0] - g) / scale).max() < 2e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# Beyond one block.  600 rows in three blocks of 256 lanes: block 0 holds lanes of envs 0, 1 and 2 (env = g / N inside a block),
# the last block has 88 live lanes (g >= B), the handle is built for 6 envs and called with 5 (check-point stride 5 N inside a 6 N
# allocation), the action limits are not +-1, and L, previous_input, target_position and target_equilibrium differ per env.
XB = dict(E_handle=6, E=5, N=120, H=12, lo=-0.5, hi=0.8)
XB_COSTS = {"quadratic_boundary_grad_minimal": O.COST_QBGM, "quadratic_boundary_grad": 3}
_xb_cache = {}


def xb_inputs():
    """Inputs of the cross-block cases (the same for every case): env 0 starts at the track edge (envs(edge=True): bounces under
    predictor_ODE_v0, runs past the edge under predictor_ODE), the others near the middle of the track."""
    E, N, H = XB["E"], XB["N"], XB["H"]
    s0, tp, Lv, rng = envs(E, 33)
    s0[0] = envs(E, 33, edge=True)[0][0]
    Q = (0.3 * rng.standard_normal((E, N, H))).astype(f32)
    Q[:, :3] *= 4.0                                              # rows with controls beyond both limits
    Q[:, 3, ::2], Q[:, 4, 1::2] = -0.75, 0.9                     # and rows that sit beyond one limit at every other step
    prev = np.asarray([0.2, -0.1, 0.0, 0.6, -0.4], dtype=f32)
    # (target "down" for the two envs whose pole stays away from upright: under quadratic_boundary_grad with admissible_angle 0 the stage
    # cost of te = -1 jumps by ~3000 where cos(angle) == 1, which float32 reaches for |angle| < 2.4e-4 and float64 never does)
    te = np.asarray([1.0, 1.0, -1.0, -1.0, 1.0], dtype=f32)
    return s0.astype(f32), Q, tp, te, Lv, prev


def xb_reference(predictor_type, name):
    """Float64 autograd of the oracle and the oracle's flags, once per case: (J [E,N], g [E,N,H], flagged [E,N], bounced)."""
    key = (predictor_type, name)
    if key not in _xb_cache:
        s0, Q, tp, te, Lv, prev = xb_inputs()
        cost_id, lo, hi = XB_COSTS[name], XB["lo"], XB["hi"]
        J, g, fl, bounced = [], [], [], 0
        for e in range(XB["E"]):
            Je, ge = OT.cost_and_grad(cost_id, s0[e], Q[e], tp[e], te[e], L=Lv[e], previous_input=prev[e], qbg_weights=QBG_W,
                                      clip=(lo, hi), integrator=predictor_type)
            traj = O.predict_core(s0[e], np.clip(Q[e], f32(lo), f32(hi)), L=Lv[e], integrator=predictor_type)
            # (envs(edge=True)'s check, plus what it misses at H = 12: the cart bounces BETWEEN two control-step samples and no sample
            # reaches 0.197.  A bounce reverses the cart's velocity: >= 0.68 m/s within one control step here, where the ODE alone moves
            # it by <= 0.16 m/s under these limits)
            x, v = traj[:, :, O.POSITION_IDX], traj[:, :, O.POSITIOND_IDX]
            reversed_at_edge = ((v[:, :-1] * v[:, 1:] < 0) & (np.abs(np.diff(v, axis=1)) > 0.4) & (np.abs(x[:, :-1]) > 0.19)).any(axis=1)
            bounced += int(((np.abs(x).max(axis=1) >= 0.197) | reversed_at_edge).sum())
            f = (PU.flag_discontinuities(traj) if predictor_type == "ODE_v0" else np.zeros(XB["N"], bool)) \
                | PU.flag_indicators(traj, "qbgm" if cost_id == O.COST_QBGM else "qbg", tp[e])
            f |= ((np.abs(Q[e] - f32(lo)) < 1e-3) | (np.abs(Q[e] - f32(hi)) < 1e-3)).any(axis=1)
            if te[e] < 0:                                        # clear of the cos(angle) == cos(admissible_angle) threshold (see xb_inputs)
                assert np.abs(traj[:, :, O.ANGLE_IDX]).min() > 0.1
            J.append(Je); g.append(ge); fl.append(f)
        for a in (J, g, fl):
            for x in a:
                x.setflags(write=False)
        _xb_cache[key] = (np.stack(J), np.stack(g), np.stack(fl), bounced)
    return _xb_cache[key]


def report(capsys, text):
    with capsys.disabled():
        print("\n[optim] " + text)


def test_cross_block_case_is_mostly_clear_of_branches():
    """A condition on the inputs, from the oracle alone: at most a quarter of the 600 rollouts are flagged (env 0, at the edge, is -
    all of it under predictor_ODE_v0), so the 5e-4 bound applies to the rest; and env 0 does bounce / leave the track."""
    for predictor_type in ("ODE_v0", "ODE"):
        for name in XB_COSTS:
            _, g, flagged, bounced = xb_reference(predictor_type, name)
            assert flagged.mean() <= 0.25 and bounced > 0
            assert (np.abs(g).max(axis=2) > 0).all()                                # every rollout has a gradient scale of its own


@pytest.mark.parametrize("predictor_type", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("name", list(XB_COSTS))
def test_gradient_across_blocks(name, predictor_type, capsys):
    """The adjoint kernel on three blocks (see XB) against float64 autograd, under the rules of test_gradient_vs_autograd: rollouts clear
    of every branch within 5e-4 of their gradient scale, flagged ones within 2e-3 (5 % of them may miss), costs to rtol 5e-4, gradient
    exactly 0 beyond either limit.  quadratic_boundary_grad couples step k to k + 1 through u_before (the kernel's `carry`).  Then
    indexing alone: every env by itself through the same handle gives the same bits, and the defaults are L_default and zeros."""
    E, N, H, lo, hi = XB["E"], XB["N"], XB["H"], XB["lo"], XB["hi"]
    eng = make(XB["E_handle"], N, H, cost_function_specification=name, cost_weights=QBG_W if XB_COSTS[name] == 3 else None,
               predictor_type=predictor_type, action_low=lo, action_high=hi)
    s0, Q, tp, te, Lv, prev = xb_inputs()
    J, g, flagged, bounced = xb_reference(predictor_type, name)
    assert flagged.mean() <= 0.25
    St, Gt = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)
    S, G = St.cpu().numpy(), Gt.cpu().numpy()
    beyond = (Q < f32(lo)) | (Q > f32(hi))
    assert beyond.any(axis=2).sum() >= 5 * E and (Q < f32(lo)).any() and (Q > f32(hi)).any()
    assert np.all(G[beyond] == 0.0) and np.all(g[beyond] == 0.0)
    scale = np.abs(g).max(axis=2) + 1e-6
    err = (np.abs(G - g).max(axis=2)) / scale
    cost_err = np.abs(S - J) / np.abs(J)
    n_fl, n_fl_off = int(flagged.sum()), int(((err >= 2e-3) & flagged).sum())
    report(capsys, f"gradient across blocks {name} / {predictor_type}: worst clear {err[~flagged].max():.2e} (bound 5e-4), worst flagged "
                   f"{err[flagged].max():.2e} (bound 2e-3, {n_fl_off} of {n_fl} outside, cap 5 %), flagged share {flagged.mean():.3f} "
                   f"(bound 0.25), cost rel. {cost_err.max():.2e} (bound 5e-4), bounced {bounced}")
    np.testing.assert_allclose(S, J, rtol=5e-4)
    clear_off = int(((err >= 5e-4) & ~flagged).sum())
    assert clear_off == 0, (f"{clear_off} of {int((~flagged).sum())} rollouts clear of every branch differ by more than 5e-4 "
                            f"(worst {err[~flagged].max():.2e})")
    assert n_fl_off <= int(np.ceil(0.05 * n_fl)), f"{n_fl_off} of {n_fl} flagged rollouts outside 2e-3"
    assert bounced > 0
    # isolation: lane arithmetic is per rollout, so an env alone through the same handle gives the same bits - only indexing differs
    for e in range(E):
        S1, G1 = eng.rollout_cost_grad(s0[e:e + 1], Q[e:e + 1], tp[e:e + 1], te[e:e + 1], L=Lv[e:e + 1], previous_input=prev[e:e + 1])
        assert np.array_equal(S1.cpu().numpy()[0], S[e]) and np.array_equal(G1.cpu().numpy()[0], G[e]), f"env {e} alone"
    # (the 5-env call did not depend on what the single-env ones left in the check-points)
    S5, G5 = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)
    assert np.array_equal(S5.cpu().numpy(), S) and np.array_equal(G5.cpu().numpy(), G)
    # defaults: no L and no previous input = the handle's L and zeros
    Sa, Ga = eng.rollout_cost_grad(s0, Q, tp, te)
    Sb, Gb = eng.rollout_cost_grad(s0, Q, tp, te, L=np.full(E, eng.phys.L, f32), previous_input=np.zeros(E, f32))
    assert np.array_equal(Sa.cpu().numpy(), Sb.cpu().numpy()) and np.array_equal(Ga.cpu().numpy(), Gb.cpu().numpy())
    assert not np.array_equal(Sa.cpu().numpy(), S)
    eng.close()


@pytest.mark.parametrize("what,kw", [
    ("legacy cost", dict(cost_function_specification="legacy_mppi_cartpole")),
    ("quadratic_boundary", dict(cost_function_specification="quadratic_boundary")),
    ("PRECISE math", dict(math_mode="precise")),
    ("S > 25", dict(intermediate_steps=26))])
def test_gradient_refusals_leave_the_handle_usable(what, kw):
    """cpmppi_rollout_cost_grad has no adjoint for these four: each is refused with CpmppiError, before anything is launched, and the
    handle goes on serving what it does support."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 24, 5
    eng = make(E, N, H, **kw)
    s0, tp, Lv, rng = envs(E, 9)
    te = np.ones(E, f32)
    Q = (0.4 * rng.standard_normal((E, N, H))).astype(f32)
    legacy = what == "legacy cost"
    before = None if legacy else eng.rollout_cost(s0, Q, tp, te, L=Lv).cpu().numpy()
    for _ in range(2):
        with pytest.raises(CpmppiError, match="cpmppi_rollout_cost_grad"):
            eng.rollout_cost_grad(s0, Q, tp, te, L=Lv)
    if legacy:
        with pytest.raises(CpmppiError):
            eng.rollout_cost(s0, Q, tp, te, L=Lv)                                   # (plugin costs only, as well)
    else:
        after = eng.rollout_cost(s0, Q, tp, te, L=Lv).cpu().numpy()
        assert np.isfinite(after).all() and np.array_equal(after, before)
    gr = rng.standard_normal((E, N, H)).astype(f32)
    Qd = eng.sgd_step(eng.tensor(Q.copy()), eng.tensor(gr), 0.1, 0.0).cpu().numpy()
    np.testing.assert_allclose(Qd, np.clip(Q.astype(np.float64) - 0.1 * gr.astype(np.float64), -1, 1), atol=2e-6)
    if what == "S > 25":                                                            # the largest S with an adjoint still launches and matches
        ok = make(1, 8, 3, intermediate_steps=25)
        S, G = ok.rollout_cost_grad(s0[:1], Q[:1, :8, :3].copy(), tp[:1], te[:1], L=Lv[:1])
        J, g = OT.cost_and_grad(O.COST_QBGM, s0[0], Q[0, :8, :3], tp[0], 1.0, L=Lv[0], S=25)
        np.testing.assert_allclose(S.cpu().numpy()[0], J, rtol=5e-4)
        assert (np.abs(G.cpu().numpy()[0] - g) / (np.abs(g).max(axis=1, keepdims=True) + 1e-6)).max() < 2e-3
        ok.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# The update kernels on 600 rows (E, N, H = 3, 200, 7: three blocks, the last with 88 live lanes), asymmetric limits.
def step_engine():
    return make(3, 200, 7, action_low=-0.5, action_high=0.8)


def step_gradients(rng, it, scales=(0.1, 1.0, 30.0)):
    """[3,200,7] float32: per-row scales (the default: row norms below and above the clip norm 5), rows with an all-zero gradient."""
    g = (rng.standard_normal((3, 200, 7)) * rng.choice(list(scales), (3, 200, 1))).astype(f32)
    g[:, 7 + it] = 0.0                                           # norm exactly 0 (another row each iteration)
    g[:, 150] = 0.0                                              # and one row with no gradient at any iteration
    return g


def clip_by_norm(g, c):
    nrm = np.sqrt((g.astype(np.float64) ** 2).sum(-1, keepdims=True))
    return g.astype(np.float64) * (np.minimum(1.0, c / np.maximum(nrm, 1e-300)) if c > 0 else 1.0), nrm


@pytest.mark.parametrize("clipn,lr,big", [(5.0, 0.05, False), (0.0, 2e-4, True)])
def test_sgd_step_vs_numpy(clipn, lr, big, capsys):
    """cem-naive-grad's update, clip(Q - lr g min(1, c / |g|), lo, hi), against float64 numpy over three iterations: rows with |g| below
    the clip norm, above it and exactly 0; clipping off (gradmax_clip = 0) with large gradients; |lr g| <= 1 throughout."""
    E, N, H, lo, hi = 3, 200, 7, f32(-0.5), f32(0.8)
    eng = step_engine()
    rng = np.random.Generator(np.random.SFC64(31))
    Q = rng.uniform(-0.45, 0.75, (E, N, H)).astype(f32)
    Qd, worst = eng.tensor(Q.copy()), 0.0
    scales = (40.0, 200.0, 800.0) if big else (0.1, 1.0, 30.0)
    Q = Q.astype(np.float64)
    for it in range(3):
        g = step_gradients(rng, it, scales)
        gc, nrm = clip_by_norm(g, clipn)
        assert np.abs(lr * gc).max() <= 1.0 and (nrm == 0).sum() >= 2 * E
        if clipn > 0:
            assert (nrm[nrm > 0] < clipn).any() and (nrm > clipn).any()
        else:
            assert nrm[nrm > 0].min() > 5.0
        eng.sgd_step(Qd, eng.tensor(g), lr, clipn)
        Qn = np.clip(Q - lr * gc, lo, hi)
        zero = (nrm == 0)[..., 0]
        assert np.array_equal(Qd.cpu().numpy()[zero], Q[zero].astype(f32))           # no gradient: the row stays as it is
        assert ((Qn == lo).any() and (Qn == hi).any()) or not big
        worst = max(worst, np.abs(Qd.cpu().numpy() - Qn).max())
        np.testing.assert_allclose(Qd.cpu().numpy(), Qn, atol=2e-6)
        Q = Qd.cpu().numpy().astype(np.float64)                                      # (the next iteration starts from the device's float32)
    report(capsys, f"sgd_step gradmax_clip {clipn}: worst |Q - numpy| {worst:.2e} (bound 2e-6)")
    # E = 2 on the 3-env tensor: rows >= E N are not touched
    keep = Qd.cpu().numpy().copy()
    g = step_gradients(rng, 0, scales)
    eng.sgd_step(Qd[:2], eng.tensor(g)[:2], lr, clipn)
    out = Qd.cpu().numpy()
    assert np.array_equal(out[2], keep[2]) and not np.array_equal(out[:2], keep[:2])
    np.testing.assert_allclose(out[:2], np.clip(keep[:2].astype(np.float64) - lr * clip_by_norm(g[:2], clipn)[0], lo, hi), atol=2e-6)
    eng.close()


@pytest.mark.parametrize("clipn", [5.0, 0.0])
def test_adam_step_across_blocks_vs_numpy(clipn, capsys):
    """600 rows; m AND v compared; rows with an all-zero gradient (norm 0: no division by it) keep m = v = 0 and Q unchanged at
    iteration 1 and stay finite; gradmax_clip = 0 switches the norm clipping off (row norms above 5 go through whole).  Gradient elements
    stay O(1) in both cases, as in test_adam_step_vs_numpy: m sums terms of both signs, a float32 sum that cancels is off by an ulp of its
    TERMS, and atol = 1e-7 is an ulp of terms below 1 (measured with |g| ~ 1e3 and clipping off: 2.6e-6 on m ~ 0.02 from terms ~ 100)."""
    E, N, H, lo, hi = 3, 200, 7, f32(-0.5), f32(0.8)
    eng = step_engine()
    rng = np.random.Generator(np.random.SFC64(32))
    Q0 = rng.uniform(-0.45, 0.75, (E, N, H)).astype(f32)
    Qd, md, vd = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
    Q, m, v = Q0.astype(np.float64), np.zeros((E, N, H)), np.zeros((E, N, H))
    lr, b1, b2, eps = 0.05, f32(0.9), f32(0.999), f32(1e-8)
    worst = dict(Q=0.0, m=0.0, v=0.0)
    scales = (0.1, 1.0, 30.0) if clipn > 0 else (0.1, 0.5, 1.5)
    for it in range(1, 4):
        g = step_gradients(rng, it, scales)
        gc, nrm = clip_by_norm(g, clipn)
        assert (nrm > 5.0).any() and (nrm[nrm > 0] < 5.0).any() and np.abs((1 - float(b1)) * gc).max() < 1.0
        eng.adam_step(Qd, eng.tensor(g), md, vd, it, lr, float(b1), float(b2), float(eps), clipn)
        m = float(b1) * m + (1 - float(b1)) * gc
        v = float(b2) * v + (1 - float(b2)) * gc * gc
        lr_t = lr * np.sqrt(1 - float(b2) ** it) / (1 - float(b1) ** it)
        Q = np.clip(Q - lr_t * m / (np.sqrt(v) + float(eps)), lo, hi)
        Qh, mh, vh = Qd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()
        assert np.isfinite(Qh).all() and np.isfinite(mh).all() and np.isfinite(vh).all()
        if it == 1:
            zero = (nrm == 0)[..., 0]
            assert zero.sum() >= 2 * E
            assert np.array_equal(Qh[zero], Q0[zero]) and np.all(mh[zero] == 0.0) and np.all(vh[zero] == 0.0)
        worst["Q"] = max(worst["Q"], np.abs(Qh - Q).max())
        np.testing.assert_allclose(Qh, Q, atol=2e-6)
    assert np.array_equal(Qh[:, 150], Q0[:, 150]) and np.all(mh[:, 150] == 0.0) and np.all(vh[:, 150] == 0.0)   # never had a gradient
    worst["m"] = (np.abs(mh - m) / np.maximum(np.abs(m), 1e-30))[np.abs(m) > 1e-2].max()
    worst["v"] = (np.abs(vh - v) / np.maximum(np.abs(v), 1e-30))[np.abs(v) > 1e-2].max()
    report(capsys, f"adam_step gradmax_clip {clipn}: worst |Q - numpy| {worst['Q']:.2e} (bound 2e-6), rel. m {worst['m']:.2e}, "
                   f"rel. v {worst['v']:.2e} (bound 1e-5 + 1e-7 abs)")
    np.testing.assert_allclose(mh, m, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(vh, v, rtol=1e-5, atol=1e-7)
    # E = 2 on the 3-env tensors: env 2 of Q, m and v is not touched
    g = step_gradients(rng, 0, scales)
    gd = eng.tensor(g)
    eng.adam_step(Qd[:2], gd[:2], md[:2], vd[:2], 4, lr, float(b1), float(b2), float(eps), clipn)
    for dev, was in ((Qd, Qh), (md, mh), (vd, vh)):
        now = dev.cpu().numpy()
        assert np.array_equal(now[2], was[2]) and not np.array_equal(now[:2], was[:2])
    gc = clip_by_norm(g[:2], clipn)[0]
    np.testing.assert_allclose(md.cpu().numpy()[:2], float(b1) * mh[:2].astype(np.float64) + (1 - float(b1)) * gc, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(vd.cpu().numpy()[:2], float(b2) * vh[:2].astype(np.float64) + (1 - float(b2)) * gc * gc, rtol=1e-5, atol=1e-7)
    eng.close()
