"""GPU: the per-env controller tuning of the fused MPPI step (cpmppi_set_tuning_rows: quadratic_boundary_grad_minimal's seven cost
entries, LBD and sigma per env) - modelled on tests/test_gpu_pole_mass_rows.py.  A row computes what a handle whose scalars are that
row computes, BIT FOR BIT, in every build of the rollout kernel the plan can select and for both ODE predictors; rows equal to the
configuration are the untuned launch; the fused step against the C oracle run per env under that env's weights and LBD
(parity_util's existing cost and control rules); the C entry point's refusals."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
from numpy.random import SFC64, Generator

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402  (the checker)
import parity_util as PU  # noqa: E402
from cartpolesimulation_amd import _lib as L  # noqa: E402
from cartpolesimulation_amd.configs import TUNING_COLUMNS, MPPIConfig, tuning_rows  # noqa: E402

f32 = np.float32
LANE_MODES = [("precise", 1), ("fast", 1), ("fast", 2)]
PREDICTORS = ["ODE_v0", "ODE"]
WEIGHT_KEYS = TUNING_COLUMNS[:7]


def config(N, H, predictor, math_mode, rpl, **kw):
    return MPPIConfig(num_rollouts=N, mpc_horizon=H, predictor_type=predictor, math_mode=math_mode, rollouts_per_lane=rpl, **kw)


def engine(E, cfg):
    from cartpolesimulation_amd.engine import MPPIEngine
    return MPPIEngine(E, cfg)


def random_envs(E, H, seed):
    rng = Generator(SFC64(seed))
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.8, 0.8), rng.uniform(-3, 3), rng.uniform(-0.12, 0.12),
                                           rng.uniform(-0.3, 0.3)) for _ in range(E)])
    tp = rng.uniform(-0.08, 0.08, E).astype(f32)
    Lv = rng.uniform(0.25, 0.45, E).astype(f32)
    u0 = (0.3 * rng.standard_normal((E, H))).astype(f32)
    return s0, tp, Lv, u0, rng


def random_columns(E, rng, sigma=True):
    """Rows that differ from the configuration and from each other in every column (the permissible track fraction low enough for
    the boundary term to count for carts near +-0.12 m)."""
    cols = dict(dd_quadratic_weight_up=rng.uniform(5, 40, E), db_weight_up=rng.uniform(2000, 20000, E), ep_weight_up=rng.uniform(10, 90, E),
                ekp_weight_up=rng.uniform(0.2, 3, E), cc_weight_up=rng.uniform(1, 9, E), R=rng.uniform(0.5, 2, E),
                permissible_track_fraction=rng.uniform(0.4, 0.9, E), LBD=rng.uniform(20, 300, E))
    if sigma:
        cols["SQRTRHOINV"] = rng.uniform(0.01, 0.06, E)
    return cols


def philox_step(eng, s0, u0, tp, Lv, seed=11, offset=4):
    E = s0.shape[0]
    un, S = eng.tensor(u0.copy()), eng.empty(E, eng.N)
    Q, _ = eng.step(s0, un, tp, np.ones(E, f32), L=Lv, seed=seed, offset=offset, env_offset=0, S_out=S)
    return Q.cpu().numpy(), un.cpu().numpy(), S.cpu().numpy()


def scalar_engine(E, cfg, cols, e):
    """An engine of the same shape whose configuration is env e's row: LBD and SQRTRHOINV at creation, the weights through set_cost."""
    cfg_e = replace(cfg, LBD=float(cols["LBD"][e]), SQRTRHOINV=float(cols.get("SQRTRHOINV", [cfg.SQRTRHOINV] * E)[e]))
    eng = engine(E, cfg_e)
    eng.set_cost("quadratic_boundary_grad_minimal", {k: float(cols[k][e]) for k in WEIGHT_KEYS})
    return eng


def rows_match_scalar_engines(E, cfg, seed, envs):
    """One launch with rows; for every env of `envs` a launch of a second engine configured with that env's row: the same build,
    that env bit for bit, another env not.  -> the build variant."""
    H = cfg.mpc_horizon
    s0, tp, Lv, u0, rng = random_envs(E, H, seed)
    cols = random_columns(E, rng)
    eng = engine(E, cfg)
    eng.set_tuning_rows(tuning_rows(cfg, E, **cols))
    Q, un, S = philox_step(eng, s0, u0, tp, Lv)
    info = eng.last_launch()
    eng.close()
    assert np.isfinite(S).all() and np.isfinite(un).all()
    for e in envs:
        other = scalar_engine(E, cfg, cols, e)
        Qe, une, Se = philox_step(other, s0, u0, tp, Lv)
        info_e = other.last_launch()
        other.close()
        assert {k: info_e[k] for k in ("build_variant", "rollouts_per_lane", "math_mode", "blocks")} == \
               {k: info[k] for k in ("build_variant", "rollouts_per_lane", "math_mode", "blocks")}
        assert np.array_equal(Se[e], S[e]) and np.array_equal(une[e], un[e]) and Qe[e] == Q[e], f"env {e}"
        o = (e + 1) % E
        assert not np.array_equal(Se[o], S[o]) and not np.array_equal(une[o], un[o]), f"env {o} under env {e}'s scalars"
    return info["build_variant"]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predictor", PREDICTORS)
@pytest.mark.parametrize("math_mode,rpl", LANE_MODES)
def test_equal_rows_are_the_scalar(math_mode, rpl, predictor):
    """E=3, N=200 (a ragged last block): rows that all equal the configuration give Q, u_nom and S of the launch without rows bit
    for bit; rows that differ do not."""
    E, N, H = 3, 200, 12
    cfg = config(N, H, predictor, math_mode, rpl)
    eng = engine(E, cfg)
    s0, tp, Lv, u0, rng = random_envs(E, H, 3)
    plain = philox_step(eng, s0, u0, tp, Lv)
    rows = eng.set_tuning_rows(tuning_rows(cfg, E))
    same = philox_step(eng, s0, u0, tp, Lv)
    for a, b in zip(plain, same):
        assert np.array_equal(a, b)
    # the pointer is what a launch fixes: the CONTENTS may change between launches
    rows.copy_(torch.from_numpy(tuning_rows(cfg, E, **random_columns(E, rng))))
    moved = philox_step(eng, s0, u0, tp, Lv)
    assert all(not np.array_equal(a[e], b[e]) for a, b in zip(plain[1:], moved[1:]) for e in range(E))
    eng.set_tuning_rows(None)
    assert eng._tuning is None
    for a, b in zip(plain, philox_step(eng, s0, u0, tp, Lv)):
        assert np.array_equal(a, b)
    eng.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predictor", PREDICTORS)
@pytest.mark.parametrize("math_mode,rpl", LANE_MODES)
def test_rows_are_independent(math_mode, rpl, predictor):
    E, N, H = 5, 200, 12
    rows_match_scalar_engines(E, config(N, H, predictor, math_mode, rpl), 6, range(E))


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
# the smallest shapes at which the plan selects each of the other builds (tests/launch_table.py's boundary rows; predictor_ODE:
# tests/test_gpu_pole_mass_rows.py's 100 / 300 envs x 1024), H = 12 and 13: the stage-only last stage for even and odd horizons
OTHER_BUILDS = [
    ("ODE_v0", "fast", 2, 2, 512, 12, 3),         # the lone-wave form of the mid-size build
    ("ODE_v0", "fast", 2, 257, 512, 13, 2),       # the mid-size build
    ("ODE_v0", "fast", 1, 512, 256, 13, 1),       # the throughput build, one rollout per lane: ENV_FOLD
    ("ODE_v0", "fast", 2, 3073, 512, 12, 1),      # the throughput build, two per lane: ENV_FOLD
    ("ODE_v0", "precise", 1, 40, 300, 13, 1),     # PRECISE: the throughput unit, stage_qbgm on the last stage from the kernarg copy
    ("ODE", "fast", 1, 100, 1024, 13, 1),
    ("ODE", "fast", 2, 300, 1024, 12, 1),
    ("ODE", "fast", 2, 256, 512, 13, 3),          # predictor_ODE's lone-wave form
    ("ODE", "precise", 1, 40, 300, 12, 1),
]


@pytest.mark.parametrize("predictor,math_mode,rpl,E,N,H,variant", OTHER_BUILDS)
def test_the_same_in_the_other_builds(predictor, math_mode, rpl, E, N, H, variant):
    got = rows_match_scalar_engines(E, config(N, H, predictor, math_mode, rpl), 7, sorted({0, E // 2, E - 1}))
    assert got == variant


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predictor", PREDICTORS)
@pytest.mark.parametrize("math_mode,rpl", LANE_MODES)
def test_fused_step_vs_the_c_oracle(math_mode, rpl, predictor):
    """Rows that share sigma and differ in weights and LBD; the draws are the sampler's for the same seed / offset (eng.sample); the
    C oracle is run per env under that env's weights and LBD."""
    E, N, H = 4, 1000, 30
    cfg = config(N, H, predictor, math_mode, rpl)
    eng = engine(E, cfg)
    s0, tp, Lv, u0, rng = random_envs(E, H, 41)
    te = np.ones(E, f32)
    cols = random_columns(E, rng, sigma=False)
    _, du = eng.sample(seed=11, offset=4, env_offset=0, knots=False, delta_u=True)
    du = du.cpu().numpy()
    eng.set_tuning_rows(tuning_rows(cfg, E, **cols))
    Q, un, S = philox_step(eng, s0, u0, tp, Lv, seed=11, offset=4)
    eng.close()
    rule = dict(rule=PU.PREDICTOR_ODE) if predictor == "ODE" else {}
    moved = 0.0
    for e in range(E):
        sl = slice(e, e + 1)
        w = {k: float(f32(cols[k][e])) for k in WEIGHT_KEYS}
        cost = O.CostConfig(qbgm_dd_quadratic_weight=w["dd_quadratic_weight_up"], qbgm_db_weight=w["db_weight_up"],
                            qbgm_ep_weight=w["ep_weight_up"], qbgm_ekp_weight=w["ekp_weight_up"], qbgm_cc_weight=w["cc_weight_up"],
                            qbgm_R=w["R"], qbgm_permissible_track_fraction=w["permissible_track_fraction"])
        ocfg = O.MPPIConfig(N=N, H=H, cc_weight=cfg.cc_weight, R=cfg.R, LBD=float(f32(cols["LBD"][e])), NU=cfg.NU, cost_id=O.COST_QBGM,
                            integrator=predictor, cost=cost)
        r = PU.c_oracle_step_with_flags(ocfg, s0[sl], u0[sl], du[sl], tp[sl], te[sl], L=Lv[sl], probes=True)
        PU.assert_costs(S[sl], r["S_a"], None, np.zeros_like(r["flags"]), f"env {e} costs", S_alt=r["S_alt"], flag_sensitive=True, **rule)
        PU.assert_controls(un[sl], r["u_a"], None, f"env {e} u_new", u_alt=r["u_alt"])
        np.testing.assert_allclose(Q[sl], r["Q_a"], atol=1e-4 + float(PU.envelope(r["u_a"], *r["u_alt"]).max()))
        d = PU.c_oracle_step_with_flags(replace(ocfg, cost=O.CostConfig(), LBD=cfg.LBD), s0[sl], u0[sl], du[sl], tp[sl], te[sl], L=Lv[sl])
        moved = max(moved, float((np.abs(d["S_a"] - r["S_a"]) / np.abs(r["S_a"])).max()))
    assert moved > 1e-3                                            # the default weights would not have passed


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_c_level_refusals():
    """Every refusal of include/cpmppi.h through ctypes: BAD_ARG, a text that names the call, nothing launched (outputs untouched);
    NULL restores the scalar result bit for bit."""
    E, N, H = 3, 200, 12
    cfg = config(N, H, "ODE", "fast", 1)
    eng = engine(E, cfg)
    lib, h = eng.lib, eng._h
    s0, tp, Lv, u0, rng = random_envs(E, H, 5)
    plain = philox_step(eng, s0, u0, tp, Lv)
    rows = eng.tensor(tuning_rows(cfg, E + 1, **random_columns(E + 1, rng)))
    err = lambda: lib.cpmppi_last_error(h).decode()                                       # noqa: E731

    # registration
    assert lib.cpmppi_set_tuning_rows(h, rows.data_ptr(), 0) == -1 and err().startswith("cpmppi_set_tuning_rows: ")
    assert lib.cpmppi_set_tuning_rows(h, rows.data_ptr() + 16, E) == -1 and "misaligned" in err()
    masses = eng.tensor(np.full(E, 0.05, f32))
    assert lib.cpmppi_set_pole_mass_rows(h, masses.data_ptr(), E) == 0
    assert lib.cpmppi_set_tuning_rows(h, rows.data_ptr(), E) == -1 and "cpmppi_set_pole_mass_rows" in err()
    assert lib.cpmppi_set_pole_mass_rows(h, None, 0) == 0
    for a, b in zip(plain, philox_step(eng, s0, u0, tp, Lv)):                                # (nothing was registered by a refused call)
        assert np.array_equal(a, b)
    other = engine(E, replace(cfg, cost_function_specification="default"))
    assert other.lib.cpmppi_set_tuning_rows(other._h, rows.data_ptr(), E) == -1
    assert other.lib.cpmppi_last_error(other._h).decode().startswith("cpmppi_set_tuning_rows: ")
    other.close()

    # while rows are registered
    assert lib.cpmppi_set_tuning_rows(h, rows.data_ptr(), E - 1) == 0                          # fewer rows than the launch has envs
    un, S, Q = eng.tensor(u0.copy()), torch.full((E, N), -7.0, device=rows.device), torch.full((E,), -7.0, device=rows.device)
    te = eng.tensor(np.ones(E, f32))
    s0_t, tp_t, L_t = eng.tensor(s0), eng.tensor(tp), eng.tensor(Lv)

    def step_block(**over):
        a = L.cpmppi_step_args()
        a.E, a.s0, a.u_nom, a.target_position, a.target_equilibrium, a.L = E, s0_t.data_ptr(), un.data_ptr(), tp_t.data_ptr(), te.data_ptr(), L_t.data_ptr()
        a.noise_kind, a.seed, a.offset, a.Q_out, a.S_out = L.NOISE_PHILOX, 11, 4, Q.data_ptr(), S.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.all(S == -7.0)) and bool(torch.all(Q == -7.0)) and np.array_equal(un.cpu().numpy(), u0)

    assert lib.cpmppi_step(h, C.byref(step_block()), eng._stream()) == -1 and "registered 2 rows" in err() and untouched()
    assert lib.cpmppi_set_tuning_rows(h, rows.data_ptr(), E + 1) == 0
    knots = eng.zeros(E, N, cfg.num_knots)
    assert lib.cpmppi_step(h, C.byref(step_block(noise_kind=L.NOISE_KNOTS, noise=knots.data_ptr())), eng._stream()) == -1
    assert err().startswith("cpmppi_step: ") and "CPMPPI_NOISE_PHILOX" in err() and untouched()
    assert lib.cpmppi_set_pole_mass_rows(h, masses.data_ptr(), E) == -1 and "cpmppi_set_tuning_rows" in err()
    w = (C.c_float * 4)(600.0, 20000.0, 1.0, 1.0)
    assert lib.cpmppi_set_cost_weights(h, L.COST_DEFAULT, w, 4) == -1 and err().startswith("cpmppi_set_cost_weights: ")
    # the other entry points refuse by name: every call below has a VALID argument list (it succeeds once the rows are gone, see the
    # control at the end), so the refusal it meets is the one about the rows - its text says so
    def refused_for_rows(rc, who):
        text = err()
        return rc == -1 and text.startswith(who + ": ") and "cpmppi_set_tuning_rows" in text

    st = eng._stream
    inputs, out = eng.zeros(E, N, H), torch.full((E, N), -7.0, device=rows.device)
    vp = lambda t: C.c_void_p(t.data_ptr())                                                # noqa: E731
    grad = torch.full((E, N, H), -7.0, device=rows.device)
    traj_in, traj = eng.zeros(E, H + 1, 6), torch.full((E, H + 1, 6), -7.0, device=rows.device)
    knots_out = torch.full((E, N, cfg.num_knots), -7.0, device=rows.device)
    tiled = torch.full((int(lib.cpmppi_tiled_floats(h, E)),), -7.0, device=rows.device)
    rwa = torch.full((E, H), -7.0, device=rows.device)
    Sin = eng.zeros(E, N)
    hp = dict(learning_rate=0.05, beta1=0.9, beta2=0.999, epsilon=1e-2, gradmax_clip=5.0)
    Qp, mp, vv = eng.tensor((0.1 * rng.standard_normal((E, N, H))).astype(f32)), eng.zeros(E, N, H), eng.zeros(E, N, H)
    Qp0 = Qp.clone()
    u_rpgd = torch.full((E,), -7.0, device=rows.device)
    rpgd = eng.prepare_rpgd_step(s0_t, Qp, mp, vv, tp_t, te, L=L_t, iterations=2, Q_out=u_rpgd, **hp)
    mean, stdev = eng.zeros(E, H), eng.tensor(np.full((E, H), 0.5, f32))
    u_cem = torch.full((E,), -7.0, device=rows.device)
    cem = eng.prepare_cem_step(s0_t, mean, stdev, tp_t, te, L=L_t, iterations=2, best_k=20, stdev_min=0.1, seed=3, Q_out=u_cem)
    calls = {
        "cpmppi_rollout_cost": lambda: lib.cpmppi_rollout_cost(h, E, vp(s0_t), vp(inputs), vp(tp_t), vp(te), vp(L_t), vp(out), st()),
        "cpmppi_rollout_cost_grad": lambda: lib.cpmppi_rollout_cost_grad(h, E, vp(s0_t), vp(inputs), vp(tp_t), vp(te), vp(L_t), None, vp(out),
                                                                         vp(grad), st()),
        "cpmppi_predict": lambda: lib.cpmppi_predict(h, E, H, vp(s0_t), vp(un), vp(L_t), vp(traj), st()),
        "cpmppi_trajectory_cost": lambda: lib.cpmppi_trajectory_cost(h, E, H, vp(traj_in), vp(un), 0.0, 1.0, None, None, None, None, vp(Q), st()),
        "cpmppi_rpgd_step": lambda: lib.cpmppi_rpgd_step(h, rpgd.ref, st()),
        "cpmppi_cem_step": lambda: lib.cpmppi_cem_step(h, cem.ref, st()),
        "cpmppi_sample": lambda: lib.cpmppi_sample(h, E, 11, 4, 0, vp(knots_out), None, st()),
        "cpmppi_sample_tiled": lambda: lib.cpmppi_sample_tiled(h, E, 11, 4, 0, None, vp(tiled), st()),
        "cpmppi_reward_weighted_average": lambda: lib.cpmppi_reward_weighted_average(h, E, vp(Sin), vp(inputs), vp(rwa), st()),
    }
    for who, call in calls.items():
        assert refused_for_rows(call(), who), (who, err())
    # (the GRU cost entry points: before the model is looked for, as the GRU step)
    assert refused_for_rows(lib.cpmppi_rollout_cost_gru(h, E, vp(s0_t), vp(inputs), vp(tp_t), vp(te), None, vp(out), st()), "cpmppi_rollout_cost_gru")
    assert refused_for_rows(lib.cpmppi_rollout_cost_grad_gru(h, E, vp(s0_t), vp(inputs), vp(tp_t), vp(te), None, vp(out), vp(grad), st()),
                            "cpmppi_rollout_cost_grad_gru")
    torch.cuda.synchronize()
    for t in (out, grad, traj, knots_out, tiled, rwa, u_rpgd, u_cem):
        assert bool(torch.all(t == -7.0))
    assert torch.equal(Qp, Qp0) and bool(torch.all(mean == 0.0)) and bool(torch.all(stdev == 0.5)) and untouched()

    # the rows work once nothing stands in the way, and NULL restores the scalar result bit for bit
    tuned = philox_step(eng, s0, u0, tp, Lv)
    assert not np.array_equal(tuned[2], plain[2])
    assert lib.cpmppi_set_tuning_rows(h, None, 0) == 0
    for a, b in zip(plain, philox_step(eng, s0, u0, tp, Lv)):
        assert np.array_equal(a, b)
    # the control: the very calls refused above go through now (the rows were all that stood in their way)
    for who, call in calls.items():
        assert call() == 0, (who, err())
    torch.cuda.synchronize()
    for t in (out, grad, traj, knots_out, tiled, rwa, u_rpgd, u_cem):
        assert not bool(torch.all(t == -7.0))
    eng.close()


def test_gru_step_and_env_groups_refuse():
    """While rows are registered a GRU step is refused by name (before the model is even looked for), and cpmppi_groups_run refuses
    a group whose handle holds rows; nothing is launched."""
    E, N, H = 2, 64, 8
    cfg = config(N, H, "ODE_v0", "fast", 1)
    from cartpolesimulation_amd.configs import build_c_config
    lib = L.load()
    g = C.c_void_p()
    assert lib.cpmppi_groups_create(C.byref(build_c_config(E, cfg)), 0, 2, 0, C.byref(g)) == 0
    h0 = lib.cpmppi_groups_handle(g, 0)
    rows = torch.as_tensor(tuning_rows(cfg, E), device="cuda")
    assert lib.cpmppi_set_tuning_rows(h0, rows.data_ptr(), E) == 0
    s0 = torch.zeros(E, 6, device="cuda"); s0[:, 2] = 1.0                                 # noqa: E702
    un, tp, te, Q = (torch.zeros(E, H, device="cuda"), torch.zeros(E, device="cuda"), torch.ones(E, device="cuda"),
                     torch.full((E,), -7.0, device="cuda"))
    a = L.cpmppi_step_args()
    a.E, a.s0, a.u_nom, a.target_position, a.target_equilibrium = E, s0.data_ptr(), un.data_ptr(), tp.data_ptr(), te.data_ptr()
    a.noise_kind, a.seed, a.Q_out = L.NOISE_PHILOX, 3, Q.data_ptr()
    assert lib.cpmppi_groups_run(g, C.byref(a), None, 1) == -1
    text = lib.cpmppi_groups_last_error(g).decode()
    assert text.startswith("cpmppi_groups_run: group 0: cpmppi_groups_run: ") and "cpmppi_set_tuning_rows" in text
    torch.cuda.synchronize()
    assert bool(torch.all(Q == -7.0))
    a.predictor, a.E = L.PREDICTOR_GRU, 1                                                 # (group 0 holds one of the two envs)
    assert lib.cpmppi_step(h0, C.byref(a), None) == -1
    text = lib.cpmppi_last_error(h0).decode()
    assert text.startswith("cpmppi_step: ") and "cpmppi_set_tuning_rows" in text and "GRU" in text
    torch.cuda.synchronize()
    assert bool(torch.all(Q == -7.0))
    lib.cpmppi_groups_destroy(g)


# ---- the step without the fused finalize ---------------------------------------------------------------------------------------
# envs of more than one block (one block's partial is merged with weight exp(0): no LBD in it), and of more than eight (the merge
# rescales its running sums between batches of eight blocks): N = 600 -> 3 blocks, 1300 at two per lane -> 3, 2400 -> 10
SEPARATE_FINALIZE = [("ODE_v0", "fast", 1, 3, 600, 12, 3), ("ODE", "fast", 2, 3, 1300, 13, 3), ("ODE", "precise", 1, 2, 2400, 12, 10)]


@pytest.mark.parametrize("predictor,math_mode,rpl,E,N,H,nb", SEPARATE_FINALIZE)
def test_separate_finalize_merges_with_the_rows_lbd(monkeypatch, predictor, math_mode, rpl, E, N, H, nb):
    """A handle created with CPMPPI_FUSE_FINALIZE=0 (read at creation) merges the envs' block partials in a kernel of its own behind
    the rollout kernel: with rows registered that kernel takes the soft-min's LBD from the env's row, as the partials were scaled -
    env e is, bit for bit, env e of a handle (created the same way) whose scalars are its row; another env is not."""
    monkeypatch.setenv("CPMPPI_FUSE_FINALIZE", "0")
    cfg = config(N, H, predictor, math_mode, rpl)
    s0, tp, Lv, u0, rng = random_envs(E, H, 17)
    cols = random_columns(E, rng)
    eng = engine(E, cfg)
    eng.set_tuning_rows(tuning_rows(cfg, E, **cols))
    eng.set_profiling(True)
    Q, un, S = philox_step(eng, s0, u0, tp, Lv)
    _, finalize_ms = eng.get_profile()
    info = eng.last_launch()
    eng.close()
    assert len(finalize_ms) == 1 and finalize_ms[0] > 0.0          # (a kernel ran behind the rollout kernel: the finalize)
    assert info["blocks"] == E * nb and np.isfinite(un).all()
    for e in (0, E - 1):
        other = scalar_engine(E, cfg, cols, e)
        Qe, une, Se = philox_step(other, s0, u0, tp, Lv)
        assert other.last_launch()["blocks"] == info["blocks"]
        other.close()
        assert np.array_equal(Se[e], S[e]) and np.array_equal(une[e], un[e]) and Qe[e] == Q[e], f"env {e}"
        o = (e + 1) % E
        assert not np.array_equal(une[o], un[o]), f"env {o} under env {e}'s scalars"


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def test_device_loop_with_tuning_rows():
    """E=4, N=512, H=20, a 0.3 s schedule batch: run_schedule(tuning=rows) is the loop paced by hand around set_tuning_rows bit for
    bit; the captured loop is the launched one; an env whose row is the configuration is that env of an untuned run; the handle is
    left without rows.  The same for the plain `run` loop."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    E, N, H = 4, 512, 20
    scfg = dict(seed=33, length_of_experiment=0.3, keep_target_equilibrium_x_seconds_up=0.1, turning_points=dict(track_relative_complexity=12),
                random_initial_state=dict(init_limits=dict(angle=[0.0, 20.0], angleD=40.0, position=0.4, positionD=0.2)))
    b = SC.RandomExperimentSetter(scfg).draw(E, 78)
    cfg = MPPIConfig(num_rollouts=N, mpc_horizon=H)
    eng = engine(E, cfg)
    cols = random_columns(E, Generator(SFC64(9)))
    rows = tuning_rows(cfg, E, **cols)
    rows[0] = tuning_rows(cfg, 1)[0]                                  # env 0: the configuration itself
    exp = BatchedCartPoleExperiment(eng, seed=7)
    plain = exp.run_schedule(b)
    tuned = exp.run_schedule(b, tuning=rows)
    assert eng._tuning is None and tuned["tuning"].shape == (E, L.TUNING_ROW_FLOATS)
    captured = exp.run_schedule(b, tuning=rows, graph=True, steps_per_graph=5)
    assert eng._tuning is None
    for key in ("states", "Q", "dd", "u_nom"):
        assert torch.equal(tuned[key], captured[key]), key
    assert torch.equal(tuned["states"][:, 0], plain["states"][:, 0]) and torch.equal(tuned["Q"][:, 0], plain["Q"][:, 0])
    assert not torch.equal(tuned["Q"][:, 1:], plain["Q"][:, 1:])
    # paced by hand: the controller calls of the run, each from the state the recording holds for its row
    assert b.n_ctrl % b.n_save == 0                                   # (every controller call falls on a saved row)
    eng.set_tuning_rows(rows)
    u = eng.zeros(E, H)
    states = tuned["states"].cpu().numpy()
    for c in range(b.n_periods + 1):
        row = int(b.rows_at(c * b.n_ctrl))
        s = states[c * b.n_ctrl // b.n_save]
        Q, _ = eng.step(s, u, b.target_position[row].astype(f32), b.target_equilibrium[row].astype(f32), seed=7, offset=c)
        assert torch.equal(Q, tuned["Q"][c]), c
    eng.set_tuning_rows(None)
    # the plain loop, launched and captured
    s0 = b.s0
    r0 = exp.run(s0, 12)
    r1 = exp.run(s0, 12, tuning=rows)
    r2 = exp.run(s0, 12, tuning=rows, graph=True, steps_per_graph=4)
    assert eng._tuning is None
    assert torch.equal(r1["states"], r2["states"]) and torch.equal(r1["Q"], r2["Q"])
    assert torch.equal(r1["Q"][:, 0], r0["Q"][:, 0]) and not torch.equal(r1["Q"][:, 1:], r0["Q"][:, 1:])
    # the score of the tuned run, from its logs where they lie, against the numpy restatement on the recording's own columns
    from cartpolesimulation_amd.recording import recording_block, score_rows
    from cartpolesimulation_amd.configs import PhysicalParameters
    got = eng.score_runs(tuned["states"], tuned["Q"], target_position_table=eng.tensor(b.target_position.astype(f32)),
                         save_every=b.n_save, sched_stride=b.stride, period_steps=b.n_ctrl).cpu().numpy()
    block = recording_block(tuned, PhysicalParameters())
    ref = score_rows(block["states"], block["target_position"].astype(f32), tuned["Q"].cpu().numpy())
    R = block["states"].shape[0]
    assert np.all(np.abs(got[:, :4] - ref[:, :4]) <= R * 2.0 ** -24 * np.abs(ref[:, :4])) and np.array_equal(got[:, 4], ref[:, 4])
    eng.close()
