"""GPU: CEM over the same rollout + cost kernel — sampler (statistics, and sample by sample against Philox),
cost-only launch, top-k refit (and its edges: best_k = 1 / N, +-inf, +-0.0, ties, NaN), optimizer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O
import parity_util as PU  # noqa: E402

f32 = np.float32


def make(E, N, H, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    return MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, shift_mode="none", **kw))


def test_cem_sample_cost_update_vs_oracle():
    E, N, H, K = 3, 200, 35, 40                                   # the shipped cem-tf sizes, 3 envs
    eng = make(E, N, H)
    rng = np.random.Generator(np.random.SFC64(4))
    mean = (0.2 * rng.standard_normal((E, H))).astype(f32)
    stdev = rng.uniform(0.05, 0.6, (E, H)).astype(f32)
    Q = eng.cem_sample(mean, stdev, seed=8, offset=2)
    Qh = Q.cpu().numpy()
    assert Qh.shape == (E, N, H) and np.abs(Qh).max() <= 1.0
    # far from the limits nothing is clipped: the samples are mean + stdev * N(0,1)
    m0, sd0 = np.zeros((E, H), f32) + 0.1, np.zeros((E, H), f32) + 0.05
    z = (eng.cem_sample(m0, sd0, seed=8, offset=9).cpu().numpy() - 0.1) / 0.05
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1.0) < 0.03 and abs((z ** 3).mean()) < 0.1
    assert np.array_equal(eng.cem_sample(mean, stdev, seed=8, offset=2).cpu().numpy(), Qh)
    assert not np.array_equal(eng.cem_sample(mean, stdev, seed=8, offset=3).cpu().numpy(), Qh)
    # cost-only launch == cost_function.get_trajectory_cost(predictor.predict_core(s, Q), Q)
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1), 0.0)
                   for _ in range(E)])
    tp = rng.uniform(-0.05, 0.05, E).astype(f32)
    Lv = rng.uniform(0.25, 0.45, E).astype(f32)
    S = eng.rollout_cost(s0, Q, tp, np.ones(E, f32), L=Lv)
    Sh = S.cpu().numpy()
    for e in range(E):
        traj = O.predict_core(s0[e], Qh[e], L=Lv[e])
        ref = O.trajectory_cost(O.COST_QBGM, traj, Qh[e], tp[e], f32(1.0))
        ref_b = O.trajectory_cost(O.COST_QBGM, O.predict_core(s0[e], Qh[e], L=Lv[e], mode="f64sub"), Qh[e], tp[e], f32(1.0))
        PU.assert_costs(Sh[e], ref, ref_b, PU.flag_discontinuities(traj), f"env {e} costs")
    # top-k refit on the device's own costs: exact elite set, mean/std to rounding
    m2, s2, el = eng.cem_update(S, Q, K, 0.01, return_elites=True)
    for e in range(E):
        mr, sr, idx = O.cem_update(Sh[e], Qh[e], K, 0.01)
        assert np.array_equal(el.cpu().numpy()[e], idx)
        np.testing.assert_allclose(m2.cpu().numpy()[e], mr, atol=1e-6)
        np.testing.assert_allclose(s2.cpu().numpy()[e], sr, atol=2e-6)
    # ties and N not a power of two: equal costs keep index order
    St = torch.zeros(E, N, device=S.device)
    _, _, el2 = eng.cem_update(St, Q, 7, 0.0, return_elites=True)
    assert np.array_equal(el2.cpu().numpy(), np.tile(np.arange(7), (E, 1)))


def test_cem_update_at_the_largest_population():
    """N = 16384 needs 128 KB of dynamic LDS for the top-k sort (the opt-in above the default 64 KB): exact elite set
    and refit against the oracle; N one above that is refused cleanly."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H, K = 2, 16384, 6, 300
    eng = make(E, N, H)
    rng = np.random.Generator(np.random.SFC64(12))
    S = rng.uniform(0.0, 1e4, (E, N)).astype(f32)
    Q = rng.uniform(-1, 1, (E, N, H)).astype(f32)
    m, sd, el = eng.cem_update(S, Q, K, 0.01, return_elites=True)
    for e in range(E):
        mr, sr, idx = O.cem_update(S[e], Q[e], K, 0.01)
        assert np.array_equal(el.cpu().numpy()[e], idx)
        np.testing.assert_allclose(m.cpu().numpy()[e], mr, atol=2e-6)
        np.testing.assert_allclose(sd.cpu().numpy()[e], sr, atol=5e-6)
    big = make(1, 16385, 4)
    with pytest.raises(CpmppiError):
        big.cem_update(np.zeros((1, 16385), f32), np.zeros((1, 16385, 4), f32), 5, 0.01)


def test_optimizer_cem_improves_and_controls():
    from types import SimpleNamespace
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    vp = SimpleNamespace(target_position=f32(0.0), target_equilibrium=f32(1.0))
    opt = optimizer_cem(control_limits=(np.array([-1.0]), np.array([1.0])), seed=2, mpc_horizon=35, num_rollouts=200,
                        cem_outer_it=3, cem_best_k=40, variable_parameters=vp, cost_function_specification="default",
                        optimizer_logging=True)
    opt.configure(dt=0.02)
    s = O.create_cartpole_state(0.25, 0.0, 0.02, 0.0)
    u = opt.step(s)
    assert u.shape == (1,) and abs(float(u[0])) <= 1.0
    assert float(opt.stdev[0, -1]) == pytest.approx(np.sqrt(0.5)) and float(opt.dist_mue[0, -1]) == 0.0
    assert (opt.stdev[0, :-1] >= 0.01 - 1e-7).all() and float(opt.stdev[0, :5].mean()) < 0.5        # refit tightened it
    # the refit distribution is better than the prior: mean cost of fresh samples drops over the outer iterations
    eng = opt.engine
    prior = eng.rollout_cost(s[None], eng.cem_sample(eng.zeros(1, 35), eng.zeros(1, 35) + 0.5, 5), 0.0, 1.0).mean()
    opt.optimizer_reset()
    opt.step(s)
    mue = torch.cat([opt.dist_mue[:, -1:], opt.dist_mue[:, :-1]], 1)                                # undo the shift
    sd = torch.cat([opt.stdev[:, -1:] * 0 + 0.01, opt.stdev[:, :-1]], 1)
    post = eng.rollout_cost(s[None], eng.cem_sample(mue.contiguous(), sd.contiguous(), 5), 0.0, 1.0).mean()
    assert float(post) < float(prior)
    # through the controller seam, closed loop with the device plant: stays upright
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0},
                          (np.array([-1.0], f32), np.array([1.0], f32)),
                          config=dict(num_rollouts=256, mpc_horizon=35, seed=1, cost_function_specification="default"))
    ctrl.configure("cem")
    assert ctrl.optimizer.optimizer_name == "cem"
    st = eng.tensor(O.create_cartpole_state(0.1, 0.0, 0.0, 0.0)[None].copy())
    for t in range(60):
        q = ctrl.step(st.cpu().numpy()[0], time=0.02 * t)
        eng.plant_advance(st, q.astype(f32), n_substeps=10, dt_sim=0.002)
    fin = st.cpu().numpy()[0]
    assert abs(fin[0]) < 0.3 and abs(fin[4]) < 0.198


@pytest.mark.parametrize("name,N", [("cem-naive-grad-tf", 200), ("cem-grad-bharadhwaj-tf", 32), ("random-action-tf", 640)])
def test_cem_hybrids_and_random_action_through_the_controller_seam(name, N):
    """The remaining sampling optimizers of config_optimizers.yml (:21-48, :98-102) with their shipped sizes: the
    controller seam builds them, a step returns admissible controls, and a mildly perturbed pole stays up."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    E = 6
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                          control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=11))
    ctrl.configure(name)
    opt = ctrl.optimizer
    assert opt.num_rollouts == N and opt.mpc_horizon == 35 and name.startswith(opt.optimizer_name)
    eng = opt.engine
    rng = np.random.Generator(np.random.SFC64(6))
    s = eng.tensor(np.stack([O.create_cartpole_state(rng.uniform(-0.2, 0.2), rng.uniform(-0.4, 0.4), rng.uniform(-0.05, 0.05), 0.0)
                             for _ in range(E)]))
    Lv = np.full(E, 0.395, f32)
    Q0 = ctrl.step(s, 0.0, {})
    assert Q0.shape == (E, 1) and np.abs(Q0).max() <= 1.0
    for k in range(50):
        Q = opt.step(s, as_tensor=True)
        eng.plant_advance(s, Q, L=Lv, n_substeps=10)
    sh = s.cpu().numpy()
    assert np.abs(sh[:, O.POSITION_IDX]).max() < 0.198
    if name != "random-action-tf":          # (640 random plans per step do not balance a pole reliably; the CEM hybrids do)
        assert (np.abs(sh[:, O.ANGLE_IDX]) < 0.35).mean() >= 0.8
    with pytest.raises(NotImplementedError):
        ctrl.configure("no-such-optimizer")


def test_cem_gmm_sampler_and_optimizer():
    """cem-gmm-tf (config_optimizers.yml:12-20): the mixture sampler — uniform components, samples = centre + stdev z
    with the same z stream as the plain CEM sampler — and the optimizer over it through the controller seam."""
    from types import SimpleNamespace
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    E, N, H, K = 2, 4096, 10, 8
    eng = make(E, N, H)
    rng = np.random.Generator(np.random.SFC64(6))
    centres = rng.uniform(-0.5, 0.5, (E, K, H)).astype(f32)
    sd = rng.uniform(0.01, 0.05, (E, H)).astype(f32)
    Q, comp = eng.cem_gmm_sample(centres, sd, seed=3, offset=7, return_components=True)
    Qh, ch = Q.cpu().numpy(), comp.cpu().numpy()
    assert ch.min() == 0 and ch.max() == K - 1
    counts = np.stack([np.bincount(ch[e], minlength=K) for e in range(E)])
    assert np.abs(counts - N / K).max() < 5 * np.sqrt(N / K)                      # uniform over the components
    z = (Qh - centres[np.arange(E)[:, None], ch]) / sd[:, None, :]                # nothing clipped at these magnitudes
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    # the normals are the plain CEM sampler's for the same (seed, offset): Q - centre == stdev * z of cem_sample around 0
    plain = eng.cem_sample(np.zeros((E, H), f32), sd, seed=3, offset=7).cpu().numpy()
    np.testing.assert_allclose(Qh - centres[np.arange(E)[:, None], ch], plain, atol=2e-7)
    assert np.array_equal(eng.cem_gmm_sample(centres, sd, seed=3, offset=7).cpu().numpy(), Qh)
    # one component == the plain sampler
    one = eng.cem_gmm_sample(centres[:, :1].copy(), sd, seed=3, offset=7).cpu().numpy()
    np.testing.assert_array_equal(one, eng.cem_sample(centres[:, 0].copy(), sd, seed=3, offset=7).cpu().numpy())
    # the optimizer: stabilises the pole near upright and its sampling distribution contracts
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0}, control_limits=([-1.0], [1.0]),
                          config=dict(seed=4, mpc_horizon=35, num_rollouts=200, cem_outer_it=3, cem_best_k=40,
                                      cem_stdev_min=0.01, cem_initial_action_stdev=0.5))
    ctrl.configure("cem-gmm-tf")
    assert ctrl.optimizer.optimizer_name == "cem-gmm"
    s = O.create_cartpole_state(0.15, 0.0, 0.0, 0.0)
    for it in range(60):
        u = ctrl.step(s, 0.02 * it)
        s = O.ode_v0_step(s[None], np.asarray(u, f32))[0]
    assert abs(s[O.ANGLE_IDX]) < 0.1 and abs(s[O.POSITION_IDX]) < 0.15
    assert ctrl.optimizer.centres.shape == (1, 40, 35) and torch.isfinite(ctrl.optimizer.stdev).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# The samplers word for word against Philox (oracle/philox_np.py, pinned to Random123's vectors by tests/test_oracle_philox.py), and
# the top-k at its edges.
from oracle import philox_np as PH  # noqa: E402
from test_gpu_philox import Z_ATOL  # noqa: E402  (the measured bound of the same v_log / v_sqrt / v_sin / v_cos chain)

SEED, OFFSET, ENV_OFFSET = 2 ** 40 + 5, 2 ** 33 + 11, 123456        # a seed with a high word, an offset beyond 2^32, a large global env index
LO, HI = -0.5, 0.8


def report(capsys, text):
    with capsys.disabled():
        print("\n[optim] " + text)


def sampler_bound(stdev):
    """|Q_dev - oracle| per element: the normal's hardware error scaled by stdev[e, k], plus the rounding of the float32 fma result (half
    an ulp below 4 = 2^-23; beyond that both sides sit on a limit).  The clamp is 1-Lipschitz: clipped elements need no exemption."""
    return np.asarray(stdev, np.float64)[:, None, :] * Z_ATOL + 2.0 ** -23


@pytest.mark.parametrize("E,N,H", [(3, 300, 35), (2, 64, 1)])     # odd H over two blocks (900 rows: four); the H = 1 tail
def test_cem_sample_is_philox(E, N, H, capsys):
    eng = make(E, N, H, action_low=LO, action_high=HI)
    rng = np.random.Generator(np.random.SFC64(14))
    mean = rng.uniform(-0.1, 0.4, (E, H)).astype(f32)
    stdev = rng.uniform(0.15, 0.5, (E, H)).astype(f32)
    if H == 1:                                                   # (128 samples: one env towards each limit)
        mean, stdev = np.asarray([[0.45], [-0.15]], f32), np.asarray([[0.3], [0.3]], f32)
    Q = eng.cem_sample(mean, stdev, SEED, OFFSET, ENV_OFFSET).cpu().numpy()
    ref = PH.cem_samples(mean, stdev, SEED, OFFSET, ENV_OFFSET, N, LO, HI)
    clipped = ((ref == ref.min()) | (ref == ref.max())).mean()
    assert ref.min() == LO and ref.max() == float(f32(HI)) and 0.05 < clipped < 0.2        # about a tenth of the samples sit on a limit
    err = np.abs(Q.astype(np.float64) - ref)
    report(capsys, f"cem_sample {E}x{N}x{H}: worst |Q - philox| / bound {np.max(err / sampler_bound(stdev)):.3f}, worst abs {err.max():.2e}, "
                   f"clipped share {clipped:.3f}")
    assert np.all(err <= sampler_bound(stdev)), (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert Q.min() == f32(LO) and Q.max() == f32(HI)
    # the global env index keys the stream: env 1 at env_offset a == env 0 at env_offset a + 1, bit for bit; other words, other samples
    shifted = eng.cem_sample(mean[1:2].copy(), stdev[1:2].copy(), SEED, OFFSET, ENV_OFFSET + 1).cpu().numpy()
    assert np.array_equal(shifted[0], Q[1])
    assert not np.array_equal(eng.cem_sample(mean, stdev, SEED, OFFSET, 0).cpu().numpy(), Q)
    assert not np.array_equal(eng.cem_sample(mean, stdev, SEED, OFFSET - 2 ** 33, ENV_OFFSET).cpu().numpy(), Q)
    assert not np.array_equal(eng.cem_sample(mean, stdev, SEED - 2 ** 40, OFFSET, ENV_OFFSET).cpu().numpy(), Q)
    eng.close()


@pytest.mark.parametrize("K", [1, 3, 8])
def test_cem_gmm_sample_is_philox(K, capsys):
    E, N, H = 2, 300, 5
    eng = make(E, N, H, action_low=LO, action_high=HI)
    rng = np.random.Generator(np.random.SFC64(15 + K))
    centres = rng.uniform(-0.3, 0.6, (E, K, H)).astype(f32)
    stdev = rng.uniform(0.1, 0.4, (E, H)).astype(f32)
    Qt, ct = eng.cem_gmm_sample(centres, stdev, SEED, OFFSET, ENV_OFFSET, return_components=True)
    Q, comp = Qt.cpu().numpy(), ct.cpu().numpy()
    ref, comp_ref = PH.cem_gmm_samples(centres, stdev, SEED, OFFSET, ENV_OFFSET, N, LO, HI)
    assert np.array_equal(comp, comp_ref)                                            # every rollout's component, not only their histogram
    assert set(np.unique(comp)) == set(range(K))
    err = np.abs(Q.astype(np.float64) - ref)
    report(capsys, f"cem_gmm_sample K={K}: components equal, worst |Q - philox| / bound {np.max(err / sampler_bound(stdev)):.3f}")
    assert np.all(err <= sampler_bound(stdev)), (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert (ref == LO).any() and (ref == float(f32(HI))).any()
    Q1, c1 = eng.cem_gmm_sample(centres[1:2].copy(), stdev[1:2].copy(), SEED, OFFSET, ENV_OFFSET + 1, return_components=True)
    assert np.array_equal(c1.cpu().numpy()[0], comp[1]) and np.array_equal(Q1.cpu().numpy()[0], Q[1])
    Q0, c0 = eng.cem_gmm_sample(centres, stdev, SEED, OFFSET, 0, return_components=True)
    assert not np.array_equal(Q0.cpu().numpy(), Q) and (K == 1 or not np.array_equal(c0.cpu().numpy(), comp))
    eng.close()


def edge_costs(N, kind, seed):
    """Three cost vectors [3, N] with the values a sort can get wrong: +-inf, +-0.0, ties - and, kind "nan", NaNs among them (one in env
    0; several in env 1; in env 2 one with the sign bit set and a payload)."""
    rng = np.random.Generator(np.random.SFC64(seed))
    S = np.stack([(1e3 * rng.standard_normal(N)).astype(f32), rng.integers(-1, 3, N).astype(f32),
                  (1e3 * rng.standard_normal(N)).astype(f32)])
    specials = [[np.inf, -np.inf, 0.0, -0.0, np.inf, -0.0], [-0.0, 0.0, -0.0, np.inf, -np.inf, 0.0], [np.inf, np.inf, -np.inf, -np.inf, 0.0, -0.0]]
    nans = [[np.nan], [np.nan, np.nan, np.nan], [np.nan, np.nan]]
    for e in range(3):
        vals = (nans[e] if kind == "nan" else []) + (specials[e] if N > 1 else [])
        where = rng.choice(N, min(len(vals), N), replace=False)
        S[e, where] = np.asarray(vals, f32)[:len(where)]
    if kind == "nan":
        S[2].view(np.uint32)[np.flatnonzero(np.isnan(S[2]))[0]] = 0xFFC12345
        assert np.isnan(S).any(axis=1).all()
    return S


@pytest.mark.parametrize("kind", ["inf-zero-ties", "nan"])
@pytest.mark.parametrize("N,H,best_ks", [(1, 3, (1,)), (37, 5, (1, 37)), (300, 4, (1, 40, 300)), (200, 300, (40, 200))])
def test_cem_update_edges(N, H, best_ks, kind):
    """best_k = 1 and = N; N = 1, N = 37 (padded to 64 < one block), N = 300 (padded to 512: two passes per lane), H = 300 (more time-steps
    than lanes); costs with +-inf, +-0.0 and ties; and with NaN, which sorts last (oracle_np.cem_update = stable argsort; the network:
    tests/test_oracle_topk.py): one NaN with best_k = 40, NaNs with best_k = N - every elite index < N, Q allocated exactly [E, N, H]."""
    E = 3
    eng = make(E, N, H)
    rng = np.random.Generator(np.random.SFC64(16))
    S = edge_costs(N, kind, 40 + N)
    Q = rng.uniform(-1, 1, (E, N, H)).astype(f32)
    Sd, Qd = eng.tensor(S), eng.tensor(Q)
    assert np.array_equal(Sd.cpu().numpy().view(np.uint32), S.view(np.uint32))       # the costs reach the device bit for bit
    for best_k in best_ks:
        m, sd, el = eng.cem_update(Sd, Qd, best_k, 0.01, return_elites=True)
        el = el.cpu().numpy()
        assert el.min() >= 0 and el.max() < N
        for e in range(E):
            mr, sr, idx = O.cem_update(S[e], Q[e], best_k, 0.01)
            assert np.array_equal(el[e], idx), (best_k, e)
            np.testing.assert_allclose(m.cpu().numpy()[e], mr, atol=1e-6)
            np.testing.assert_allclose(sd.cpu().numpy()[e], sr, atol=2e-6)
        if kind == "nan" and best_k < N - 3:
            assert not np.isnan(S[np.arange(E)[:, None], el]).any()                  # enough other costs: no NaN among the elite
    eng.close()
