"""GPU: the fused rpgd / gradient control step over the GRU predictor (gru_rpgd_step_kernel, cpmppi_rpgd_step_gru,
MPPIEngine.rpgd_step_gru, optimizer_rpgd / optimizer_gradient(gru_model=..., gru_fused=True)) - against the entry points it fuses
composed in the test, its memory, its device step counter, the optimizers and the closed loop, its refusals.

Shapes: N = 16 (half a tile, the shipped rpgd size), 33 (one plan in the second wave), 40 (the gradient size), 128 (full); H = 1 (no
reverse step), 2 (one), 7 (odd, no multiple of the period 4), 8, and 16 x 35 once; E = 1 and 3; 1 and 3 iterations; shift 0, 1, 2;
keep_k = N and below N, the step count on and off a resampling; normal with a mean and uniform; both costs, both math modes, h0
NULL and a non-zero memory, the golden model (tests/golden/gru_c5.npz) and one set of random weights (test_gpu_gru_edges.model_of);
limits -0.9 / 0.8 with start plans beyond both.

Bounds.  Against the composition - `iterations` x (rollout_cost_grad(predictor="GRU", h0) -> adam_step), rollout_cost(predictor=
"GRU", h0), cem_update(return_elites=True) for the order, then gather, redraw and shift as optimizer_rpgd.step makes them - Q, m, v,
S, Q_out, plan_out and the order are compared on their bits: the kernel's statements are the staged kernels' (the precedents:
test_gpu_rpgd_fused.py measured Q, m, v bitwise over the ODE, test_gpu_gru_cost_only.py asserts S bit-equal between kernels that
share GruRollout).  One statement differs: the UNIFORM redraw maps a normal draw through erff in the kernel and through torch.erf in
the composition (optimizer_rpgd._shape_samples); the redrawn rows of the uniform cases are therefore bounded by 4 x the worst
deviation measured on an MI355X over all cases of this file (REDRAW_UNIFORM_MEASURED: no word differed in any redrawn row of the three
uniform cases that resample, so the bound, 4 x 0, is equality there too); every other row and every other quantity is bitwise."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from test_gpu_gru_edges import bits, draw_env, engine, model_of  # noqa: E402
from test_gpu_rpgd_fused import shifted  # noqa: E402

f32 = np.float32
SEED, ENV_OFFSET = 2 ** 40 + 11, 1000
QBGM, DEFAULT = "quadratic_boundary_grad_minimal", "default"
PERIOD, STDEV, LOW, HIGH = 4, 0.5, -0.9, 0.8
HP = dict(learning_rate=0.05, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=5.0)
MEAN, ULO, UHI = 0.15, -0.6, 0.7
# the uniform redraw, kernel (erff) against composition (torch.erf): worst |difference| of a redrawn control measured on an MI355X
# over the uniform cases below -> bound = 4 x worst
REDRAW_UNIFORM_MEASURED = 0.0
REDRAW_UNIFORM_TOL = 4.0 * REDRAW_UNIFORM_MEASURED


def report(capsys, text):
    with capsys.disabled():
        print("\n[rpgd-gru] " + text)


def make(E, N, H, model="golden", **kw):
    kw.setdefault("SQRTRHOINV", STDEV * math.sqrt(0.02))         # the sampler's sigma = the optimizer's sample_stdev
    return engine(E, N, H, model, shift_mode="none", control_mode="clip", period_interpolation_inducing_points=PERIOD,
                  action_low=LOW, action_high=HIGH, **kw)


def problem(E, N, H, seed, h_scale=0.2):
    """Per env: state, target position and memory as draw_env draws them; start plans with controls beyond either limit."""
    rng = np.random.Generator(np.random.SFC64(seed))
    envs = [draw_env(rng, H, 0.2, h_scale) for _ in range(E)]
    s0, tp, h0 = (np.stack([e[i] for e in envs]).astype(f32) for i in (0, 1, 3))
    Q = (0.3 * rng.standard_normal((E, N, H))).astype(f32)
    Q[:, 0] *= 4.0
    Q[:, 0, 0], Q[:, 1, 0] = 1.2, -1.3                           # (H = 1 as well: one control beyond each limit)
    return s0, tp, np.ones(E, f32), h0, Q


def fused(eng, s0, Q0, tp, te, h0, iterations, shift, m0=None, v0=None, **kw):
    E, N, H = Q0.shape
    Q = eng.tensor(Q0.copy())
    m = eng.tensor(m0.copy()) if m0 is not None else torch.zeros_like(Q)
    v = eng.tensor(v0.copy()) if v0 is not None else torch.zeros_like(Q)
    S, plan = eng.empty(E, N), eng.empty(E, H)
    order = torch.empty(E, N, dtype=torch.int32, device=Q.device)
    u = eng.rpgd_step_gru(s0, Q, m, v, tp, te, h0, iterations=iterations, shift=shift, S_out=S, plan_out=plan, order_out=order,
                          seed=SEED, env_offset=ENV_OFFSET, **dict(HP, **kw))[0]
    torch.cuda.synchronize()
    return dict(Q=Q.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), S=S.cpu().numpy(), plan=plan.cpu().numpy(),
                Q_out=u.cpu().numpy(), order=order.cpu().numpy())


def composed(eng, s0, Q0, tp, te, h0, iterations, shift, m0=None, v0=None, keep_k=None, resamp_per=0, count=0, adam_iteration=0,
             draw_offset=0, distribution="normal", sample_mean=0.0, uniform_lo=0.0, uniform_hi=0.0, **hp):
    """The same step from the existing entry points; gather, redraw and shift as optimizer_rpgd.step makes them.  -> numpy dict;
    `grad0` is the first iteration's staged gradient, `fresh` marks the redrawn rows."""
    hp = dict(HP, **hp)
    E, N, H = Q0.shape
    keep_k = N if keep_k is None else keep_k
    Q = eng.tensor(Q0.copy())
    m = eng.tensor(m0.copy()) if m0 is not None else torch.zeros_like(Q)
    v = eng.tensor(v0.copy()) if v0 is not None else torch.zeros_like(Q)
    grad0 = None
    for i in range(iterations):
        _, G = eng.rollout_cost_grad(s0, Q, tp, te, predictor="GRU", h0=h0)
        grad0 = G.cpu().numpy() if grad0 is None else grad0
        eng.adam_step(Q, G, m, v, adam_iteration + 1 + i, hp["learning_rate"], hp["beta1"], hp["beta2"], hp["epsilon"], hp["gradmax_clip"])
    S = eng.rollout_cost(s0, Q, tp, te, predictor="GRU", h0=h0)
    order = eng.cem_update(S, Q, N, 0.0, return_elites=True)[2]
    rows = torch.arange(E, device=Q.device)
    best = order[:, 0].long()
    out = dict(S=S.cpu().numpy(), order=order.cpu().numpy(), Q_out=Q[rows, best, 0].cpu().numpy(), plan=Q[rows, best].cpu().numpy(),
               grad0=grad0, fresh=np.zeros(N, bool))
    if resamp_per > 0 and keep_k < N and (count + 1) % resamp_per == 0:
        z = eng.sample(SEED, offset=draw_offset, env_offset=ENV_OFFSET, knots=False, delta_u=True)[1]
        if distribution == "normal":
            z = z + sample_mean if sample_mean != 0.0 else z
        else:
            z = uniform_lo + (uniform_hi - uniform_lo) * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))
        fresh = z.clamp_(LOW, HIGH)
        idx = order[:, :keep_k].long().unsqueeze(-1).expand(-1, -1, H)
        Q = torch.cat([torch.gather(Q, 1, idx), fresh[:, keep_k:]], dim=1)
        m = torch.cat([torch.gather(m, 1, idx), torch.zeros_like(m[:, keep_k:])], dim=1)
        v = torch.cat([torch.gather(v, 1, idx), torch.zeros_like(v[:, keep_k:])], dim=1)
        out["fresh"][keep_k:] = True
    out.update(Q=shifted(Q.cpu().numpy(), shift, True), m=shifted(m.cpu().numpy(), shift, False), v=shifted(v.cpu().numpy(), shift, False))
    return out


# ---- 1. equals the composition, bit for bit -------------------------------------------------------------------------------------
# (N, H, E, iterations, shift, keep_k, resamp_per, count, distribution, cost, math mode, a memory?, model, gradmax_clip)
COMPOSED_CASES = [
    (16, 1, 1, 1, 0, 16, 0, 0, "normal", QBGM, "fast", False, "golden", 5.0),          # no reverse step, no resampling, no shift
    (16, 2, 3, 3, 1, 12, 2, 3, "normal", DEFAULT, "precise", True, "random", 5.0),     # one reverse step; resamples
    (16, 7, 3, 3, 1, 12, 2, 2, "uniform", QBGM, "fast", True, "golden", 5.0),          # keep_k < N off the period: no resampling
    (16, 8, 1, 1, 2, 12, 5, 4, "uniform", DEFAULT, "fast", True, "golden", 5.0),       # resamples, uniform
    (33, 7, 3, 3, 2, 20, 3, 2, "normal", QBGM, "precise", True, "golden", 5.0),
    (33, 8, 1, 1, 0, 33, 2, 1, "normal", DEFAULT, "fast", False, "random", 5.0),       # keep_k = N on the period: no resampling
    (33, 2, 3, 3, 0, 1, 1, 0, "uniform", QBGM, "precise", False, "random", 5.0),       # keep_k = 1, shift 0: resampling alone
    (40, 7, 3, 3, 1, 40, 0, 0, "normal", QBGM, "fast", True, "golden", 5.0),           # gradient: never resamples
    (40, 8, 3, 1, 1, 30, 2, 1, "normal", DEFAULT, "precise", True, "golden", 0.0),     # the norm clip off
    (128, 7, 3, 3, 1, 96, 2, 1, "normal", DEFAULT, "fast", True, "golden", 5.0),
    (128, 8, 1, 3, 2, 128, 0, 0, "normal", QBGM, "precise", True, "random", 5.0),
    (128, 1, 3, 1, 1, 64, 1, 0, "uniform", DEFAULT, "precise", False, "golden", 5.0),
    (40, 7, 3, 3, 1, 40, 0, 0, "normal", QBGM, "fast", True, "random", "split"),        # the norm clip between the plans' norms
    (16, 35, 3, 4, 1, 12, 10, 9, "normal", QBGM, "fast", True, "golden", 5.0),         # the shipped rpgd shape, resampling
]


@pytest.mark.parametrize("N,H,E,iterations,shift,keep_k,resamp_per,count,distribution,cost,math_mode,memory,model,clipn", COMPOSED_CASES)
def test_fused_equals_the_composed_entry_points(N, H, E, iterations, shift, keep_k, resamp_per, count, distribution, cost, math_mode,
                                                memory, model, clipn, capsys):
    sigma = 1.0 if distribution == "uniform" else STDEV
    eng = make(E, N, H, model, cost_function_specification=cost, math_mode=math_mode, SQRTRHOINV=sigma * math.sqrt(0.02))
    s0, tp, te, h0, Q0 = problem(E, N, H, 500 + N + H)
    h0 = h0 if memory else None
    rng = np.random.Generator(np.random.SFC64(7 * N + H))
    m0 = (0.1 * rng.standard_normal(Q0.shape)).astype(f32) if count else None          # (a first step starts from zero moments)
    v0 = (0.01 * rng.uniform(0.1, 1.0, Q0.shape)).astype(f32) if count else None
    if clipn == "split":          # a clip between the smallest and the largest gradient norm of the start plans, from the staged gradient
        g = eng.rollout_cost_grad(s0, eng.tensor(Q0), tp, te, predictor="GRU", h0=h0)[1].cpu().numpy()
        nrm = np.sqrt((g.astype(np.float64) ** 2).sum(-1))
        clipn = float(np.median(nrm))
        assert (nrm > 1.01 * clipn).any() and (nrm < 0.99 * clipn).any()
    kw = dict(m0=m0, v0=v0, keep_k=keep_k, resamp_per=resamp_per, count=count, adam_iteration=count * iterations, draw_offset=5,
              distribution=distribution, sample_mean=MEAN, uniform_lo=ULO, uniform_hi=UHI, gradmax_clip=clipn)
    ref = composed(eng, s0, Q0, tp, te, h0, iterations, shift, **kw)
    got = fused(eng, s0, Q0, tp, te, h0, iterations, shift, **kw)
    eng.close()
    resamples = resamp_per > 0 and keep_k < N and (count + 1) % resamp_per == 0
    keys = ("Q", "m", "v", "S", "Q_out", "plan")
    fresh = ref["fresh"]
    redraw = float(np.abs(got["Q"][:, fresh] - ref["Q"][:, fresh]).max()) if fresh.any() else 0.0
    report(capsys, f"fused vs composed {model} {cost} {math_mode} N {N} H {H} E {E} it {iterations} shift {shift} keep {keep_k} "
                   f"per {resamp_per} count {count} {distribution} h0 {memory}: "
                   + ", ".join(f"{k} {int((bits(got[k]) != bits(ref[k])).sum())}" for k in keys) + " words differ; order "
                   + f"{int((got['order'] != ref['order']).sum())}; redrawn rows {int(fresh.sum())}, worst redraw deviation {redraw:.3e}")
    # conditions on the reference alone
    assert np.isfinite(ref["S"]).all() and np.isfinite(ref["grad0"]).all()
    assert (Q0 < f32(LOW)).any() and (Q0 > f32(HIGH)).any()
    assert np.array_equal(np.sort(ref["order"], axis=1), np.tile(np.arange(N), (E, 1)))
    assert fresh.any() == resamples
    if H > 1:
        assert np.abs(ref["grad0"]).max() > 1e-4
    # the step
    for k in ("m", "v", "S", "Q_out", "plan"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(got["order"], ref["order"])
    assert np.array_equal(bits(got["Q"][:, ~fresh]), bits(ref["Q"][:, ~fresh]))
    if distribution == "uniform":
        assert redraw <= REDRAW_UNIFORM_TOL, f"redrawn rows: {redraw:.3e} > {REDRAW_UNIFORM_TOL:.3e}"
    else:
        assert np.array_equal(bits(got["Q"][:, fresh]), bits(ref["Q"][:, fresh]))
    if resamples:
        assert np.ptp(ref["Q"][:, fresh]) > 0.2 and not ref["m"][:, fresh].any()
    assert not np.array_equal(ref["Q"], shifted(Q0, shift, True))                       # the plans moved


# ---- 2. the memory --------------------------------------------------------------------------------------------------------------
def test_the_memory_is_read_and_not_written():
    E, N, H = 3, 33, 7
    eng = make(E, N, H)
    s0, tp, te, h0, Q0 = problem(E, N, H, 77)
    h = eng.tensor(h0.copy())
    with_h = fused(eng, s0, Q0, tp, te, h, 2, 1)
    assert np.array_equal(bits(h.cpu().numpy()), bits(h0))
    without = fused(eng, s0, Q0, tp, te, None, 2, 1)
    zeros = fused(eng, s0, Q0, tp, te, np.zeros_like(h0), 2, 1)
    eng.close()
    assert not np.array_equal(with_h["S"], without["S"])
    for k in ("S", "Q", "m", "v", "Q_out"):
        assert np.array_equal(bits(without[k]), bits(zeros[k])), k


# ---- 3. the device step counter -------------------------------------------------------------------------------------------------
def test_device_counter_equals_the_host_counters():
    """12 steps with the step counter on the device and resamp_per = 5 against the same steps told by the host: Q, m, v and the
    controls bitwise after every step; the counter ends at 12."""
    E, N, H, rp, iters, keep_k = 3, 16, 7, 5, 3, 12
    eng = make(E, N, H)
    s0, tp, te, h0, Q0 = problem(E, N, H, 51)
    kw = dict(iterations=iters, keep_k=keep_k, resamp_per=rp, shift=1, seed=13, sample_mean=0.05, **HP)
    bufs = [[eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E), eng.tensor(h0.copy())] for _ in range(2)]
    counter = torch.zeros(1, dtype=torch.int64, device=bufs[0][0].device)
    s = eng.tensor(s0)
    for c in range(12):
        Qh, mh, vh, uh, hh = bufs[0]
        eng.rpgd_step_gru(s, Qh, mh, vh, tp, te, hh, count=c, adam_iteration=c * iters, draw_offset=4 + c // rp, Q_out=uh, **kw)
        eng.gru_advance(s, uh, hh)
        Qd, md, vd, ud, hd = bufs[1]
        eng.rpgd_step_gru(s, Qd, md, vd, tp, te, hd, count_dev=counter, draw_offset=4, Q_out=ud, **kw)
        eng.gru_advance(s, ud, hd)
        for a, b in zip(bufs[0], bufs[1]):
            assert torch.equal(a, b), f"step {c}"
        assert int(counter.item()) == c + 1
        eng.plant_advance(s, uh, n_substeps=10)                              # the next step sees another state
    assert int(counter.item()) == 12
    assert bufs[0][0][:, keep_k:].abs().max() > 0 and bufs[0][4].abs().max() > 1e-3
    eng.close()


# ---- 4. the optimizers and the closed loop --------------------------------------------------------------------------------------
def _states(E):
    return np.stack([O.create_cartpole_state(0.3, -0.5, 0.02, 0.1), O.create_cartpole_state(-0.4, 1.0, -0.05, -0.1),
                     O.create_cartpole_state(0.1, 0.3, 0.08, 0.15)])[:E]


OPTS = {"rpgd": dict(num_rollouts=16, mpc_horizon=7, outer_its=3, resamp_per=3, sample_mean=0.05, seed=9),
        "gradient": dict(num_rollouts=16, mpc_horizon=7, gradient_steps=3, seed=9)}


def _optimizer(name, E, **kw):
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    cls = optimizer_rpgd if name == "rpgd" else optimizer_gradient
    return cls(control_limits=(np.array([-1.0]), np.array([1.0])), num_envs=E, gru_model=model_of("golden"), **OPTS[name], **kw)


@pytest.mark.parametrize("name", ["rpgd", "gradient"])
def test_fused_optimizer_equals_the_staged_one(name):
    """optimizer_rpgd / optimizer_gradient(gru_model, gru_fused=True) against (gru_model, gru_adjoint=True) staged over 4 control
    steps at E = 3, N = 16, H = 7 (rpgd: one resampling among them): controls, Q, m, v and the memory h bitwise after every step -
    and the same through controller_mpc(config=dict(gru_model=..., gru_fused=True))."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    from cartpolesimulation_amd.harness import FusedOptimizer, HostPacedOptimizer, optimizer_controller
    E = 3
    target = np.array([-0.05, 0.0, 0.04], f32)

    def make_opt(**kw):
        vp = SimpleNamespace(target_position=target.copy(), target_equilibrium=np.ones(E, f32))
        opt = _optimizer(name, E, variable_parameters=vp, optimizer_logging=True, **kw)
        opt.configure()
        return opt

    staged, fused_opt = make_opt(gru_adjoint=True), make_opt(gru_fused=True)
    ctrl = controller_mpc("CartPole", {"target_position": target.copy(), "target_equilibrium": np.ones(E, f32)},
                          (np.array([-1.0]), np.array([1.0])), num_envs=E,
                          config=dict(gru_model=model_of("golden"), gru_fused=True, **OPTS[name]))
    ctrl.configure(name)
    seam = ctrl.optimizer
    assert fused_opt.fused and fused_opt.gru_fused and seam.fused and seam.gru_fused and not staged.fused
    assert optimizer_controller(fused_opt) is FusedOptimizer and optimizer_controller(staged) is HostPacedOptimizer
    s = _states(E)
    for step in range(4):
        u_s, u_f, u_c = staged.step(s), fused_opt.step(s), ctrl.step(s, time=0.02 * step)
        for who, other, u_o in (("optimizer", fused_opt, u_f), ("controller_mpc", seam, u_c)):
            assert u_o.shape == (E, 1) and np.array_equal(bits(u_o), bits(u_s)), f"step {step} {who}: controls"
            for attr in ("Q", "m", "v", "h"):
                assert np.array_equal(bits(getattr(other, attr).cpu().numpy()), bits(getattr(staged, attr).cpu().numpy())), \
                    f"step {step} {who}: {attr}"
            assert (other.count, other.adam_it, other.draws) == (staged.count, staged.adam_it, staged.draws)
        assert np.array_equal(bits(fused_opt.logging_values["J_logged"]), bits(staged.logging_values["J_logged"]))
        s = np.stack([O.ode_v0_step(s[e][None], u_s[e].astype(f32))[0] for e in range(E)])
    assert np.abs(staged.h.cpu().numpy()).max() > 1e-3 and np.abs(u_s).max() > 1e-3
    assert staged.draws == (2 if name == "rpgd" else 1)                      # rpgd: the start draw and one resampling
    fused_opt.optimizer_reset()
    assert float(fused_opt.h.abs().max()) == 0.0 and fused_opt.count == 0
    for opt in (staged, fused_opt, seam):
        opt.engine.close()


def _schedule_batch(E):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=31, length_of_experiment=0.2, keep_target_equilibrium_x_seconds_up=0.1, turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    return SC.RandomExperimentSetter(cfg).draw(E, 83)


def _run(E, graph, **kw):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    b = _schedule_batch(E)
    opt = _optimizer("rpgd", E, **kw)
    opt.configure()
    res = BatchedCartPoleExperiment(opt.engine, b.dt_simulation, b.dt_control, seed=0).run_schedule(b, graph=graph, steps_per_graph=5, optimizer=opt)
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state")}
    out["memory"] = opt.h.cpu().numpy()
    opt.engine.close()
    return b, out


def test_captured_loop_equals_the_launched_loop_and_the_staged_optimizer():
    """run_schedule with the fused GRU rpgd optimizer, three experiments of 0.2 s at 16 x 7 with resamp_per = 3: captured
    (graph=True) equals launched - states, controls, recording rows and the final memory, bitwise -, and launched equals the same
    batch under the staged optimizer object (HostPacedOptimizer)."""
    E = 3
    b, launched = _run(E, False, gru_fused=True)
    _, captured = _run(E, True, gru_fused=True)
    _, staged = _run(E, False, gru_adjoint=True)
    assert b.n_periods == 10 and launched["Q"].shape == (11, E) and np.abs(launched["Q"]).max() > 0.02
    assert np.isfinite(launched["states"]).all() and np.abs(launched["memory"]).max() > 1e-3
    for k in launched:
        assert np.array_equal(bits(launched[k]), bits(captured[k])), ("captured", k)
        assert np.array_equal(bits(launched[k]), bits(staged[k])), ("staged", k)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
R_E, R_N, R_H = 2, 16, 7
R_OK = dict(iterations=2, keep_k=12, resamp_per=2, shift=1, seed=3, **HP)


class _Buffers:
    def __init__(self, eng, Q0):
        E, N, H = Q0.shape
        self.Q0 = Q0
        self.Q, self.m, self.v = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
        self.out = dict(Q_out=eng.zeros(E), S_out=eng.zeros(E, N), plan_out=eng.zeros(E, H))

    def untouched(self):
        torch.cuda.synchronize()
        return np.array_equal(self.Q.cpu().numpy(), self.Q0) and not self.m.any() and not self.v.any() and \
            not any(t.any() for t in self.out.values())


def _good_call(eng):
    s0, tp, te, h0, Q0 = problem(R_E, R_N, R_H, 10)
    got = fused(eng, s0, Q0, tp, te, h0, 2, 1)
    assert np.isfinite(got["S"]).all() and not np.array_equal(got["Q"], shifted(Q0, 1, True))


@pytest.mark.parametrize("case", ["no model", "tuning rows", "another cost", "N beyond one workgroup"])
def test_refusals_about_the_handle(case):
    from cartpolesimulation_amd._lib import CpmppiError
    from cartpolesimulation_amd.configs import MPPIConfig, tuning_rows
    from cartpolesimulation_amd.engine import MPPIEngine
    N = 129 if case == "N beyond one workgroup" else R_N
    cfg = dict(num_rollouts=N, mpc_horizon=R_H, shift_mode="none", control_mode="clip", period_interpolation_inducing_points=PERIOD)
    if case == "another cost":
        cfg.update(cost_function_specification="quadratic_boundary_grad")
    eng = MPPIEngine(R_E, MPPIConfig(**cfg))
    if case != "no model":
        eng.set_gru(model_of("golden"))
    if case == "tuning rows":
        eng.set_tuning_rows(tuning_rows(eng.mppi, R_E))
    s0, tp, te, h0, Q0 = problem(R_E, N, R_H, 10)
    bufs = _Buffers(eng, Q0)
    text = {"no model": "cpmppi_rpgd_step_gru: no model set", "tuning rows": "cpmppi_rpgd_step_gru: per-env tuning rows are registered",
            "another cost": "cpmppi_rpgd_step_gru: the GRU predictor supports quadratic_boundary_grad_minimal and default",
            "N beyond one workgroup": r"cpmppi_rpgd_step_gru: one workgroup per env holds at most 128 plans \(N = 129\)"}[case]
    with pytest.raises(CpmppiError, match=text) as ei:
        eng.rpgd_step_gru(s0, bufs.Q, bufs.m, bufs.v, tp, te, h0, **dict(R_OK, keep_k=min(12, N)), **bufs.out)
    assert ei.value.code == -1 and bufs.untouched()
    if case in ("no model", "another cost", "N beyond one workgroup"):       # the reserve says the same under its own name
        with pytest.raises(CpmppiError, match=text.replace("cpmppi_rpgd_step_gru", "cpmppi_rpgd_gru_reserve")):
            eng.rpgd_gru_reserve()
    if case == "tuning rows":
        eng.set_tuning_rows(None)
        _good_call(eng)
    elif case == "no model":
        eng.set_gru(model_of("golden"))
        _good_call(eng)
    eng.close()


def test_refusals_about_the_arguments_leave_the_handle_usable():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = make(R_E, R_N, R_H)
    s0, tp, te, h0, Q0 = problem(R_E, R_N, R_H, 10)
    bufs = _Buffers(eng, Q0)

    def call(**over):
        return eng.rpgd_step_gru(s0, bufs.Q, bufs.m, bufs.v, tp, te, h0, **dict(R_OK, **over), **bufs.out)

    for over, text in ((dict(keep_k=0), "keep_k"), (dict(keep_k=R_N + 1), "keep_k"), (dict(iterations=0), "iterations must be > 0"),
                       (dict(shift=R_H + 1), "shift exceeds the horizon")):
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: .*" + text):
            call(**over)
    assert bufs.untouched()
    prep = eng.prepare_rpgd_step_gru(s0, bufs.Q, bufs.m, bufs.v, tp, te, h0, **R_OK, **bufs.out)
    prep.args.distribution = 2
    with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: unknown distribution"):
        prep.run()
    prep.args.distribution = 0
    for field in ("s0", "target_position", "target_equilibrium", "Q", "m", "v", "Q_out"):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, None)
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: null pointer"):
            prep.run()
        setattr(prep.args, field, keep + 2)
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: misaligned pointer"):
            prep.run()
        setattr(prep.args, field, keep)
    keep = prep.args.h0
    prep.args.h0 = keep + 1
    with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: misaligned pointer"):
        prep.run()
    prep.args.h0 = keep
    counter = torch.zeros(2, dtype=torch.int64, device=bufs.Q.device)
    prep.args.count_dev = counter.data_ptr() + 4
    with pytest.raises(CpmppiError, match=r"cpmppi_rpgd_step_gru: misaligned pointer \(count_dev: 8 bytes\)"):
        prep.run()
    prep.args.count_dev = None
    for bad_E in (0, R_E + 1):
        prep.args.E = bad_E
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: bad argument .0 < E <= config.E."):
            prep.run()
        with pytest.raises(CpmppiError, match="cpmppi_rpgd_gru_reserve: bad argument .0 < E <= config.E."):
            eng.rpgd_gru_reserve(bad_E)
    prep.args.E = R_E
    assert eng.lib.cpmppi_rpgd_step_gru(eng._h, None, eng._stream()) == -1
    assert eng.lib.cpmppi_last_error(eng._h).decode().startswith("cpmppi_rpgd_step_gru: null argument block")
    assert bufs.untouched() and int(counter.sum().item()) == 0
    _good_call(eng)
    eng.close()


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_capture_without_a_reserved_workspace_is_refused_and_the_capture_survives(math_mode):
    """On a capturing stream the step must not allocate: without cpmppi_rpgd_gru_reserve it is refused with a text before any HIP
    call that a capture forbids - the capture goes on, ends and replays; after the reserve the same step + cpmppi_gru_advance are
    captured, and two replays equal two launched periods."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 16, 7
    eng = make(E, N, H, math_mode=math_mode)
    s0, tp, te, h0, Q0 = problem(E, N, H, 12)
    s, tpd, ted = eng.tensor(s0), eng.tensor(tp), eng.tensor(te)
    Q, m, v, u, h = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E), eng.tensor(h0.copy())
    counter = torch.zeros(1, dtype=torch.int64, device=Q.device)
    marker = eng.zeros(4)
    step = dict(iterations=2, keep_k=12, resamp_per=2, shift=1, seed=SEED, draw_offset=3, **HP)
    prep = eng.prepare_rpgd_step_gru(s, Q, m, v, tpd, ted, h, count_dev=counter, Q_out=u, **step)
    side = torch.cuda.Stream(device=Q.device)
    side.wait_stream(torch.cuda.current_stream(Q.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_gru: the stream is being captured .*cpmppi_rpgd_gru_reserve"):
                prep.run()
            marker.add_(1.0)
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.array_equal(Q.cpu().numpy(), Q0) and int(counter.item()) == 0
    eng.rpgd_gru_reserve()
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(Q.device))
    fixed = eng.use_stream(side)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            prep.run()
            eng.gru_advance(s, u, h)
    eng.use_stream(fixed)
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g2.replay()
    g2.replay()
    torch.cuda.synchronize()
    Qr, mr, vr, hr = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.tensor(h0.copy())
    for c in range(2):
        ur = eng.rpgd_step_gru(s, Qr, mr, vr, tpd, ted, hr, count=c, adam_iteration=2 * c, **dict(step, draw_offset=3 + c // 2))[0]
        eng.gru_advance(s, ur, hr)
    torch.cuda.synchronize()
    assert int(counter.item()) == 2 and torch.equal(Q, Qr) and torch.equal(m, mr) and torch.equal(v, vr) and torch.equal(u, ur)
    assert torch.equal(h, hr)
    eng.close()
