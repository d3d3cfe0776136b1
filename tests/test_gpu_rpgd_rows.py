"""GPU: the fused rpgd / gradient step with a row per env (cpmppi_rpgd_step_rows: quadratic_boundary_grad_minimal's seven cost
weights, Adam's learning rate and the gradient clip read per env) - against the plain step cpmppi_rpgd_step bit for bit, row by row
against handles whose scalars are the row, its device counter and capture, the optimizers, the device loop, the sweep and the
refusals.

Shapes: E = 3; (N, H) = (16, 35) a quarter of a wave, (40, 7) a ragged wave, (80, 7) two waves with the ranking across them; both
predictors.  Every comparison is equality: the rows kernel is rpgd_step_kernel compiled a second time with nine values loaded per env
where the plain one reads its argument block, so an env computes what a handle with those scalars computes, instruction for
instruction; no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_rpgd_fused import HP, _schedule_batch, make, problem  # noqa: E402

f32 = np.float32
SHAPES = [(16, 35), (40, 7), (80, 7)]
OUTPUTS = ("Q", "m", "v", "Q_out", "S", "plan", "order")
WEIGHTS = ("dd_quadratic_weight_up", "db_weight_up", "ep_weight_up", "ekp_weight_up", "cc_weight_up", "R", "permissible_track_fraction")
MASSES = np.asarray([0.080, 0.087, 0.095], f32)


def report(capsys, text):
    with capsys.disabled():
        print("\n[rpgd rows] " + text)


def different_rows(eng, E, seed=3):
    """Rows that differ from the engine's configuration and from each other in all nine columns; the clips two decades apart,
    around the gradient norms of problem()'s plans (some tens to a thousand)."""
    from cartpolesimulation_amd.configs import rpgd_rows
    rng = np.random.Generator(np.random.SFC64(seed))
    base = rpgd_rows(eng.mppi, E, HP["learning_rate"], HP["gradmax_clip"])
    rows = base.copy()
    rows[:, :6] *= rng.uniform(0.5, 0.8, (E, 6)).astype(f32) + np.arange(E, dtype=f32)[:, None]
    rows[:, 6] = np.linspace(0.6, 0.8, E)
    rows[:, 7] = np.linspace(0.02, 0.1, E)
    rows[:, 8] = 3.0 * 100.0 ** np.arange(E)
    for col in range(9):
        assert len(set(rows[:, col])) == E and not np.isin(base[0, col], rows[:, col]), col
    return rows


def step(eng, data, rows=None, m0=None, v0=None, **kw):
    """One fused step from the buffers of `data` (problem()) -> the seven outputs as numpy."""
    s0, tp, te, Lv, prev, Q0 = data
    E, N, H = Q0.shape
    Q = eng.tensor(Q0.copy())
    m = torch.zeros_like(Q) if m0 is None else eng.tensor(m0.copy())
    v = torch.zeros_like(Q) if v0 is None else eng.tensor(v0.copy())
    S, plan, order = eng.empty(E, N), eng.empty(E, H), torch.empty(E, N, dtype=torch.int32, device=Q.device)
    kw = dict(dict(HP, iterations=3, shift=1), **kw)
    u = eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev, S_out=S, plan_out=plan, order_out=order, rows=rows, **kw)[0]
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in zip(OUTPUTS, (Q, m, v, u, S, plan, order))}


RESAMPLE = dict(resamp_per=1, seed=21, draw_offset=2, sample_mean=0.05)


@pytest.mark.parametrize("predictor", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_equal_rows_are_the_plain_step(N, H, predictor):
    """Every row = the handle's weights and the argument block's learning rate and clip: all seven outputs are cpmppi_rpgd_step's bit
    for bit (N = 16: a resampling step with a shift).  Rewriting the array where it lies changes every env's result."""
    from cartpolesimulation_amd.configs import rpgd_rows
    E = 3
    eng = make(E, N, H, predictor_type=predictor, cost_weights=dict(ep_weight_up=55.0))
    data = problem(E, N, H, 61)
    kw = dict(RESAMPLE, keep_k=(3 * N) // 4) if N == 16 else {}
    plain = step(eng, data, **kw)
    rows = eng.tensor(rpgd_rows(eng.mppi, E, HP["learning_rate"], HP["gradmax_clip"]))
    assert rows[0, 2] == 55.0 and rows.data_ptr() % 64 == 0
    # (the argument block's own two are not read: another value there changes nothing)
    got = step(eng, data, rows=rows, **dict(kw, learning_rate=0.5, gradmax_clip=0.01))
    for k in OUTPUTS:
        assert np.array_equal(got[k], plain[k]), k
    assert np.isfinite(plain["S"]).all() and not np.array_equal(plain["Q"], data[5])
    if kw:                                                           # the redraw happened, with the handle's sigma
        assert not plain["m"][:, kw["keep_k"]:].any() and np.ptp(plain["Q"][:, kw["keep_k"]:]) > 0.3
    address = rows.data_ptr()
    rows.copy_(eng.tensor(different_rows(eng, E)))
    assert rows.data_ptr() == address
    other = step(eng, data, rows=rows, **kw)
    for e in range(E):
        assert not np.array_equal(other["Q"][e], plain["Q"][e]) and not np.array_equal(other["S"][e], plain["S"][e]), e
    eng.close()


@pytest.mark.parametrize("predictor", ["ODE_v0", "ODE"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_a_row_is_a_handle_with_those_scalars(N, H, predictor, capsys):
    """Rows that differ in all nine columns; env e of the rows launch against env e of a second engine whose cost weights are row e,
    with row e's learning rate and clip in the argument block: equal bit for bit in all seven outputs, and env e + 1 is not.
    predictor ODE: with pole-mass rows registered.  The previous input is non-zero throughout.  The clip bites in some envs and
    not in others (the first iteration's gradient norms, from rollout_cost_grad on the scalar engines)."""
    E = 3
    cfg = dict(predictor_type=predictor)
    eng = make(E, N, H, **cfg)
    data = problem(E, N, H, 67)
    s0, tp, te, Lv, prev, Q0 = data
    assert np.abs(prev).min() > 0
    if predictor == "ODE":
        eng.set_pole_mass_rows(MASSES)
    rows = different_rows(eng, E)
    kw = dict(RESAMPLE, keep_k=(3 * N) // 4) if N == 16 else {}
    got = step(eng, data, rows=eng.tensor(rows), **kw)
    eng.close()
    above = below = 0
    for e in range(E):
        scalar = make(E, N, H, cost_weights={k: float(x) for k, x in zip(WEIGHTS, rows[e, :7])}, **cfg)
        if predictor == "ODE":
            scalar.set_pole_mass_rows(MASSES)
        ref = step(scalar, data, learning_rate=float(rows[e, 7]), gradmax_clip=float(rows[e, 8]), **kw)
        for k in OUTPUTS:
            assert np.array_equal(got[k][e], ref[k][e]), (e, k)
        assert not np.array_equal(got["Q"][(e + 1) % E], ref["Q"][(e + 1) % E]) and not np.array_equal(got["S"][(e + 1) % E], ref["S"][(e + 1) % E])
        G = scalar.rollout_cost_grad(s0, Q0, tp, te, L=Lv, previous_input=prev)[1][e]
        norms = G.double().pow(2).sum(dim=1).sqrt().cpu().numpy()
        above += int((norms > rows[e, 8]).sum())
        below += int((norms < rows[e, 8]).sum())
        report(capsys, f"{predictor} N {N} H {H} env {e}: clip {rows[e, 8]:g}, gradient norms {norms.min():.3g} .. {norms.max():.3g}")
        scalar.close()
    assert above > 0 and below > 0, (above, below)


def test_device_counter_and_capture():
    """Three steps with the counter on the device = three host-counted steps; a captured rows step replayed three times = three
    launched steps, bit for bit, with the rows' contents rewritten before the second step in both (the replay reads the values when
    it runs) - and that rewrite shows in the result."""
    E, N, H, iters, keep_k, rp = 3, 16, 35, 2, 12, 2
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 71)
    first, second = eng.tensor(different_rows(eng, E, 5)), eng.tensor(different_rows(eng, E, 6))
    kw = dict(iterations=iters, keep_k=keep_k, resamp_per=rp, shift=1, seed=13, sample_mean=0.05, draw_offset=4, **HP)
    s, tpd, ted, Ld = eng.tensor(s0), eng.tensor(tp), eng.tensor(te), eng.tensor(Lv)
    eng.rpgd_reserve()

    def run(mode, rewrite=True):
        rows = first.clone()
        Q, m, v, u = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E)
        counter = torch.zeros(1, dtype=torch.int64, device=Q.device)
        prep = eng.prepare_rpgd_step(s, Q, m, v, tpd, ted, L=Ld, previous_input=u, Q_out=u, rows=rows,
                                     count_dev=None if mode == "host" else counter, **kw)
        if mode == "captured":
            side = torch.cuda.Stream(device=Q.device)
            side.wait_stream(torch.cuda.current_stream(Q.device))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    prep.run()
            torch.cuda.current_stream(Q.device).wait_stream(side)
        controls = []
        for c in range(3):
            if c == 1 and rewrite:
                rows.copy_(second)
            if mode == "host":
                prep.run(count=c, adam_iteration=c * iters, draw_offset=4 + c // rp)
            elif mode == "device":
                prep.run()
            else:
                g.replay()
            controls.append(u.clone())
        torch.cuda.synchronize()
        assert mode == "host" or int(counter.item()) == 3
        return [x.cpu().numpy() for x in (Q, m, v, torch.stack(controls))]

    host, device, captured = run("host"), run("device"), run("captured")
    for h, d, c in zip(host, device, captured):
        assert np.array_equal(h, d) and np.array_equal(h, c)
    unchanged = run("device", rewrite=False)
    assert np.array_equal(unchanged[3][0], host[3][0]) and not np.array_equal(unchanged[0], host[0])
    assert np.abs(host[0][:, keep_k:]).max() > 0                    # (the second step redrew)
    eng.close()


def _states(E, steps, seed):
    from oracle import oracle_np as O
    rng = np.random.Generator(np.random.SFC64(seed))
    return [np.stack([O.create_cartpole_state(rng.uniform(-0.4, 0.4), rng.uniform(-1.0, 1.0), rng.uniform(-0.05, 0.05),
                                              rng.uniform(-0.1, 0.1)) for _ in range(E)]).astype(f32) for _ in range(steps)]


@pytest.mark.parametrize("name", ["rpgd", "gradient"])
def test_optimizers_with_rows_equal_the_scalar_optimizers(name):
    """optimizer_rpgd / optimizer_gradient(fused=True, rows=...) on 4 envs over 4 control steps (rpgd: resamp_per = 2, so a redraw
    happens): env e's controls, plans and moments are those of env e of a 4-env scalar fused optimizer built with row e's cost
    weights, learning rate and clip and the same seed, bit for bit."""
    from cartpolesimulation_amd import optimizer_gradient as OG
    from cartpolesimulation_amd.configs import MPPIConfig, rpgd_rows
    E = 4
    if name == "rpgd":
        cls, kw = OG.optimizer_rpgd, dict(num_rollouts=16, mpc_horizon=10, outer_its=3, resamp_per=2, opt_keep_k_ratio=0.5)
    else:
        cls, kw = OG.optimizer_gradient, dict(num_rollouts=24, mpc_horizon=7, gradient_steps=3)
    kw.update(seed=17, num_envs=E, fused=True)
    rows = rpgd_rows(MPPIConfig(), E, [0.02, 0.05, 0.08, 0.11], [0.5, 2.0, 5.0, 0.0], ep_weight_up=[20.0, 40.0, 60.0, 80.0],
                     dd_quadratic_weight_up=[5.0, 10.0, 15.0, 20.0], R=[0.5, 1.0, 1.5, 2.0])
    states = _states(E, 4, 19)

    def run(**more):
        opt = cls(**dict(kw, **more))
        opt.configure(predictor_specification="ODE")
        controls = [opt.step(s, as_tensor=True).clone() for s in states]
        torch.cuda.synchronize()
        out = [x.cpu().numpy() for x in (torch.stack(controls), opt.Q, opt.m, opt.v)]
        assert opt.count == 4
        opt.engine.close()
        return out

    # (the constructor's own learning rate and clip are unused with rows)
    got = run(rows=rows, learning_rate=0.9, gradmax_clip=0.001)
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0.01
    for e in range(E):
        ref = run(cost_weights={k: float(x) for k, x in zip(WEIGHTS, rows[e, :7])}, learning_rate=float(rows[e, 7]),
                  gradmax_clip=float(rows[e, 8]))
        assert np.array_equal(got[0][:, e], ref[0][:, e]), e
        for a, b in zip(got[1:], ref[1:]):
            assert np.array_equal(a[e], b[e]), e
        other = (e + 1) % E
        assert not np.array_equal(got[1][other], ref[1][other])


def _rows_rpgd(E, rows=None, **over):
    from cartpolesimulation_amd.optimizer_gradient import optimizer_rpgd
    opt = optimizer_rpgd(seed=9, num_envs=E, fused=True, rows=rows, resamp_per=10, **over)
    opt.configure(predictor_specification="ODE")
    return opt


def test_device_loop_launched_equals_captured():
    """run_schedule(batch, optimizer=<rows optimizer>): 4 envs, 25 control periods at the shipped rpgd sizes, graph=True against
    graph=False - recorded states and controls bitwise equal; the envs' rows show in the controls."""
    from cartpolesimulation_amd.configs import MPPIConfig, rpgd_rows
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    E, outs = 4, []
    rows = rpgd_rows(MPPIConfig(), E, [0.02, 0.05, 0.08, 0.11], 5.0, ep_weight_up=[20.0, 40.0, 60.0, 80.0])
    for graph in (False, True):
        b = _schedule_batch(E)
        opt = _rows_rpgd(E, rows)
        res = BatchedCartPoleExperiment(opt.engine, seed=0).run_schedule(b, graph=graph, steps_per_graph=5, optimizer=opt)
        torch.cuda.synchronize()
        outs.append({k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state")})
        opt.engine.close()
    assert b.n_periods == 25 and outs[0]["Q"].shape == (26, E) and np.abs(outs[0]["Q"]).max() > 0.05 and np.isfinite(outs[0]["states"]).all()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    plain = _rows_rpgd(E)
    res = BatchedCartPoleExperiment(plain.engine, seed=0).run_schedule(_schedule_batch(E), optimizer=plain)
    assert not np.array_equal(res["Q"].cpu().numpy(), outs[0]["Q"])
    plain.engine.close()


GRID = dict(ep_weight_up=[20.0, 80.0], learning_rate=[0.02, 0.1])


def test_sweep_of_rpgd_and_one_setting_against_a_scalar_optimizer():
    """run_sweep(optimizer="rpgd") on a 2 x 2 grid x 2 experiments of 0.5 s: the table's shape and order; setting 2's logged controls,
    states and scores are those of a scalar fused optimizer with that setting on the tiled batch, at the setting's env indices."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd import sweep as SW
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    from cartpolesimulation_amd.optimizer_gradient import optimizer_rpgd
    cfg = MPPIConfig(predictor_type="ODE")
    batch = SC.RandomExperimentSetter(dict(seed=4, length_of_experiment=0.5)).draw(2, 12)
    sw = SW.run_sweep(cfg, GRID, batch, seed=6, optimizer="rpgd")
    assert [(s["ep_weight_up"], s["learning_rate"]) for s in sw["settings"]] == [(20, 0.02), (20, 0.1), (80, 0.02), (80, 0.1)]
    assert sw["scores"].shape == (4, 2, 5) and sw["mean"].shape == sw["worst"].shape == (4, 5) and np.isfinite(sw["scores"]).all()
    assert len({tuple(r) for r in sw["mean"].round(9)}) == 4                              # the settings differ
    k = 2
    s = sw["settings"][k]
    tiled = SW.tile_batch(batch, 4)
    opt = optimizer_rpgd(seed=6, num_envs=8, fused=True, cost_weights=dict(ep_weight_up=s["ep_weight_up"]), learning_rate=s["learning_rate"])
    opt.configure(predictor_specification="ODE")
    eng = opt.engine
    plain = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=6).run_schedule(tiled, optimizer=opt)
    mine = slice(2 * k, 2 * k + 2)
    assert torch.equal(plain["Q"][:, mine], sw["result"]["Q"][:, mine]) and torch.equal(plain["states"][:, mine], sw["result"]["states"][:, mine])
    assert not torch.equal(plain["Q"][:, :2], sw["result"]["Q"][:, :2])
    got = eng.score_runs(plain["states"], plain["Q"], target_position_table=tiled.target_position, save_every=batch.n_save,
                         sched_stride=batch.stride, period_steps=batch.n_ctrl).cpu().numpy()
    assert np.array_equal(got[mine], sw["scores"][k])
    eng.close()
    with pytest.raises(ValueError, match="'LBD'; available: .*learning_rate, gradmax_clip"):
        SW.run_sweep(cfg, dict(LBD=[50.0]), batch, optimizer="rpgd")


def test_command_line_prints_the_table(capsys):
    from cartpolesimulation_amd import sweep as SW
    SW.main(["--grid", "learning_rate=0.02,0.1", "--grid", "ep_weight_up=20,80", "--experiments", "2", "--length", "0.5",
             "--optimizer", "rpgd", "--graph"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0].split()[:3] == ["learning_rate", "ep_weight_up", "mean_abs_distance:mean"] and len(lines) == 5
    assert [tuple(float(x) for x in ln.split()[:2]) for ln in lines[1:]] == [(0.02, 20), (0.02, 80), (0.1, 20), (0.1, 80)]
    assert all(len(ln.split()) == 12 and np.isfinite([float(x) for x in ln.split()]).all() for ln in lines[1:])


# ---------------------------------------------------------------------------------------------------------------------------------
def raw_call(eng, prep, rows_address, n_rows):
    """cpmppi_rpgd_step_rows through ctypes with the block of `prep` -> (return code, the handle's last error)."""
    rc = eng.lib.cpmppi_rpgd_step_rows(eng._h, prep.ref, C.c_void_p(rows_address), n_rows, eng._stream())
    return rc, eng.lib.cpmppi_last_error(eng._h).decode()


def test_refusals_leave_the_outputs_untouched_and_the_call_succeeds_once_the_cause_is_removed():
    from cartpolesimulation_amd._lib import CpmppiError
    from cartpolesimulation_amd.configs import rpgd_rows, tuning_rows
    E, N, H = 3, 16, 7
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 10)
    Q, m, v, u = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E) + 7.0
    rows = eng.tensor(rpgd_rows(eng.mppi, E + 1, 0.05, 5.0))
    prep = eng.prepare_rpgd_step(s0, Q, m, v, tp, te, L=Lv, previous_input=prev, Q_out=u, rows=rows, iterations=2, keep_k=12, resamp_per=2,
                                 shift=1, **HP)
    address = rows.data_ptr()

    def refused(text, rows_address=address, n_rows=E + 1):
        rc, error = raw_call(eng, prep, rows_address, n_rows)
        assert rc == -1 and error.startswith("cpmppi_rpgd_step_rows: ") and text in error, (rc, error)
        torch.cuda.synchronize()
        assert np.array_equal(Q.cpu().numpy(), Q0) and not m.any() and not v.any() and (u == 7.0).all()

    # what is new about the rows
    refused("null pointer (rows)", rows_address=0)
    for off in (4, 32):
        refused("misaligned pointer (rows are 64 bytes", rows_address=address + off)
    refused("3 envs, but rows holds 2 rows", n_rows=2)
    refused("3 envs, but rows holds 0 rows", n_rows=0)
    eng.set_cost("default")
    refused("quadratic_boundary_grad_minimal: the handle has another cost plugin")
    eng.set_cost("quadratic_boundary_grad_minimal", eng.mppi.cost_weights)
    registered = eng.set_tuning_rows(tuning_rows(eng.mppi, E))
    refused("per-env tuning rows are registered (cpmppi_set_tuning_rows)")
    with pytest.raises(CpmppiError, match="cpmppi_rpgd_step: per-env tuning rows are registered"):      # (the plain step, as before)
        eng.rpgd_step(s0, Q, m, v, tp, te, L=Lv, iterations=2, **HP)
    eng.set_tuning_rows(None)
    del registered
    # everything cpmppi_rpgd_step refuses, under this caller's name
    for field, bad, text in (("keep_k", 0, "keep_k"), ("keep_k", N + 1, "keep_k"), ("iterations", 0, "iterations must be > 0"),
                             ("shift", H + 1, "shift exceeds the horizon"), ("distribution", 2, "unknown distribution"),
                             ("E", 0, "0 < E <= config.E"), ("E", E + 1, "0 < E <= config.E")):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, bad)
        refused(text)
        setattr(prep.args, field, keep)
    for field in ("s0", "target_position", "target_equilibrium", "Q", "m", "v", "Q_out"):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, None)
        refused("null pointer (s0, target_position")
        setattr(prep.args, field, keep + 2)
        refused("misaligned pointer")
        setattr(prep.args, field, keep)
    counter = torch.zeros(2, dtype=torch.int64, device=Q.device)
    prep.args.count_dev = counter.data_ptr() + 4
    refused("misaligned pointer (count_dev: 8 bytes)")
    prep.args.count_dev = None
    eng.set_pole_mass_rows(eng.tensor(np.full(2, 0.09, f32)))
    refused("3 rows, but cpmppi_set_pole_mass_rows registered 2 pole masses")
    eng.set_pole_mass_rows(None)
    # ... and the very call succeeds once nothing is wrong with it
    rc, _ = raw_call(eng, prep, address, E + 1)
    torch.cuda.synchronize()
    assert rc == 0 and not np.array_equal(Q.cpu().numpy(), Q0) and np.isfinite(u.cpu().numpy()).all() and (u != 7.0).all()
    eng.close()


@pytest.mark.parametrize("what,kw", [
    ("legacy cost", dict(cost_function_specification="legacy_mppi_cartpole")),
    ("PRECISE math", dict(math_mode="precise")),
    ("N beyond one workgroup", dict(num_rollouts=320))])
def test_refusals_about_the_handle(what, kw):
    """What the plain step refuses about the handle itself, under this caller's name; nothing is launched."""
    E, H = 2, 5
    N = kw.pop("num_rollouts", 24)
    eng = make(E, N, H, **kw)
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 9)
    Q, m, v = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H)
    rows = eng.zeros(E, 16)
    prep = eng.prepare_rpgd_step(s0, Q, m, v, tp, te, L=Lv, rows=rows, iterations=2, **HP)
    rc, error = raw_call(eng, prep, rows.data_ptr(), E)
    torch.cuda.synchronize()
    assert rc == -1 and error.startswith("cpmppi_rpgd_step_rows: "), (what, error)
    assert np.array_equal(Q.cpu().numpy(), Q0)
    eng.close()


def test_capture_without_a_reserved_workspace_is_refused_and_the_capture_survives():
    """As the plain step: on a capturing stream the rows step does not allocate - refused with a text, the capture goes on, ends and
    replays; after cpmppi_rpgd_reserve the same step is captured and replayed."""
    from cartpolesimulation_amd._lib import CpmppiError
    from cartpolesimulation_amd.configs import rpgd_rows
    E, N, H = 2, 16, 7
    eng = make(E, N, H)
    s0, tp, te, Lv, prev, Q0 = problem(E, N, H, 12)
    s, tpd, ted, Ld = eng.tensor(s0), eng.tensor(tp), eng.tensor(te), eng.tensor(Lv)
    Q, m, v, u = eng.tensor(Q0.copy()), eng.zeros(E, N, H), eng.zeros(E, N, H), eng.zeros(E)
    rows = eng.tensor(different_rows(eng, E))
    counter = torch.zeros(1, dtype=torch.int64, device=Q.device)
    marker = eng.zeros(4)
    prep = eng.prepare_rpgd_step(s, Q, m, v, tpd, ted, L=Ld, iterations=2, count_dev=counter, Q_out=u, rows=rows, **HP)
    side = torch.cuda.Stream(device=Q.device)
    side.wait_stream(torch.cuda.current_stream(Q.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_rpgd_step_rows: the stream is being captured .*cpmppi_rpgd_reserve"):
                prep.run()
            marker.add_(1.0)
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.array_equal(Q.cpu().numpy(), Q0) and int(counter.item()) == 0
    eng.rpgd_reserve()
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(Q.device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            prep.run()
    torch.cuda.current_stream(Q.device).wait_stream(side)
    g2.replay()
    torch.cuda.synchronize()
    data = (s0, tp, te, Lv, None, Q0)
    ref = step(eng, data, rows=rows, iterations=2, count=0, adam_iteration=0)
    assert int(counter.item()) == 1 and np.array_equal(Q.cpu().numpy(), ref["Q"]) and np.array_equal(u.cpu().numpy(), ref["Q_out"])
    eng.close()
