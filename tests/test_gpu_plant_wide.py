"""GPU: plant_kernel (cpmppi_plant_step) beyond one wave - 321 envs = a full first workgroup, a full wave of the second and one live
lane in the wave after it - with every table of the schedule, at the bounce and the +-pi wrap, as a slice of wider buffers, at the
end of its tables and under a device counter the recording cannot name.  Inputs, the oracle loop and the flag rule: plant_cases.py
(judged on the host by test_plant_cases_host.py)."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import plant_cases as PC  # noqa: E402
from oracle import schedule_np as S  # noqa: E402

f32 = np.float32
E_ALL = 321
GUARD = 777.0
LATENCY = 0.0085                 # 4.25 simulation steps
HISTORY_LEN = 7                  # more than latency_steps + 2: the ring's modulus is not its minimum


@pytest.fixture(scope="module")
def eng():
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    e = MPPIEngine(E_ALL, MPPIConfig(num_rollouts=64, mpc_horizon=10))
    yield e
    e.close()


@pytest.fixture(scope="module")
def wide():
    """The wide case and its oracle rows: computed once, shared, never modified."""
    case = PC.wide_case()
    return case, PC.oracle_rows(case)


def check_rows(st_h, dd_h, ref, label):
    """Every compared row of every env within the tolerances of test_plant_step_follows_the_oracle_loop_row_by_row; prints the headroom."""
    es, ea, ep = PC.errors(st_h, dd_h, ref)
    mask = PC.compared(ref)
    bounced = (ref["bounce_step"] > 0)[None, :] & (ref["step_of_row"][:, None] >= ref["bounce_step"][None, :])
    for name, err in (("state", es), ("angleDD", ea), ("positionDD", ep)):
        a, b = np.where(mask & bounced, err, 0.0), np.where(mask & ~bounced, err, 0.0)
        print(f"{label} {name}: largest error / tolerance {a.max():.3f} in rows after a bounce, {b.max():.3f} in the rest")
    for name, err in (("state", es), ("angleDD", ea), ("positionDD", ep)):
        bad = np.argwhere(mask & ~(err <= 1.0))
        assert len(bad) == 0, (label, name, [(int(r), int(e), float(err[r, e])) for r, e in bad[:8]])


def test_wide_plant_against_the_oracle(eng, wide):
    """321 envs through eng.plant_step with every table, both logs, the controls' log and the four published vectors: every saved row
    of every unflagged env against the oracle loop; exact for all envs - the controls' log, the applied control, the published rows,
    the rows beyond the logs' end."""
    case, ref = wide
    t0 = time.perf_counter()
    E, T, n_ctrl, n_save = case["E"], case["T"], case["n_ctrl"], case["n_save"]
    n_sim = T * n_ctrl
    R = n_sim // n_save + 1
    s = eng.tensor(case["s0"].copy())
    states, dd, Qlog = eng.zeros(R + 2, E, 6) + GUARD, eng.zeros(R + 2, E, 2) + GUARD, eng.zeros(T + 1, E) + GUARD
    states[0] = s
    cur_tp, cur_te, cur_L, Qa_out = (eng.zeros(E) + GUARD for _ in range(4))
    kw = dict(dt_sim=case["dt"], period_steps=n_ctrl, states_log=states[:R], dd_log=dd[:R], save_every=n_save, Q_log=Qlog,
              target_position_table=eng.tensor(case["tp"]), target_equilibrium_table=eng.tensor(case["te"]),
              L_table=eng.tensor(case["Ltab"]), sched_stride=case["stride"], target_position_out=cur_tp, target_equilibrium_out=cur_te,
              L_out=cur_L, m_pole_table=eng.tensor(case["mtab"]), L_controller_table=eng.tensor(case["Lctab"]),
              Q_disturbance_table=eng.tensor(case["qd"]), Q_bias=float(case["qb"]), Q_applied_out=Qa_out)
    Qa = PC.applied(case)
    for c in range(T):
        eng.plant_step(s, case["Qs"][c], n_ctrl, period=c, **kw)
        g1 = (c + 1) * n_ctrl
        assert np.array_equal(cur_tp.cpu().numpy(), case["tp"][g1]) and np.array_equal(cur_te.cpu().numpy(), case["te"][g1]), c
        assert np.array_equal(cur_L.cpu().numpy(), case["Lctab"][g1]), c
        assert np.array_equal(Qa_out.cpu().numpy(), Qa[c]), c
    eng.plant_step(s, case["Qs"][T], 0, period=T, **kw)                  # the run's last controller call: record only
    assert np.array_equal(Qa_out.cpu().numpy(), Qa[T])
    assert np.array_equal(cur_tp.cpu().numpy(), case["tp"][n_sim])       # (a record-only call publishes nothing)
    st_h, dd_h = states.cpu().numpy(), dd.cpu().numpy()
    assert np.array_equal(Qlog.cpu().numpy(), case["Qs"])
    assert (st_h[R:] == GUARD).all() and (dd_h[R:] == GUARD).all()        # nothing beyond the logs' rows
    assert (st_h[:R] != GUARD).all() and (dd_h[:R] != GUARD).all()        # every row of every env was written
    check_rows(st_h[:R], dd_h[:R], ref, "wide")
    # the branches did happen on the device: the unflagged envs the oracle saw bounce have their velocity reversed in the first
    # row saved after it (the comparison above holds them to 3e-5 there), the wrapped ones their angle's sign
    ok = PC.unflagged(ref)
    assert (ok & (ref["bounce_step"] > 0)).sum() >= 24 and (ok & ref["wrapped"]).sum() >= 24 and ok[320] and ref["bounce_step"][320] > 0
    print(f"wide: wall time {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------------------
# cpmppi_plant_step through ctypes: every buffer of the call, full width or as a slice moved to its first env

# pointer field -> elements per env (the widths cpmppi_groups_run moves each pointer by)
WIDTH = dict(s=6, Q=1, L=1, m_pole=1, states_log=6, dd_log=2, Q_log=1, target_position_table=1, target_equilibrium_table=1, L_table=1,
             m_pole_table=1, L_controller_table=1, target_position_out=1, target_equilibrium_out=1, L_out=1, Q_applied_out=1,
             Q_disturbance_table=1, s_measured=6, state_history=6, measurement_noise_table=4, angle_offset_table=1, informed_table=1)
OUTPUTS = ("s", "states_log", "dd_log", "Q_log", "target_position_out", "target_equilibrium_out", "L_out", "Q_applied_out", "s_measured",
           "state_history")


def inputs_of(eng, case, ctrl_rows=None):
    """The read-only device buffers of a call on `case`, full width."""
    dev = eng.device
    rows = slice(0, ctrl_rows)
    rng = np.random.default_rng(3)                                        # (the two vectors are read only where their tables are left out)
    return dict(Qs=eng.tensor(case["Qs"]), L=eng.tensor(rng.uniform(0.2, 0.5, case["E"]).astype(f32)),
                m_pole=eng.tensor(rng.uniform(0.03, 0.15, case["E"]).astype(f32)),
                target_position_table=eng.tensor(case["tp"]), target_equilibrium_table=eng.tensor(case["te"]), L_table=eng.tensor(case["Ltab"]),
                m_pole_table=eng.tensor(case["mtab"]), L_controller_table=eng.tensor(case["Lctab"]),
                Q_disturbance_table=eng.tensor(case["qd"][rows]), measurement_noise_table=eng.tensor(case["nz"][rows]),
                angle_offset_table=torch.as_tensor(case["off"], device=dev), informed_table=torch.as_tensor(case["told"], device=dev))


def outputs_of(eng, case, ctrl_rows=None, live=None):
    """The buffers a call writes, filled with GUARD; in the columns `live` (a slice of envs; None: none) the state is the case's initial
    one and the ring holds what the caller is to put there before a run (zeros, cos = 1)."""
    E, T = case["E"], case["T"]
    R = T * case["n_ctrl"] // case["n_save"] + 1
    g = lambda *shape: eng.zeros(*shape) + GUARD                         # noqa: E731
    out = dict(s=g(E, 6), states_log=g(R + 2, E, 6), dd_log=g(R + 2, E, 2), Q_log=g(ctrl_rows or T + 1, E), target_position_out=g(E),
               target_equilibrium_out=g(E), L_out=g(E), Q_applied_out=g(E), s_measured=g(E, 6), state_history=g(HISTORY_LEN, E, 6))
    if live is not None:
        out["s"][live] = eng.tensor(case["s0"])[live]
        out["state_history"][:, live] = 0.0
        out["state_history"][:, live, 2] = 1.0
    return out


def launch(eng, case, inp, out, period, n_sub=None, E=None, e0=0, row_envs=0, period_dev=None, Q_row=None, drop=(), sched_rows=None,
           ctrl_rows=None):
    """One cpmppi_plant_step on the buffers `inp` + `out`, every pointer moved to env e0 by its own element width; `drop`: fields
    left NULL."""
    from cartpolesimulation_amd import _lib as L
    a = L.cpmppi_plant_args()
    bufs = dict(inp, **out)
    bufs["Q"] = bufs.pop("Qs")[period if Q_row is None else Q_row]
    for name, width in WIDTH.items():
        t = bufs.get(name)
        if t is not None and name not in drop:
            assert t.is_contiguous()
            setattr(a, name, t.data_ptr() + e0 * width * t.element_size())
    R = case["T"] * case["n_ctrl"] // case["n_save"] + 1
    a.E, a.row_envs = case["E"] if E is None else E, row_envs
    a.n_substeps, a.period_steps, a.dt_sim = case["n_ctrl"] if n_sub is None else n_sub, case["n_ctrl"], case["dt"]
    a.period, a.save_rows, a.save_every = period, R, case["n_save"]
    a.ctrl_rows = ctrl_rows if ctrl_rows is not None else case["T"] + 1
    a.sched_rows = sched_rows if sched_rows is not None else inp["L_table"].shape[0]
    a.sched_stride, a.Q_bias = case["stride"], float(case["qb"])
    steps = LATENCY / case["dt"]
    a.history_len, a.latency_steps, a.latency_frac = HISTORY_LEN, int(steps), steps - int(steps)
    if period_dev is not None:
        a.period_dev = period_dev.data_ptr()
    rc = eng.lib.cpmppi_plant_step(eng._h, C.byref(a), eng._stream())
    assert rc == 0, eng.lib.cpmppi_last_error(eng._h).decode()


def test_a_slice_of_wider_buffers_in_place(eng, wide):
    """E = 130 envs of 321-wide buffers, every pointer moved to env 67 (an odd start; the slice begins and ends inside a wave) with
    the element width cpmppi_groups_run uses for it - floats x 6 / 2 / 4 / 1, a double, a byte: its columns equal a full-width launch's
    bit for bit, and every other column of every buffer written still holds its guard value."""
    case, _ = wide
    t0 = time.perf_counter()
    e0, n = 67, 130
    live = slice(e0, e0 + n)
    inp = inputs_of(eng, case)
    full, part = outputs_of(eng, case, live=slice(0, E_ALL)), outputs_of(eng, case, live=live)
    for c in range(case["T"]):
        launch(eng, case, inp, full, c)
        launch(eng, case, inp, part, c, E=n, e0=e0, row_envs=E_ALL)
    torch.cuda.synchronize()
    steps = LATENCY / case["dt"]
    assert int(steps) == 4 and abs(steps - 4.25) < 1e-9 and HISTORY_LEN > int(steps) + 2
    for name in OUTPUTS:
        f, p = full[name].cpu().numpy(), part[name].cpu().numpy()
        env_axis = 0 if f.shape[0] == E_ALL else 1
        f, p = np.moveaxis(f, env_axis, 0), np.moveaxis(p, env_axis, 0)
        assert np.array_equal(p[live], f[live]), name
        assert (p[:e0] == GUARD).all() and (p[e0 + n:] == GUARD).all(), name
        written = f[live] != GUARD                                        # the comparison is of values the kernel wrote
        if name in ("states_log", "dd_log"):                              # (row 0 of the states is the caller's)
            R, first = case["T"] * case["n_ctrl"] // case["n_save"] + 1, 1 if name == "states_log" else 0
            assert written[:, first:R].all() and not written[:, R:].any() and not written[:, :first].any(), name
        elif name == "Q_log":
            assert written[:, :case["T"]].all() and not written[:, case["T"]:].any()
        else:
            assert written.all(), name
    # the slice's chain read ITS columns of the noise, offset and informer tables: what it was handed differs from the true state
    assert np.abs(part["s_measured"][live].cpu().numpy() - part["s"][live].cpu().numpy()).max() > 0.01
    # the per-env vectors L and m_pole are read only without their tables: one period more without them, on fresh buffers
    no_tables = ("L_table", "m_pole_table", "L_controller_table")
    full2, part2 = outputs_of(eng, case, live=slice(0, E_ALL)), outputs_of(eng, case, live=live)
    launch(eng, case, inp, full2, 0, drop=no_tables)
    launch(eng, case, inp, part2, 0, E=n, e0=e0, row_envs=E_ALL, drop=no_tables)
    torch.cuda.synchronize()
    f, p = full2["s"].cpu().numpy(), part2["s"].cpu().numpy()
    assert np.array_equal(p[live], f[live]) and (p[:e0] == GUARD).all() and (p[e0 + n:] == GUARD).all()
    assert not np.array_equal(f[live], full["s"].cpu().numpy()[live]) and (part2["L_out"] == GUARD).all()     # (no L_table: L_out is left alone)
    # ... and the vectors matter: the plant of env e0 with env 0's pole length and mass ends elsewhere
    swapped = dict(inp, L=inp["L"].roll(e0), m_pole=inp["m_pole"].roll(e0))
    part3 = outputs_of(eng, case, live=live)
    launch(eng, case, swapped, part3, 0, E=n, e0=e0, row_envs=E_ALL, drop=no_tables)
    torch.cuda.synchronize()
    assert not np.array_equal(part3["s"].cpu().numpy()[live], f[live])
    print(f"slice: wall time {time.perf_counter() - t0:.2f} s")


def test_the_table_s_end(eng):
    """Tables of 17 rows for a run of 30 steps: from step 17 on the plant, the published values and the measured state use row 16 -
    against the oracle on the tables continued with their last row, and bit for bit against those continued tables on the device.
    The 17 rows lie in buffers whose following rows hold OTHER values, so a row read past the end is seen, not a fault."""
    t0 = time.perf_counter()
    E, rows_short = 70, 17
    case = dict(E=E, T=3, n_ctrl=10, n_save=4, dt=0.002, stride=1)
    rng = np.random.Generator(np.random.SFC64(17))
    case["s0"] = PC.draw_states(rng, E)
    PC.draw_tables(rng, case)
    T, n_ctrl = case["T"], case["n_ctrl"]
    n_sim = T * n_ctrl
    names = ("tp", "te", "Ltab", "mtab", "Lctab", "off", "told")
    assert all((case[k][rows_short:] != case[k][rows_short - 1]).any() for k in names)       # what follows the 17 rows is different
    short = dict(case, **{k: case[k][:rows_short] for k in names})
    padded = PC.pad_tables(short, n_sim + 1)
    ref = PC.oracle_rows(padded)
    R = n_sim // case["n_save"] + 1
    dev = eng.device

    def run(tables, rows):
        t = {k: (eng.tensor(tables[k]) if tables[k].dtype == f32 else torch.as_tensor(tables[k], device=dev))[:rows] for k in names}
        assert all(x.is_contiguous() and x.shape[0] == rows for x in t.values())
        s = eng.tensor(case["s0"].copy())
        states, dd, Qlog = eng.zeros(R, E, 6), eng.zeros(R, E, 2), eng.zeros(T + 1, E)
        states[0] = s
        cur_tp, cur_te, cur_L, s_meas = eng.zeros(E), eng.zeros(E), eng.zeros(E), eng.zeros(E, 6)
        kw = dict(dt_sim=case["dt"], period_steps=n_ctrl, states_log=states, dd_log=dd, save_every=case["n_save"], Q_log=Qlog,
                  target_position_table=t["tp"], target_equilibrium_table=t["te"], L_table=t["Ltab"], sched_stride=1,
                  target_position_out=cur_tp, target_equilibrium_out=cur_te, L_out=cur_L, m_pole_table=t["mtab"],
                  L_controller_table=t["Lctab"], Q_disturbance_table=eng.tensor(case["qd"]), Q_bias=float(case["qb"]),
                  s_measured=s_meas, angle_offset_table=t["off"], informed_table=t["told"])
        seen = []
        for c in range(T):
            eng.plant_step(s, case["Qs"][c], n_ctrl, period=c, **kw)
            seen.append([x.cpu().numpy().copy() for x in (cur_tp, cur_te, cur_L, s_meas, s)])
        eng.plant_step(s, case["Qs"][T], 0, period=T, **kw)
        return states.cpu().numpy(), dd.cpu().numpy(), seen

    st_s, dd_s, seen_s = run(case, rows_short)                           # 17 rows of the 31-row buffers: rows 17.. hold other values
    st_p, dd_p, seen_p = run(padded, n_sim + 1)
    assert np.array_equal(st_s, st_p) and np.array_equal(dd_s, dd_p)
    for c in range(T):
        row = min((c + 1) * n_ctrl, rows_short - 1)
        tp, te, Lc, sm, s_true = seen_s[c]
        assert np.array_equal(tp, case["tp"][row]) and np.array_equal(te, case["te"][row]) and np.array_equal(Lc, case["Lctab"][row]), c
        assert all(np.array_equal(x, y) for x, y in zip(seen_s[c], seen_p[c])), c
        # the measured state (no latency, no noise): the true one with the angle offset of that row, taken out again where informed
        for e in range(E):
            m = s_true[e].astype(np.float64)
            off = float(case["off"][row, e])
            m[0] = S.wrap_angle_rad(m[0] + off)
            if case["told"][row, e]:
                m[0] = S.wrap_angle_rad(m[0] - off)
            m[2], m[3] = np.cos(m[0]), np.sin(m[0])
            assert np.all(np.abs(sm[e] - m) <= 2e-7 + 2e-7 * np.abs(m)), (c, e, sm[e], m)
    assert (case["told"][rows_short - 1] == 0).any() and (case["told"][rows_short - 1] == 1).any()
    check_rows(st_s, dd_s, ref, "table end")
    # teeth: the plant with the tables' true continuation leaves these rows by far more than the tolerance
    es, _, _ = PC.errors(st_s, dd_s, PC.oracle_rows(case))
    assert es[-1].max() > 10.0
    print(f"table end: wall time {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("counter", [0, "T + 1", 2 ** 40])
def test_a_counter_the_recording_cannot_name_with_the_whole_schedule(eng, wide, counter):
    """period_dev = 0, one past the recording's last period, 2^40 - with every buffer of the call given and filled with a guard value:
    exactly what include/cpmppi.h says is written, and the advanced state bit for bit that of the host-named launch the header calls
    equivalent (0: period 0 without the disturbance; past the end: the tables' last row, no disturbance or noise row)."""
    case, _ = wide
    t0 = time.perf_counter()
    T, n_ctrl = case["T"], case["n_ctrl"]
    counter = T + 1 if counter == "T + 1" else counter
    c = max(counter - 1, 0)
    everyone = slice(0, E_ALL)
    inp = inputs_of(eng, case, ctrl_rows=T)                               # the recording holds T periods: counter T + 1 names period T, outside it
    got = outputs_of(eng, case, ctrl_rows=T, live=everyone)
    got["state_history"][:] = GUARD                                       # (a period reads only the ring slots it has written: latency 4.25 < 10 steps)
    cnt = torch.tensor([counter], dtype=torch.int64, device=eng.device)
    launch(eng, case, inp, got, 12345, period_dev=cnt, Q_row=0, ctrl_rows=T)     # (the host's `period` is not read)
    # the host-named launch the header calls equivalent: no logs, no disturbance, no noise; past the end, tables of their last row alone
    want = outputs_of(eng, case, ctrl_rows=T, live=everyone)
    want["state_history"][:] = GUARD
    drop = ("states_log", "dd_log", "Q_log", "Q_disturbance_table", "measurement_noise_table")
    if counter == 0:
        launch(eng, case, inp, want, 0, Q_row=0, drop=drop, ctrl_rows=T)
    else:
        tables = ("target_position_table", "target_equilibrium_table", "L_table", "m_pole_table", "L_controller_table", "angle_offset_table",
                  "informed_table")
        last = dict(inp, **{k: inp[k][-1:].contiguous() for k in tables})
        launch(eng, case, last, want, c, Q_row=0, drop=drop, sched_rows=1, ctrl_rows=T)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in got.items()}
    w = {k: v.cpu().numpy() for k, v in want.items()}
    assert np.array_equal(h["s"], w["s"]) and not np.array_equal(h["s"], case["s0"])          # advanced, as the equivalent launch
    for k in ("states_log", "dd_log", "Q_log"):                           # never recorded
        assert (h[k] == GUARD).all(), k
    assert np.array_equal(h["Q_applied_out"], case["Qs"][0])              # the control the plant was driven by: no disturbance row to add
    published = ("target_position_out", "target_equilibrium_out", "L_out", "s_measured", "state_history")
    if counter == 0:
        for k in published:                                               # a period nobody computed a control for publishes nothing
            assert (h[k] == GUARD).all(), k
        # the disturbance WOULD have moved the plant: the equivalence above is not one of two launches that ignore it
        with_d = outputs_of(eng, case, ctrl_rows=T, live=everyone)
        launch(eng, case, inp, with_d, 0, Q_row=0, ctrl_rows=T)
        assert not np.array_equal(with_d["s"].cpu().numpy(), h["s"])
    else:
        for k in published:
            assert np.array_equal(h[k], w[k]) and (h[k] != GUARD).all(), k
        assert np.array_equal(h["target_position_out"], case["tp"][-1]) and np.array_equal(h["target_equilibrium_out"], case["te"][-1])
        assert np.array_equal(h["L_out"], case["Lctab"][-1])
    print(f"counter {counter}: wall time {time.perf_counter() - t0:.2f} s")


def test_launched_graph_and_three_env_groups_agree_at_321_envs():
    """The schedule of test_everything_on_launched_graph_and_groups_agree - every table at once - at 321 envs: launched, as a replayed
    HIP graph of 6 periods (10 periods: a partial last graph) and as three env groups of 107 envs (no multiple of a wave) enqueued
    from C: the same recording bit for bit."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    from cartpolesimulation_amd.pipeline import EnvGroups, run_schedule_groups
    t0 = time.perf_counter()
    E, N, H = E_ALL, 64, 10
    cfg = dict(seed=41, length_of_experiment=0.2, dt=dict(saving=0.004), keep_target_equilibrium_x_seconds_up=0.1,
               turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 20.0], angleD=40.0, position=0.4, positionD=0.2)))
    upd = lambda init, every, inc, lo, hi, mode="bounce": dict(init_value=init, change_every_x_seconds=every, mode=mode,   # noqa: E731
                                                                range_random=[lo, hi], range_clip=[lo, hi], increment=inc, reset_every_x_seconds="inf")
    prm = dict(L=upd(0.395, 0.014, 0.01, 0.3, 0.45), m_pole=upd(0.087, 0.03, 0.004, 0.05, 0.12, "random walk"),
               inform_controller_about_parameters_change=dict(mode="switching_random", change_to_on_after_x_seconds_off=0.08,
                                                              change_to_off_after_x_seconds_on=0.1),
               controlDisturbance=0.2, controlBias=0.01, seed=13, latency=0.0085,
               noise=dict(noise_mode="ON", sigma_angle=0.002, sigma_position=0.0005, sigma_angleD=0.075, sigma_positionD=0.005),
               vertical_angle_offset=upd(1.5, 0.02, 0.005, -0.03, 0.06))
    b = SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(E, 91, stride=1), prm, seed=92)
    assert all(x is not None for x in (b.L_table, b.m_pole_table, b.informed, b.Q_disturbance, b.measurement_noise, b.angle_offset))
    assert 0 < b.informed.mean() < 1 and b.latency == 0.0085 and b.n_periods == 10
    t_draw = time.perf_counter() - t0
    mppi = MPPIConfig(num_rollouts=N, mpc_horizon=H, cost_function_specification="quadratic_boundary")
    outs = []
    for form in ("launched", "graph", "groups"):
        eng = MPPIEngine(E, mppi)
        if form == "groups":
            eg = EnvGroups(E, mppi, 3)
            assert [hi - lo for lo, hi in eg.slices] == [107, 107, 107]
            res = run_schedule_groups(eg, b, 7)
            torch.cuda.synchronize()
        else:
            res = BatchedCartPoleExperiment(eng, seed=7).run_schedule(b, graph=form == "graph", steps_per_graph=6)
        outs.append({k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state", "u_nom")})
        if form == "groups":
            eg.close()
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), ("graph", k)
        assert np.array_equal(outs[0][k], outs[2][k]), ("groups", k)
    assert outs[0]["states"].shape == (b.n_sim // b.n_save + 1, E, 6) and outs[0]["Q"].shape == (b.n_periods + 1, E)
    assert np.isfinite(outs[0]["states"]).all() and np.abs(outs[0]["Q"]).max() > 0.05
    print(f"three forms: wall time {time.perf_counter() - t0:.2f} s, of which drawing the 321 experiments {t_draw:.2f} s")
