"""Inputs and the oracle loop of the wide plant tests (test_plant_cases_host.py judges them on the host, test_gpu_plant_wide.py runs
them against plant_kernel).  Pure numpy + the oracle: no GPU, and the package is not imported.

`wide_case(seed)`: 321 envs = 256 + 64 + 1 - a full first workgroup, a full wave of the second and one live lane in the wave after
it - through three control periods of ten simulation steps with every table of cpmppi_plant_step; every 8th env is a cart about to
hit an end of the track (the plant's bounce), every 8th + 4 a pole about to cross +-pi (the wrap).
`oracle_rows(case)`: the per-env update_state loop over O.plant_ode / O.plant_substep, with what happened to each env on the way.

The flag rule.  A float32 plant and the oracle may decide `|x| >= TrackHalfLength` differently when the integrated position lies
within the state tolerance of the edge, and the wrap when the angle lies within a rounding of +-pi; either moves the state by far
more than any tolerance, on one side only.  An env is FLAGGED from the first simulation step at which
    | |x1| - THL | < 3e-5 + 3e-5 * THL     (x1: the integrated position the bounce test reads; the bound is the state tolerance there)
 or pi - |angle| < 1e-4                     (angle: the wrapped angle after the step)
and from that step on its states and second derivatives are not compared by tolerance.  What is exact about it still is."""
import dataclasses

import numpy as np
from numpy.random import SFC64, Generator

from oracle import oracle_np as O

f32 = np.float32
THL = O.DEFAULT_PARAMS.TrackHalfLength
EDGE_FLAG = 3e-5 + 3e-5 * float(THL)
SEAM_FLAG = 1e-4
STATE_TOL, ADD_TOL, PDD_TOL = (3e-5, 3e-5), (2e-3, 1e-4), (5e-4, 1e-4)      # (absolute, relative): test_plant_step_follows_the_oracle_loop_row_by_row
BLOCK, WAVE = 256, 64
SEED = 2026                                                                # chosen with test_plant_cases_host.py


def draw_states(rng, E):
    """Initial states as test_plant_step_follows_the_oracle_loop_row_by_row draws them."""
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-3, 3), rng.uniform(-4, 4), rng.uniform(-0.19, 0.19), rng.uniform(-0.6, 0.6))
                   for _ in range(E)])
    s0[:, 2], s0[:, 3] = np.cos(s0[:, 0]), np.sin(s0[:, 0])
    return s0


def draw_tables(rng, case):
    """The schedule of that test for `case` (E, T, n_ctrl set): controls, every table, the disturbance - in its order of draws."""
    E, T, n_sim = case["E"], case["T"], case["T"] * case["n_ctrl"]
    rows = n_sim + 1
    case["Qs"] = rng.uniform(-1, 1, (T + 1, E)).astype(f32)
    case["tp"] = rng.uniform(-0.15, 0.15, (rows, E)).astype(f32)
    case["te"] = rng.choice([-1.0, 1.0], (rows, E)).astype(f32)
    case["Ltab"] = np.repeat(rng.uniform(0.2, 0.5, (n_sim // 7 + 1, E)).astype(f32), 7, axis=0)[:rows]      # changes every 7 steps
    case["mtab"] = np.repeat(rng.uniform(0.03, 0.15, (n_sim // 11 + 1, E)).astype(f32), 11, axis=0)[:rows]  # the pole MASS: every 11
    case["Lctab"] = rng.uniform(0.2, 0.5, (rows, E)).astype(f32)          # what the controller is told instead of the true length
    case["qd"], case["qb"] = rng.normal(0, 0.3, (T + 1, E)).astype(f32), f32(0.05)
    # the measurement chain's tables (drawn last: the draws above are those of the test named)
    case["nz"] = rng.normal(0, 0.05, (T + 1, E, 4)).astype(f32)
    case["off"] = np.cumsum(rng.normal(0, 0.02, (rows, E)), axis=0)       # float64, moves every step
    case["told"] = (rng.uniform(size=(rows, E)) < 0.5).astype(np.uint8)
    return case


def applied(case):
    """What drives the plant: (Q + disturbance) + bias, two float32 additions (add_control_noise)."""
    return ((case["Qs"] + case["qd"]).astype(f32) + case["qb"]).astype(f32)


def wide_case(seed=SEED):
    E, T, n_ctrl = 321, 3, 10
    case = dict(E=E, T=T, n_ctrl=n_ctrl, n_save=4, dt=0.002, stride=1)
    rng = Generator(SFC64(seed))
    s0 = draw_states(rng, E)
    draw_tables(rng, case)
    for e in range(0, E, 8):                                               # a cart 3..13 mm from an end, moving toward it
        sign = 1.0 if (e // 8) % 2 == 0 else -1.0
        s0[e, 4] = sign * (float(THL) - rng.uniform(0.003, 0.013))
        s0[e, 5] = sign * rng.uniform(0.4, 0.8)
    for e in range(4, E, 8):                                               # a pole just inside +-pi, turning outward
        sign = 1.0 if (e // 8) % 2 == 0 else -1.0
        s0[e, 0] = sign * rng.uniform(3.05, 3.13)
        s0[e, 1] = sign * rng.uniform(3.0, 6.0)
        s0[e, 2], s0[e, 3] = np.cos(s0[e, 0]), np.sin(s0[e, 0])
    case["s0"] = s0
    return case


def pad_tables(case, rows):
    """`case` with every schedule table continued to `rows` rows by its last row: what the kernel's clamp of the table row means."""
    out = dict(case)
    for k in ("tp", "te", "Ltab", "mtab", "Lctab", "off", "told"):
        t = case[k]
        out[k] = np.concatenate([t, np.repeat(t[-1:], rows - len(t), axis=0)]) if len(t) < rows else t
    return out


def oracle_rows(case):
    """The update_state loop of test_plant_step_follows_the_oracle_loop_row_by_row for every env: pole length and mass of the step,
    integrate, (controller), derivatives, save.  -> dict of
      states [R,E,6], add [R,E], pdd [R,E]   the saved rows (float32 states, the derivatives as the oracle gives them)
      step_of_row [R]                        the simulation step of each saved row
      bounce_step [E]                        the first step at which the env bounced (0: never), bounces [E] how often
      wrapped [E]                            the angle crossed +-pi
      edge_margin [E], seam_margin [E]       the run's smallest | |x1| - THL | and pi - |angle|
      flag_step [E]                          the first flagged step (n_sim + 1: never)."""
    E, n_ctrl, n_save, dt = case["E"], case["n_ctrl"], case["n_save"], case["dt"]
    n_sim = case["T"] * n_ctrl
    Ltab, mtab, Qa = case["Ltab"], case["mtab"], applied(case)
    R = n_sim // n_save + 1
    states, add_r, pdd_r = np.zeros((R, E, 6), f32), np.zeros((R, E)), np.zeros((R, E))
    bounce_step, bounces, wrapped = np.zeros(E, np.int64), np.zeros(E, np.int64), np.zeros(E, bool)
    edge_margin, seam_margin = np.full(E, np.inf), np.full(E, np.inf)
    flag_step = np.full(E, n_sim + 1, np.int64)
    pi = float(np.pi)
    for e in range(E):
        pm = lambda gs: dataclasses.replace(O.DEFAULT_PARAMS, m_pole=mtab[gs, e])   # noqa: E731
        r = case["s0"][e].copy()
        Q = Qa[0, e]
        add, pdd = O.plant_ode(r, Q, Ltab[0, e], pm(0))
        states[0, e], add_r[0, e], pdd_r[0, e] = r, add, pdd
        i = 1
        for g in range(1, n_sim + 1):
            L = Ltab[g, e]
            x1 = r[4] + (r[5] + pdd * dt) * dt                             # the integrated position, as O.plant_substep forms it
            hit = bool(x1 >= THL or -x1 >= THL)
            em = abs(abs(float(x1)) - float(THL))
            before = float(r[0])
            r = O.plant_substep(r, add, pdd, dt, L, pm(g))
            if hit:
                bounces[e] += 1
                bounce_step[e] = bounce_step[e] or g
            if abs(float(r[0]) - before) > pi:
                wrapped[e] = True
            sm = pi - abs(float(r[0]))
            edge_margin[e], seam_margin[e] = min(edge_margin[e], em), min(seam_margin[e], sm)
            if (em < EDGE_FLAG or sm < SEAM_FLAG) and flag_step[e] > n_sim:
                flag_step[e] = g
            if g % n_ctrl == 0:
                Q = Qa[g // n_ctrl, e]
            add, pdd = O.plant_ode(r, Q, L, pm(g))
            if g % n_save == 0:
                states[i, e], add_r[i, e], pdd_r[i, e] = r, add, pdd
                i += 1
        assert i == R
    return dict(n_sim=n_sim, states=states, add=add_r, pdd=pdd_r, step_of_row=np.arange(R) * n_save, bounce_step=bounce_step, bounces=bounces,
                wrapped=wrapped, edge_margin=edge_margin, seam_margin=seam_margin, flag_step=flag_step)


def compared(ref):
    """[R,E] bool: the saved rows whose states and derivatives are compared by tolerance (rows before the env's flag step)."""
    return ref["step_of_row"][:, None] < ref["flag_step"][None, :]


def errors(got_states, got_dd, ref):
    """The three errors of the saved rows in units of their tolerance: -> (state [R,E], angleDD [R,E], positionDD [R,E]); <= 1 passes."""
    rs = ref["states"].astype(np.float64)
    es = (np.abs(got_states.astype(np.float64) - rs) / (STATE_TOL[0] + STATE_TOL[1] * np.abs(rs))).max(axis=2)
    ea = np.abs(got_dd[:, :, 0].astype(np.float64) - ref["add"]) / (ADD_TOL[0] + ADD_TOL[1] * np.abs(ref["add"]))
    ep = np.abs(got_dd[:, :, 1].astype(np.float64) - ref["pdd"]) / (PDD_TOL[0] + PDD_TOL[1] * np.abs(ref["pdd"]))
    return es, ea, ep


def unflagged(ref):
    """[E] bool: the envs that are compared by tolerance through the whole run."""
    return ref["flag_step"] > ref["n_sim"]
