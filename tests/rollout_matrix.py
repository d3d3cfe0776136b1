"""Every instantiation of the rollout kernel at the smallest launch that selects it: the table behind the oracle comparison of
all 256 builds (4 costs x 4 noise sources x 6 builds of predictor_ODE_v0, x 5 of predictor_ODE, x 5 again with the pole mass read per
env).  A plain table in the style of launch_table.py, shared by the host test (test_rollout_matrix_host.py: the table visits exactly
the kernels the library holds, plan_rollout gives every row its build, the inputs exercise what they are meant to) and the GPU test
(test_gpu_rollout_matrix.py: every cell against the oracle).

A row: predictor, whether a pole mass per env is registered, the forced MPPIConfig options, E envs x N rollouts, the knot period -
and what the launch must be: FAST, R (rollouts per lane), VARIANT (0 latency, 1 throughput, 2 mid-size, 3 the lone-wave form),
grid size in blocks, and whether in-kernel Philox parks its knots in LDS.  The limits compare BLOCKS, so E is what selects the build.
Every row: H = 66 (two lane registers of nominal sequence, 17 tile quads - the last batch of four partial -, a second 64-column pass
with 2 live lanes), S = 4 substeps (5 ms: inside the envelope FAST is validated for).  N = 300 is ragged: with two rollouts per lane
one block per env whose wave 2 is partly filled and wave 3 empty, with one rollout per lane two blocks."""
from collections import namedtuple

import numpy as np

import launch_table as T

Row = namedtuple("Row", "name predictor mass_rows options E N period costs noises fast rpl variant blocks stash")

H, SUBSTEPS, PERIOD = 66, 4, 10
COSTS = T.COSTS[:4]                      # the kernel's COST template argument = the index
NOISES = T.NOISES                        # by noise_kind = the kernel's NOISE template argument
# Weights other than the shipped ones.  legacy: its control-change-rate term (u + du - u_prev)^2 has weight 1, which leaves it at 1e-5
# of the cost of a swinging pole (12 500 (1 - cos)^2 per stage) - the kernel could read u_prev one step off and stay inside every
# relative bound (tried: it did).  At 1e4 the term is 1e-2 .. 1e-1 of a rollout's cost, and the read is pinned.
COST_WEIGHTS = {"legacy_mppi_cartpole": {"ccrc_weight": 1.0e4}}
R1, R2, PRECISE = {"rollouts_per_lane": 1}, {"rollouts_per_lane": 2}, {"math_mode": "precise"}

_V0 = [  # name, options, E -> FAST, R, VARIANT, blocks
    ("latency", R1, 6, 1, 1, 0, 12),
    ("throughput-R1", R1, 256, 1, 1, 1, 512),
    ("precise", PRECISE, 6, 0, 1, 1, 12),
    ("lone", R2, 6, 1, 2, 3, 6),
    ("mid", R2, 257, 1, 2, 2, 257),
    ("throughput-R2", R2, 3073, 1, 2, 1, 3073),
]
_ODE = [
    ("latency", R1, 6, 1, 1, 0, 12),
    ("throughput-R1", R1, 129, 1, 1, 1, 258),
    ("precise", PRECISE, 6, 0, 1, 1, 12),
    ("lone", R2, 6, 1, 2, 3, 6),
    ("throughput-R2", R2, 257, 1, 2, 1, 257),
]
# 16 rows x 4 costs x 4 noise sources: the 256 instantiations (period 10, P = 8 knots: Philox parks them in both lane mappings)
MAIN_ROWS = [Row(f"ODE_v0-{n}", "ODE_v0", False, o, E, 300, PERIOD, COSTS, NOISES, *exp, 1) for n, o, E, *exp in _V0] + \
            [Row(f"ODE{'-rows' if rows else ''}-{n}", "ODE", rows, o, E, 300, PERIOD, COSTS, NOISES, *exp, 1)
             for rows in (False, True) for n, o, E, *exp in _ODE]
# secondary shapes, quadratic_boundary_grad_minimal only.  N = 700: two blocks per env with two rollouts per lane, the last ragged
# (wave 2 of block 1 partly filled)
N700_ROWS = [Row("ODE_v0-mid-N700", "ODE_v0", False, R2, 129, 700, PERIOD, COSTS[:1], NOISES, 1, 2, 2, 258, 1),
             Row("ODE_v0-throughput-R2-N700", "ODE_v0", False, R2, 1537, 700, PERIOD, COSTS[:1], NOISES, 1, 2, 1, 3074, 1)]
# knot period 2: P = 34 knots do not fit in LDS beside the weighted sums in either lane mapping, so the reduction regenerates them
REGEN_ROWS = [Row(f"ODE_v0-{n}-period2", "ODE_v0", False, o, 6, 300, 2, COSTS[:1], ["philox"], 1, rpl, v, b, 0)
              for n, o, rpl, v, b in (("latency", R1, 1, 0, 12), ("lone", R2, 2, 3, 6))] + \
             [Row("ODE_v0-throughput-R2-period2", "ODE_v0", False, R2, 3073, 300, 2, COSTS[:1], ["philox"], 1, 2, 1, 3073, 0)]
ROWS = MAIN_ROWS + N700_ROWS + REGEN_ROWS
BY_NAME = {r.name: r for r in ROWS}
# builds of one lane mapping integrate an env identically (test_gpu_rollout_matrix.py, across builds): (reference row, others)
BUILD_GROUPS = [("ODE_v0-throughput-R2", ["ODE_v0-mid", "ODE_v0-lone"]), ("ODE_v0-throughput-R1", ["ODE_v0-latency"]),
                ("ODE-throughput-R2", ["ODE-lone"]), ("ODE-throughput-R1", ["ODE-latency"]),
                ("ODE-rows-throughput-R2", ["ODE-rows-lone"]), ("ODE-rows-throughput-R1", ["ODE-rows-latency"])]
COMMON_ENVS = [0, 1, 2, 3]               # checked in every row: one env of each regime


def row_id(row):
    return row.name


def knot_count(row):
    return (H + row.period - 1) // row.period + 1


def integ(row):
    """The kernel's INTEG template argument (the rows kernel is a second compilation of predictor_ODE's)."""
    return 0 if row.predictor == "ODE_v0" else 1


def cells(row):
    return [(c, n) for c in row.costs for n in row.noises]


def instantiation(row, cost, noise):
    """(rows kernel?, COST, FAST, NOISE, R, VARIANT, INTEG): the template arguments of the kernel a cell runs."""
    return (row.mass_rows, COSTS.index(cost), row.fast, NOISES.index(noise), row.rpl, row.variant, integ(row))


def mangled_fragment(inst):
    rows, cost, fast, noise, rpl, variant, integ_ = inst
    return "%s_kernelILi%dELb%dELi%dELi%dELi%dELi%dEEE" % ("rollout_cost_rows" if rows else "rollout_cost", cost, fast, noise, rpl,
                                                            variant, integ_)


def expected_launch(row, cost, noise):
    """What cpmppi_last_launch must report for a cell, `kernel` (as test_gpu_launch_table.py forms it) included."""
    c, ode = COSTS.index(cost), row.predictor == "ODE"
    return dict(math_mode=row.fast, rollouts_per_lane=row.rpl, build_variant=row.variant, ode_predictor=int(ode), blocks=row.blocks,
                noise_kind=NOISES.index(noise), cost_id=c, cost_plugin=c,
                kernel="rollout_cost%s_kernel<%d, %s, %d, %d, %d%s>" % ("_rows" if row.mass_rows else "", c, "true" if row.fast else "false",
                                                                          NOISES.index(noise), row.rpl, row.variant,
                                                                          ", PREDICTOR_ODE" if ode else ""))


def checked_envs(E):
    """The first and the last block of the grid, and one in the middle."""
    return sorted({0, 1, 2, 3, E // 2, E - 3, E - 2, E - 1})


# ---- inputs ---------------------------------------------------------------------------------------------------------------
f32 = np.float32
THL = float(f32((44.0e-2 - 4.4e-2) / 2.0))
INPUT_SEED, NOISE_SEED, NOISE_OFFSET = 20, 77, 5
MILD_UP, MILD_DOWN, EDGE, SPIN = range(4)
M_LO, M_HI = 0.015, 0.15                 # the pole-mass updater's range (test_gpu_pole_mass_rows.py)


def regime(e):
    return e % 4


def inputs(E, seed=INPUT_SEED):
    """All E envs from one generator, by regime e % 4: 0 mild with the upright target (angle anywhere, |angleD| <= 6, |x| <= 0.5 THL),
    1 the same with the hanging target, 2 a start at 0.85 .. 0.97 THL moving outward at 0.2 .. 0.6 m/s under a nominal sequence that
    pushes outward, 3 a fast spin (|angleD| up to 12).  Per env: pole length, target position, pole mass, a nonzero nominal sequence.
    Env e's values do not depend on E (one row of uniform draws per env), so builds launched at different sizes see the same env e.
    -> dict(s0 [E,6], tp, te, L, m [E], u0 [E,H])."""
    U = np.random.Generator(np.random.SFC64(seed)).uniform(size=(E, 10 + H))
    sym = lambda col: 2.0 * U[:, col] - 1.0          # noqa: E731
    reg = np.arange(E) % 4
    ang = np.pi * sym(0)
    angD = np.where(reg == SPIN, 12.0, 6.0) * sym(1)
    x = 0.5 * THL * sym(2)
    v = 0.3 * sym(3)
    side = np.where(U[:, 4] < 0.5, -1.0, 1.0)
    edge = reg == EDGE
    x = np.where(edge, side * (0.85 + 0.12 * U[:, 2]) * THL, x)
    v = np.where(edge, side * (0.2 + 0.4 * U[:, 3]), v)
    s0 = np.zeros((E, 6), f32)
    s0[:, 0], s0[:, 1], s0[:, 4], s0[:, 5] = ang, angD, x, v
    s0[:, 2], s0[:, 3] = np.cos(s0[:, 0]), np.sin(s0[:, 0])
    u0 = 0.6 * (2.0 * U[:, 10:] - 1.0)
    u0 = np.where(edge[:, None], side[:, None] * (0.3 + 0.5 * U[:, 10:]), u0)
    return dict(s0=s0, tp=(0.5 * THL * sym(5)).astype(f32), te=np.where(reg == MILD_DOWN, -1.0, 1.0).astype(f32),
                L=(0.25 + 0.2 * U[:, 6]).astype(f32), m=(M_LO + (M_HI - M_LO) * U[:, 7]).astype(f32), u0=u0.astype(f32))


# ---- the reference --------------------------------------------------------------------------------------------------------
def oracle_config(row, cost):
    from oracle import oracle_np as O
    cfg = O.MPPIConfig(N=row.N, H=H, S=SUBSTEPS, period=row.period, cost_id=COSTS.index(cost), integrator=row.predictor)
    for k, v in COST_WEIGHTS.get(cost, {}).items():
        assert cost == "legacy_mppi_cartpole" and hasattr(cfg.cost, "leg_" + k)
        setattr(cfg.cost, "leg_" + k, v)
    return cfg


def reference(row, cost, inp, du, envs, trajectories=False):
    """The oracle's step for the envs `envs` of a launch (inp: inputs(row.E); du [len(envs), N, H]: their perturbations), once per
    cost and shared by the four noise sources.  quadratic_boundary_grad_minimal / default / legacy: the C oracle in both arithmetic
    modes with the probes one rounding away and the H2 flags; quadratic_boundary_grad: the numpy oracle in modes f32 and f64sub.  With
    a pole mass per env every env runs under its own.  -> dict(S_a, S_b [n,N], u_a, u_b [n,H], flags [n,N], S_alt, u_alt: lists) and,
    with `trajectories` (C oracle only), x_max [n,N]: how far out each rollout's cart gets in the oracle (control-step samples)."""
    from dataclasses import replace
    from oracle import oracle_np as O
    from oracle import oracle_c as OC
    from oracle import parity as PU
    ocfg = oracle_config(row, cost)
    s0, u0, tp, te, L = (inp[k][envs] for k in ("s0", "u0", "tp", "te", "L"))
    groups = [[i] for i in range(len(envs))] if row.mass_rows else [list(range(len(envs)))]
    parts = []
    for g in groups:
        p = replace(O.DEFAULT_PARAMS, m_pole=inp["m"][envs[g[0]]]) if row.mass_rows else None
        if cost == "quadratic_boundary_grad":
            a, b = ([O.mppi_step(s0[i], u0[i], du[i], tp[i], te[i], ocfg, L=L[i], p=p or O.DEFAULT_PARAMS, mode=m) for i in g]
                    for m in ("f32", "f64sub"))
            parts.append(dict(S_a=np.stack([r["S"] for r in a]), S_b=np.stack([r["S"] for r in b]),
                              u_a=np.stack([r["u_new"] for r in a]), u_b=np.stack([r["u_new"] for r in b]),
                              flags=np.stack([PU.flag_discontinuities(r["traj"]) for r in a]), S_alt=[], u_alt=[]))
            continue
        r = PU.c_oracle_step_with_flags(ocfg, s0[g], u0[g], du[g], tp[g], te[g], L=L[g], params=p,
                                        cost={"default": "default", "legacy_mppi_cartpole": "legacy"}.get(cost), probes=True)
        r.pop("Q_a")
        if trajectories:
            u_run = np.clip(np.concatenate([u0[g][:, 1:], u0[g][:, -1:]], axis=1)[:, None, :] + du[g], -1, 1).astype(f32)
            traj = OC.predict(OC.make_config(ocfg, p), np.repeat(s0[g], row.N, axis=0), u_run.reshape(-1, H), L=np.repeat(L[g], row.N))
            r["x_max"] = np.abs(traj[:, :, O.POSITION_IDX]).max(axis=1).reshape(len(g), row.N)
        parts.append(r)
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k not in ("S_alt", "u_alt")}
    for k in ("S_alt", "u_alt"):
        out[k] = [np.concatenate([p[k][j] for p in parts]) for j in range(len(parts[0][k]))]
    return out


def hanging_target():
    """tools/dev/hanging_target.py: the bound the fuzz tool holds default.py's cost with the hanging target to."""
    import os
    import sys
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dev")
    if d not in sys.path:
        sys.path.insert(0, d)
    import hanging_target as m
    return m


def rule(row):
    from oracle import parity as PU
    return PU.PREDICTOR_ODE if row.predictor == "ODE" else PU.ODE_V0


def buckets(row, cost, te, S, ref, i):
    """The verdict on env i's costs S [N] under the project's rules: parity's cost_buckets under the predictor's rule with the
    quarter-band sensitivity flag - or, for default.py's cost with the hanging target, hanging_default_buckets."""
    from oracle import parity as PU
    alt = [a[i] for a in ref["S_alt"]]
    if cost == "default" and te < 0:
        return hanging_target().hanging_default_buckets(S, ref["S_a"][i], ref["S_b"][i], ref["flags"][i], alt, H=H)
    return PU.cost_buckets(S, ref["S_a"][i], ref["S_b"][i], ref["flags"][i], alt, flag_sensitive=True, rule=rule(row))
