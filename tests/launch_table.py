"""Which build of the rollout kernel a launch gets, at the shapes where the rule changes its mind: the expected launch plan
(csrc/cpmppi_launch_plan.hpp) row by row.  A plain table shared by the host test of plan_rollout (test_launch_plan.py) and the
GPU test that asks the library what it launched (test_gpu_launch_table.py).

A row: the configuration (predictor, E envs x N rollouts, further MPPIConfig options, pole masses per env registered or not, the
noise source, the cost function) and what the launch must be: FAST, R (rollouts per lane), VARIANT (0 latency, 1 throughput,
2 mid-size, 3 its lone-wave form), grid size in blocks, and whether fold_env_kernel runs in front.  The limits compare BLOCKS
(x 256 lanes, x 4 waves), not E x N: 256 x 300 is 76 800 rollouts in 512 blocks = 131 072 lanes, one past the latency build."""
from collections import namedtuple

Row = namedtuple("Row", "predictor E N options mass_rows noise cost fast rpl variant blocks fold")

H, SUBSTEPS, PERIOD = 4, 2, 10          # every row: mpc_horizon, intermediate_steps, period_interpolation_inducing_points
COSTS = ["quadratic_boundary_grad_minimal", "default", "legacy_mppi_cartpole", "quadratic_boundary_grad",
         "quadratic_boundary", "quadratic_boundary_nonconvex"]          # by public cost id
KERNEL_COST = [0, 1, 2, 3, 1, 1]        # the kernel's COST template argument: 4 and 5 run on default.py's kernels
NOISES = ["delta_u", "knots", "philox", "delta_u_tiled"]               # by noise_kind
INTEG_V0, INTEG_ODE, INTEG_ODE_ROWS = 0, 1, 2

_V0 = [
    # E, N, options -> FAST, R, VARIANT, blocks, fold_first
    (255, 512, {}, 1, 1, 0, 510, False),
    (256, 512, {}, 1, 2, 3, 256, False),
    (257, 512, {}, 1, 2, 2, 257, False),
    (3072, 512, {}, 1, 2, 2, 3072, False),
    (3073, 512, {}, 1, 2, 1, 3073, True),
    (511, 256, {"rollouts_per_lane": 1}, 1, 1, 0, 511, False),
    (512, 256, {"rollouts_per_lane": 1}, 1, 1, 1, 512, True),
    (255, 300, {}, 1, 1, 0, 510, False),
    (256, 300, {}, 1, 1, 1, 512, True),
    (436, 300, {}, 1, 1, 1, 872, True),
    (437, 300, {}, 1, 2, 2, 437, False),
    (1, 512, {"rollouts_per_lane": 2}, 1, 2, 3, 1, False),
    (300, 512, {"math_mode": "precise", "rollouts_per_lane": 2}, 0, 1, 1, 600, False),
]
_ODE = [
    (256, 256, {}, 1, 1, 0, 256),
    (257, 256, {}, 1, 1, 1, 257),
    (128, 300, {}, 1, 1, 0, 256),
    (129, 300, {}, 1, 1, 1, 258),
    (256, 512, {}, 1, 2, 3, 256),
    (257, 512, {}, 1, 2, 1, 257),
    (300, 512, {"math_mode": "precise"}, 0, 1, 1, 600),
]

BOUNDARY_ROWS = [Row("ODE_v0", E, N, o, False, "philox", COSTS[0], *exp) for E, N, o, *exp in _V0] + \
                [Row("ODE", E, N, o, rows, "philox", COSTS[0], *exp, False) for rows in (False, True) for E, N, o, *exp in _ODE]
# one row per cost function (2 x 512: one rollout per lane in 4 blocks, the latency build) and per noise source other than Philox.
# (NOISE_ROWS only ask WHICH kernel runs, at one build - 256 blocks, the lone-wave form: what the buffer noise sources and the other
# costs COMPUTE in every build is held to the oracle by the matrix, rollout_matrix.py / test_gpu_rollout_matrix.py)
COST_ROWS = [Row("ODE_v0", 2, 512, {}, False, "philox", c, 1, 1, 0, 4, False) for c in COSTS]
NOISE_ROWS = [Row("ODE_v0", 256, 512, {}, False, n, COSTS[0], 1, 2, 3, 256, False) for n in ("knots", "delta_u", "delta_u_tiled")]
ROWS = BOUNDARY_ROWS + COST_ROWS + NOISE_ROWS


def integ(row):
    return INTEG_V0 if row.predictor == "ODE_v0" else (INTEG_ODE_ROWS if row.mass_rows else INTEG_ODE)


def row_id(row):
    opts = "".join(f"-{k}={v}" for k, v in row.options.items())
    return f"{row.predictor}{'-rows' if row.mass_rows else ''}-{row.E}x{row.N}{opts}-{row.noise}-{row.cost}"
