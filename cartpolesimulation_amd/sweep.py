"""Controller sweep: every setting of a grid over the MPPI controller's cost weights, LBD and SQRTRHOINV run on the SAME experiments
in ONE device loop - settings x experiments envs, each env with its own tuning row (MPPIEngine.set_tuning_rows) - and scored on the
device (MPPIEngine.score_runs: the two numbers the reference's simulator prints after an experiment, CartPole/__init__.py:727-729,
and three more).  The reference tunes these numbers with a slider window (GUI/_ControllerGUI_MPPIOptionsWindow.py), one cartpole and
one setting at a time.  The sweep reports; the user chooses.

    python -m cartpolesimulation_amd.sweep --config-root CHECKOUT --grid LBD=50,100,200 --grid ep_weight_up=20,40,80
"""
import argparse
import dataclasses
import itertools

import numpy as np

from . import _lib as _L
from .configs import TUNING_COLUMNS, MPPIConfig, tuning_rows


def expand_grid(grid):
    """``grid`` {column: values} -> (names, settings): the cartesian product in the order of the mapping, the LAST column varying
    fastest; every column a configs.TUNING_COLUMNS name (ValueError by name) with at least one value."""
    names = list(grid)
    unknown = [n for n in names if n not in TUNING_COLUMNS]
    if unknown:
        raise ValueError(f"unknown grid column(s) {', '.join(map(repr, unknown))}; available: {', '.join(TUNING_COLUMNS)}")
    values = [[float(v) for v in np.atleast_1d(grid[n])] for n in names]
    if not names or any(len(v) == 0 for v in values):
        raise ValueError("the grid needs at least one column, and every column at least one value")
    return names, [dict(zip(names, combo)) for combo in itertools.product(*values)]


def tile_batch(batch, copies):
    """The experiments of a schedule.ExperimentBatch `copies` times over, copy after copy (env = copy * E + experiment): the same
    initial states, target traces and pole lengths under every setting.  Batches with per-step parameter tables, control
    disturbance or a measurement chain are not tiled here."""
    busy = [f for f in ("L_table", "m_pole_table", "informed", "Q_disturbance", "measurement_noise", "angle_offset")
            if getattr(batch, f) is not None]
    if busy or batch.latency:
        raise ValueError(f"a sweep runs plain experiments; the batch carries {', '.join(busy) or 'a latency'}")
    return dataclasses.replace(batch, s0=np.tile(batch.s0, (copies, 1)), target_position=np.tile(batch.target_position, (1, copies)),
                               target_equilibrium=np.tile(batch.target_equilibrium, (1, copies)),
                               L=None if batch.L is None else np.tile(batch.L, copies))


def run_sweep(config, grid, experiments, seed=0, first_row=0, last_row=None, graph=False, phys=None, device=0):
    """Every setting of ``grid`` (expand_grid) on the experiments of ``experiments``, a schedule.ExperimentBatch (drawn with
    schedule.RandomExperimentSetter, or built with constant targets): one engine of settings x experiments envs, one device loop
    (``graph``: captured), one score launch over the saved rows ``first_row`` .. ``last_row``.
    -> dict: ``names``, ``settings`` (list of dicts, grid order), ``columns`` (the score names), ``scores`` [settings, experiments, 5],
    ``mean`` and ``worst`` [settings, 5] (worst: the largest value, for stable_share the smallest), ``result`` (the loop's logs)."""
    from .engine import MPPIEngine
    from .harness import BatchedCartPoleExperiment
    names, settings = expand_grid(grid)
    X, S = experiments.E, len(settings)
    batch = tile_batch(experiments, S)
    rows = tuning_rows(config, S * X, **{n: np.repeat([s[n] for s in settings], X) for n in names})
    eng = MPPIEngine(S * X, config, phys, device=device)
    try:
        exp = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=seed)
        res = exp.run_schedule(batch, tuning=rows, graph=graph)
        # (the loop's own target-position table, where it lies; the copy to the host waits for the stream)
        scores = eng.score_runs(res["states"], res["Q"], target_position_table=res["target_position_table"], save_every=batch.n_save,
                                sched_stride=batch.stride, period_steps=batch.n_ctrl, first_row=first_row,
                                last_row=last_row).cpu().numpy().reshape(S, X, _L.SCORE_FLOATS)
    finally:
        eng.close()                                # (the logs in `result` are tensors of their own: they outlive the handle)
    worst = scores.max(axis=1)
    share = _L.SCORE_COLUMNS.index("stable_share")
    worst[:, share] = scores[:, :, share].min(axis=1)
    return dict(names=names, settings=settings, columns=_L.SCORE_COLUMNS, scores=scores, mean=scores.mean(axis=1), worst=worst, result=res)


def format_table(sweep):
    """The sweep's table as text: one line per setting, the grid values, then mean and worst of each score."""
    head = list(sweep["names"]) + [f"{c}:{k}" for c in sweep["columns"] for k in ("mean", "worst")]
    lines = ["  ".join(head)]
    for i, s in enumerate(sweep["settings"]):
        cells = [f"{s[n]:g}" for n in sweep["names"]]
        cells += [f"{v:.6g}" for c in range(len(sweep["columns"])) for v in (sweep["mean"][i, c], sweep["worst"][i, c])]
        lines.append("  ".join(cells))
    return "\n".join(lines)


def main(argv=None):
    from . import schedule as SC
    from .configs import load_reference_yaml, mppi_config_from_yaml
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config-root", default=None, help="a CartPoleSimulation checkout whose YAML files configure controller and physics")
    ap.add_argument("--grid", action="append", required=True, metavar="COLUMN=v1,v2,...", help="one grid column (repeatable)")
    ap.add_argument("--experiments", type=int, default=4)
    ap.add_argument("--length", type=float, default=10.0, help="seconds per experiment")
    ap.add_argument("--seed", type=int, default=1, help="seeds the experiments' draw and the controller's noise")
    ap.add_argument("--first-row", type=int, default=0, help="first saved row scored (drops the swing-up)")
    ap.add_argument("--num-rollouts", type=int, default=None)
    ap.add_argument("--mpc-horizon", type=int, default=None)
    ap.add_argument("--graph", action="store_true", help="capture the device loop")
    args = ap.parse_args(argv)
    grid = {}
    for item in args.grid:
        name, _, values = item.partition("=")
        if not values:
            raise SystemExit(f"--grid {item!r}: expected COLUMN=v1,v2,...")
        grid[name] = [float(v) for v in values.split(",")]
    phys, config = None, MPPIConfig()
    if args.config_root:
        phys, cfgs = load_reference_yaml(args.config_root)
        config = mppi_config_from_yaml(cfgs, seed=None)
    over = {k: v for k, v in (("num_rollouts", args.num_rollouts), ("mpc_horizon", args.mpc_horizon)) if v is not None}
    config = dataclasses.replace(config, **over)
    batch = SC.RandomExperimentSetter(dict(seed=args.seed, length_of_experiment=args.length)).draw(args.experiments, args.seed)
    print(format_table(run_sweep(config, grid, batch, seed=args.seed, first_row=args.first_row, graph=args.graph, phys=phys)))


if __name__ == "__main__":
    main()
