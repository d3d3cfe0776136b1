"""Controller sweep: every setting of a grid over the MPPI controller's cost weights, LBD and SQRTRHOINV run on the SAME experiments
in ONE device loop - settings x experiments envs, each env with its own tuning row (MPPIEngine.set_tuning_rows) - and scored on the
device (MPPIEngine.score_runs: the two numbers the reference's simulator prints after an experiment, CartPole/__init__.py:727-729,
and three more).  The reference tunes these numbers with a slider window (GUI/_ControllerGUI_MPPIOptionsWindow.py), one cartpole and
one setting at a time.  The sweep reports; the user chooses.

    python -m cartpolesimulation_amd.sweep --config-root CHECKOUT --grid LBD=50,100,200 --grid ep_weight_up=20,40,80

``--optimizer rpgd`` (or ``gradient``) sweeps the controller a checkout ships instead: the fused rpgd / gradient step with a row
per env (optimizer_rpgd(fused=True, rows=...), cpmppi_rpgd_step_rows) - the grid's columns are then configs.RPGD_ROW_COLUMNS, the
cost weights, Adam's learning rate and the gradient clip - in the same single device loop, scored the same way.

    python -m cartpolesimulation_amd.sweep --config-root CHECKOUT --optimizer rpgd --grid learning_rate=0.02,0.05,0.1 --grid ep_weight_up=20,40,80
"""
import argparse
import dataclasses
import itertools

import numpy as np

from . import _lib as _L
from .configs import RPGD_ROW_COLUMNS, TUNING_COLUMNS, MPPIConfig, rpgd_rows, tuning_rows

OPTIMIZERS = ("mppi", "rpgd", "gradient")


def grid_columns(optimizer=None):
    """The grid columns of a controller: configs.TUNING_COLUMNS for the MPPI step (None or "mppi"), configs.RPGD_ROW_COLUMNS for
    "rpgd" and "gradient"."""
    if optimizer not in (None,) + OPTIMIZERS:
        raise ValueError(f"optimizer={optimizer!r}; expected one of {', '.join(OPTIMIZERS)}")
    return TUNING_COLUMNS if optimizer in (None, "mppi") else RPGD_ROW_COLUMNS


def expand_grid(grid, optimizer=None):
    """``grid`` {column: values} -> (names, settings): the cartesian product in the order of the mapping, the LAST column varying
    fastest; every column a name of the chosen controller's columns (grid_columns; ValueError by name) with at least one value."""
    names = list(grid)
    columns = grid_columns(optimizer)
    unknown = [n for n in names if n not in columns]
    if unknown:
        raise ValueError(f"unknown grid column(s) {', '.join(map(repr, unknown))}; available: {', '.join(columns)}")
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


def build_row_optimizer(optimizer, config, columns, envs, seed=0, optimizer_config=None, phys=None, device=0):
    """The fused "rpgd" / "gradient" optimizer of ``envs`` envs with a row per env: ``columns`` {RPGD_ROW_COLUMNS name: one value per
    env or a scalar} over the cost of ``config`` (an MPPIConfig: cost, cost weights, predictor, substeps, time step) and the
    optimizer's own learning rate and clip.  ``optimizer_config``: constructor keywords (a section of config_optimizers.yml, as
    controller_mpc.optimizer_section gives it), which win over ``config``.  -> the optimizer, configured."""
    import inspect
    from .optimizer_gradient import optimizer_gradient, optimizer_rpgd
    cls = {"rpgd": optimizer_rpgd, "gradient": optimizer_gradient}[optimizer]
    kw = dict(cost_function_specification=config.cost_function_specification, cost_weights=dict(config.cost_weights),
              intermediate_steps=config.intermediate_steps, mpc_timestep=config.mpc_timestep, predictor_type=config.predictor_type)
    kw.update(optimizer_config or {})
    for refused in ("rows", "gru_model", "gru_fused", "gru_adjoint"):
        if kw.get(refused) is not None and kw.get(refused) is not False:
            raise ValueError(f"optimizer_config[{refused!r}]: the sweep builds the rows itself and runs on the ODE predictors")
    defaults = inspect.signature(cls.__init__).parameters
    cost = dataclasses.replace(config, cost_function_specification=kw["cost_function_specification"], cost_weights=dict(kw["cost_weights"] or {}))
    columns = dict(columns)
    lr = columns.pop("learning_rate", kw.get("learning_rate", defaults["learning_rate"].default))
    clip = columns.pop("gradmax_clip", kw.get("gradmax_clip", defaults["gradmax_clip"].default))
    rows = rpgd_rows(cost, envs, lr, clip, **columns)
    spec = kw.pop("predictor_specification", None) or ("ODE" if kw.get("predictor_type") == "ODE" else None)
    kw.update(seed=seed, num_envs=envs, fused=True, rows=rows, phys=phys, device=device)
    opt = cls(**kw)
    opt.configure(predictor_specification=spec)
    return opt


def run_sweep(config, grid, experiments, seed=0, first_row=0, last_row=None, graph=False, phys=None, device=0, optimizer=None,
              optimizer_config=None):
    """Every setting of ``grid`` (expand_grid) on the experiments of ``experiments``, a schedule.ExperimentBatch (drawn with
    schedule.RandomExperimentSetter, or built with constant targets): one engine of settings x experiments envs, one device loop
    (``graph``: captured), one score launch over the saved rows ``first_row`` .. ``last_row``.
    ``optimizer``: None (or "mppi") - the fused MPPI step with a tuning row per env; "rpgd" / "gradient" - that fused optimizer with
    a row per env (build_row_optimizer; ``optimizer_config``: its constructor keywords), the grid over configs.RPGD_ROW_COLUMNS.
    -> dict: ``names``, ``settings`` (list of dicts, grid order), ``columns`` (the score names), ``scores`` [settings, experiments, 5],
    ``mean`` and ``worst`` [settings, 5] (worst: the largest value, for stable_share the smallest), ``result`` (the loop's logs)."""
    from .engine import MPPIEngine
    from .harness import BatchedCartPoleExperiment
    names, settings = expand_grid(grid, optimizer)
    X, S = experiments.E, len(settings)
    batch = tile_batch(experiments, S)
    columns = {n: np.repeat([s[n] for s in settings], X) for n in names}
    if optimizer in (None, "mppi"):
        if optimizer_config:
            raise ValueError("optimizer_config configures the rpgd / gradient optimizer: pass optimizer='rpgd' or 'gradient'")
        opt = None
        rows = tuning_rows(config, S * X, **columns)
        eng = MPPIEngine(S * X, config, phys, device=device)
    else:
        opt = build_row_optimizer(optimizer, config, columns, S * X, seed, optimizer_config, phys, device)
        eng = opt.engine
    try:
        exp = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=seed)
        res = exp.run_schedule(batch, tuning=rows, graph=graph) if opt is None else exp.run_schedule(batch, optimizer=opt, graph=graph)
        # (the loop's own target-position table, where it lies - an optimizer's loop hands none out: the batch's, uploaded; the
        # copy to the host waits for the stream)
        table = res["target_position_table"] if opt is None else batch.target_position
        scores = eng.score_runs(res["states"], res["Q"], target_position_table=table, save_every=batch.n_save,
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
    ap.add_argument("--optimizer", choices=OPTIMIZERS, default="mppi",
                    help="the controller swept: the fused MPPI step, or the fused rpgd / gradient optimizer (with --config-root: its "
                         "section of the checkout's config_optimizers.yml)")
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
    optimizer_config = None
    if args.optimizer == "mppi":
        config = dataclasses.replace(config, **over)
    else:
        optimizer_config = dict(over)
        if args.config_root:                         # the optimizer's own section, as controller_mpc(config_root=...) reads it
            from .controller_mpc import controller_mpc
            from .optimizer_gradient import optimizer_gradient, optimizer_rpgd
            cls = {"rpgd": optimizer_rpgd, "gradient": optimizer_gradient}[args.optimizer]
            optimizer_config = controller_mpc("CartPole", {}, config=over, config_root=args.config_root).optimizer_section(cls)
    batch = SC.RandomExperimentSetter(dict(seed=args.seed, length_of_experiment=args.length)).draw(args.experiments, args.seed)
    print(format_table(run_sweep(config, grid, batch, seed=args.seed, first_row=args.first_row, graph=args.graph, phys=phys,
                                 optimizer=args.optimizer, optimizer_config=optimizer_config)))


if __name__ == "__main__":
    main()
