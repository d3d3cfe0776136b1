"""Control along recorded trajectories - relabel recordings with a controller's output, in one device loop.

The reference computes a controller's output along recordings that exist already, whatever controller made them
(SI_Toolkit_ASF/Run/PreprocessData_Add_Control_Along_Trajectories.py, fanned out by
others/EulerClusterScripts/ControllerAlongTrajectories.sh as a SLURM array of 120 single-CPU jobs of up to two hours each); the
column it writes, ``Q_calculated_offline``, is the training target of the network the reference ships.  Here all recordings and
all evaluations of a stochastic controller are envs of ONE device loop (harness.ReplayRun): per row the fused control step and
one cpmppi_replay_step, which hands the controller the recorded row where the plant would hand it the simulated one and reduces
the evaluations of a row to one number.

THE SEMANTICS ARE THIS PACKAGE'S OWN.  The upstream function (SI_Toolkit.data_preprocessing.transform_dataset) lives in a
submodule that is empty in the reference checkout, so its rules cannot be pinned; these are ours:
  * each of the ``num_evals`` copies of a recording is an independent controller instance: env r*K + k for copy k of recording r;
  * the env index feeds Philox, so the copies draw different noise; the Philox offset of row c is c;
  * with ``warm_start`` the nominal plan is carried from row to row within a copy, without it every row is solved from a zero plan;
  * the result of a row is the mean over the copies (float64 sum in a fixed order, rounded to float32 once).
Recordings are processed in chunks of ``max_envs // num_evals`` files; every chunk numbers its envs from 0 again, so a recording's
noise depends on its place in its chunk.

Served: the fused MPPI step over ODE_v0 and ODE, and rpgd with ``fused=True`` (warm start only).  Not served, refused by name:
optimizer objects paced by the host, ``warmup=True`` under a captured graph, the GRU predictor, ``warm_start=False`` for anything
but MPPI.

  python -m cartpolesimulation_amd.along_trajectories --config-root CHECKOUT --get-files-from PATH --save-files-to DIR [-i N]
      [--num-evals 64] [--optimizer mppi|rpgd] [--no-warm-start] [--column L=NAME ...] [--output-name NAME] [--save-output-only] [--graph]
"""
import csv
import os

import numpy as np

from ._optimizer_base import is_gru_specification
from .configs import MPPIConfig, PhysicalParameters
from .harness import REPLAY_REFUSALS
from .state_utilities import STATE_VARIABLES

f32 = np.float32
FEATURES = tuple(STATE_VARIABLES)
ATTRIBUTES = ("target_position", "target_equilibrium", "L", "Q_ccrc")     # what the controller is handed besides the state
PREVIOUS_INPUT_COLUMNS = ("Q_ccrc", "Q_applied_-1")                        # the recorded control applied before a row, by its two names
OPTIMIZERS = ("mppi", "rpgd")


def load_columns(path, wanted=None):
    """A recording CSV (``#`` preamble, a row of column names, one row per saved time step) -> dict: ``names`` (the file's column
    names, in order), the six state features (float32) and every column of ``wanted`` (None: every other column that parses as
    numbers) as float32 - what brunton.load_recording drops: target_position, target_equilibrium, Q_ccrc, ...  A wanted column that
    the file lacks is a ValueError naming it."""
    with open(path, newline="") as f:
        rows = [r for r in csv.reader(line for line in f if not line.startswith("#")) if r]
    if not rows:
        raise ValueError(f"{path}: no header row")
    names, body = rows[0], rows[1:]
    missing = [c for c in FEATURES if c not in names] + [c for c in (wanted or ()) if c not in names]
    if missing:
        raise ValueError(f"{path}: columns {missing} missing (have {names})")
    out = {"names": list(names)}
    for name in dict.fromkeys(FEATURES + tuple(names if wanted is None else wanted)):
        i = names.index(name)
        try:
            out[name] = np.array([float(r[i]) for r in body], dtype=np.float64).astype(f32)
        except (ValueError, IndexError) as e:
            if wanted is None and name not in FEATURES:
                continue                                    # ('true' strings, empty Q_update_time fields)
            raise ValueError(f"{path}: column {name!r}: {e}") from None
    return out


def resolve_columns(columns, have, where="the recordings"):
    """``columns`` (controller attribute -> column name, the reference's environment_attributes_dict; None: the defaults) against
    the column names ``have`` -> {attribute: column name or None}.  A MAPPED column that is missing is refused by name; by default
    target_position and target_equilibrium are the columns of those names (required), ``L`` is the column L or None (the config's
    pole length), ``Q_ccrc`` is Q_ccrc, else Q_applied_-1, else None."""
    columns = dict(columns or {})
    unknown = [a for a in columns if a not in ATTRIBUTES]
    if unknown:
        raise ValueError(f"unknown controller attribute(s) {unknown}; a column can be mapped to {list(ATTRIBUTES)}")
    out = {}
    for attr in ATTRIBUTES:
        if attr in columns:
            if columns[attr] not in have:
                raise ValueError(f"{where}: column {columns[attr]!r} (mapped to {attr}) is missing (have {list(have)})")
            out[attr] = columns[attr]
        elif attr == "Q_ccrc":
            out[attr] = next((c for c in PREVIOUS_INPUT_COLUMNS if c in have), None)
        elif attr == "L":
            out[attr] = "L" if "L" in have else None
        elif attr not in have:
            raise ValueError(f"{where}: column {attr!r} is missing (have {list(have)}); map another one with columns={{{attr!r}: NAME}}")
        else:
            out[attr] = attr
    return out


def _one(rec, columns):
    """One recording - a path or a column dict - -> (states [T,6], {attribute: [T] or None})."""
    if isinstance(rec, (str, os.PathLike)):
        where = str(rec)
        with open(rec, newline="") as f:
            header = next((r for r in csv.reader(line for line in f if not line.startswith("#")) if r), None)
        if header is None:
            raise ValueError(f"{where}: no header row")
        names = resolve_columns(columns, header, where)
        rec = load_columns(rec, [c for c in names.values() if c is not None])
    else:
        names = resolve_columns(columns, [k for k in rec if k != "names"], "a column dict")
    if "states" in rec:
        states = np.asarray(rec["states"], f32)
    else:
        states = np.stack([np.asarray(rec[c], f32) for c in FEATURES], axis=-1)
    if states.ndim != 2 or states.shape[1] != 6 or states.shape[0] == 0:
        raise ValueError(f"a recording's states must be [T,6] with T >= 1, got {states.shape}")
    attrs = {}
    for attr, name in names.items():
        attrs[attr] = None if name is None else np.asarray(rec[name], f32).reshape(-1)
        if attrs[attr] is not None and attrs[attr].shape[0] != states.shape[0]:
            raise ValueError(f"column {name!r} has {attrs[attr].shape[0]} rows, the states {states.shape[0]}")
    return states, attrs


def stack_recordings(recordings, columns=None):
    """``recordings`` in any of its three forms - paths of recording CSVs, column dicts (a column per name; the state as its six
    feature columns or as ``states`` [T,6]), or ONE dict of arrays (``states`` [R,T,6], the columns [R,T], optionally ``rows`` [R]) -
    -> (states [R,T,6] padded with zeros, rows [R], {attribute: [R,T] or None}).  Unequal lengths are normal here."""
    if isinstance(recordings, (str, os.PathLike)):
        recordings = [recordings]
    if isinstance(recordings, dict) and np.ndim(recordings.get("states")) == 3:
        states = np.ascontiguousarray(recordings["states"], f32)
        R, T = states.shape[:2]
        rows = np.asarray(recordings.get("rows", np.full(R, T)), np.int64).reshape(-1)
        names = resolve_columns(columns, [k for k in recordings if k not in ("states", "rows")], "the arrays")
        attrs = {a: None if n is None else np.ascontiguousarray(np.asarray(recordings[n], f32).reshape(R, T)) for a, n in names.items()}
        if states.shape[2] != 6 or rows.shape != (R,) or rows.min() < 1 or rows.max() > T:
            raise ValueError(f"arrays must be states [R,T,6] with rows [R] in 1..T, got {states.shape} and rows {rows}")
        return states, rows.astype(np.uint32), attrs
    parts = [_one(r, columns) for r in recordings]
    if not parts:
        raise ValueError("no recordings")
    rows = np.array([p[0].shape[0] for p in parts], np.uint32)
    R, T = len(parts), int(rows.max())
    states = np.zeros((R, T, 6), f32)
    attrs = {}
    for attr in ATTRIBUTES:
        given = [p[1][attr] is not None for p in parts]
        if any(given) and not all(given):
            raise ValueError(f"some recordings carry a column for {attr} and some do not")
        attrs[attr] = np.zeros((R, T), f32) if all(given) else None
    for r, (s, a) in enumerate(parts):
        states[r, :rows[r]] = s
        for attr, col in a.items():
            if col is not None:
                attrs[attr][r, :rows[r]] = col
    return states, rows, attrs


def _settings(config, config_root, phys, predictor_specification):
    """-> (PhysicalParameters, the checkout's YAML files or None, the caller's config as a dict of overrides, the predictor
    specification); a GRU specification or model is refused here, before any recording is read."""
    cfgs = None
    if config_root is not None:
        from .configs import load_reference_yaml
        yaml_phys, cfgs = load_reference_yaml(config_root)
        phys = phys or yaml_phys
        if predictor_specification is None:
            predictor_specification = cfgs["controllers"]["mpc"].get("predictor_specification")
    user = dict(config) if isinstance(config, dict) else {}
    spec = predictor_specification or user.pop("predictor_specification", None)
    if spec is not None and is_gru_specification(str(spec).split(":")[0]):
        raise ValueError(REPLAY_REFUSALS["gru"] + f" (predictor_specification {spec!r})")
    if user.get("gru_model") is not None:
        raise ValueError(REPLAY_REFUSALS["gru"] + " (gru_model given)")
    return phys or PhysicalParameters(), cfgs, user, spec


def control_along_trajectories(recordings, config=None, config_root=None, optimizer="mppi", num_evals=1, warm_start=True, seed=0,
                               columns=None, graph=False, steps_per_graph=10, max_envs=8192, return_evals=False, device=0, phys=None,
                               predictor_specification=None):
    """The controller's output along ``recordings`` (paths, column dicts or one dict of arrays: ``stack_recordings``).
    -> dict(Q [R,T] float32, the mean over the ``num_evals`` copies of a recording, NaN past a recording's end; Q_std [R,T], their
    sample standard deviation (0 for one copy); rows [R]; with ``return_evals`` Q_evals [T,R,K], NaN likewise), on the host.

    The semantics are this package's own (the upstream transform_dataset is not in the reference checkout): each of the
    ``num_evals`` copies of a recording is an independent controller instance; env index r*K + k feeds Philox, so copies differ;
    the Philox offset of row c is c; with ``warm_start`` the nominal plan is carried from row to row within a copy, without it
    every row is solved from a zero plan; the result of a row is the mean over the copies.  Recordings are processed in chunks of
    ``max_envs // num_evals`` files, and every chunk numbers its envs from 0 again: a recording's noise depends on its place in
    its chunk, so the results of the first chunk alone equal an unchunked run's for the same recordings.

    ``optimizer``: "mppi" - the fused MPPI step, ``config`` an MPPIConfig or a dict of its fields (with ``config_root``: over the
    checkout's YAML) - or "rpgd" - the fused rpgd step, ``config`` a dict of optimizer_rpgd's keywords; or a fused optimizer OBJECT
    configured for R * num_evals envs (one chunk).  ``columns``: controller attribute -> column name (``resolve_columns``); a
    recording without ``L`` is controlled with the config's pole length.  ``graph``: ``steps_per_graph`` rows at a time are replays
    of one captured HIP graph."""
    K, max_envs = int(num_evals), int(max_envs)
    if K < 1:
        raise ValueError("num_evals must be at least 1")
    if K > max_envs:
        raise ValueError(f"num_evals {K} exceeds max_envs {max_envs}: the copies of one recording are the smallest chunk")
    obj = None if isinstance(optimizer, str) else optimizer
    if obj is None and optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer {optimizer!r}: control along recordings runs {' and '.join(map(repr, OPTIMIZERS))} (fused) or a "
                         "fused optimizer object")
    if obj is not None and not getattr(obj, "fused", False):
        raise ValueError(REPLAY_REFUSALS["host_paced"])
    if (obj is not None or optimizer != "mppi") and not warm_start:
        raise ValueError(REPLAY_REFUSALS["cold_optimizer"])
    phys, cfgs, user, spec = _settings(config, config_root, phys, predictor_specification)
    states, rows, attrs = stack_recordings(recordings, columns)
    R = states.shape[0]
    per_chunk = max_envs // K
    if obj is not None and (R > per_chunk or getattr(obj, "num_envs", R * K) != R * K):
        raise ValueError(f"an optimizer object serves one chunk of its own size: {R} recordings x {K} evaluations = {R * K} envs")

    from .engine import MPPIEngine
    from .harness import ReplayBuffers, ReplayRun
    T_all = int(rows.max())
    out = dict(Q=np.full((R, T_all), np.nan, f32), Q_std=np.full((R, T_all), np.nan, f32), rows=rows.copy())
    if return_evals:
        out["Q_evals"] = np.full((T_all, R, K), np.nan, f32)
    eng = None
    if obj is None and optimizer == "mppi":
        if isinstance(config, MPPIConfig):
            mppi = config
        elif cfgs is not None:
            from .configs import mppi_config_from_yaml
            mppi = mppi_config_from_yaml(cfgs, **user)
        else:
            mppi = MPPIConfig(**user)
        if spec is not None:
            from .configs import ode_predictor_type
            import dataclasses
            mppi = dataclasses.replace(mppi, predictor_type=ode_predictor_type(
                spec, f"predictor {spec!r}: control along recordings runs the ODE_v0 and ODE predictors"))
        eng = MPPIEngine(min(R, per_chunk) * K, mppi, phys, device=device)
    try:
        for r0 in range(0, R, per_chunk):
            r1 = min(r0 + per_chunk, R)
            T = int(rows[r0:r1].max())
            cut = lambda a: None if a is None else np.ascontiguousarray(a[r0:r1, :T])      # noqa: E731
            opt, run_eng = obj, eng
            if obj is None and optimizer == "rpgd":
                from .controller_mpc import controller_mpc
                ctrl = controller_mpc(config=user, config_root=config_root, phys=phys, device=device, num_envs=(r1 - r0) * K)
                ctrl.configure("rpgd", predictor_specification=spec, fused=True, seed=int(seed))
                opt = ctrl.optimizer
            if opt is not None:
                if opt.engine is None:
                    opt.configure()
                run_eng = opt.engine
            buf = ReplayBuffers(run_eng, cut(states), rows[r0:r1], K, cut(attrs["target_position"]), cut(attrs["target_equilibrium"]),
                                L=cut(attrs["L"]), previous=cut(attrs["Q_ccrc"]), keep_evals=return_evals)
            res = ReplayRun(run_eng, buf, seed, optimizer=opt, warm_start=warm_start).run(graph=graph, steps_per_graph=steps_per_graph)
            out["Q"][r0:r1, :T] = res["Q"].cpu().numpy()
            out["Q_std"][r0:r1, :T] = res["Q_std"].cpu().numpy()
            if return_evals:
                out["Q_evals"][:T, r0:r1] = res["Q_evals"].cpu().numpy()
    finally:
        if eng is not None:
            eng.close()
    return out


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def _split_lines(data):
    """bytes -> [(line without its terminator, terminator)]"""
    out = []
    for line in data.splitlines(keepends=True):
        body = line.rstrip(b"\r\n")
        out.append((body, line[len(body):]))
    return out


def append_column(src, dst, name, values, save_output_only=False):
    """``dst`` = the file ``src`` byte for byte with one field appended to the column-name row (``name``) and to every data row
    (``values``, each written as repr(float(x)): the convention of the Q_calculated column, which reads back exactly); the ``#``
    preamble is unchanged.  ``save_output_only``: the rows hold ``time`` and the new column only.  Never overwrites: an existing
    ``dst`` is a FileExistsError, a ``src`` that has the column already a ValueError."""
    if os.path.exists(dst):
        raise FileExistsError(f"{dst} exists: the package never overwrites a recording")
    with open(src, "rb") as f:
        lines = _split_lines(f.read())
    fields = iter([name] + [repr(float(x)) for x in values])
    header, out, time_at = None, [], None
    for body, end in lines:
        if body.startswith(b"#") or not body.strip():
            out.append(body + end)
            continue
        field = next(fields, None)
        if field is None:
            raise ValueError(f"{src}: more data rows than the {len(values)} values computed")
        if header is None:
            header = next(csv.reader([body.decode()]))
            if name in header:
                raise ValueError(f"{src} already has a column {name!r}: choose another controller_output_variable_name")
            if save_output_only:
                if "time" not in header:
                    raise ValueError(f"{src}: save_output_only writes time and {name}, and there is no time column")
                time_at = header.index("time")
        if time_at is not None:
            body = next(csv.reader([body.decode()]))[time_at].encode()
        out.append(body + b"," + field.encode() + end)
    if next(fields, None) is not None:
        raise ValueError(f"{src}: fewer data rows than the {len(values)} values computed")
    with open(dst, "xb") as f:
        f.write(b"".join(out))
    return dst


def input_files(get_files_from, secondary_experiment_index=None):
    """A file, or a folder's *.csv in sorted order; with an index the folder's Experiment-{i:03d}.csv (the reference's ``-i``)."""
    if os.path.isdir(get_files_from):
        if secondary_experiment_index is not None:
            return [os.path.join(get_files_from, f"Experiment-{int(secondary_experiment_index):03d}.csv")]
        return sorted(os.path.join(get_files_from, n) for n in os.listdir(get_files_from) if n.endswith(".csv"))
    return [get_files_from]


def transform_recordings(get_files_from, save_files_to, controller_output_variable_name="Q_calculated_offline", save_output_only=False,
                         secondary_experiment_index=None, **control):
    """Relabel recording files: every file of ``input_files(get_files_from, secondary_experiment_index)`` is written to the folder
    ``save_files_to`` under its own name with the column ``controller_output_variable_name`` appended (``append_column``), its
    values the result of ``control_along_trajectories(files, **control)``.  Nothing is computed when a refusal is known beforehand:
    an existing output file, an input that has the column already.  -> the paths written."""
    files = input_files(get_files_from, secondary_experiment_index)
    if not files:
        raise ValueError(f"no *.csv in {get_files_from}")
    name = controller_output_variable_name
    targets = [os.path.join(save_files_to, os.path.basename(p)) for p in files]
    for src, dst in zip(files, targets):
        if os.path.exists(dst):
            raise FileExistsError(f"{dst} exists: the package never overwrites a recording")
        with open(src, newline="") as f:
            header = next((r for r in csv.reader(line for line in f if not line.startswith("#")) if r), [])
        if name in header:
            raise ValueError(f"{src} already has a column {name!r}: choose another controller_output_variable_name")
    res = control_along_trajectories(files, **control)
    os.makedirs(save_files_to, exist_ok=True)
    return [append_column(src, dst, name, res["Q"][r, :res["rows"][r]], save_output_only)
            for r, (src, dst) in enumerate(zip(files, targets))]


def main(argv=None):
    """python -m cartpolesimulation_amd.along_trajectories --config-root CHECKOUT --get-files-from PATH --save-files-to DIR ..."""
    import argparse
    ap = argparse.ArgumentParser(description="Control along recorded trajectories on MI355X (reference: SI_Toolkit_ASF/Run/"
                                             "PreprocessData_Add_Control_Along_Trajectories.py)")
    ap.add_argument("--config-root", default=None, help="a CartPoleSimulation checkout: its YAML files configure the controller")
    ap.add_argument("--get-files-from", required=True, metavar="PATH", help="a recording or a folder of them")
    ap.add_argument("--save-files-to", required=True, metavar="DIR")
    ap.add_argument("-i", "--secondary-experiment-index", type=int, default=None, help="only Experiment-{i:03d}.csv of the folder")
    ap.add_argument("--num-evals", type=int, default=64, help="evaluations of the stochastic controller per row (integration_num_evals)")
    ap.add_argument("--optimizer", default="mppi", choices=OPTIMIZERS)
    ap.add_argument("--no-warm-start", action="store_true", help="solve every row from a zero plan (mppi)")
    ap.add_argument("--column", action="append", default=[], metavar="ATTRIBUTE=NAME", help="read a controller attribute from another column")
    ap.add_argument("--output-name", default="Q_calculated_offline")
    ap.add_argument("--save-output-only", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay captured HIP graphs of --steps-per-graph rows")
    ap.add_argument("--steps-per-graph", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-envs", type=int, default=8192)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    columns = {}
    for item in args.column:
        attr, eq, col = item.partition("=")
        if not eq or not col:
            ap.error(f"--column {item!r}: expected ATTRIBUTE=NAME")
        columns[attr] = col
    written = transform_recordings(args.get_files_from, args.save_files_to, controller_output_variable_name=args.output_name,
                                   save_output_only=args.save_output_only, secondary_experiment_index=args.secondary_experiment_index,
                                   config_root=args.config_root, optimizer=args.optimizer, num_evals=args.num_evals,
                                   warm_start=not args.no_warm_start, seed=args.seed, columns=columns or None, graph=args.graph,
                                   steps_per_graph=args.steps_per_graph, max_envs=args.max_envs, device=args.device)
    for path in written:
        print(path)
    return written


if __name__ == "__main__":
    main()
