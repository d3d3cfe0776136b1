"""Brunton test — the open-loop error of a predictor over recordings (SI_Toolkit_ASF/Run/A3_Run_Brunton_Test.py with the keys of
SI_Toolkit_ASF/config_testing.yml): "how good is this predictor on this data?", the step between generating a dataset
(recording.generate_dataset) and putting a trained model into the loop.

From every row t of a recording the predictor is rolled forward ``horizon`` control steps on the RECORDED controls and each
predicted state is compared with the recorded one, t+k+1.  The whole test of one predictor is one fused launch (cpmppi_brunton:
the recordings are read where they lie, the per-horizon-step error statistics are reduced on the device, the predictions
[starts, horizon+1, 6] are written only when asked for); the GRU first walks its memory along each recording in one launch
(cpmppi_gru_washout - the reference's ``update_before_predicting``).

Not here: the energy metrics of brunton_widget_extensions.py, the plots and the GUI; GP and Dense predictors; a pole mass per row.

  python -m cartpolesimulation_amd.brunton --config-root <CartPoleSimulation checkout> [--test-file FILE.csv | FOLDER] [--gru-model FOLDER]
"""
import csv
import os

import numpy as np

from ._optimizer_base import is_gru_specification
from .configs import MPPIConfig, PhysicalParameters, ode_predictor_type
from .state_utilities import STATE_VARIABLES

f32 = np.float32
FEATURES = tuple(STATE_VARIABLES)                       # angle, angleD, angle_cos, angle_sin, position, positionD
CONTROL_COLUMNS = ("Q", "Q_applied", "Q_calculated")    # the predictors' control input, by the names recordings have carried


def load_recording(path):
    """A recording CSV as recording.write_recording / the native writer / the reference's csv_logger write it - ``#`` comment
    preamble, a row of column names, one row per saved time step - -> dict of numpy columns: ``time`` (float64), the six state
    features and ``Q`` (float32; the control the plant was driven by: column ``Q``, else ``Q_applied``, else ``Q_calculated``),
    and ``L`` (float32) where the file has it.  A float32 the writers printed with its shortest digits is read back exactly.
    Columns the predictors do not need ('true' strings, empty Q_update_time fields) are not parsed."""
    with open(path, newline="") as f:
        rows = [r for r in csv.reader(line for line in f if not line.startswith("#")) if r]
    if not rows:
        raise ValueError(f"{path}: no header row")
    names, body = rows[0], rows[1:]
    q_name = next((c for c in CONTROL_COLUMNS if c in names), None)
    missing = [c for c in FEATURES if c not in names] + ([] if q_name else ["Q"])
    if missing:
        raise ValueError(f"{path}: columns {missing} missing (have {names})")

    def column(name, dtype):
        i = names.index(name)
        try:
            return np.array([float(r[i]) for r in body], dtype=np.float64).astype(dtype)
        except (ValueError, IndexError) as e:
            raise ValueError(f"{path}: column {name!r}: {e}") from None

    out = {"time": column("time", np.float64) if "time" in names else None}
    out.update({c: column(c, f32) for c in FEATURES})
    out["Q"] = column(q_name, f32)
    if "L" in names:
        out["L"] = column("L", f32)
    return out


def _stack(recordings):
    """``recordings`` in any of its three forms -> (states [R,T,6] f32, Q [R,T] f32, L [R,T] f32 or None, row spacing in seconds
    or None).  Recordings of unequal length are refused: one launch walks them with one (start, count)."""
    if isinstance(recordings, (str, os.PathLike)):
        recordings = [recordings]
    if isinstance(recordings, (tuple, list)) and len(recordings) == 2 and all(hasattr(x, "shape") for x in recordings):
        states, Q = (np.asarray(x, dtype=f32) for x in recordings)
        if states.ndim == 2:
            states, Q = states[None], Q[None]
        if Q.ndim == 3 and Q.shape[2] == 1:
            Q = Q[:, :, 0]
        if states.ndim != 3 or states.shape[2] != 6 or Q.shape != states.shape[:2]:
            raise ValueError(f"recordings as arrays must be states [R,T,6] and Q [R,T] of equal length, got {states.shape} and {Q.shape}")
        return np.ascontiguousarray(states), np.ascontiguousarray(Q), None, None
    cols = [load_recording(r) if isinstance(r, (str, os.PathLike)) else r for r in recordings]
    if not cols:
        raise ValueError("no recordings")
    lengths = [len(c["Q"]) for c in cols]
    if min(lengths) != max(lengths):
        raise ValueError(f"the recordings have unequal lengths ({min(lengths)} .. {max(lengths)} rows): test them in groups of one "
                         "length, or cut them to the shortest")
    states = np.stack([np.stack([np.asarray(c[name], dtype=f32) for name in FEATURES], axis=-1) for c in cols])
    Q = np.stack([np.asarray(c["Q"], dtype=f32) for c in cols])
    with_L = [c.get("L") is not None for c in cols]
    if any(with_L) and not all(with_L):
        raise ValueError("some recordings carry a pole length L and some do not")
    L = np.stack([np.asarray(c["L"], dtype=f32) for c in cols]) if all(with_L) else None
    t = cols[0].get("time")
    spacing = float(np.median(np.diff(np.asarray(t, dtype=np.float64)))) if t is not None and len(t) > 1 else None
    return states, Q, L, spacing


def _resolve(predictors, gru_model):
    """Every specification -> ("ODE_v0" | "ODE" | "GRU", the GRU's model dict or None), through the rules of the rest of the
    package (configs.ode_predictor_type, is_gru_specification, model_folder.load_gru_model); an unknown one is refused by name."""
    if isinstance(predictors, str):
        predictors = (predictors,)
    out = []
    for spec in predictors:
        folder = spec if isinstance(spec, str) and os.path.isdir(spec) else None
        if is_gru_specification(os.path.basename(os.path.normpath(spec)) if folder else spec):
            model = gru_model if gru_model is not None else folder
            if model is None:
                raise ValueError(f"predictor {spec!r} is the neural predictor and needs its weights: pass gru_model= (a model folder or "
                                 "the dict MPPIEngine.set_gru takes)")
            out.append((spec, "GRU", model))
        else:
            out.append((spec, ode_predictor_type(spec, f"predictor {spec!r}: the Brunton test runs ODE_v0, ODE and "
                                                       "GRU-6IN-32H1-32H2-5OUT* specifications"), None))
    return out


def brunton_test(recordings, predictors=("ODE",), horizon=50, start_idx=0, test_len="max", decimation=1, gru_model=None, phys=None,
                 math_mode="fast", return_predictions=False, device=0, *, dt=None, intermediate_steps=10):
    """The Brunton test of ``predictors`` (config_testing.yml: predictors_specifications_testing) on ``recordings``: paths of
    recording CSVs, a list of column dicts (``load_recording``), or arrays ``(states [R,T,6], Q [R,T])`` of equal length.
    ``horizon`` = test_max_horizon, ``start_idx`` = test_start_idx; ``test_len`` = how many start rows, "max": every start for which
    the whole horizon lies inside the recording.  ``decimation`` d keeps rows [::d] (sliced on the host before the upload) and the
    predictors' time step becomes d x the recordings' row spacing - ``dt``, default: the files' ``time`` column, 0.02 s for arrays.
    A GRU specification needs ``gru_model`` (a model folder or a weights dict); its memory is walked along each recording first.
    -> {specification: dict(mean_abs, rmse, max_abs [horizon,6] float64, n_starts, features, horizon_steps 1..horizon, and with
    ``return_predictions`` predictions [R,count,horizon+1,6] float32)}; the angle's error is wrapped into (-pi, pi]."""
    resolved = _resolve(predictors, gru_model)
    states, Q, L, spacing = _stack(recordings)
    d, horizon, start = int(decimation), int(horizon), int(start_idx)
    if d < 1 or horizon < 1 or start < 0:
        raise ValueError("decimation and horizon must be at least 1, start_idx at least 0")
    states, Q = np.ascontiguousarray(states[:, ::d]), np.ascontiguousarray(Q[:, ::d])
    L = None if L is None else np.ascontiguousarray(L[:, ::d])
    R, T = Q.shape
    room = T - start - horizon
    if room < 1:
        raise ValueError(f"horizon {horizon} from start_idx {start} does not fit into the {T} rows a recording has after decimation "
                         f"by {d}: no start row has its whole horizon inside the recording")
    count = room if test_len == "max" else int(test_len)
    if not 1 <= count <= room:
        raise ValueError(f"test_len {test_len!r}: between 1 and {room} start rows fit (or 'max')")
    step = float(d) * float(dt if dt is not None else (spacing if spacing is not None else 0.02))

    from .engine import MPPIEngine
    results, engines, uploaded = {}, {}, None
    for spec, kind, model in resolved:
        ptype = "ODE_v0" if kind == "GRU" else kind
        eng = engines.get(ptype)
        if eng is None:
            cfg = MPPIConfig(num_rollouts=1, mpc_horizon=horizon, mpc_timestep=step, intermediate_steps=int(intermediate_steps),
                             math_mode=math_mode, predictor_type=ptype)
            eng = engines[ptype] = MPPIEngine(1, cfg, phys or PhysicalParameters(), device=device)
        if uploaded is None:
            uploaded = eng.tensor(states), eng.tensor(Q), eng.tensor(L)
        s_dev, q_dev, l_dev = uploaded
        if kind == "GRU":
            if isinstance(model, (str, os.PathLike)):
                from .model_folder import load_gru_model
                model = load_gru_model(model)
            eng.set_gru(model)
            stats, pred = eng.brunton(s_dev, q_dev, horizon=horizon, start=start, count=count, predictor="GRU",
                                      h_rows=eng.gru_washout(s_dev, q_dev), return_predictions=return_predictions)
        else:
            stats, pred = eng.brunton(s_dev, q_dev, l_dev, horizon=horizon, start=start, count=count,
                                      return_predictions=return_predictions)
        st = stats.cpu().numpy()
        n = R * count
        res = dict(mean_abs=st[:, :, 0] / n, rmse=np.sqrt(st[:, :, 1] / n), max_abs=st[:, :, 2].copy(), n_starts=n,
                   features=FEATURES, horizon_steps=np.arange(1, horizon + 1), dt=step)
        if return_predictions:
            res["predictions"] = pred.cpu().numpy().reshape(R, count, horizon + 1, 6)
        results[spec] = res
    for eng in engines.values():
        eng.close()
    return results


def format_table(name, res, every=1):
    """One predictor's result as text: a row per horizon step with mean |e| and max |e| of every feature."""
    lines = [f"predictor {name}: {res['n_starts']} starts, dt {res['dt']:.6g} s", "step  " + "  ".join(
        f"{'mean|' + f + '|':>22} {'max':>10}" for f in res["features"])]
    for k in range(0, len(res["horizon_steps"]), every):
        lines.append(f"{int(res['horizon_steps'][k]):4d}  " + "  ".join(
            f"{res['mean_abs'][k, i]:22.6e} {res['max_abs'][k, i]:10.3e}" for i in range(len(res["features"]))))
    return "\n".join(lines)


def main(argv=None):
    """python -m cartpolesimulation_amd.brunton --config-root <CartPoleSimulation checkout> [--test-file ...] [--gru-model FOLDER]"""
    import argparse
    import yaml
    from .configs import load_reference_yaml
    ap = argparse.ArgumentParser(description="Brunton test on MI355X (reference: SI_Toolkit_ASF/Run/A3_Run_Brunton_Test.py)")
    ap.add_argument("--config-root", required=True,
                    help="a CartPoleSimulation checkout: SI_Toolkit_ASF/config_testing.yml (predictors, test file, horizon, start, length, "
                         "decimation), SI_Toolkit_ASF/config_predictors.yml (intermediate_steps) and cartpole_physical_parameters.yml")
    ap.add_argument("--config-testing", default=None, metavar="FILE", help="a config_testing.yml elsewhere than in the checkout")
    ap.add_argument("--test-file", default=None, nargs="+", metavar="CSV",
                    help="recording(s) or a folder of them (e.g. .../Recordings/Test/) instead of path_to_testfile + test_file")
    ap.add_argument("--gru-model", default=None, metavar="FOLDER", help="the GRU-6IN-32H1-32H2-5OUT-* model folder of a neural specification")
    ap.add_argument("--math-mode", default="fast", choices=["fast", "precise"])
    ap.add_argument("--every", type=int, default=1, help="print every n-th horizon step")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    root = args.config_root
    with open(args.config_testing or os.path.join(root, "SI_Toolkit_ASF", "config_testing.yml")) as fh:
        ct = yaml.safe_load(fh)
    phys, cfgs = load_reference_yaml(root)
    if args.test_file:
        files = []
        for p in args.test_file:
            files += sorted(os.path.join(p, n) for n in os.listdir(p) if n.endswith(".csv")) if os.path.isdir(p) else [p]
    else:
        names = ct["test_file"] if isinstance(ct["test_file"], (list, tuple)) else [ct["test_file"]]
        files = [os.path.join(root, ct.get("path_to_testfile", "."), n) for n in names]
    specs = ct["predictors_specifications_testing"]
    entries = cfgs["predictors"]["predictors"]
    steps = {int((entries.get(str(s).split(":")[0]) or entries.get(str(s).split(":")[0] + "_default") or {}).get("intermediate_steps", 10))
             for s in specs if not is_gru_specification(s)} or {10}
    if len(steps) > 1:
        raise ValueError(f"the predictors tested together must share intermediate_steps, config_predictors.yml gives {sorted(steps)}")
    res = brunton_test(files, specs, horizon=ct.get("test_max_horizon", 50), start_idx=ct.get("test_start_idx", 0),
                       test_len=ct.get("test_len", "max"), decimation=ct.get("decimation", 1), gru_model=args.gru_model, phys=phys,
                       math_mode=args.math_mode, device=args.device, intermediate_steps=steps.pop())
    for name, r in res.items():
        print(format_table(name, r, max(1, args.every)))
    return res


if __name__ == "__main__":
    main()
