"""Fitting the ODE predictor's physical parameters to recordings, on the device (reference:
SI_Toolkit_ASF/ToolkitCustomization/Modules/ODE_module.py - predictor_ODE wrapped as the Keras "fake network"
``Custom-ODE_module-ODEModel`` of SI_Toolkit_ASF/config_training.yml, whose weights are the cartpole's physical parameters and which
saves a plain ``{name: value}`` YAML of them).

The reference trains that module with SI_Toolkit under TensorFlow; SI_Toolkit is a submodule that the reference checkout does not
carry, so what is in the tree is the module, the configuration file and the YAML format.  The training semantics here - windows,
loss, parametrisation, learning-rate schedule - are therefore THIS PACKAGE'S OWN, as in ``train_gru``:

* a window is a start row of one recording and the ``horizon`` (POST_WASH_OUT_LEN) rows after it: the ODE predictor is rolled
  forward from the recorded start state on the recorded controls and every step is scored against the recorded row - the
  open-loop error the Brunton test measures.  The ODE has no memory: WASH_OUT_LEN must be 0;
* the loss is the mean squared error of angleD, angle_cos, angle_sin, position, positionD, each times ``feature_scale`` - by
  default the min-max scale of ``train_gru.normalization_from_recordings`` (the angle itself is not scored);
* a parameter is p = base * exp(theta) with theta = 0 at the start, base = the engine's own value: the parameters span five decades
  (J_fric is 5e-5, g is 9.81), must stay positive, and one learning rate has to serve them all.  Adam runs on theta;
* batches, seed and ``LR.REDUCE_LR_ON_PLATEAU`` are ``train_gru``'s.

The loss, its gradient (forward mode: the tangents of the state with respect to each trained parameter travel with the rollout)
and Adam run on the device (``MPPIEngine.ode_fit_step``: cpmppi_ode_fit_step); the host draws batches and keeps the schedule.
Trainable: k, m_cart, m_pole, g, J_fric, M_fric, u_max, L (the reference ships ``trainable_params = ['u_max']``).  TrackHalfLength is
not: only the bounce test reads it.  The engine's own physics is never changed; the fitted ``PhysicalParameters`` go into a new
engine.

Not built, and refused by name where a user can ask: several models per launch, a pole mass per row, env groups and multi-GPU, the
regularisation / pruning / quantisation / series-modification / filter keys of config_training.yml, the GP and Dense predictors.

  python -m cartpolesimulation_amd.fit_ode --recordings DIR --out params.yaml --config-root CHECKOUT [--predictor ODE|ODE_v0]
                                           [--trainable u_max,M_fric,J_fric] [--horizon P] [--validation DIR]
"""
import dataclasses
import os

import numpy as np

from ._lib import ODE_FIT_NAMES
from .configs import PhysicalParameters
from ._training import (check_recordings, load_recordings_folder, make_windows, plateau_rule,  # noqa: F401  (and re-exported)
                        refuse_unbuilt_sections, run_epochs, schedule_settings)
from .train_gru import normalization_from_recordings

f32 = np.float32
NET_NAME = "Custom-ODE_module-ODEModel"
# the weights of the reference's ODE_module, in its order: what the parameter YAML holds
PARAMETER_NAMES = ("J_fric", "L", "m_cart", "M_fric", "TrackHalfLength", "g", "k", "m_pole", "u_max")


def fitted_parameters(base, p):
    """``base`` (a PhysicalParameters) with the eight values ``p`` in the order of ``ODE_FIT_NAMES`` in place of its own."""
    return dataclasses.replace(base, **{name: float(f32(v)) for name, v in zip(ODE_FIT_NAMES, p)})


def fit_ode(engine, states, Q, lengths=None, *, trainable=("u_max",), horizon, epochs, batch_size, lr, seed, validation=None,
            feature_scale=None, L=None, reduce_lr_on_plateau=True, patience=2, decrease_factor=0.5, minimal_lr=1e-7, min_delta=1e-6,
            beta1=0.9, beta2=0.999, eps=1e-7, validation_batch=4096, log=None):
    """Fit the ``trainable`` physical parameters of ``engine``'s ODE predictor (an ``MPPIEngine``; its predictor type, math mode,
    time step and own parameters are the model and the start) to ``states`` [R,T,6], ``Q`` [R,T] (``lengths`` [R]: the recordings'
    true lengths, None = T).  ``horizon`` control steps per window, at most the engine's mpc_horizon.  ``feature_scale`` [5]: None =
    the min-max scale of the training recordings.  ``L`` [R,T]: a pole length per start row (then L is not trainable).
    ``validation`` = (states, Q, lengths or None) is scored after every epoch through the loss-only call.  The module docstring
    states windows, loss, parametrisation and schedule.
    -> (the engine's PhysicalParameters with the fitted values; history = dict(loss, val_loss, lr: one entry per epoch, batch_loss:
    every step's loss in order, theta, parameters: the final values by name))."""
    states, Q, lengths, epochs, batch_size = check_recordings(states, Q, lengths, epochs, batch_size)
    horizon, mask = int(horizon), engine.ode_fit_mask(trainable)
    windows = make_windows(lengths, 0, horizon, 1)
    if len(windows) == 0:
        raise ValueError(f"no recording holds a window of a start row and {horizon} rows after it")
    if feature_scale is None:
        feature_scale = normalization_from_recordings(states, Q, lengths)["in_scale"][1:]
    scale = np.asarray(feature_scale, f32).reshape(-1)
    s_dev, q_dev = engine.tensor(states), engine.tensor(Q)
    l_dev = engine.tensor(L, Q.shape) if L is not None else None
    loss_of = vw = None
    if validation is not None:
        vs, vq = np.ascontiguousarray(validation[0], f32), np.ascontiguousarray(validation[1], f32)
        vl = validation[2] if len(validation) > 2 and validation[2] is not None else np.full(vq.shape[0], vq.shape[1])
        vw = make_windows(vl, 0, horizon, 1)
        if len(vw) == 0:
            raise ValueError("the validation recordings hold no window")
        if L is not None:
            raise ValueError("validation with L rows is not built: validate with the pole length as a parameter")
        vs, vq = engine.tensor(vs), engine.tensor(vq)
        loss_of = lambda w: engine.ode_fit_loss_grad(vs, vq, w, horizon, mask, scale, grad=False)[0]  # noqa: E731
    engine.ode_fit_begin()

    def step(batch, rate, loss_out, _):
        engine.ode_fit_step(s_dev, q_dev, batch, horizon, mask, scale, l_dev, lr=rate, beta1=beta1, beta2=beta2, eps=eps,
                            loss_out=loss_out)

    history, _ = run_epochs(
        engine.device, lambda epoch: (windows, None), step, loss_of, vw, epochs=epochs, batch_size=batch_size, seed=seed, lr=lr, log=log,
        plateau=(reduce_lr_on_plateau, patience, decrease_factor, minimal_lr, min_delta), validation_batch=validation_batch)
    p, theta = engine.ode_fit_get()
    history["theta"] = {n: float(v) for n, v in zip(ODE_FIT_NAMES, theta)}
    history["parameters"] = {n: float(v) for n, v in zip(ODE_FIT_NAMES, p)}
    return fitted_parameters(engine.phys, p), history


def write_parameters(path, phys):
    """The plain ``{name: value}`` YAML of the nine physical parameters, as the reference's ODE_module saves its weights; a float32
    is written with the digits that read back exactly.  -> the path."""
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        for name in PARAMETER_NAMES:
            fh.write(f"{name}: {float(getattr(phys, name))!r}\n")
    return path


def read_parameters(path, base=None):
    """A parameter YAML of ``write_parameters`` (or of the reference's ODE_module) -> ``base`` (None: the defaults) with the file's
    values; the nine names must all be there, a name it does not know is refused."""
    import yaml
    with open(path) as fh:
        data = yaml.safe_load(fh)
    if not isinstance(data, dict):
        raise ValueError(f"{path}: not a {{name: value}} YAML of physical parameters")
    unknown, missing = sorted(set(data) - set(PARAMETER_NAMES)), [n for n in PARAMETER_NAMES if n not in data]
    if unknown or missing:
        raise ValueError(f"{path}: the physical parameters are {', '.join(PARAMETER_NAMES)}"
                         + (f"; unknown: {unknown}" if unknown else "") + (f"; missing: {missing}" if missing else ""))
    try:
        values = {n: float(np.asarray(data[n], np.float64).reshape(-1)[0]) for n in PARAMETER_NAMES}
    except (TypeError, ValueError) as e:
        raise ValueError(f"{path}: {e}") from None
    return dataclasses.replace(base or PhysicalParameters(), **values)


# ---------------------------------------------------------------------------------------------------------------- command line
def fit_settings(config, net=None, feature_scale=None, **overrides):
    """config_training.yml as a dict -> the keyword arguments of ``fit_ode``: EPOCHS, BATCH_SIZE, SEED, LR.*, and POST_WASH_OUT_LEN
    as the ``horizon`` (``overrides``: the same by ``fit_ode``'s names, None = the file's).  Refused by name: a net other than
    Custom-ODE_module-ODEModel (``net`` overrides modeling.NET_NAME, which names a Dense imitator in the shipped file); a non-zero
    WASH_OUT_LEN (the ODE has no memory to wash out); NORMALIZE off without an explicit ``feature_scale`` (the loss's scale would be
    undefined); and the sections ``train_gru.training_settings`` refuses."""
    t = dict(config.get("training_default") or {})
    net = net or (config.get("modeling") or {}).get("NET_NAME") or NET_NAME
    if net != NET_NAME:
        raise ValueError(f"net {net!r}: fit_ode fits {NET_NAME} (the ODE predictor's physical parameters) alone; pass --net {NET_NAME}, "
                         "or train a network with train_gru")
    if int(t.get("WASH_OUT_LEN", 0) or 0) != 0:
        raise ValueError(f"training_default.WASH_OUT_LEN = {t['WASH_OUT_LEN']}: the ODE predictor has no memory to wash out; set it to 0")
    if not bool(t.get("NORMALIZE", True)) and feature_scale is None:
        raise ValueError("training_default.NORMALIZE is off and no feature_scale is given: the loss weighs the five features by the "
                         "min-max scale of the recordings (NORMALIZE) or by an explicit --feature-scale")
    refuse_unbuilt_sections(config)
    out = dict(schedule_settings(config), horizon=t.get("POST_WASH_OUT_LEN", 1), feature_scale=feature_scale)
    out.update({k: v for k, v in overrides.items() if v is not None})
    if int(out["horizon"]) < 1:
        raise ValueError(f"horizon (POST_WASH_OUT_LEN) must be at least 1, got {out['horizon']}")
    return out


def horizon_rmse(recordings, predictor, horizon, phys, dt=0.02, intermediate_steps=10, math_mode="fast", device=0):
    """The Brunton test's rmse of angleD, angle_cos, angle_sin, position, positionD at step ``horizon`` with the parameters ``phys``."""
    from .brunton import brunton_test
    res = brunton_test(recordings, (predictor,), horizon=horizon, phys=phys, math_mode=math_mode, device=device, dt=dt,
                       intermediate_steps=intermediate_steps)[predictor]
    return res["rmse"][-1, 1:]


def main(argv=None):
    """python -m cartpolesimulation_amd.fit_ode --recordings DIR --out params.yaml --config-root CHECKOUT [--predictor ODE|ODE_v0]
    [--trainable u_max,M_fric,J_fric] [--horizon P] [--validation DIR]"""
    import argparse
    import yaml
    from .configs import MPPIConfig, load_reference_yaml
    from .engine import MPPIEngine
    ap = argparse.ArgumentParser(description="Fit the ODE predictor's physical parameters to recordings, on MI355X "
                                             "(reference: SI_Toolkit_ASF/ToolkitCustomization/Modules/ODE_module.py, config_training.yml)")
    ap.add_argument("--recordings", required=True, metavar="DIR", help="a folder of recording CSVs (recording / generate_dataset write them)")
    ap.add_argument("--validation", default=None, metavar="DIR", help="a folder of recordings scored after every epoch")
    ap.add_argument("--out", required=True, metavar="FILE", help="the {name: value} YAML of the fitted physical parameters")
    ap.add_argument("--config-root", required=True, metavar="CHECKOUT",
                    help="a CartPoleSimulation checkout: cartpole_physical_parameters.yml (the start) and SI_Toolkit_ASF/config_training.yml "
                         "(EPOCHS, BATCH_SIZE, SEED, LR.*, POST_WASH_OUT_LEN = the horizon)")
    ap.add_argument("--config-training", default=None, metavar="FILE", help="a config_training.yml elsewhere than in the checkout")
    ap.add_argument("--net", default=NET_NAME, help=f"{NET_NAME} is what this command fits (instead of the file's NET_NAME)")
    ap.add_argument("--predictor", default="ODE", choices=["ODE", "ODE_v0"])
    ap.add_argument("--trainable", default="u_max", metavar="NAME,NAME,...", help=f"out of {', '.join(ODE_FIT_NAMES)}")
    ap.add_argument("--horizon", type=int, default=None, metavar="P", help="control steps per window instead of POST_WASH_OUT_LEN")
    ap.add_argument("--feature-scale", default=None, metavar="A,B,C,D,E",
                    help="the loss's weights of angleD, angle_cos, angle_sin, position, positionD instead of the recordings' min-max scale")
    for flag, typ in (("--epochs", int), ("--batch-size", int), ("--seed", int), ("--lr", float)):
        ap.add_argument(flag, type=typ, default=None, help="instead of the file's value")
    ap.add_argument("--dt", type=float, default=0.02, help="the recordings' row spacing in seconds")
    ap.add_argument("--intermediate-steps", type=int, default=10)
    ap.add_argument("--math-mode", default="fast", choices=["fast", "precise"])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    with open(args.config_training or os.path.join(args.config_root, "SI_Toolkit_ASF", "config_training.yml")) as fh:
        config = yaml.safe_load(fh) or {}
    try:
        scale = None if args.feature_scale is None else [float(x) for x in args.feature_scale.split(",")]
        settings = fit_settings(config, net=args.net, feature_scale=scale, epochs=args.epochs, batch_size=args.batch_size,
                                seed=args.seed, lr=args.lr, horizon=args.horizon)
        trainable = tuple(x.strip() for x in args.trainable.split(",") if x.strip())
        MPPIEngine.ode_fit_mask(trainable)
    except ValueError as e:
        raise SystemExit(f"fit_ode: {e}")
    phys = load_reference_yaml(args.config_root)[0]
    states, Q, lengths, names = load_recordings_folder(args.recordings)
    validation = load_recordings_folder(args.validation)[:3] if args.validation else None
    horizon = int(settings["horizon"])
    cfg = MPPIConfig(num_rollouts=1, mpc_horizon=horizon, mpc_timestep=args.dt, intermediate_steps=args.intermediate_steps,
                     math_mode=args.math_mode, predictor_type=args.predictor)
    engine = MPPIEngine(1, cfg, phys, device=args.device)
    fitted, history = fit_ode(engine, states, Q, lengths, trainable=trainable, validation=validation, log=print, **settings)
    engine.close()
    out = write_parameters(args.out, fitted)
    for name in trainable:
        print(f"{name}: {getattr(phys, name):.6g} -> {getattr(fitted, name):.6g}")
    if lengths.min() == lengths.max():                  # (the Brunton test walks recordings of one length)
        kw = dict(dt=args.dt, intermediate_steps=args.intermediate_steps, math_mode=args.math_mode, device=args.device)
        before = horizon_rmse((states, Q), args.predictor, horizon, phys, **kw)
        after = horizon_rmse((states, Q), args.predictor, horizon, fitted, **kw)
        print(f"Brunton rmse at step {horizon} (angleD, angle_cos, angle_sin, position, positionD)")
        print("  before: " + "  ".join(f"{x:.4e}" for x in before))
        print("  after:  " + "  ".join(f"{x:.4e}" for x in after))
    else:
        print("Brunton rmse not printed: the recordings have unequal lengths")
    print(f"fitted on {len(names)} recordings, final loss {history['loss'][-1]:.6e}; parameters: {out}")
    return fitted, history


if __name__ == "__main__":
    main()
