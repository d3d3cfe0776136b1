"""Training the GRU predictor on recordings, on the device (reference: SI_Toolkit_ASF/Run/A2_Train_Network.py with
SI_Toolkit_ASF/config_training.yml).

The reference trains its networks with SI_Toolkit under TensorFlow; SI_Toolkit is a submodule that the reference checkout does not
carry, so what is in the tree is the configuration file and the model-folder format.  The semantics here - windows, normalisation,
loss, learning-rate schedule - are therefore THIS PACKAGE'S OWN, chosen to match what the configuration keys say:

* a window is ``WASH_OUT_LEN + POST_WASH_OUT_LEN`` consecutive rows of one recording, fed as recorded from a zero memory; the first
  ``WASH_OUT_LEN`` rows only build the memory, the others are scored against the features ``SHIFT_LABELS`` rows on (mean squared error
  of the normalised values);
* normalisation is min-max to [-1, 1] per feature over the training recordings;
* a batch is ``BATCH_SIZE`` windows drawn without replacement from a permutation of ``numpy.random.default_rng(SEED)`` per epoch;
* Adam; ``LR.REDUCE_LR_ON_PLATEAU`` multiplies the rate by ``DECREASE_FACTOR`` (not below ``MINIMAL``) after ``PATIENCE`` epochs
  without an improvement of more than ``MIN_DELTA`` of the validation loss (the training loss without validation data).

The loss, its gradient (back-propagation through time), Adam and the rebuild of the kernels' weight images run on the device
(``MPPIEngine.gru_train_step``: cpmppi_gru_train_step); the host draws batches and keeps the schedule.

Two training modes.  Teacher forced (the default): every row of a window is fed as recorded, the one-step map is fitted.  Open-loop
rollout (``rollout=True``, ``--rollout``: cpmppi_gru_rollout_train_step): the wash-out and the first scored row are fed as recorded,
every later row takes the model's own normalised outputs of the row before with the recorded control - the free run that
``gru_predict``, the Brunton test and the controllers put a trained model through -, and the gradient runs through that feedback;
``SHIFT_LABELS`` must be 1.  ``post_wash_out`` may then be a sequence, one horizon per epoch, the last entry repeating (the usual
horizon curriculum, ``--post-wash-out-schedule 5,10,20``); validation always scores the last entry.  The expected use is to
fine-tune a teacher-forced model: ``--init FOLDER`` starts from a model folder and keeps its normalisation.

Built for GRU-6IN-32H1-32H2-5OUT, the dynamics model (Q and five state features in, the five features of the next row out).  Not
built, and refused by name where a user can ask: other network sizes or cell types, Dense nets, gradient-norm clipping, scheduled
sampling (fed-back and recorded rows mixed at random), a non-zero start memory, the regularisation / pruning / quantisation /
series-modification / filter keys of config_training.yml, several models per launch, env groups and multi-GPU.

  python -m cartpolesimulation_amd.train_gru --recordings DIR --out FOLDER --net GRU-32H1-32H2 --dynamics-model [--config-root CHECKOUT]
                                             [--rollout] [--post-wash-out-schedule 5,10,20] [--init FOLDER]
"""
import os

import numpy as np

from ._training import (check_recordings, load_recordings_folder, make_windows, plateau_rule,  # noqa: F401  (and re-exported)
                        refuse_unbuilt_sections, run_epochs, schedule_settings)
from .model_folder import GRU_KEYS, GRU_SHAPES, KERNEL_INPUTS, KERNEL_OUTPUTS

f32 = np.float32
NET_NAME = "GRU-32H1-32H2"
NORM_KEYS = ("in_scale", "in_shift", "out_scale", "out_shift")
# column of states [.., 6] = (angle, angleD, angle_cos, angle_sin, position, positionD) of every output feature
_STATE_COLUMNS = (1, 2, 3, 4, 5)


def normalization_from_recordings(states, Q, lengths=None):
    """Min-max normalisation to [-1, 1] per feature over ``states`` [R,T,6], ``Q`` [R,T] (rows at or past ``lengths[r]`` do not
    count): normalised = a x + b with a = 2 / (max - min), b = -(max + min) / (max - min); de-normalisation is the inverse,
    x = A y + B with A = (max - min) / 2, B = (max + min) / 2.  SI_Toolkit is not in the reference checkout: these semantics are
    the package's own.  -> dict(in_scale, in_shift [6] in the order of ``model_folder.KERNEL_INPUTS``, out_scale, out_shift [5] in the
    order of ``KERNEL_OUTPUTS``), float32.  A feature that never varies is refused by name."""
    states, Q = np.asarray(states, np.float64), np.asarray(Q, np.float64)
    if states.ndim != 3 or states.shape[2] != 6 or Q.shape != states.shape[:2]:
        raise ValueError(f"states must be [R,T,6] and Q [R,T], got {states.shape} and {Q.shape}")
    R, T = Q.shape
    lengths = np.full(R, T) if lengths is None else np.asarray(lengths).reshape(-1)
    keep = np.arange(T)[None, :] < lengths[:, None]
    if not keep.any():
        raise ValueError("no rows")
    cols = [Q[keep]] + [states[:, :, c][keep] for c in _STATE_COLUMNS]
    lo, hi = np.array([c.min() for c in cols]), np.array([c.max() for c in cols])
    flat = [KERNEL_INPUTS[i] for i in range(6) if not hi[i] > lo[i]]
    if flat:
        raise ValueError(f"feature(s) {flat} never vary over the recordings: min-max normalisation is undefined")
    a, b = 2.0 / (hi - lo), -(hi + lo) / (hi - lo)
    A, B = (hi - lo) / 2.0, (hi + lo) / 2.0
    return dict(in_scale=a.astype(f32), in_shift=b.astype(f32), out_scale=A[1:].astype(f32), out_shift=B[1:].astype(f32))


def initial_weights(seed):
    """A fresh GRU-6IN-32H1-32H2-5OUT: every weight uniform in +-1/sqrt(32) (the torch.nn.GRU rule) from
    ``numpy.random.default_rng(seed)``, in the order of ``GRU_KEYS``."""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(32.0)
    return {key: rng.uniform(-k, k, size=shp).astype(f32) for key, shp in zip(GRU_KEYS, GRU_SHAPES)}


def horizon_schedule(post_wash_out):
    """``post_wash_out`` as train_gru takes it - one P, a sequence with one P per epoch, or the command line's "5,10,20" - -> the
    tuple of P per epoch; the last entry repeats (``horizon_of_epoch``)."""
    if isinstance(post_wash_out, str):
        parts = [x.strip() for x in post_wash_out.split(",")]
        if not all(x.isdigit() for x in parts):
            raise ValueError(f"post_wash_out schedule {post_wash_out!r}: comma-separated whole numbers, e.g. 5,10,20")
        post_wash_out = [int(x) for x in parts]
    sched = tuple(int(p) for p in np.atleast_1d(np.asarray(post_wash_out)).reshape(-1))
    if not sched or min(sched) < 1:
        raise ValueError(f"post_wash_out must be at least 1 in every epoch, got {sched}")
    return sched


def horizon_of_epoch(schedule, epoch):
    """The P of ``epoch`` (from 0): the schedule's entry, its last one beyond the end."""
    return schedule[min(int(epoch), len(schedule) - 1)]


def _check_model(model):
    for key, shp in zip(GRU_KEYS, GRU_SHAPES):
        if key not in model or np.shape(model[key]) != shp:
            raise ValueError(f"model: weight {key} must have shape {shp} (GRU-6IN-32H1-32H2-5OUT is the network built)")


def train_gru(engine, states, Q, lengths=None, *, epochs, batch_size, lr, seed, wash_out, post_wash_out, shift_labels=1,
              validation=None, init=None, reduce_lr_on_plateau=True, patience=2, decrease_factor=0.5, minimal_lr=1e-7,
              min_delta=1e-6, beta1=0.9, beta2=0.999, eps=1e-7, validation_batch=4096, log=None, rollout=False):
    """Train GRU-6IN-32H1-32H2-5OUT on ``states`` [R,T,6], ``Q`` [R,T] (``lengths`` [R]: the recordings' true lengths, None = T)
    with ``engine`` (an ``MPPIEngine``; its model is replaced).  ``init``: the model dict to start from - weights in the order of
    ``GRU_KEYS``, and the normalisation if it carries one; None: ``initial_weights(seed)``.  Without a normalisation in ``init`` it
    is ``normalization_from_recordings`` of the training data.  ``validation`` = (states, Q, lengths or None) is scored after every
    epoch through the loss-only call.  ``eps`` defaults to Keras's Adam epsilon.  The module docstring states batches and schedule.
    ``rollout``: every training step and the validation loss run through the open-loop rollout (``shift_labels`` must be 1).
    ``post_wash_out``: one P, or a sequence with one P per epoch whose last entry repeats; the windows are remade when P changes, the
    workspace is reserved once for the largest P, validation always scores the last entry.
    -> (the model dict ``MPPIEngine.set_gru`` takes, which the engine holds on return; history = dict(loss, val_loss, lr,
    post_wash_out: one entry per epoch, batch_loss: every step's loss in order))."""
    rollout = bool(rollout)
    if rollout and int(shift_labels) != 1:
        raise ValueError(f"rollout: shift_labels must be 1 (the output of a row is the input of the next), got {shift_labels}")
    schedule = horizon_schedule(post_wash_out)
    states, Q, lengths, epochs, batch_size = check_recordings(states, Q, lengths, epochs, batch_size)
    by_horizon = {p: make_windows(lengths, wash_out, p, shift_labels) for p in sorted(set(schedule[:epochs]))}
    for p, w in by_horizon.items():
        if len(w) == 0:
            raise ValueError(f"no recording holds a window of {wash_out} + {p} rows with its labels {shift_labels} rows on")
    model = dict(init) if init is not None else initial_weights(seed)
    _check_model(model)
    norm = {k: np.asarray(model[k], f32) for k in NORM_KEYS if model.get(k) is not None}
    if len(norm) != 4:
        norm = normalization_from_recordings(states, Q, lengths)
    model = {**{k: np.asarray(model[k], f32) for k in GRU_KEYS}, **norm}
    engine.set_gru(model)
    engine.gru_train_begin()
    s_dev, q_dev = engine.tensor(states), engine.tensor(Q)
    loss_of = vw = None
    if validation is not None:
        vs, vq = np.ascontiguousarray(validation[0], f32), np.ascontiguousarray(validation[1], f32)
        vl = validation[2] if len(validation) > 2 and validation[2] is not None else np.full(vq.shape[0], vq.shape[1])
        vw = make_windows(vl, wash_out, schedule[-1], shift_labels)
        if len(vw) == 0:
            raise ValueError("the validation recordings hold no window")
        vs, vq = engine.tensor(vs), engine.tensor(vq)
        loss_of = lambda w: engine.gru_loss_grad(vs, vq, w, wash_out, schedule[-1], shift_labels, grad=False,  # noqa: E731
                                                 rollout=rollout)[0]
    if len(schedule) > 1:
        widest = max(batch_size, min(int(validation_batch), len(vw)) if vw is not None else 0)
        engine.gru_train_reserve(widest, int(wash_out) + max(schedule))

    def step(batch, rate, loss_out, horizon):
        engine.gru_train_step(s_dev, q_dev, batch, wash_out, horizon, shift_labels, lr=rate, beta1=beta1, beta2=beta2, eps=eps,
                              loss_out=loss_out, rollout=rollout)

    per_epoch = [(by_horizon[p], p) for p in (horizon_of_epoch(schedule, epoch) for epoch in range(epochs))]
    history, horizons = run_epochs(
        engine.device, per_epoch.__getitem__, step, loss_of, vw, epochs=epochs, batch_size=batch_size, seed=seed, lr=lr, log=log,
        plateau=(reduce_lr_on_plateau, patience, decrease_factor, minimal_lr, min_delta), validation_batch=validation_batch)
    history["post_wash_out"] = horizons
    trained = {**engine.gru_train_get(), **norm}
    engine.set_gru(trained)            # (the rollout kernels' split-f16 image is built, and range-checked, on the host)
    return trained, history


def write_model_folder(folder, model, name=None, info=None):
    """A model folder in the format ``model_folder.load_gru_model`` reads, for which it returns the arrays of ``model``: the net-info
    file ``<name>.txt`` (``name`` None: the folder's own name), the four normalisation CSVs (identity where ``model`` has none) and
    ``weights.npz`` with the weights in the order of ``GRU_KEYS``, features in the kernel's order.  ``info``: further
    ``KEY: value`` entries of the net-info file.  -> the folder."""
    _check_model(model)
    folder = os.path.abspath(os.fspath(folder))
    name = name or os.path.basename(folder.rstrip(os.sep))
    os.makedirs(folder, exist_ok=True)
    normalize = all(model.get(k) is not None for k in NORM_KEYS)
    entries = {"LIBRARY": "cartpolesimulation_amd", "NET NAME": NET_NAME, "NET FULL NAME": name,
               "INPUTS": ", ".join(KERNEL_INPUTS), "OUTPUTS": ", ".join(KERNEL_OUTPUTS), "TYPE": "GRU",
               "NORMALIZE": str(normalize), "PARENT NET": "Network trained from scratch"}
    entries.update({str(k).upper(): str(v) for k, v in (info or {}).items()})
    with open(os.path.join(folder, name + ".txt"), "w") as fh:
        for key, value in entries.items():
            fh.write(f"{key}:\n{value}\n\n")
    vectors = (("normalization_vec_a.csv", "in_scale", 6, 1.0), ("normalization_vec_b.csv", "in_shift", 6, 0.0),
               ("denormalization_vec_A.csv", "out_scale", 5, 1.0), ("denormalization_vec_B.csv", "out_shift", 5, 0.0))
    for fname, key, n, fill in vectors:
        v = np.asarray(model[key], f32).reshape(-1) if normalize else np.full(n, fill, f32)
        if v.shape != (n,):
            raise ValueError(f"model: {key} must have {n} entries")
        with open(os.path.join(folder, fname), "w") as fh:      # (repr of the float32's double: read back exactly)
            fh.write(",".join(repr(float(x)) for x in v) + "\n")
    np.savez(os.path.join(folder, "weights.npz"), **{k: np.asarray(model[k], f32) for k in GRU_KEYS})
    return folder


# ---------------------------------------------------------------------------------------------------------------- command line
_DYNAMICS = dict(control_inputs=["Q"], state_inputs=list(KERNEL_INPUTS[1:]), outputs=list(KERNEL_OUTPUTS))


def training_settings(config, net=None, dynamics_model=False, **overrides):
    """config_training.yml as a dict -> the keyword arguments of ``train_gru`` (EPOCHS, BATCH_SIZE, SEED, LR.*, WASH_OUT_LEN,
    POST_WASH_OUT_LEN, SHIFT_LABELS; ``overrides``: the same by ``train_gru``'s names, None = the file's) and ``normalize``.  What the
    trainer is not built for is refused by name: a net other than GRU-32H1-32H2 (``net`` overrides modeling.NET_NAME, which names a
    Dense imitator in the shipped file), features other than the dynamics model's (``dynamics_model``: take those instead of the
    file's), and the activated regularisation, pruning, quantisation, series-modification, filter and on-the-fly keys."""
    t = dict(config.get("training_default") or {})
    net = net or (config.get("modeling") or {}).get("NET_NAME")
    if net != NET_NAME:
        raise ValueError(f"net {net!r}: the trainer is built for {NET_NAME} (GRU-6IN-32H1-32H2-5OUT) alone - no Dense nets, no other "
                         f"sizes or cell types; pass --net {NET_NAME}")
    feats = _DYNAMICS if dynamics_model else {k: list(t.get(k) or []) for k in _DYNAMICS}
    if (sorted(feats["control_inputs"]) != ["Q"] or sorted(feats["state_inputs"]) != sorted(KERNEL_INPUTS[1:])
            or sorted(feats["outputs"]) != sorted(KERNEL_OUTPUTS)):
        raise ValueError(f"features {feats['control_inputs']} + {feats['state_inputs']} -> {feats['outputs']}: the trainer is built for "
                         f"the dynamics model {list(KERNEL_INPUTS)} -> {list(KERNEL_OUTPUTS)}; pass --dynamics-model")
    for key in ("setpoint_inputs", "translation_invariant_variables"):
        if t.get(key):
            raise ValueError(f"training_default.{key} = {t[key]}: not built (the dynamics model has none)")
    refuse_unbuilt_sections(config)
    out = dict(schedule_settings(config), wash_out=t.get("WASH_OUT_LEN", 0), post_wash_out=t.get("POST_WASH_OUT_LEN", 1),
               shift_labels=t.get("SHIFT_LABELS", 1))
    out.update({k: v for k, v in overrides.items() if v is not None})
    if int(out["shift_labels"]) == 0:
        raise ValueError("SHIFT_LABELS 0 with the dynamics model's features trains the identity map (the shipped value belongs to the "
                         "imitator's outputs): pass --shift-labels 1")
    return out, bool(t.get("NORMALIZE", True))


def run_settings(settings, normalize, rollout=False, schedule=None, init_folder=None):
    """What the command line adds to ``training_settings``: -> (the keyword arguments of ``train_gru`` with ``rollout`` and, from
    ``schedule`` ("5,10,20"), ``post_wash_out`` as a sequence; the model to start from - the one of ``init_folder`` with its
    normalisation, else ``initial_weights(seed)``, with the identity normalisation unless ``normalize``; the entries of the
    net-info file)."""
    settings = dict(settings, rollout=bool(rollout))
    if schedule is not None:
        settings["post_wash_out"] = horizon_schedule(schedule)
    sched = horizon_schedule(settings["post_wash_out"])
    if rollout and int(settings["shift_labels"]) != 1:
        raise ValueError(f"--rollout: shift_labels must be 1 (the output of a row is the input of the next), got "
                         f"{settings['shift_labels']}")
    if init_folder is not None:
        from .model_folder import load_gru_model
        init = dict(load_gru_model(os.fspath(init_folder)))
        _check_model(init)
        if any(init.get(k) is None for k in NORM_KEYS):       # (a folder with NORMALIZE False: the identity, not the recordings')
            init.update(in_scale=np.ones(6, f32), in_shift=np.zeros(6, f32), out_scale=np.ones(5, f32), out_shift=np.zeros(5, f32))
    else:
        init = initial_weights(settings["seed"])
        if not normalize:
            init.update(in_scale=np.ones(6, f32), in_shift=np.zeros(6, f32), out_scale=np.ones(5, f32), out_shift=np.zeros(5, f32))
    info = {"WASH OUT LENGTH": settings["wash_out"], "POST WASH OUT LENGTH": sched[-1],
            "POST WASH OUT SCHEDULE": ", ".join(str(p) for p in sched), "SHIFT LABELS": settings["shift_labels"],
            "TRAINING MODE": "open-loop rollout" if rollout else "teacher forced"}
    if init_folder is not None:
        info["PARENT NET"] = os.path.abspath(os.fspath(init_folder))
    return settings, init, info


def main(argv=None):
    """python -m cartpolesimulation_amd.train_gru --recordings DIR --out FOLDER --net GRU-32H1-32H2 --dynamics-model [--config-root CHECKOUT]
    [--rollout] [--post-wash-out-schedule 5,10,20] [--init FOLDER]"""
    import argparse
    import yaml
    ap = argparse.ArgumentParser(description="Train the GRU predictor on recordings, on MI355X "
                                             "(reference: SI_Toolkit_ASF/Run/A2_Train_Network.py, config_training.yml)")
    ap.add_argument("--recordings", required=True, metavar="DIR", help="a folder of recording CSVs (recording / generate_dataset write them)")
    ap.add_argument("--validation", default=None, metavar="DIR", help="a folder of recordings scored after every epoch")
    ap.add_argument("--out", required=True, metavar="FOLDER", help="the model folder to write (e.g. .../GRU-6IN-32H1-32H2-5OUT-0)")
    ap.add_argument("--config-root", default=None, metavar="CHECKOUT",
                    help="a CartPoleSimulation checkout: SI_Toolkit_ASF/config_training.yml (EPOCHS, BATCH_SIZE, SEED, LR.*, WASH_OUT_LEN, "
                         "POST_WASH_OUT_LEN, SHIFT_LABELS); without it the values of the shipped file")
    ap.add_argument("--config-training", default=None, metavar="FILE", help="a config_training.yml elsewhere than in the checkout")
    ap.add_argument("--net", default=None, help=f"the network to train instead of the file's NET_NAME: {NET_NAME} is the one built")
    ap.add_argument("--dynamics-model", action="store_true",
                    help="train the dynamics model (Q and five state features -> the next row's features) instead of the file's features")
    for flag, typ in (("--epochs", int), ("--batch-size", int), ("--seed", int), ("--lr", float), ("--wash-out", int),
                      ("--post-wash-out", int), ("--shift-labels", int)):
        ap.add_argument(flag, type=typ, default=None, help="instead of the file's value")
    ap.add_argument("--rollout", action="store_true",
                    help="train through the open-loop rollout: behind the first scored row the model's own outputs are fed back")
    ap.add_argument("--post-wash-out-schedule", default=None, metavar="P,P,...",
                    help="one POST_WASH_OUT_LEN per epoch, the last entry repeating (e.g. 5,10,20), instead of --post-wash-out")
    ap.add_argument("--init", default=None, metavar="FOLDER",
                    help="fine-tune the model of this folder, with its normalisation, instead of fresh weights")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    path = args.config_training or (os.path.join(args.config_root, "SI_Toolkit_ASF", "config_training.yml") if args.config_root else None)
    config = {}
    if path is not None:
        with open(path) as fh:
            config = yaml.safe_load(fh) or {}
    try:
        settings, normalize = training_settings(config, net=args.net, dynamics_model=args.dynamics_model, epochs=args.epochs,
                                                batch_size=args.batch_size, seed=args.seed, lr=args.lr, wash_out=args.wash_out,
                                                post_wash_out=args.post_wash_out, shift_labels=args.shift_labels)
        settings, init, info = run_settings(settings, normalize, rollout=args.rollout, schedule=args.post_wash_out_schedule,
                                            init_folder=args.init)
    except ValueError as e:
        raise SystemExit(f"train_gru: {e}")
    states, Q, lengths, names = load_recordings_folder(args.recordings)
    validation = load_recordings_folder(args.validation)[:3] if args.validation else None
    from .configs import MPPIConfig
    from .engine import MPPIEngine
    engine = MPPIEngine(1, MPPIConfig(num_rollouts=1, mpc_horizon=2), device=args.device)
    model, history = train_gru(engine, states, Q, lengths, validation=validation, init=init, log=print, **settings)
    engine.close()
    folder = write_model_folder(args.out, model, info={**info, "TRAINING_FILES": os.path.abspath(args.recordings)})
    print(f"trained on {len(names)} recordings, final loss {history['loss'][-1]:.6e}; model folder: {folder}")
    return model, history


if __name__ == "__main__":
    main()
