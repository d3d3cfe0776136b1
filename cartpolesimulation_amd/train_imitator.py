"""Training the neural imitator of the MPC on recordings, on the device (reference: SI_Toolkit_ASF/Run/A2_Train_Network.py with
SI_Toolkit_ASF/config_training.yml AS SHIPPED: NET_NAME Dense-32H1-32H2, seven inputs, the output Q_calculated).

The network is the one the reference ships trained under GymlikeCartPole/Dense-7IN-32H1-32H2-1OUT-0/: position, positionD,
angle_cos, angle_sin, angleD, target_equilibrium, target_position -> the controller's output, two tanh layers of 32 units and a
linear head (C_implementation/network.c).  Its training target is the column ``along_trajectories`` writes, Q_calculated_offline:
the chain is  along_trajectories -> train_imitator -> recording --imitator FOLDER  (INTEGRATION.md).

SI_Toolkit is a submodule that the reference checkout does not carry, so the semantics - windows, normalisation, loss, schedule - are
THIS PACKAGE'S OWN, chosen to match what the configuration keys say, and shared with ``train_gru`` (its docstring states batches and
the learning-rate schedule):

* a window is ``POST_WASH_OUT_LEN`` consecutive rows of one recording; the network has no memory, so every row is one sample, scored
  against the label ``SHIFT_LABELS`` rows on (mean squared error of the normalised values); ``WASH_OUT_LEN`` must be 0;
* normalisation is min-max to [-1, 1] over the training recordings for the five state features and the label
  (``train_gru.normalization_from_recordings``'s rule); a TARGET column that never varies (target_equilibrium often does not) gets the
  identity (a = 1, b = 0); a state feature or label that never varies is refused by name;
* fresh weights are uniform in +-1/sqrt(fan_in) from ``numpy.random.default_rng(seed)``.

The loss, its gradient and Adam run on the device in two launches per step (``MPPIEngine.dense_train_step``).

Built for Dense-7IN-32H1-32H2-1OUT alone.  Not built, refused by name where a user can ask: other layer sizes, activations or
feature lists, a Dense dynamics model inside an optimizer, regularisation / pruning / quantisation / series modification / filters,
several models per launch, env groups and multi-GPU.

  python -m cartpolesimulation_amd.train_imitator --recordings DIR --out FOLDER --config-root CHECKOUT
                                                  [--label-column Q_calculated_offline] [--validation DIR] [--init FOLDER]

``dagger`` closes that chain on the device (DAgger, Ross et al. 2011: the reference does its rounds by hand - run, relabel with
PreprocessData_Add_Control_Along_Trajectories.py, retrain): per iteration the MPC labels every state of fresh experiments and, with
probability beta, drives them, the imitator otherwise (cpmppi_dagger_step, harness.DaggerController); the samples land in the layout
the trainer reads, and the Adam steps follow on the aggregate where it lies.  Schedule, windows (single rows drawn uniformly) and the
fixed normalisation are again THIS PACKAGE'S OWN.  Not built: the GRU predictor or a GRU-model optimizer as the expert, env groups
and several GPUs, beta per episode, sample weighting or eviction.

  python -m cartpolesimulation_amd.train_imitator --dagger ITERATIONS --beta 1,0.5,0.25,0 --experiments E --steps-per-iteration K
                                                  --config-root CHECKOUT --out FOLDER [--optimizer rpgd] [--init FOLDER] [--graph]
"""
import os

import numpy as np

from ._training import make_windows, plateau_rule, refuse_unbuilt_sections, run_epochs, schedule_settings  # noqa: F401  (re-exported)
from .model_folder import DENSE_INPUTS, DENSE_KEYS, DENSE_NET_NAME, DENSE_SHAPES

f32 = np.float32
NET_NAME = DENSE_NET_NAME
NORM_KEYS = ("in_scale", "in_shift", "out_scale", "out_shift")
LABEL_COLUMN = "Q_calculated_offline"        # what along_trajectories writes; config_training.yml calls the output Q_calculated
CONFIG_OUTPUTS = ("Q_calculated", "Q_calculated_offline")
# column of states [.., 6] = (angle, angleD, angle_cos, angle_sin, position, positionD) of the five state inputs
_STATE_COLUMNS = (1, 2, 3, 4, 5)


def check_recordings(states, target_position, target_equilibrium, labels, lengths=None):
    """-> (states [R,T,6], target_position, target_equilibrium, labels [R,T] as float32, lengths [R] - None: T each)."""
    states = np.ascontiguousarray(states, f32)
    if states.ndim != 3 or states.shape[2] != 6:
        raise ValueError(f"states must be [R,T,6], got {states.shape}")
    R, T = states.shape[:2]
    cols = []
    for name, c in (("target_position", target_position), ("target_equilibrium", target_equilibrium), ("labels", labels)):
        c = np.ascontiguousarray(c, f32)
        if c.shape != (R, T):
            raise ValueError(f"{name} must be [{R},{T}] for states [{R},{T},6], got {c.shape}")
        cols.append(c)
    lengths = np.full(R, T) if lengths is None else np.asarray(lengths).reshape(-1)
    if lengths.shape != (R,) or lengths.min() < 0 or lengths.max() > T:
        raise ValueError(f"lengths must hold one length 0..{T} per recording ({R})")
    return (states, *cols, lengths)


def normalization_from_recordings(states, target_position, target_equilibrium, labels, lengths=None):
    """Min-max normalisation to [-1, 1] (normalised = a x + b, a = 2 / (max - min), b = -(max + min) / (max - min); the label's
    inverse Q = A y + B, A = (max - min) / 2, B = (max + min) / 2) over the rows before ``lengths[r]``.  A target column that never
    varies gets a = 1, b = 0; a state feature or the label that never varies is refused by name.
    -> dict(in_scale, in_shift [7] in the order of ``model_folder.DENSE_INPUTS``, out_scale, out_shift [1]), float32."""
    states, tp, te, labels, lengths = check_recordings(states, target_position, target_equilibrium, labels, lengths)
    keep = np.arange(states.shape[1])[None, :] < lengths[:, None]
    if not keep.any():
        raise ValueError("no rows")
    cols = [states[:, :, c][keep].astype(np.float64) for c in _STATE_COLUMNS] + [te[keep].astype(np.float64), tp[keep].astype(np.float64),
                                                                                 labels[keep].astype(np.float64)]
    return normalization_from_extrema(np.array([c.min() for c in cols]), np.array([c.max() for c in cols]))


def normalization_from_extrema(lo, hi):
    """``normalization_from_recordings`` from the minima and maxima [8] alone: the seven inputs in the order of
    ``model_folder.DENSE_INPUTS``, then the label."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    names = DENSE_INPUTS + ("the label",)
    flat = [names[i] for i in (0, 1, 2, 3, 4, 7) if not hi[i] > lo[i]]
    if flat:
        raise ValueError(f"feature(s) {flat} never vary over the recordings: min-max normalisation is undefined")
    varies = hi > lo
    span = np.where(varies, hi - lo, 1.0)
    a, b = np.where(varies, 2.0 / span, 1.0), np.where(varies, -(hi + lo) / span, 0.0)
    return dict(in_scale=a[:7].astype(f32), in_shift=b[:7].astype(f32),
                out_scale=np.array([(hi[7] - lo[7]) / 2.0], f32), out_shift=np.array([(hi[7] + lo[7]) / 2.0], f32))


def initial_weights(seed):
    """A fresh Dense-7IN-32H1-32H2-1OUT: every weight and bias uniform in +-1/sqrt(fan_in) (the torch.nn.Linear rule) from
    ``numpy.random.default_rng(seed)``, in the order of ``DENSE_KEYS``."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shp in zip(DENSE_KEYS, DENSE_SHAPES):
        k = 1.0 / np.sqrt(7.0 if key in ("w1", "b1") else 32.0)
        out[key] = rng.uniform(-k, k, size=shp).astype(f32)
    return out


def _check_model(model):
    for key, shp in zip(DENSE_KEYS, DENSE_SHAPES):
        if key not in model or np.shape(model[key]) != shp:
            raise ValueError(f"model: weight {key} must have shape {shp} (Dense-7IN-32H1-32H2-1OUT is the network built)")


def train_imitator(engine, states, target_position, target_equilibrium, labels, lengths=None, *, epochs, batch_size, lr, seed,
                   post_wash_out=1, shift_labels=0, validation=None, init=None, reduce_lr_on_plateau=True, patience=2,
                   decrease_factor=0.5, minimal_lr=1e-7, min_delta=1e-6, beta1=0.9, beta2=0.999, eps=1e-7, validation_batch=4096,
                   log=None):
    """Train Dense-7IN-32H1-32H2-1OUT on ``states`` [R,T,6], ``target_position``, ``target_equilibrium``, ``labels`` [R,T]
    (``lengths`` [R]: the recordings' true lengths, None = T) with ``engine`` (an ``MPPIEngine``; its imitator is replaced).
    ``init``: the model dict to start from - weights in the order of ``DENSE_KEYS``, and the normalisation if it carries one; None:
    ``initial_weights(seed)``.  Without a normalisation in ``init`` it is ``normalization_from_recordings`` of the training data.
    ``validation`` = (states, target_position, target_equilibrium, labels, lengths or None) is scored after every epoch through the
    loss-only call.  ``eps`` defaults to Keras's Adam epsilon.
    -> (the model dict ``MPPIEngine.set_dense`` takes, which the engine holds on return; history = dict(loss, val_loss, lr: one
    entry per epoch, batch_loss: every step's loss in order))."""
    states, tp, te, labels, lengths = check_recordings(states, target_position, target_equilibrium, labels, lengths)
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be at least 1")
    windows = make_windows(lengths, 0, post_wash_out, shift_labels)
    if len(windows) == 0:
        raise ValueError(f"no recording holds a window of {post_wash_out} rows with its labels {shift_labels} rows on")
    model = dict(init) if init is not None else initial_weights(seed)
    _check_model(model)
    norm = {k: np.asarray(model[k], f32) for k in NORM_KEYS if model.get(k) is not None}
    if len(norm) != 4:
        norm = normalization_from_recordings(states, tp, te, labels, lengths)
    model = {**{k: np.asarray(model[k], f32) for k in DENSE_KEYS}, **norm}
    engine.set_dense(model)
    engine.dense_train_begin()
    dev = tuple(engine.tensor(x) for x in (states, tp, te, labels))
    loss_of = vw = None
    if validation is not None:
        vs, vtp, vte, vlab, vl = check_recordings(*validation[:4], validation[4] if len(validation) > 4 else None)
        vw = make_windows(vl, 0, post_wash_out, shift_labels)
        if len(vw) == 0:
            raise ValueError("the validation recordings hold no window")
        vdev = tuple(engine.tensor(x) for x in (vs, vtp, vte, vlab))
        loss_of = lambda w: engine.dense_loss_grad(*vdev, w, post_wash_out, shift_labels, grad=False)[0]  # noqa: E731

    def step(batch, rate, loss_out, tag):
        engine.dense_train_step(*dev, batch, post_wash_out, shift_labels, lr=rate, beta1=beta1, beta2=beta2, eps=eps, loss_out=loss_out)

    history, _ = run_epochs(engine.device, lambda epoch: (windows, None), step, loss_of, vw, epochs=epochs, batch_size=batch_size,
                            seed=seed, lr=lr, log=log, validation_batch=validation_batch,
                            plateau=(reduce_lr_on_plateau, patience, decrease_factor, minimal_lr, min_delta))
    trained = {**engine.dense_train_get(), **norm}
    engine.set_dense(trained)          # (ends the run: the engine holds the trained model as any other)
    return trained, history


# ---------------------------------------------------------------------------------------------------------------- the task cost
def finetune_on_cost(engine, states, target_position, target_equilibrium, lengths=None, *, horizon, epochs, batch_size, lr, clip_norm,
                     seed, init, validation=None, pole_lengths=None, beta1=0.9, beta2=0.999, eps=1e-7, validation_batch=4096, log=None):
    """Fine-tune the model ``init`` (weights and normalisation: a clone, or what ``dagger`` returns) on the cost the MPC minimises:
    every row of ``states`` [R,T,6] with its ``target_position`` / ``target_equilibrium`` [R,T] is a start state from which the net
    drives ``engine``'s ODE predictor for ``horizon`` control steps, scored by ``engine``'s cost; Adam follows the exact gradient of
    the batch's mean cost (``MPPIEngine.dense_policy_train_step``), clipped to the global norm ``clip_norm`` (<= 0: off).  The three
    tensors may be a ``harness.DaggerDataset``'s, where they lie on the device.  ``lengths`` [R]: the recordings' true lengths (None
    = T); ``pole_lengths`` [R]: the pole length per recording (None: the engine's).  ``validation`` = (states, target_position,
    target_equilibrium, lengths or None) is scored after every epoch through the loss-only call.  No label is read: the net is not
    told what the MPC did.  A batch whose loss or gradient norm is not finite changes nothing (its loss is recorded as it is).
    -> (the model dict ``MPPIEngine.set_dense`` takes, which the engine holds on return; history as ``train_imitator``'s)."""
    import torch
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be at least 1")
    _check_model(init)
    norm = {k: np.asarray(init[k], f32) for k in NORM_KEYS if init.get(k) is not None}
    if len(norm) != 4:
        raise ValueError("init must carry its normalisation (in_scale, in_shift, out_scale, out_shift): fine-tuning starts from a trained model")

    def recordings(s, tp, te, n):
        s = s if torch.is_tensor(s) else np.ascontiguousarray(s, f32)
        R, T = s.shape[0], s.shape[1]
        n = np.full(R, T) if n is None else np.asarray(n).reshape(-1)
        if tuple(s.shape[2:]) != (6,) or tuple(tp.shape) != (R, T) or tuple(te.shape) != (R, T) or n.shape != (R,) or n.min() < 0 or n.max() > T:
            raise ValueError("states must be [R,T,6], target_position and target_equilibrium [R,T], lengths one length 0..T per recording")
        windows = make_windows(n, 0, 1, 0)
        if len(windows) == 0:
            raise ValueError("the recordings hold no row")
        return tuple(engine.tensor(x) for x in (s, tp, te)), windows

    dev, windows = recordings(states, target_position, target_equilibrium, lengths)
    engine.set_dense({**{k: np.asarray(init[k], f32) for k in DENSE_KEYS}, **norm})
    engine.dense_train_begin()
    loss_of = vw = None
    if validation is not None:
        vdev, vw = recordings(*validation[:3], validation[3] if len(validation) > 3 else None)
        loss_of = lambda w: engine.dense_policy_loss_grad(*vdev, w, horizon, pole_lengths, grad=False)[0]  # noqa: E731

    def step(batch, rate, loss_out, tag):
        engine.dense_policy_train_step(*dev, batch, horizon, pole_lengths, lr=rate, beta1=beta1, beta2=beta2, eps=eps,
                                       clip_norm=clip_norm, loss_out=loss_out)

    history, _ = run_epochs(engine.device, lambda epoch: (windows, None), step, loss_of, vw, epochs=epochs, batch_size=batch_size,
                            seed=seed, lr=lr, log=log, validation_batch=validation_batch, plateau=(False, 0, 1.0, 0.0, 0.0))
    trained = {**engine.dense_train_get(), **norm}
    engine.set_dense(trained)          # (ends the run: the engine holds the trained model as any other)
    return trained, history


# ---------------------------------------------------------------------------------------------------------------- DAgger
def beta_schedule(beta, iterations):
    """The probability that the expert drives, per iteration: a number (every iteration), a sequence of at most ``iterations``
    numbers (the last one is kept for the iterations behind it) or the command line's text "1,0.5,0.25,0".  Every entry finite and
    in [0, 1].  -> a list of ``iterations`` floats."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"iterations must be at least 1, got {iterations}")
    if isinstance(beta, str):
        try:
            beta = [float(x) for x in beta.split(",")]
        except ValueError:
            raise ValueError(f"beta {beta!r}: numbers separated by commas, e.g. 1,0.5,0.25,0") from None
    values = [float(x) for x in np.asarray(beta, np.float64).reshape(-1)]
    if not values or len(values) > iterations:
        raise ValueError(f"beta holds {len(values)} entries for {iterations} iterations: one, or at most one per iteration")
    if not all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in values):
        raise ValueError(f"beta {values}: every entry is a probability in [0, 1]")
    return values + [values[-1]] * (iterations - len(values))


def normalization_from_dataset(dataset, first, stop):
    """``normalization_from_recordings`` over recordings ``first .. stop - 1`` of a ``harness.DaggerDataset``: the sixteen extrema
    are reduced on the device, and they alone come down."""
    import torch
    s = dataset.states[first:stop].reshape(-1, 6)
    cols = torch.cat([s[:, 1:6], dataset.target_equilibrium[first:stop].reshape(-1, 1), dataset.target_position[first:stop].reshape(-1, 1),
                      dataset.labels[first:stop].reshape(-1, 1)], dim=1)
    ext = torch.stack([cols.min(dim=0).values, cols.max(dim=0).values]).cpu().numpy()
    return normalization_from_extrema(ext[0], ext[1])


def dagger(engine, setter_config, *, experiments, iterations, beta, steps_per_iteration, batch_size, lr, seed, init=None, optimizer=None,
           graph=False, log=None, beta1=0.9, beta2=0.999, eps=1e-7):
    """DAgger (Ross, Gordon, Bagnell 2011) for Dense-7IN-32H1-32H2-1OUT, the loop closed on the device.  Per iteration i:
    ``experiments`` fresh random experiments (``schedule.RandomExperimentSetter(setter_config).draw(experiments, seed + i)``) run
    through ``run_schedule(dagger=...)`` - the MPC of ``engine`` (its fused MPPI step; ``optimizer``: a fused rpgd / gradient object
    configured for as many envs) labels every state and drives with probability ``beta[i]`` (``beta_schedule``), the imitator as
    trained so far otherwise -, their samples land in the next recordings of ONE ``harness.DaggerDataset``, and
    ``steps_per_iteration`` Adam steps follow on batches of ``batch_size`` rows drawn on the host uniformly over all rows of all
    recordings filled so far (``numpy.random.default_rng(seed)``).  The dataset is trained where it lies: it never leaves the device.
    The normalisation is fixed ONCE: ``init``'s if it carries one, else the min-max of iteration 0's recordings
    (``normalization_from_dataset``), which must then run with beta = 1 - its states do not depend on the net, and its columns
    ``imitator`` / ``sq_err`` are re-evaluated with the normalised initial net.  Adam's moments and step counter persist across the
    iterations (one ``dense_train_begin``).  ``graph``: the runs are captured.
    -> (the model dict ``MPPIEngine.set_dense`` takes, which the engine holds on return; history = dict(beta, disagreement - the mean
    over the iteration's samples of (imitator - expert)^2 on the states visited -, expert_share - of its periods the expert drove -,
    batch_loss [iterations][steps], scores [iterations][experiments,5] - ``MPPIEngine.score_runs`` of its runs -, normalization,
    dataset: the DaggerDataset))."""
    import torch
    from . import schedule as SC
    from .harness import ENGINE_MODEL, BatchedCartPoleExperiment, DaggerDataset
    E, iterations, steps, B = int(experiments), int(iterations), int(steps_per_iteration), int(batch_size)
    betas = beta_schedule(beta, iterations)
    if E < 1 or steps < 1 or B < 1:
        raise ValueError("experiments, steps_per_iteration and batch_size must be at least 1")
    if optimizer is not None and not getattr(optimizer, "fused", False):
        raise ValueError("dagger: a host-paced optimizer cannot be the expert (the fused MPPI step, or rpgd / gradient with fused=True)")
    model = dict(init) if init is not None else initial_weights(seed)
    _check_model(model)
    norm = {k: np.asarray(model[k], f32) for k in NORM_KEYS if model.get(k) is not None}
    if len(norm) != 4:
        norm = None
        if betas[0] != 1.0:
            raise ValueError(f"dagger: without a normalisation in init, iteration 0's recordings fix it and must be the expert's own: "
                             f"beta[0] must be 1, got {betas[0]}")
    weights = {k: np.asarray(model[k], f32) for k in DENSE_KEYS}
    setter = SC.RandomExperimentSetter(setter_config)
    rng = np.random.default_rng(seed)
    dataset = None
    history = dict(beta=betas, disagreement=[], expert_share=[], batch_loss=[], scores=[])
    for i in range(iterations):
        batch = setter.draw(E, int(seed) + i)
        T = batch.n_periods + 1
        if dataset is None:
            dataset = DaggerDataset(engine, iterations * E, T)
            engine.set_dense({**weights, **(norm or identity_normalization())})
            engine.dense_train_reserve(B)
            if norm is not None:
                engine.dense_train_begin()
        exp = BatchedCartPoleExperiment(engine, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=int(seed) + i)
        if optimizer is not None and getattr(optimizer, "engine", None) is not None:
            optimizer.optimizer_reset()                              # (plans, moments and counters of the runs before)
        res = exp.run_schedule(batch, optimizer=optimizer, graph=graph, imitator=ENGINE_MODEL,
                               dagger=dict(dataset=dataset, beta=betas[i], seed=int(seed) + i))
        r0, r1 = res["recordings"]
        if norm is None:                                             # iteration 0 fixes the normalisation, and the run begins
            norm = normalization_from_dataset(dataset, r0, r1)
            engine.set_dense({**weights, **norm})
            engine.dense_train_begin()
            q = engine.dense_control(dataset.states[r0:r1].reshape(-1, 6), dataset.target_position[r0:r1].reshape(-1),
                                     dataset.target_equilibrium[r0:r1].reshape(-1))[0].reshape(r1 - r0, T)
            dataset.imitator[r0:r1] = q
            dataset.sq_err[r0:r1] = ((q.double() - dataset.labels[r0:r1].double()) ** 2).sum(dim=1)
        summary = torch.stack([dataset.sq_err[r0:r1].sum() / (E * T), dataset.gate[r0:r1].double().mean()])
        scores = engine.score_runs(res["states"], res["Q"], target_position_table=batch.target_position, save_every=batch.n_save,
                                   sched_stride=batch.stride, period_steps=batch.n_ctrl)
        losses = torch.empty(steps, dtype=torch.float64, device=engine.device)
        for k in range(steps):
            windows = np.stack([rng.integers(0, r1, B), rng.integers(0, T, B)], axis=1)
            engine.dense_train_step(*dataset.tensors, windows, 1, 0, lr=lr, beta1=beta1, beta2=beta2, eps=eps, loss_out=losses[k:k + 1])
        disagreement, share = (float(x) for x in summary.cpu().numpy())
        history["disagreement"].append(disagreement)
        history["expert_share"].append(share)
        history["batch_loss"].append([float(x) for x in losses.cpu().numpy()])
        history["scores"].append(scores.cpu().numpy())
        if log is not None:
            log(f"iteration {i + 1}/{iterations}: beta {betas[i]:g}, expert drove {share:.3f}, disagreement {disagreement:.6e}, "
                f"loss {history['batch_loss'][-1][0]:.6e} -> {history['batch_loss'][-1][-1]:.6e}")
    trained = {**engine.dense_train_get(), **norm}
    engine.set_dense(trained)              # (ends the run: the engine holds the trained model as any other)
    history.update(normalization=norm, dataset=dataset)
    return trained, history


def write_model_folder(folder, model, name=None, info=None):
    """A model folder in the format ``model_folder.load_dense_model`` reads, for which it returns the arrays of ``model`` bit for
    bit: the net-info file ``<name>.txt`` (``name`` None: the folder's own name), the four normalisation CSVs (identity where
    ``model`` has none) and ``weights.npz`` with the weights in the order of ``DENSE_KEYS``, inputs in the kernel's order.
    ``info``: further ``KEY: value`` entries of the net-info file.  -> the folder."""
    _check_model(model)
    folder = os.path.abspath(os.fspath(folder))
    name = name or os.path.basename(folder.rstrip(os.sep))
    os.makedirs(folder, exist_ok=True)
    normalize = all(model.get(k) is not None for k in NORM_KEYS)
    entries = {"LIBRARY": "cartpolesimulation_amd", "NET NAME": NET_NAME, "NET FULL NAME": name,
               "INPUTS": ", ".join(DENSE_INPUTS), "OUTPUTS": LABEL_COLUMN, "TYPE": "Dense",
               "NORMALIZE": str(normalize), "PARENT NET": "Network trained from scratch"}
    entries.update({str(k).upper(): str(v) for k, v in (info or {}).items()})
    with open(os.path.join(folder, name + ".txt"), "w") as fh:
        for key, value in entries.items():
            fh.write(f"{key}:\n{value}\n\n")
    vectors = (("normalization_vec_a.csv", "in_scale", 7, 1.0), ("normalization_vec_b.csv", "in_shift", 7, 0.0),
               ("denormalization_vec_A.csv", "out_scale", 1, 1.0), ("denormalization_vec_B.csv", "out_shift", 1, 0.0))
    for fname, key, n, fill in vectors:
        v = np.asarray(model[key], f32).reshape(-1) if normalize else np.full(n, fill, f32)
        if v.shape != (n,):
            raise ValueError(f"model: {key} must have {n} entries")
        with open(os.path.join(folder, fname), "w") as fh:      # (repr of the float32's double: read back exactly)
            fh.write(",".join(repr(float(x)) for x in v) + "\n")
    np.savez(os.path.join(folder, "weights.npz"), **{k: np.asarray(model[k], f32) for k in DENSE_KEYS})
    return folder


# ---------------------------------------------------------------------------------------------------------------- command line
def training_settings(config, net=None, **overrides):
    """config_training.yml as a dict -> (the keyword arguments of ``train_imitator``: EPOCHS, BATCH_SIZE, SEED, LR.*,
    POST_WASH_OUT_LEN, SHIFT_LABELS - ``overrides``: the same by ``train_imitator``'s names, None = the file's -, ``normalize``).
    The shipped file is taken as it stands.  Refused by name: a net other than Dense-32H1-32H2, inputs other than the seven of
    ``model_folder.DENSE_INPUTS`` (in any order, split between control / state / setpoint inputs as the file likes), an output other
    than the one control Q_calculated / Q_calculated_offline, a wash-out, translation-invariant variables, and the activated
    regularisation, pruning, quantisation, series-modification, filter and on-the-fly keys."""
    t = dict(config.get("training_default") or {})
    net = net or (config.get("modeling") or {}).get("NET_NAME")
    if net != NET_NAME:
        raise ValueError(f"net {net!r}: the imitator's trainer is built for {NET_NAME} (Dense-7IN-32H1-32H2-1OUT) alone - no other "
                         "layer sizes, activations or cell types (train_gru trains GRU-32H1-32H2, fit_ode the ODE's parameters)")
    inputs = [*(t.get("control_inputs") or []), *(t.get("state_inputs") or []), *(t.get("setpoint_inputs") or [])]
    if sorted(inputs) != sorted(DENSE_INPUTS):
        raise ValueError(f"inputs {inputs}: the imitator is built for the seven inputs {list(DENSE_INPUTS)}")
    outputs = list(t.get("outputs") or [])
    if len(outputs) != 1 or outputs[0] not in CONFIG_OUTPUTS:
        raise ValueError(f"outputs {outputs}: the imitator has one output, the controller's Q ({' / '.join(CONFIG_OUTPUTS)})")
    if t.get("translation_invariant_variables"):
        raise ValueError(f"training_default.translation_invariant_variables = {t['translation_invariant_variables']}: not built")
    if int(t.get("WASH_OUT_LEN", 0)) != 0:
        raise ValueError(f"WASH_OUT_LEN = {t['WASH_OUT_LEN']}: a Dense net has no memory to wash out; set it to 0")
    refuse_unbuilt_sections(config)
    out = dict(schedule_settings(config), post_wash_out=t.get("POST_WASH_OUT_LEN", 1), shift_labels=t.get("SHIFT_LABELS", 0))
    out.update({k: v for k, v in overrides.items() if v is not None})
    if int(out["post_wash_out"]) < 1 or int(out["shift_labels"]) < 0:
        raise ValueError(f"post_wash_out >= 1 and shift_labels >= 0, got {out['post_wash_out']}, {out['shift_labels']}")
    return out, bool(t.get("NORMALIZE", True))


def identity_normalization():
    return dict(in_scale=np.ones(7, f32), in_shift=np.zeros(7, f32), out_scale=np.ones(1, f32), out_shift=np.zeros(1, f32))


def load_recordings_folder(folder, label_column=LABEL_COLUMN):
    """Every recording CSV of ``folder`` (``along_trajectories.load_columns``) -> (states [R,T,6], target_position,
    target_equilibrium, labels [R,T] padded with zeros to the longest, lengths [R], the file names).  A file without
    ``label_column`` is refused by name; ``label_column`` None: no label is read (``labels`` stays zero).  The lengths are those of
    the target_position column."""
    from .along_trajectories import FEATURES, load_columns
    names = sorted(n for n in os.listdir(folder) if n.endswith(".csv"))
    if not names:
        raise ValueError(f"{folder}: no recording (*.csv)")
    wanted = ["target_position", "target_equilibrium"] + ([label_column] if label_column is not None else [])
    cols = [load_columns(os.path.join(folder, n), wanted) for n in names]
    lengths = np.array([len(c["target_position"]) for c in cols])
    R, T = len(cols), int(lengths.max())
    states = np.zeros((R, T, 6), f32)
    tp, te, labels = np.zeros((R, T), f32), np.zeros((R, T), f32), np.zeros((R, T), f32)
    for r, c in enumerate(cols):
        n = lengths[r]
        states[r, :n] = np.stack([c[f] for f in FEATURES], axis=-1)
        tp[r, :n], te[r, :n] = c["target_position"], c["target_equilibrium"]
        if label_column is not None:
            labels[r, :n] = c[label_column]
    return states, tp, te, labels, lengths, names


def check_command_line(args):
    """What the two modes of the command line exclude, refused by name (SystemExit) before anything is read."""
    if args.finetune_cost:
        for flag, given in (("--init FOLDER", args.init is None), ("--recordings DIR", args.recordings is None),
                            ("--horizon H", args.horizon is None), ("--config-root CHECKOUT", args.config_root is None)):
            if given:
                raise SystemExit(f"train_imitator: --finetune-cost needs {flag}")
        if args.dagger is not None:
            raise SystemExit("train_imitator: --finetune-cost and --dagger are two runs: the second takes the first's folder as --init")
        for flag, given in (("--label-column", args.label_column is not None), ("--post-wash-out", args.post_wash_out is not None),
                            ("--shift-labels", args.shift_labels is not None)):
            if given:
                raise SystemExit(f"train_imitator: --finetune-cost reads no label: {flag} belongs to the training on recordings")
    elif args.horizon is not None or args.clip_norm is not None:
        raise SystemExit("train_imitator: --horizon and --clip-norm belong to --finetune-cost")
    if args.dagger is None:
        if args.recordings is None:
            raise SystemExit("train_imitator: --recordings DIR (or --dagger ITERATIONS) is required")
        for flag, given in (("--experiments", args.experiments is not None), ("--steps-per-iteration", args.steps_per_iteration is not None),
                            ("--optimizer", args.optimizer is not None), ("--graph", args.graph)):
            if given:
                raise SystemExit(f"train_imitator: {flag} belongs to --dagger")
        return
    for flag, given in (("--recordings", args.recordings is not None), ("--validation", args.validation is not None)):
        if given:
            raise SystemExit(f"train_imitator: --dagger and {flag}: DAgger gathers its own recordings on the device")
    if args.config_root is None:
        raise SystemExit("train_imitator: --dagger needs --config-root CHECKOUT (the data generator's and the controller's configuration)")
    try:
        beta_schedule(args.beta, args.dagger)
    except ValueError as e:
        raise SystemExit(f"train_imitator: --beta: {e}")


def dagger_command(args, settings, init):
    """``--dagger``: the engine and the expert from the checkout's configuration, as ``recording.main`` builds them -> ``dagger(...)``."""
    from .configs import load_reference_yaml, mppi_config_from_yaml
    from .engine import MPPIEngine
    phys, cfgs = load_reference_yaml(args.config_root)
    dg = dict(cfgs["data_gen"])
    E = args.experiments if args.experiments is not None else int(dg.get("number_of_experiments", 64))
    optimizer = None
    if args.optimizer == "rpgd":
        from .controller_mpc import controller_mpc
        ctrl = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), config=dict(fused=True, seed=settings["seed"]), phys=phys,
                              device=args.device, num_envs=E, config_root=args.config_root)
        ctrl.configure("rpgd")
        optimizer, engine = ctrl.optimizer, ctrl.optimizer.engine
    else:
        engine = MPPIEngine(E, mppi_config_from_yaml(cfgs), phys=phys, device=args.device)
    steps = args.steps_per_iteration if args.steps_per_iteration is not None else 256
    try:
        return dagger(engine, dg, experiments=E, iterations=args.dagger, beta=args.beta, steps_per_iteration=steps,
                      batch_size=settings["batch_size"], lr=settings["lr"], seed=settings["seed"], init=init, optimizer=optimizer,
                      graph=args.graph, log=print)
    finally:
        engine.close()


def finetune_command(args, settings, init):
    """``--finetune-cost``: the engine - predictor, cost, dt, substeps, physics - from the checkout's configuration; every row of
    the recordings (no control or label column is read) is a start state -> ``finetune_on_cost(...)``."""
    from .configs import load_reference_yaml, mppi_config_from_yaml
    from .engine import MPPIEngine
    phys, cfgs = load_reference_yaml(args.config_root)
    states, tp, te, _, lengths, names = load_recordings_folder(args.recordings, None)
    validation = None
    if args.validation:
        vs, vtp, vte, _, vl, _ = load_recordings_folder(args.validation, None)
        validation = (vs, vtp, vte, vl)
    engine = MPPIEngine(1, mppi_config_from_yaml(cfgs), phys=phys, device=args.device)
    try:
        model, history = finetune_on_cost(engine, states, tp, te, lengths, horizon=args.horizon, epochs=settings["epochs"],
                                          batch_size=settings["batch_size"], lr=settings["lr"], seed=settings["seed"], init=init,
                                          clip_norm=args.clip_norm if args.clip_norm is not None else 10.0, validation=validation, log=print)
    finally:
        engine.close()
    return model, history, names


def main(argv=None):
    """python -m cartpolesimulation_amd.train_imitator --recordings DIR --out FOLDER --config-root CHECKOUT
    [--label-column Q_calculated_offline] [--validation DIR] [--init FOLDER]
    python -m cartpolesimulation_amd.train_imitator --dagger ITERATIONS --beta 1,0.5,0.25,0 --experiments E --steps-per-iteration K
    --config-root CHECKOUT --out FOLDER [--optimizer rpgd] [--init FOLDER] [--graph]
    python -m cartpolesimulation_amd.train_imitator --finetune-cost --init FOLDER --recordings DIR --horizon H [--clip-norm C]
    --out FOLDER --config-root CHECKOUT [--validation DIR]"""
    import argparse
    import yaml
    ap = argparse.ArgumentParser(description="Train the neural imitator (Dense-7IN-32H1-32H2-1OUT) on relabelled recordings, on MI355X "
                                             "(reference: SI_Toolkit_ASF/Run/A2_Train_Network.py, config_training.yml as shipped)")
    ap.add_argument("--recordings", default=None, metavar="DIR", help="a folder of recording CSVs with the label column (along_trajectories writes them)")
    ap.add_argument("--dagger", type=int, default=None, metavar="ITERATIONS",
                    help="DAgger instead of recordings: this many rounds of (run the experiments with the MPC labelling and, with "
                         "probability beta, driving; train on everything gathered so far), all on the device; needs --config-root")
    ap.add_argument("--beta", default="1,0.5,0.25,0", help="--dagger: the expert's share per iteration, the last one kept (default 1,0.5,0.25,0)")
    ap.add_argument("--experiments", type=int, default=None, metavar="E", help="--dagger: experiments per iteration (default: the data generator's)")
    ap.add_argument("--steps-per-iteration", type=int, default=None, metavar="K", help="--dagger: Adam steps after every iteration's runs")
    ap.add_argument("--optimizer", default=None, choices=["mppi", "rpgd"], help="--dagger: the expert (rpgd: the fused step; default mppi)")
    ap.add_argument("--graph", action="store_true", help="--dagger: the runs captured as graphs of control periods")
    ap.add_argument("--finetune-cost", action="store_true",
                    help="fine-tune --init on the task cost instead of labels: from every row of --recordings the net drives the "
                         "configured ODE predictor for --horizon control steps, scored by the configured cost; needs --config-root")
    ap.add_argument("--horizon", type=int, default=None, metavar="H", help="--finetune-cost: control steps of the differentiated closed loop")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="C", help="--finetune-cost: the gradient's global norm is clipped to this (default 10; 0: off)")
    ap.add_argument("--validation", default=None, metavar="DIR", help="a folder of recordings scored after every epoch")
    ap.add_argument("--out", required=True, metavar="FOLDER", help="the model folder to write (e.g. .../Dense-7IN-32H1-32H2-1OUT-0)")
    ap.add_argument("--config-root", default=None, metavar="CHECKOUT",
                    help="a CartPoleSimulation checkout: SI_Toolkit_ASF/config_training.yml, taken as shipped; without it its values")
    ap.add_argument("--config-training", default=None, metavar="FILE", help="a config_training.yml elsewhere than in the checkout")
    ap.add_argument("--label-column", default=None, help=f"the column to imitate (default: what along_trajectories writes, {LABEL_COLUMN})")
    for flag, typ in (("--epochs", int), ("--batch-size", int), ("--seed", int), ("--lr", float), ("--post-wash-out", int),
                      ("--shift-labels", int)):
        ap.add_argument(flag, type=typ, default=None, help="instead of the file's value")
    ap.add_argument("--init", default=None, metavar="FOLDER", help="fine-tune the model of this folder, with its normalisation")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    check_command_line(args)
    label_column = args.label_column or LABEL_COLUMN
    path = args.config_training or (os.path.join(args.config_root, "SI_Toolkit_ASF", "config_training.yml") if args.config_root else None)
    config = {"modeling": {"NET_NAME": NET_NAME},
              "training_default": {"state_inputs": list(DENSE_INPUTS), "outputs": ["Q_calculated"], "SEED": 1873, "SHIFT_LABELS": 0}}
    if path is not None:
        with open(path) as fh:
            config = yaml.safe_load(fh) or {}
    try:
        settings, normalize = training_settings(config, epochs=args.epochs, batch_size=args.batch_size, seed=args.seed, lr=args.lr,
                                                post_wash_out=args.post_wash_out, shift_labels=args.shift_labels)
    except ValueError as e:
        raise SystemExit(f"train_imitator: {e}")
    info = {"WASH OUT LENGTH": 0, "POST WASH OUT LENGTH": settings["post_wash_out"], "SHIFT LABELS": settings["shift_labels"],
            "TRAINING_FILES": f"DAgger, {args.dagger} iterations" if args.dagger is not None else os.path.abspath(args.recordings)}
    if args.init is not None:
        from .model_folder import load_dense_model
        init = dict(load_dense_model(os.fspath(args.init)))
        if any(init.get(k) is None for k in NORM_KEYS):       # (a folder with NORMALIZE False: the identity, not the recordings')
            init.update(identity_normalization())
        info["PARENT NET"] = os.path.abspath(os.fspath(args.init))
    else:
        init = initial_weights(settings["seed"])
        if not normalize:
            init.update(identity_normalization())
    if args.dagger is not None:
        model, history = dagger_command(args, settings, init)
        folder = write_model_folder(args.out, model, info=info)
        print(f"DAgger: {args.dagger} iterations, disagreement {history['disagreement'][0]:.6e} -> "
              f"{history['disagreement'][-1]:.6e}; model folder: {folder}")
        return model, history
    if args.finetune_cost:
        info["TRAINING_FILES"] = f"task cost over {args.horizon} control steps from the rows of {os.path.abspath(args.recordings)}"
        model, history, names = finetune_command(args, settings, init)
        folder = write_model_folder(args.out, model, info=info)
        print(f"fine-tuned on the cost from the rows of {len(names)} recordings, loss {history['loss'][0]:.6e} -> "
              f"{history['loss'][-1]:.6e}; model folder: {folder}")
        return model, history
    *train, lengths, names = load_recordings_folder(args.recordings, label_column)
    validation = load_recordings_folder(args.validation, label_column)[:5] if args.validation else None
    from .configs import MPPIConfig
    from .engine import MPPIEngine
    engine = MPPIEngine(1, MPPIConfig(num_rollouts=1, mpc_horizon=2), device=args.device)
    model, history = train_imitator(engine, *train, lengths, validation=validation, init=init, log=print, **settings)
    engine.close()
    folder = write_model_folder(args.out, model, info=info)
    print(f"trained on {len(names)} recordings, final loss {history['loss'][-1]:.6e}; model folder: {folder}")
    return model, history


if __name__ == "__main__":
    main()
