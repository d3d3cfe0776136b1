"""What the trainers on windows of recordings share (``train_gru``, ``fit_ode``): the windows, the check of the recordings, the
schedule keys of config_training.yml, the epoch loop with its validation and ``LR.REDUCE_LR_ON_PLATEAU``, the recordings folder.
Each trainer keeps what is its own: the model, the window-less refusals, normalisation, its files and its command line."""
import os

import numpy as np


def make_windows(lengths, wash_out, post_wash_out, shift_labels=1):
    """Every legal window (r, t0) of recordings with ``lengths`` rows: t0 + wash_out + post_wash_out - 1 + shift_labels <= length - 1.
    -> int64 [n,2], recordings in order and t0 ascending; a recording too short for one window has none."""
    W, P, shift = int(wash_out), int(post_wash_out), int(shift_labels)
    if W < 0 or P < 1 or shift < 0:
        raise ValueError(f"wash_out >= 0, post_wash_out >= 1 and shift_labels >= 0, got {W}, {P}, {shift}")
    out = []
    for r, n in enumerate(np.asarray(lengths).reshape(-1)):
        starts = int(n) - (W + P - 1 + shift)
        if starts > 0:
            out.append(np.stack([np.full(starts, r, np.int64), np.arange(starts, dtype=np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def plateau_rule(monitored, best, wait, rate, reduce_lr_on_plateau, patience, decrease_factor, minimal_lr, min_delta):
    """``LR.REDUCE_LR_ON_PLATEAU`` after one epoch (shared with fit_ode): an improvement of the monitored loss by more than
    ``min_delta`` resets the wait; otherwise, with the rule on, ``patience`` such epochs multiply the rate by ``decrease_factor``
    (not below ``minimal_lr``).  -> (best, wait, rate)."""
    if monitored < best - float(min_delta):
        return monitored, 0, rate
    if reduce_lr_on_plateau:
        wait += 1
        if wait >= int(patience):
            rate, wait = max(rate * float(decrease_factor), float(minimal_lr)), 0
    return best, wait, rate


def check_recordings(states, Q, lengths, epochs, batch_size):
    """What every trainer is handed, checked: -> (states [R,T,6], Q [R,T] as float32, lengths [R] - None: T each -, epochs, batch_size)."""
    states, Q = np.ascontiguousarray(states, np.float32), np.ascontiguousarray(Q, np.float32)
    if states.ndim != 3 or states.shape[2] != 6 or Q.shape != states.shape[:2]:
        raise ValueError(f"states must be [R,T,6] and Q [R,T], got {states.shape} and {Q.shape}")
    R, T = Q.shape
    lengths = np.full(R, T) if lengths is None else np.asarray(lengths).reshape(-1)
    if lengths.shape != (R,) or lengths.min() < 0 or lengths.max() > T:
        raise ValueError(f"lengths must hold one length 0..{T} per recording ({R})")
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 1 or batch_size < 1:
        raise ValueError("epochs and batch_size must be at least 1")
    return states, Q, lengths, epochs, batch_size


def run_epochs(device, windows_of_epoch, step, loss_of=None, validation_windows=None, *, epochs, batch_size, seed, lr, plateau,
               validation_batch, log):
    """The epoch loop of both trainers (``train_gru``'s docstring states batches and schedule).  ``windows_of_epoch(epoch)`` -> (the
    epoch's windows [n,2], a tag for ``step``); ``step(batch, rate, loss_out, tag)`` enqueues one training step whose loss goes to
    ``loss_out``, one float64 element on ``device``; ``loss_of(windows)`` -> the loss tensor [1] of up to ``validation_batch`` of the
    ``validation_windows`` (None: the training loss is monitored); ``plateau``: what ``plateau_rule`` takes behind the rate.
    -> (history = dict(loss, val_loss, lr: one entry per epoch, batch_loss: every step's loss in order), the epochs' tags)."""
    import torch
    rng = np.random.default_rng(seed)
    rate, best, wait = float(lr), np.inf, 0
    history, tags = dict(loss=[], val_loss=[], lr=[], batch_loss=[]), []
    for epoch in range(epochs):
        windows, tag = windows_of_epoch(epoch)
        order = rng.permutation(len(windows))
        steps = -(-len(order) // batch_size)
        losses = torch.empty(steps, dtype=torch.float64, device=device)
        for i in range(steps):
            step(windows[order[i * batch_size:(i + 1) * batch_size]], rate, losses[i:i + 1], tag)
        batch_loss = losses.cpu().numpy()
        history["batch_loss"] += [float(x) for x in batch_loss]
        history["loss"].append(float(batch_loss.mean()))
        history["lr"].append(rate)
        tags.append(tag)
        if loss_of is not None:                              # the mean over the validation windows, batch by batch
            parts = [validation_windows[i:i + int(validation_batch)] for i in range(0, len(validation_windows), int(validation_batch))]
            total = 0.0
            for loss, w in zip(torch.cat([loss_of(w) for w in parts]).cpu().numpy(), parts):
                total += float(loss) * len(w)
            history["val_loss"].append(total / len(validation_windows))
        monitored = history["val_loss" if loss_of is not None else "loss"][-1]
        if log is not None:
            log(f"epoch {epoch + 1}/{epochs}: loss {history['loss'][-1]:.6e}"
                + (f", val_loss {monitored:.6e}" if loss_of is not None else "") + f", lr {rate:.3e}")
        best, wait, rate = plateau_rule(monitored, best, wait, rate, *plateau)
    return history, tags


def refuse_unbuilt_sections(config):
    """The keys of config_training.yml that neither trainer of this package (train_gru, fit_ode) is built for, refused by name
    where they are activated: on-the-fly data generation, NNI, regularisation, quantisation, pruning, series modification, filters."""
    t = dict(config.get("training_default") or {})
    if t.get("ON_FLY_DATA_GENERATION"):
        raise ValueError("training_default.ON_FLY_DATA_GENERATION: not built (generate recordings first: generate_dataset)")
    if t.get("USE_NNI"):
        raise ValueError("training_default.USE_NNI: not built")
    for section in ("REGULARIZATION", "QUANTIZATION", "PRUNING"):
        if (config.get(section) or {}).get("ACTIVATED"):
            raise ValueError(f"{section}.ACTIVATED: not built (the loss is the mean squared error alone, the weights float32)")
    mode = (config.get("CONFIG_SERIES_MODIFICATION") or {}).get("MODE")
    noise = ((config.get("CONFIG_SERIES_MODIFICATION") or {}).get("NOISE_LEVEL") or {}).get("FEATURES", 0.0)
    if (mode not in (None, "None")) or noise:
        raise ValueError(f"CONFIG_SERIES_MODIFICATION (MODE {mode!r}, NOISE_LEVEL.FEATURES {noise}): not built")
    if config.get("FILTERS"):
        raise ValueError("FILTERS: not built (filter the recordings before training)")


def schedule_settings(config):
    """config_training.yml as a dict -> the keyword arguments every trainer takes: EPOCHS, BATCH_SIZE, SEED and LR.* by the
    trainers' names."""
    t = dict(config.get("training_default") or {})
    lr = t.get("LR") or {}
    return dict(epochs=t.get("EPOCHS", 30), batch_size=t.get("BATCH_SIZE", 64), seed=t.get("SEED", 0), lr=lr.get("INITIAL", 2e-3),
                reduce_lr_on_plateau=bool(lr.get("REDUCE_LR_ON_PLATEAU", True)), patience=lr.get("PATIENCE", 2),
                decrease_factor=lr.get("DECREASE_FACTOR", 0.5), minimal_lr=lr.get("MINIMAL", 1e-7), min_delta=lr.get("MIN_DELTA", 1e-6))


def load_recordings_folder(folder):
    """Every recording CSV of ``folder`` (``brunton.load_recording``) -> (states [R,T,6], Q [R,T] padded with zeros to the longest,
    lengths [R], the file names)."""
    from .brunton import FEATURES, load_recording
    names = sorted(n for n in os.listdir(folder) if n.endswith(".csv"))
    if not names:
        raise ValueError(f"{folder}: no recording (*.csv)")
    cols = [load_recording(os.path.join(folder, n)) for n in names]
    lengths = np.array([len(c["Q"]) for c in cols])
    states, Q = np.zeros((len(cols), lengths.max(), 6), np.float32), np.zeros((len(cols), lengths.max()), np.float32)
    for r, c in enumerate(cols):
        states[r, :lengths[r]] = np.stack([c[f] for f in FEATURES], axis=-1)
        Q[r, :lengths[r]] = c["Q"]
    return states, Q, lengths, names
