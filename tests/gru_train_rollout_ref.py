"""The reference of the open-loop rollout training tests: the loss of cpmppi_gru_rollout_loss_grad restated with the ``Net`` of
gru_train_ref (torch.nn.GRU + Linear) stepped row by row with the feedback, differentiated by torch.autograd (float64; float32 as
a second realisation, to judge the reference's own conditioning), and the same loss driven by torch.optim.Adam - what
cpmppi_gru_rollout_train_step is compared against.

Per window (r, t0): memory zero; rows t0 .. t0+W are fed as recorded (the wash-out and the first scored row - one call of the net
over W + 1 rows, exactly the call gru_train_ref makes, so that P = 1 is its loss and gradient to the last bit); every later row j
takes the head's normalised output of row j-1, unchanged, as its five features and the recorded Q[t0+j] times in_scale[0] plus
in_shift[0] as its control.  The output of row j >= W is scored against (features of row t0+j+1 - out_shift) / out_scale; the
loss is the mean of the squared differences over B x P x 5.

tests/test_train_gru_rollout_host.py pins float32 against float64; tests/test_gpu_gru_train_rollout.py compares the kernels against
float64."""
import numpy as np
import torch

import gru_train_ref as TR
from gru_train_ref import GRU_KEYS, Net, window_tensors

f32 = np.float32


def rollout_outputs(net, x, W):
    """``x`` [B,W+P,6] normalised recorded inputs (column 0 = Q) -> the head's outputs [B,P,5] of rows W .. W+P-1 of the open-loop
    rollout: of ``x`` only the rows 0..W and, behind them, the control column are read."""
    out, h = net.gru(x[:, :W + 1])
    y = net.head(out)[:, W:]                                  # [B,1,5], as Net.forward forms it
    ys = [y]
    for j in range(W + 1, x.shape[1]):
        out, h = net.gru(torch.cat([x[:, j:j + 1, :1], y], dim=2), h)
        y = net.head(out)
        ys.append(y)
    return torch.cat(ys, dim=1)


def loss_of(net, x, labels, W):
    return ((rollout_outputs(net, x, W) - labels) ** 2).mean()


def loss_and_grad(model, states, Q, windows, W, P, dtype=torch.float64):
    """-> (loss as a float, {key: d loss / d weight as a float64 array} in the order of GRU_KEYS); shift_labels is 1."""
    net = Net(model, dtype)
    x, labels = window_tensors(model, states, Q, windows, W, P, 1, dtype)
    loss = loss_of(net, x, labels, W)
    grads = torch.autograd.grad(loss, net.tensors())
    return float(loss.detach()), {k: g.detach().numpy().astype(np.float64) for k, g in zip(GRU_KEYS, grads)}


def loss_only(model, states, Q, windows, W, P, dtype=torch.float64):
    with torch.no_grad():
        net = Net(model, dtype)
        x, labels = window_tensors(model, states, Q, windows, W, P, 1, dtype)
        return float(loss_of(net, x, labels, W))


def adam_training(model, states, Q, batches, W, P, rollout=True, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """gru_train_ref.adam_training with the rollout loss.  ``rollout``: one flag for every batch, or a sequence with one flag per
    batch (False: that step is teacher-forced - steps of the two kinds on one set of weights and one Adam state).  ``P``: one
    horizon, or one per batch.  -> (every step's loss BEFORE its update, the trained weights {key: float64 array})."""
    net = Net(model, dtype)
    opt = torch.optim.Adam(net.tensors(), lr=float(f32(lr)), betas=(float(f32(betas[0])), float(f32(betas[1]))), eps=float(f32(eps)))
    flags = [bool(rollout)] * len(batches) if np.ndim(rollout) == 0 else [bool(r) for r in rollout]
    horizons = [int(P)] * len(batches) if np.ndim(P) == 0 else [int(p) for p in P]
    losses = []
    for w, flag, p in zip(batches, flags, horizons):
        x, labels = window_tensors(model, states, Q, w, W, p, 1, dtype)
        opt.zero_grad()
        loss = loss_of(net, x, labels, W) if flag else TR.loss_of(net, x, labels, W)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), {k: t.detach().numpy().astype(np.float64) for k, t in zip(GRU_KEYS, net.tensors())}


# ---- the shapes of the gradient tests (the GPU test runs them, the host test checks the reference's own conditioning at each)
R, T = 3, 40
BATCHES = (1, 31, 33, 129)                                   # below and across the wave's 32-window tile, beyond the workgroup's 128
ROWS = ((0, 1), (0, 2), (3, 4), (0, 6), (2, 12))             # (W, P)
MODELS = (("golden", True), ("golden", False), ("random", True), ("random", False))


def case_model(name, norm):
    from test_gpu_gru_edges import model_of
    m = dict(model_of(name))
    return m if norm else {k: m[k] for k in GRU_KEYS}


def case_windows(B, W, P):
    """The windows of tests/test_gpu_gru_train.py: drawn from the legal ones, one repeated, two overlapping, the last one ending at
    the recording's last legal row."""
    from test_gpu_gru_train import windows_of
    return windows_of(B, W, P)
