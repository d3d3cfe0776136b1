"""Shapes, windows, references and the gradient bound of the WIDE GRU training tests (test_gru_train_wide_host.py judges them on the
host, test_gpu_gru_train_wide.py runs them against cpmppi_gru_loss_grad / cpmppi_gru_rollout_loss_grad).  Pure numpy + torch on the
CPU: neither the package nor its library is imported.

What the shapes are for: launch_loss_grad (csrc/cpmppi_gru_train.hip) cuts the (row, window tile) sequence of gru_wgrad_kernel into
at most WG_MAX_SLICES slices of at least WG_MIN_TILES tiles, and gru_loss_finalize_kernel strides over the waves' partial losses by
64.  With Bp = B rounded up to 32, tpr = Bp / 32 window tiles per row, tiles = (W + P) tpr, per_slice = max(ceil(tiles / 64), 8):

  case   B     W, P    Bp / tpr    tiles   per_slice, slices    what it reaches
  A      1024  4, 12   1024 / 32   512     8, 64                the cap reached exactly at the minimum slice
  B      810   4, 16   832 / 26    520     9, 58 (last 7)       first per_slice > 8; boundaries inside rows; ragged window tile
  C      1030  34, 6   1056 / 33   1320    21, 63 (last 18)     long BPTT (40 rows); 6 live lanes in the last tile
  D      2070  0, 2    2080 / 65   130     8, 17 (last 2)       65 loss partials; tpr > per_slice, so slices 0..7 are row 0 only
  E      250   1, 3    256 / 8     32      8, 4                 slice 0 is exactly row 0

Recordings: gru_train_ref.random_recordings(3, 64).  Windows as test_gpu_gru_train.windows_of draws them: from the legal ones, [1] =
[0] (a window twice), [2] one row on from [0] (overlapping), [-1] the last recording's last legal window.

The bound (share_min): the gradient of w_out is a plain sum over (scored row, window tile of 32) of sum_windows dy (x) h2 with
dy = 2 (y - label) / (B P 5).  share_min is the smallest max-abs entry of one such contribution relative to max |g_w_out|, from
the float64 reference, teacher-forced (the slice plan is the same for both modes): a slice plan that loses or doubles ONE tile moves
w_out's gradient by at least share_min in the measure of gru_train_ref.worst_relative.  The GPU test asserts share_min / 4 at A, B
and C; the host test holds the reference's own float32 realisation to share_min / 16.

Case C scores the last 6 of its 40 rows, not 30 of them.  The plan depends on W + P alone, and the share of the ragged tile - 6 live
windows of 1030 - falls with the number of scored rows: (10, 30) gives 1.3e-4, (34, 6) 1.2e-3.  The float32 realisation's error
depends on how the host's float32 GEMM accumulates over the B (W + P) terms of a weight gradient: 3.5e-7 at (10, 30) on one host,
up to 3.3e-5 on another, which is beyond 1.3e-4 / 16.  At (34, 6) the second host measures 1.7e-5 against 1.17e-3 / 16 = 7.3e-5."""
import functools
import os
import re

import numpy as np
import torch

import gru_train_ref as TR
import gru_train_rollout_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_gru_train.hip")
R, T = 3, 64
CASES = {"A": (1024, 4, 12), "B": (810, 4, 16), "C": (1030, 34, 6), "D": (2070, 0, 2), "E": (250, 1, 3)}      # B, W, P
SHARE_CASES = ("A", "B", "C")                                # where share_min / 4 is asserted on the GPU
# the table above, as the host test asserts it: Bp, tpr, tiles, per_slice, slices, tiles of the last slice
TABLE = {"A": (1024, 32, 512, 8, 64, 8), "B": (832, 26, 520, 9, 58, 7), "C": (1056, 33, 1320, 21, 63, 18),
         "D": (2080, 65, 130, 8, 17, 2), "E": (256, 8, 32, 8, 4, 8)}
FINALIZE_STRIDE = 64                                         # gru_loss_finalize_kernel: one wave, t += 64


def source_constants(text=None):
    """-> (WG_MAX_SLICES, WG_MIN_TILES) as csrc/cpmppi_gru_train.hip defines them."""
    text = open(SOURCE).read() if text is None else text
    found = [re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text) for name in ("WG_MAX_SLICES", "WG_MIN_TILES")]
    assert all(found), "WG_MAX_SLICES / WG_MIN_TILES are no longer defined as `constexpr int NAME = n;`"
    return tuple(int(m.group(1)) for m in found)


def slice_plan(B, W, P, max_slices, min_tiles):
    """launch_loss_grad's arithmetic -> dict(Bp, tpr, tiles, per_slice, slices, last: the tiles of the last slice, partials: the wave
    partials of the loss)."""
    Bp = (B + 31) // 32 * 32
    tpr = Bp // 32
    tiles = (W + P) * tpr
    per_slice = max(-(-tiles // max_slices), min_tiles)
    slices = -(-tiles // per_slice)
    return dict(Bp=Bp, tpr=tpr, tiles=tiles, per_slice=per_slice, slices=slices, last=tiles - (slices - 1) * per_slice,
                partials=(B + 31) // 32)


def legal_windows(W, P, shift=1):
    """Every legal window (r, t0) of the R x T recordings, recordings in order and t0 ascending (train_gru.make_windows; the GPU test
    holds the two against each other)."""
    starts = T - (W + P - 1 + shift)
    assert starts > 5
    return np.stack([np.repeat(np.arange(R, dtype=np.int64), starts), np.tile(np.arange(starts, dtype=np.int64), R)], axis=1)


@functools.lru_cache(maxsize=None)
def windows_of(B, W, P):
    legal = legal_windows(W, P)
    w = legal[np.random.Generator(np.random.SFC64([B, W, P])).integers(0, len(legal) - 1, B)].copy()
    w[0] = (0, 4)
    w[1] = w[0]
    w[2] = (0, 5)
    w[-1] = legal[-1]
    assert w[-1, 0] == R - 1 and w[-1, 1] + W + P == T - 1
    w.setflags(write=False)
    return w


def case_windows(key):
    return windows_of(*CASES[key])


@functools.lru_cache(maxsize=None)
def reference(key, name, norm, rollout, dtype=torch.float64):
    """-> (loss, {key: gradient as float64 array}) of the case under RR.case_model(name, norm), teacher-forced or through the rollout."""
    B, W, P = CASES[key]
    states, Q = TR.random_recordings(R, T)
    fn = RR.loss_and_grad if rollout else TR.loss_and_grad
    loss, grads = fn(RR.case_model(name, norm), states, Q, case_windows(key), W, P, dtype=dtype)
    for g in grads.values():
        g.setflags(write=False)
    return loss, grads


@functools.lru_cache(maxsize=None)
def share_min(key, name, norm):
    """-> (the smallest share over the full window tiles, over the ragged tile - None when B is a multiple of 32): per (window tile,
    scored row) the max-abs entry of its contribution to w_out's gradient over max |g_w_out|, float64, teacher-forced."""
    B, W, P = CASES[key]
    states, Q = TR.random_recordings(R, T)
    model = RR.case_model(name, norm)
    with torch.no_grad():
        net = TR.Net(model)
        x, lab = TR.window_tensors(model, states, Q, case_windows(key), W, P, 1)
        h2 = net.gru(x)[0]                                   # [B,L,32]
        y = net.head(h2)[:, W:]
        dy = 2 * (y - lab) / (B * P * 5)                     # [B,P,5]
        Bp = (B + 31) // 32 * 32
        dyp = torch.zeros(Bp, P, 5, dtype=dy.dtype)
        dyp[:B] = dy
        hp = torch.zeros(Bp, P, 32, dtype=dy.dtype)
        hp[:B] = h2[:, W:]
        cw = torch.einsum("tcpo,tcpk->tpok", dyp.view(Bp // 32, 32, P, 5), hp.view(Bp // 32, 32, P, 32))
        gw = cw.sum((0, 1))
        sw = (cw.abs().amax((2, 3)) / gw.abs().max()).numpy()      # [tile, row]
    g_ref = reference(key, name, norm, False)[1]["w_out"]
    assert np.abs(gw.numpy() - g_ref).max() <= 1e-12 * np.abs(g_ref).max(), "the contributions do not add up to autograd's w_out gradient"
    if B % 32:
        return float(sw[:-1].min()), float(sw[-1].min())
    return float(sw.min()), None


def share_bound(key, name, norm):
    """The smaller of the two figures of share_min: what one lost or doubled tile moves the gradient by, at the least."""
    full, ragged = share_min(key, name, norm)
    return full if ragged is None else min(full, ragged)
