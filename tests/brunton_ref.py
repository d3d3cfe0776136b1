"""Reference of the Brunton test (cpmppi_brunton), shared by tests/test_brunton_host.py and tests/test_gpu_brunton.py: the windows a
staged run would materialise, and the statistics in float64 numpy from GIVEN float32 predictions.  Plain builders, no GPU.

The error is the header's: e = predicted - recorded in float32, the angle's (feature 0) wrapped afterwards, e - 2 pi rint(e / 2 pi),
every operation rounded to float32 once.  stats[k][f] = (sum |e|, sum e^2, max |e|) over the starts; horizon step k+1 at index k.
|e| and e^2 = |e| |e| are float32 values (as the kernels form them); only their accumulation is float64 here."""
import numpy as np

f32 = np.float32
TWO_PI = f32(2.0 * np.pi)


def windows(states, Q, start, count, horizon, L=None):
    """states [R,T,6], Q [R,T] -> (s0 [B,6], Qw [B,horizon], recorded [B,horizon,6], L0 [B] or None), B = R count, b = r count + i,
    start row t = start + i: Qw[b,k] = Q[r,t+k], recorded[b,k] = states[r,t+k+1]."""
    states, Q = np.asarray(states, f32), np.asarray(Q, f32)
    R, T = Q.shape
    assert start + count + horizon <= T
    t = start + np.arange(count)
    k = np.arange(horizon)
    s0 = states[:, t].reshape(R * count, 6)
    Qw = Q[:, t[:, None] + k[None, :]].reshape(R * count, horizon)
    rec = states[:, t[:, None] + k[None, :] + 1].reshape(R * count, horizon, 6)
    L0 = None if L is None else np.asarray(L, f32)[:, t].reshape(R * count)
    return np.ascontiguousarray(s0), np.ascontiguousarray(Qw), np.ascontiguousarray(rec), L0


def errors(pred, recorded):
    """pred [B,horizon+1,6] float32 (pred[:,0] the start state), recorded [B,horizon,6] -> e [B,horizon,6] float32."""
    e = (np.asarray(pred, f32)[:, 1:] - np.asarray(recorded, f32)).astype(f32)
    a = e[:, :, 0]
    n = np.rint((a / TWO_PI).astype(f32)).astype(f32)
    e[:, :, 0] = (a - (TWO_PI * n).astype(f32)).astype(f32)
    return e


def stats(pred, recorded):
    """-> stats [horizon,6,3] float64 and the float32 |e| [B,horizon,6] they were formed from."""
    a = np.abs(errors(pred, recorded))
    sq = (a * a).astype(f32)
    out = np.stack([a.astype(np.float64).sum(axis=0), sq.astype(np.float64).sum(axis=0), a.max(axis=0).astype(np.float64)], axis=-1)
    return out, a


def by_loops(pred, recorded):
    """The same statistics start by start and step by step in Python floats - what `stats` is checked against on a small case."""
    B, H = recorded.shape[0], recorded.shape[1]
    out = np.zeros((H, 6, 3))
    for b in range(B):
        for k in range(H):
            for f in range(6):
                e = f32(f32(pred[b, k + 1, f]) - f32(recorded[b, k, f]))
                if f == 0:
                    e = f32(e - f32(TWO_PI * f32(np.rint(f32(e / TWO_PI)))))
                a = abs(e)
                out[k, f, 0] += float(a)
                out[k, f, 1] += float(f32(a * a))
                out[k, f, 2] = max(out[k, f, 2], float(a))
    return out
