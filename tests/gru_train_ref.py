"""The reference of the GRU training tests: the teacher-forced loss of cpmppi_gru_loss_grad restated with torch.nn.GRU + Linear
and differentiated by torch.autograd (float64; float32 as a second realisation, to judge the reference's own conditioning), and
the same loss driven by torch.optim.Adam - what cpmppi_gru_train_step is compared against.

Per window (r, t0): memory zero, rows t0 .. t0+W+P-1 fed as recorded - (Q, angleD, angle_cos, angle_sin, position, positionD)
times in_scale plus in_shift -, the head's output at window row j >= W against (features of row t0+j+shift - out_shift) / out_scale;
the loss is the mean of the squared differences over B x P x 5.

tests/test_train_gru_host.py pins float32 against float64; tests/test_gpu_gru_train.py compares the kernels against float64."""
import functools

import numpy as np
import torch

from oracle import oracle_np as O

f32 = np.float32
GRU_KEYS = ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_out", "b_out")
NORM_KEYS = ("in_scale", "in_shift", "out_scale", "out_shift")
FEATURE_COLUMNS = (1, 2, 3, 4, 5)        # angleD, angle_cos, angle_sin, position, positionD of a state row


class Net(torch.nn.Module):
    """torch.nn.GRU(6, 32, 2 layers) + Linear(32, 5) holding the weights of a model dict."""

    def __init__(self, model, dtype=torch.float64):
        super().__init__()
        self.gru = torch.nn.GRU(6, 32, num_layers=2, batch_first=True).to(dtype)
        self.head = torch.nn.Linear(32, 5).to(dtype)
        with torch.no_grad():
            for l in range(2):
                getattr(self.gru, f"weight_ih_l{l}").copy_(torch.as_tensor(np.asarray(model[f"w_ih{l}"], f32)))
                getattr(self.gru, f"weight_hh_l{l}").copy_(torch.as_tensor(np.asarray(model[f"w_hh{l}"], f32)))
                getattr(self.gru, f"bias_ih_l{l}").copy_(torch.as_tensor(np.asarray(model[f"b_ih{l}"], f32)))
                getattr(self.gru, f"bias_hh_l{l}").copy_(torch.as_tensor(np.asarray(model[f"b_hh{l}"], f32)))
            self.head.weight.copy_(torch.as_tensor(np.asarray(model["w_out"], f32)))
            self.head.bias.copy_(torch.as_tensor(np.asarray(model["b_out"], f32)))

    def tensors(self):
        """The parameters in the order of GRU_KEYS."""
        g = self.gru
        return [g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, g.weight_ih_l1, g.weight_hh_l1, g.bias_ih_l1,
                g.bias_hh_l1, self.head.weight, self.head.bias]

    def forward(self, x):
        return self.head(self.gru(x)[0])


def norm_of(model, dtype=torch.float64):
    """-> (in_scale, in_shift [6], out_scale, out_shift [5]) tensors; identity where the model has none."""
    fill = dict(in_scale=np.ones(6), in_shift=np.zeros(6), out_scale=np.ones(5), out_shift=np.zeros(5))
    return [torch.as_tensor(np.asarray(model[k] if model.get(k) is not None else fill[k], f32)).to(dtype) for k in NORM_KEYS]


def window_tensors(model, states, Q, windows, W, P, shift, dtype=torch.float64):
    """-> (x [B,W+P,6] normalised inputs, labels [B,P,5] normalised) of the windows, formed in ``dtype`` from the float32 data."""
    states, Q, windows = np.asarray(states, f32), np.asarray(Q, f32), np.asarray(windows)
    rows = windows[:, 1:2] + np.arange(W + P)[None, :]
    r = windows[:, 0:1]
    raw = np.concatenate([Q[r, rows][..., None], states[r, rows][..., FEATURE_COLUMNS]], axis=-1)
    lab = states[r, rows[:, W:] + shift][..., FEATURE_COLUMNS]
    a, b, A, Bv = norm_of(model, dtype)
    return torch.as_tensor(raw).to(dtype) * a + b, (torch.as_tensor(lab).to(dtype) - Bv) / A


def loss_of(net, x, labels, W):
    return ((net(x)[:, W:] - labels) ** 2).mean()


def loss_and_grad(model, states, Q, windows, W, P, shift=1, dtype=torch.float64):
    """-> (loss as a float, {key: d loss / d weight as a float64 array} in the order of GRU_KEYS)."""
    net = Net(model, dtype)
    x, labels = window_tensors(model, states, Q, windows, W, P, shift, dtype)
    loss = loss_of(net, x, labels, W)
    grads = torch.autograd.grad(loss, net.tensors())
    return float(loss.detach()), {k: g.detach().numpy().astype(np.float64) for k, g in zip(GRU_KEYS, grads)}


def flatten(tensors_by_key):
    return np.concatenate([np.asarray(tensors_by_key[k]).reshape(-1) for k in GRU_KEYS])


def worst_relative(grad, ref):
    """The project's gradient measure (test_gpu_grad.py): per parameter tensor max |g - ref| / max |ref|, -> the worst tensor's.
    ``grad``, ``ref``: {key: array}.  A tensor whose reference is exactly zero (the recurrent matrices of a one-row window, whose
    previous memory is zero) must be exactly zero: it counts 0 if it is, inf if not."""
    worst = 0.0
    for k in GRU_KEYS:
        err, top = float(np.abs(np.asarray(grad[k], np.float64) - ref[k]).max()), float(np.abs(ref[k]).max())
        worst = max(worst, err / top if top > 0 else (0.0 if err == 0 else np.inf))
    return worst


def adam_training(model, states, Q, batches, W, P, shift=1, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """torch.optim.Adam over the given ``batches`` (a list of window arrays) from ``model`` -> (every step's loss BEFORE its update,
    the trained weights {key: float64 array}).  The hyper-parameters enter as the float32 values the library is handed."""
    net = Net(model, dtype)
    opt = torch.optim.Adam(net.tensors(), lr=float(f32(lr)), betas=(float(f32(betas[0])), float(f32(betas[1]))), eps=float(f32(eps)))
    losses = []
    for w in batches:
        x, labels = window_tensors(model, states, Q, w, W, P, shift, dtype)
        opt.zero_grad()
        loss = loss_of(net, x, labels, W)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), {k: t.detach().numpy().astype(np.float64) for k, t in zip(GRU_KEYS, net.tensors())}


# ---- data shared by the tests (computed once and left unchanged)
@functools.lru_cache(maxsize=None)
def random_recordings(R=3, T=40, seed=77):
    """Recordings for the gradient tests: states of moderate size with a consistent (cos, sin) pair, controls in [-1, 1]."""
    rng = np.random.Generator(np.random.SFC64(seed))
    angle = rng.uniform(-np.pi, np.pi, (R, T))
    states = np.stack([angle, rng.uniform(-3, 3, (R, T)), np.cos(angle), np.sin(angle), rng.uniform(-0.2, 0.2, (R, T)),
                       rng.uniform(-1, 1, (R, T))], axis=-1).astype(f32)
    Q = rng.uniform(-1, 1, (R, T)).astype(f32)
    states.setflags(write=False)
    Q.setflags(write=False)
    return states, Q


@functools.lru_cache(maxsize=None)
def oracle_recordings(R=8, T=120, seed=5):
    """The training run's data: ``R`` recordings of ``T`` rows of the CPU oracle's predict_core (the plant model, float32) from
    random starts under smooth random controls - a sum of three sinusoids of random phase, scaled into [-0.9, 0.9]."""
    rng = np.random.Generator(np.random.SFC64(seed))
    t = np.arange(T - 1)
    states, Q = [], []
    for _ in range(R):
        amp, freq, phase = rng.uniform(0.1, 0.3, 3), rng.uniform(0.02, 0.2, 3), rng.uniform(0, 2 * np.pi, 3)
        q = np.clip(sum(a * np.sin(f * t + p) for a, f, p in zip(amp, freq, phase)), -0.9, 0.9).astype(f32)
        s0 = O.create_cartpole_state(rng.uniform(-0.5, 0.5), rng.uniform(-1, 1), rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2))
        traj = np.asarray(O.predict_core(np.asarray(s0, f32), q[None, :]), f32)[0]      # [T,6]
        states.append(traj)
        Q.append(np.concatenate([q, q[-1:]]))
    states, Q = np.stack(states).astype(f32), np.stack(Q).astype(f32)
    states.setflags(write=False)
    Q.setflags(write=False)
    return states, Q
