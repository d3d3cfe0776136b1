"""CPU-only: what train_gru and fit_ode share (cartpolesimulation_amd/_training.py) and the engine's seam under both - the epoch loop
over a stand-in with no library, the order of engine calls of both trainers, and the two slots in which the engine holds the batches
of ``gru_train_step`` and ``ode_fit_step`` while their launches run."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402

f32 = np.float32
# what plateau_rule takes behind the rate: reduce_lr_on_plateau, patience, decrease_factor, minimal_lr, min_delta
PLATEAU = (True, 1, 0.5, 8e-4, 1e-6)


def _run(train_losses, val_losses=None, **kw):
    """``run_epochs`` over 10 windows, batch_size 4, 3 epochs, seed 5; every step and validation batch takes its loss from the
    scripts.  -> (history, tags, the steps as (batch, rate, tag), the validation batches, the log lines)."""
    from cartpolesimulation_amd._training import run_epochs
    windows = np.stack([np.arange(10) % 3, 100 + np.arange(10)], axis=1)
    val_windows = np.stack([np.zeros(10, np.int64), 200 + np.arange(10)], axis=1)
    steps, scored, lines = [], [], []
    train, val = iter(train_losses), iter(val_losses or ())

    def step(batch, rate, loss_out, tag):
        assert loss_out.dtype == torch.float64 and loss_out.shape == (1,)
        steps.append((batch.copy(), rate, tag))
        loss_out.fill_(next(train))

    def loss_of(w):
        scored.append(w.copy())
        return torch.tensor([next(val)], dtype=torch.float64)

    validation = (loss_of, val_windows) if val_losses else ()
    history, tags = run_epochs(torch.device("cpu"), lambda epoch: (windows, 10 * epoch), step, *validation, epochs=3, batch_size=4,
                               seed=5, lr=1e-3, plateau=PLATEAU, validation_batch=4, log=lines.append, **kw)
    return windows, val_windows, history, tags, steps, scored, lines


def test_epoch_loop_batches_rates_and_history():
    """The training loss monitored: 3.0 in every step, so epoch 1 does not improve on epoch 0 and, with patience 1, epoch 2 runs at
    max(1e-3 x 0.5, minimal_lr = 8e-4)."""
    from cartpolesimulation_amd._training import plateau_rule
    windows, _, history, tags, steps, scored, lines = _run([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 2.0, 1.0, 0.5])
    rng = np.random.default_rng(5)                           # one generator, one permutation per epoch
    expected = [windows[order[lo:lo + 4]] for order in (rng.permutation(10) for _ in range(3)) for lo in (0, 4, 8)]
    assert len(steps) == 9 and [len(b) for b, _, _ in steps] == [4, 4, 2] * 3
    for (batch, _, _), want in zip(steps, expected):
        np.testing.assert_array_equal(batch, want)
    rate, best, wait, rates = 1e-3, np.inf, 0, []
    for monitored in (3.0, 3.0, (2.0 + 1.0 + 0.5) / 3):
        rates.append(rate)
        best, wait, rate = plateau_rule(monitored, best, wait, rate, *PLATEAU)
    assert rates == [1e-3, 1e-3, 8e-4]                       # (the floor: 5e-4 without it)
    assert [r for _, r, _ in steps] == [x for x in rates for _ in range(3)]
    assert [t for _, _, t in steps] == [0] * 3 + [10] * 3 + [20] * 3 and tags == [0, 10, 20]
    assert list(history) == ["loss", "val_loss", "lr", "batch_loss"]
    assert history["loss"] == [3.0, 3.0, (2.0 + 1.0 + 0.5) / 3] and history["lr"] == rates and history["val_loss"] == []
    assert history["batch_loss"] == [3.0] * 6 + [2.0, 1.0, 0.5] and not scored
    assert lines == ["epoch 1/3: loss 3.000000e+00, lr 1.000e-03", "epoch 2/3: loss 3.000000e+00, lr 1.000e-03",
                     "epoch 3/3: loss 1.166667e+00, lr 8.000e-04"]


def test_epoch_loop_monitors_the_weighted_validation_loss():
    """Validation batches of 4, 4 and 2 windows: the epoch's loss is their mean weighted by size, and it - not the training loss,
    which falls throughout - drives the plateau rule: 2.0, 2.0 (a plateau), then 1.0."""
    _, val_windows, history, _, steps, scored, lines = _run([9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0],
                                                             [1.0, 2.0, 4.0, 2.0, 2.0, 2.0, 0.5, 0.5, 3.0])
    assert history["val_loss"] == [(4 * 1.0 + 4 * 2.0 + 2 * 4.0) / 10, 2.0, (4 * 0.5 + 4 * 0.5 + 2 * 3.0) / 10]
    assert history["val_loss"][0] == 2.0 != (1.0 + 2.0 + 4.0) / 3
    assert [r for _, r, _ in steps] == [1e-3] * 6 + [8e-4] * 3 and history["lr"] == [1e-3, 1e-3, 8e-4]
    assert len(scored) == 9
    for i, w in enumerate(scored):
        np.testing.assert_array_equal(w, val_windows[4 * (i % 3):4 * (i % 3) + 4])
    assert [len(history[k]) for k in ("loss", "val_loss", "lr", "batch_loss")] == [3, 3, 3, 9]
    assert lines[1] == "epoch 2/3: loss 5.000000e+00, val_loss 2.000000e+00, lr 1.000e-03"


class _RecordingEngine:
    """Stands in for MPPIEngine under the trainers: records the names of the calls, in order."""

    def __init__(self):
        from cartpolesimulation_amd.configs import PhysicalParameters
        from cartpolesimulation_amd.engine import MPPIEngine
        self.calls, self.device, self.phys = [], torch.device("cpu"), PhysicalParameters()
        self.ode_fit_mask = MPPIEngine.ode_fit_mask

    def tensor(self, x, shape=None):
        self.calls.append("tensor")
        return torch.as_tensor(np.array(x))

    def _step(self, *args, loss_out, **kw):
        loss_out.fill_(1.0)

    def _loss(self, *args, **kw):
        return torch.ones(1, dtype=torch.float64), None

    def __getattr__(self, name):
        from cartpolesimulation_amd.train_gru import initial_weights
        result = {"gru_train_step": self._step, "ode_fit_step": self._step, "gru_loss_grad": self._loss, "ode_fit_loss_grad": self._loss,
                  "gru_train_get": lambda: initial_weights(1), "ode_fit_get": lambda: (np.ones(8, f32), np.zeros(8, f32)),
                  "set_gru": lambda model: None, "gru_train_begin": lambda: None, "gru_train_reserve": lambda B, rows: None,
                  "ode_fit_begin": lambda: None}
        if name not in result:
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append(name)
            return result[name](*args, **kw)
        return call


def test_trainers_issue_their_engine_calls_in_the_same_order():
    from cartpolesimulation_amd.fit_ode import fit_ode
    from cartpolesimulation_amd.train_gru import train_gru
    states, Q = TR.random_recordings(3, 40)
    # 3 x (40 - 5) = 105 windows in batches of 64: two steps per epoch; the validation recording holds 35 windows: two batches of 20
    kw = dict(epochs=2, batch_size=64, lr=1e-3, seed=0, validation=(states[:1], Q[:1]), validation_batch=20)
    eng = _RecordingEngine()
    _, history = train_gru(eng, states, Q, wash_out=2, post_wash_out=3, **kw)
    epoch = ["gru_train_step"] * 2 + ["gru_loss_grad"] * 2
    assert eng.calls == ["set_gru", "gru_train_begin"] + ["tensor"] * 4 + epoch * 2 + ["gru_train_get", "set_gru"]
    assert list(history) == ["loss", "val_loss", "lr", "batch_loss", "post_wash_out"] and history["post_wash_out"] == [3, 3]
    eng = _RecordingEngine()                                 # a horizon per epoch: the workspace is reserved before the first step
    _, history = train_gru(eng, states, Q, wash_out=2, post_wash_out=(3, 5), rollout=True, **{**kw, "validation": None})
    assert eng.calls == (["set_gru", "gru_train_begin"] + ["tensor"] * 2 + ["gru_train_reserve"] + ["gru_train_step"] * 4
                         + ["gru_train_get", "set_gru"])
    assert history["post_wash_out"] == [3, 5] and history["val_loss"] == []
    eng = _RecordingEngine()
    _, history = fit_ode(eng, states, Q, horizon=4, **kw)
    epoch = ["ode_fit_step"] * 2 + ["ode_fit_loss_grad"] * 2
    assert eng.calls == ["tensor"] * 4 + ["ode_fit_begin"] + epoch * 2 + ["ode_fit_get"]
    assert list(history) == ["loss", "val_loss", "lr", "batch_loss", "theta", "parameters"] and len(history["batch_loss"]) == 4


def test_shared_helpers_and_constants_have_one_definition():
    from cartpolesimulation_amd import _training, fit_ode, model_folder, train_gru
    from cartpolesimulation_amd.engine import MPPIEngine
    for name in ("make_windows", "plateau_rule", "refuse_unbuilt_sections", "load_recordings_folder"):
        assert getattr(train_gru, name) is getattr(fit_ode, name) is getattr(_training, name), name
    assert train_gru.GRU_KEYS is MPPIEngine.GRU_KEYS is model_folder.GRU_KEYS == TR.GRU_KEYS
    assert train_gru.GRU_SHAPES is MPPIEngine.GRU_SHAPES is model_folder.GRU_SHAPES
    assert sum(int(np.prod(s)) for s in model_folder.GRU_SHAPES) == 10341


# ---------------------------------------------------------------------------------------------- the engine's two slots
class _Lib:
    """Stands in for libcpmppi.so: records every call with a copy of the argument block it was handed by reference."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("cpmppi_"):
            raise AttributeError(name)

        def call(h, ref, *rest):
            block = ref._obj
            self.calls.append((name, {f: getattr(block, f) for f, _ in block._fields_}, rest))
            return 0
        return call


def _int32_tensors(keep):
    return [t for t in keep if torch.is_tensor(t) and t.dtype == torch.int32]


def test_engine_holds_the_batch_of_each_kind_until_the_next_of_that_kind(monkeypatch):
    from cartpolesimulation_amd import engine as E
    from test_ode_fit_host import _engine
    monkeypatch.setattr(E, "device_tensor", lambda name, t, dtype=torch.float32, tail=None, note="": t)   # (host tensors stand in)
    eng = _engine()
    eng.lib, eng.has_gru = _Lib(), True
    states, Q = (torch.as_tensor(np.array(x)) for x in TR.random_recordings(2, 30))
    scale = np.ones(5, f32)
    w1, w2, w3 = np.array([[0, 0], [1, 5]]), np.array([[1, 2], [0, 7], [1, 17]]), np.array([[1, 24]])
    loss = torch.zeros(1, dtype=torch.float64)

    def held(slot, block):
        """The slot's latest batch is the one of ``block``: the library was handed the addresses of tensors the engine still has."""
        keep = getattr(eng, slot)[1]
        (w_dev,) = _int32_tensors(keep)
        (w_host,) = [a for a in keep if isinstance(a, np.ndarray)]
        assert w_dev.data_ptr() == block["windows"] and w_host.ctypes.data == block["windows_host"]
        assert any(t is states for t in keep) and any(t is Q for t in keep)
        return w_dev, w_host

    assert eng.gru_train_step(states, Q, w1, 2, 3, lr=0.01, loss_out=loss) is loss
    name, first, hyper = eng.lib.calls[-1]
    assert name == "cpmppi_gru_train_step" and hyper[:4] == (0.01, 0.9, 0.999, 1e-8) and len(hyper) == 5
    w_dev, w_host = held("_train_keep", first)
    assert w_dev.tolist() == w1.tolist() and w_host.dtype == np.uint32 and w_host.tolist() == w1.tolist()

    eng.ode_fit_step(states, Q, w2, 12, "u_max", scale, lr=0.02)
    name, second, hyper = eng.lib.calls[-1]
    assert name == "cpmppi_ode_fit_step" and hyper[:4] == (0.02, 0.9, 0.999, 1e-8)
    assert held("_fit_keep", second)[0].tolist() == w2.tolist()
    held("_train_keep", first)                               # the GRU step's batch is still there

    eng.gru_train_step(states, Q, w3, 2, 3, lr=0.01, beta1=0.8, eps=1e-7, rollout=True)
    name, third, hyper = eng.lib.calls[-1]
    assert name == "cpmppi_gru_rollout_train_step" and hyper[:4] == (0.01, 0.8, 0.999, 1e-7)
    assert held("_train_keep", third)[0].tolist() == w3.tolist()
    held("_fit_keep", second)                                # ... and so is the fit's

    # the block of a training step is the loss-only call's for the same inputs
    call = eng.prepare_gru_loss_grad(states, Q, w1, 2, 3, grad=False, loss_out=loss)
    want = {f: getattr(call.args, f) for f, _ in call.args._fields_}
    assert first["grad_out"] is None and want["grad_out"] is None
    for field in ("B", "R", "T", "wash_out", "post_wash_out", "shift_labels", "states", "Q", "loss_out"):
        assert first[field] == want[field], field
    assert (first["B"], first["R"], first["T"], first["wash_out"], first["post_wash_out"], first["shift_labels"]) == (2, 2, 30, 2, 3, 1)
    assert first["states"] == states.data_ptr() and first["Q"] == Q.data_ptr() and first["loss_out"] == loss.data_ptr()
    (again,) = _int32_tensors(call.keep)                     # (a fresh upload: the same windows at another address)
    assert again.tolist() == w1.tolist()

    # a step refused before the library is called leaves both slots as they were
    with pytest.raises(ValueError, match="t0 \\+ 2 \\+ 3 - 1 \\+ 1 <= 29"):
        eng.gru_train_step(states, Q, np.array([[0, 25]]), 2, 3, lr=0.01)
    held("_train_keep", third)
    held("_fit_keep", second)
