"""GPU: cpmppi_gru_advance (gru_advance_kernel) - the in-place hand-over of the GRU memory h[E,2,32] between two control periods.

What is asserted, and where the bounds come from (none is measured):
  * bit-identity with the predict seam: gru_advance(s, Q, h) == gru_predict(s, Q[:, None], h0 = h.transpose(0, 1)) hidden output,
    transposed back.  Both kernels run the same gru_step on the same exact-f32 weights image with the same env-to-lane mapping, and
    an MFMA column depends on its own column only - so the two must agree in every bit, whatever the other lanes hold.
  * the oracle (oracle_np.gru_predict, float32 and float64): 1e-4 + |oracle32 - oracle64|, test_gpu_gru_edges' hidden-state rule.
  * the direct C call: 64 sentinel rows behind h_io untouched, s and Q unchanged, every refusal launches nothing.
  * capture: three replays of the captured call == three launched calls, bit for bit.
Sizes: one row, a tile less one, a tile plus one, a full block, a second block with one live row, a tail in the third block.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_c5.npz")
SIZES = [1, 31, 33, 128, 129, 300]
E_MAX = 300


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model_of(name):
    """"golden": tests/golden/gru_c5.npz.  "random": uniform weights at scale 0.3 (SFC64(30)) with input and output normalisation -
    the two models of test_gpu_gru_edges."""
    if name == "golden":
        g = np.load(GOLDEN)
        return {k: g[k] for k in g.files if k not in ("s0", "Q", "h0", "traj", "h_final")}
    scale = 0.3
    rng = np.random.Generator(np.random.SFC64(30))
    u = lambda *s: (scale * rng.uniform(-1, 1, s)).astype(f32)  # noqa: E731
    return dict(w_ih0=u(96, 6), w_hh0=u(96, 32), b_ih0=u(96), b_hh0=u(96), w_ih1=u(96, 32), w_hh1=u(96, 32), b_ih1=u(96),
                b_hh1=u(96), w_out=(0.3 * rng.uniform(-1, 1, (5, 32))).astype(f32), b_out=(0.1 * rng.uniform(-1, 1, 5)).astype(f32),
                in_scale=rng.uniform(0.5, 2.0, 6).astype(f32), in_shift=(0.1 * rng.uniform(-1, 1, 6)).astype(f32),
                out_scale=rng.uniform(0.5, 1.5, 5).astype(f32), out_shift=(0.05 * rng.uniform(-1, 1, 5)).astype(f32))


@functools.lru_cache(maxsize=None)
def engine_of(model):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(E_MAX, MPPIConfig(num_rollouts=64, mpc_horizon=8))
    eng.set_gru(model_of(model))
    return eng


@functools.lru_cache(maxsize=None)
def case(model, E):
    """States drawn as test_gpu_gru_edges.predict_case draws them, Q in U(-1, 1), h = 0.5 N(0, 1) in the rollout kernels' layout
    [E,2,32]; the oracle's hidden states after one step, float32 and float64, with that memory and with none."""
    rng = np.random.Generator(np.random.SFC64(100 * E + 1))
    s = np.stack([O.create_cartpole_state(rng.uniform(-3, 3), rng.uniform(-8, 8), rng.uniform(-0.19, 0.19), rng.uniform(-0.8, 0.8))
                  for _ in range(E)])
    Q = rng.uniform(-1, 1, E).astype(f32)
    h = (0.5 * rng.standard_normal((E, 2, 32))).astype(f32)
    refs = {}
    for key, hh in (("h", h), ("zero", np.zeros_like(h))):
        h_2e = np.ascontiguousarray(hh.transpose(1, 0, 2))
        r32 = O.gru_predict(model_of(model), s, Q[:, None], h_2e)[1]
        r64 = O.gru_predict(model_of(model), s, Q[:, None], h_2e, dtype=np.float64)[1]
        refs[key] = (np.asarray(r32).transpose(1, 0, 2), np.asarray(r64).transpose(1, 0, 2))
    return s, Q, h, refs


@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("model", ["golden", "random"])
def test_advance_is_the_predict_seams_hidden_state(model, E, capsys):
    s, Q, h, refs = case(model, E)
    eng = engine_of(model)
    s_t, Q_t = eng.tensor(s), eng.tensor(Q)
    for key, h0 in (("h", h), ("zero", np.zeros_like(h))):
        h_t = eng.tensor(h0).clone()
        _, seam = eng.gru_predict(s_t, Q_t.reshape(E, 1), h0=h_t.transpose(0, 1).contiguous(), return_hidden=True)
        seam = seam.transpose(0, 1).contiguous().cpu().numpy()                   # [2,E,32] -> [E,2,32]
        out = eng.gru_advance(s_t, Q_t, h_t)
        assert out is h_t, "gru_advance returns the tensor it advanced"
        got = h_t.cpu().numpy()
        assert np.array_equal(bits(got), bits(seam)), (
            f"{key}: {int((bits(got) != bits(seam)).sum())} of {got.size} values differ from the predict seam, worst "
            f"{np.abs(got - seam).max():.3e} at env {int(np.argmax(np.abs(got - seam).max(axis=(1, 2))))}")
        r32, r64 = refs[key]
        d, gap = np.abs(got - r32), np.abs(r32 - r64)
        with capsys.disabled():
            print(f"\n[gru-advance] {model} E {E} {key}: |advance - oracle32| {d.max():.2e}, oracle gap {gap.max():.2e}")
        assert np.all(d <= 1e-4 + gap), f"{key}: hidden off by {d.max():.2e} at env {int(np.argmax(d.max(axis=(1, 2))))}"
    assert np.array_equal(bits(s_t.cpu().numpy()), bits(s)) and np.array_equal(bits(Q_t.cpu().numpy()), bits(Q))


@pytest.mark.parametrize("E", [33, 129])
def test_direct_call_bounds_and_refusals(E):
    """The C entry point on caller-owned buffers: 64 sentinel rows behind h_io stay untouched, s and Q are only read, and every
    refusal (E = 0, E > cfg.E, a NULL pointer, no model) returns CPMPPI_ERR_BAD_ARG with its name and launches nothing."""
    import ctypes as C
    from cartpolesimulation_amd.engine import MPPIEngine, _ptr
    from cartpolesimulation_amd.configs import MPPIConfig
    s, Q, h, _ = case("golden", E)
    eng = engine_of("golden")
    SENT = f32(-7.25)
    buf = torch.full((E + 64, 2, 32), float(SENT), dtype=torch.float32, device=eng.device)
    buf[:E] = eng.tensor(h)
    s_t, Q_t = eng.tensor(s), eng.tensor(Q)
    want = eng.gru_advance(s_t, Q_t, eng.tensor(h).clone()).cpu().numpy()
    call = lambda e, E_, sp, Qp, hp: e.lib.cpmppi_gru_advance(e._h, E_, sp, Qp, hp, e._stream())  # noqa: E731
    assert call(eng, E, _ptr(s_t), _ptr(Q_t), _ptr(buf)) == 0
    got = buf.cpu().numpy()
    assert np.all(got[E:] == SENT), "rows behind h_io were written"
    assert np.array_equal(bits(got[:E]), bits(want))
    assert np.array_equal(bits(s_t.cpu().numpy()), bits(s)) and np.array_equal(bits(Q_t.cpu().numpy()), bits(Q))

    before = buf.clone()
    null = C.c_void_p(0)
    refusals = [("E = 0", eng, 0, _ptr(s_t), _ptr(Q_t), _ptr(buf)), ("E > cfg.E", eng, E_MAX + 1, _ptr(s_t), _ptr(Q_t), _ptr(buf)),
                ("s NULL", eng, E, null, _ptr(Q_t), _ptr(buf)), ("Q NULL", eng, E, _ptr(s_t), null, _ptr(buf)),
                ("h_io NULL", eng, E, _ptr(s_t), _ptr(Q_t), null)]
    bare = MPPIEngine(E, MPPIConfig(num_rollouts=64, mpc_horizon=8))
    refusals.append(("no model", bare, E, _ptr(s_t), _ptr(Q_t), _ptr(buf)))
    for what, e, E_, sp, Qp, hp in refusals:
        assert call(e, E_, sp, Qp, hp) == -1, what                              # CPMPPI_ERR_BAD_ARG
        assert e.lib.cpmppi_last_error(e._h).decode().startswith("cpmppi_gru_advance: "), what
        torch.cuda.synchronize()
        assert torch.equal(buf, before), f"{what}: h_io changed"
    bare.close()
    with pytest.raises(ValueError):
        eng.gru_advance(s_t, Q_t[:E - 1].contiguous(), buf[:E])
    with pytest.raises(ValueError):
        eng.gru_advance(s_t, Q_t, buf[:E].transpose(1, 2))                       # not contiguous, not [E,2,32]


def test_advance_can_be_captured():
    """One launch, no allocation, no synchronisation: captured once and replayed three times == three launched calls."""
    E = 129
    s, Q, h, _ = case("random", E)
    eng = engine_of("random")
    s_t, Q_t = eng.tensor(s), eng.tensor(Q)
    launched = eng.tensor(h).clone()
    for _ in range(3):
        eng.gru_advance(s_t, Q_t, launched)
    replayed = eng.tensor(h).clone()
    start = replayed.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.gru_advance(s_t, Q_t, replayed)
    torch.cuda.current_stream(eng.device).wait_stream(side)
    replayed.copy_(start)                                                       # (whether or not the capture itself ran the kernel)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, launched)
    assert not torch.equal(replayed, start)
