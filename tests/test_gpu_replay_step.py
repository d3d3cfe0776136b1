"""GPU: replay_kernel (cpmppi_replay_step) alone, against a numpy restatement kept here - the recorded row in the plant's place:
collect (mean / standard deviation / every control of a row), publish (the next row to all copies of a recording), prime, reset.
Shapes (R recordings, K copies): one copy, a few, a copy set wider than a wave, more than one workgroup of 256 envs, 300 copies of
one recording; ragged lengths; periods at, before and past every recording's end.  Everything is bit-equal except the standard
deviation (1 float32 ulp: float64 sums in another order differ by ~2^-29 of that, so only a straddled rounding boundary shows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

f32 = np.float32
T, LENGTHS, H = 9, (5, 9, 7), 7
SHAPES = [(3, 1), (5, 3), (2, 70), (5, 70), (1, 300)]
PERIODS = (0, 3, 4, 5, 6, 7, 8, 9, T + 3)        # 0, an inner one, rows[r] - 1 and rows[r] of every length, past the longest
GUARD, PAD = 777.0, 64
COLUMNS = ("target_position", "target_equilibrium", "L", "previous_input")
OUTPUTS = ("Q_mean_out", "Q_std_out", "Q_all_out", "s_out", "target_position_out", "target_equilibrium_out", "L_out",
           "previous_input_out", "u_nom_reset")


@pytest.fixture(scope="module")
def eng():
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    e = MPPIEngine(350, MPPIConfig(num_rollouts=64, mpc_horizon=10))
    yield e
    e.close()


def case(R, K, seed=5):
    rng = np.random.Generator(np.random.SFC64(seed + 1000 * R + K))
    rows = np.array([LENGTHS[r % 3] for r in range(R)], np.uint32)
    c = dict(R=R, K=K, E=R * K, rows=rows, states=rng.standard_normal((R, T, 6)).astype(f32))
    for name in COLUMNS:
        c[name] = rng.standard_normal((R, T)).astype(f32)
    # controls that are multiples of 2^-20 in [-1, 1]: any float64 summation order is exact (1 + 20 + log2 K bits < 53)
    c["Q"] = (rng.integers(-2 ** 20, 2 ** 20 + 1, size=(len(PERIODS) + 1, R * K)) / 2.0 ** 20).astype(f32)
    return c


class Arena:
    """Every output buffer between two canaries of PAD floats."""

    def __init__(self, eng, c, h=H, skip=()):
        R, K, E = c["R"], c["K"], c["E"]
        shapes = dict(Q_mean_out=(R, T), Q_std_out=(R, T), Q_all_out=(T, E), s_out=(E, 6), target_position_out=(E,),
                      target_equilibrium_out=(E,), L_out=(E,), previous_input_out=(E,), u_nom_reset=(E, h))
        self.full, self.view = {}, {}
        for name, shape in shapes.items():
            if name in skip:
                continue
            n = int(np.prod(shape))
            self.full[name] = eng.zeros(n + 2 * PAD) + GUARD
            self.view[name] = self.full[name][PAD:PAD + n].view(*shape)
        self.expected = {name: np.full(shape, GUARD, f32) for name, shape in shapes.items() if name not in skip}

    def check(self, label):
        for name, full in self.full.items():
            got = full.cpu().numpy()
            assert (got[:PAD] == GUARD).all() and (got[-PAD:] == GUARD).all(), (label, name, "canary")
            body, want = got[PAD:-PAD].reshape(self.expected[name].shape), self.expected[name]
            if name == "Q_std_out":
                assert ((body == GUARD) == (want == GUARD)).all(), (label, name)
                ulps = np.abs(body.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
                assert ulps.max() <= 1, (label, name, int(ulps.max()))
            else:
                assert body.tobytes() == want.tobytes(), (label, name, np.argwhere(body != want)[:6].tolist())


def restate(c, exp, Q, period, prime=False):
    """The call in numpy, on the expected arrays ``exp`` (only those present are written)."""
    R, K, rows = c["R"], c["K"], c["rows"]
    q = Q.reshape(R, K).astype(np.float64)
    if "u_nom_reset" in exp:
        exp["u_nom_reset"][:] = 0.0
    for r in range(R):
        n, e = int(rows[r]), slice(r * K, (r + 1) * K)
        if not prime and period < n:
            if "Q_mean_out" in exp:
                exp["Q_mean_out"][r, period] = f32(q[r].mean())
            if "Q_std_out" in exp:
                exp["Q_std_out"][r, period] = f32(np.sqrt(((q[r] - q[r].mean()) ** 2).sum() / (K - 1))) if K > 1 else f32(0.0)
            if "Q_all_out" in exp:
                exp["Q_all_out"][period, e] = Q[e]
        p = 0 if prime else min(period + 1, n - 1)
        if "s_out" in exp:
            exp["s_out"][e] = c["states"][r, p]
        for name in COLUMNS:
            if name + "_out" in exp:
                exp[name + "_out"][e] = c[name][r, p]


def arguments(eng, c, arena, skip=()):
    kw = {name: eng.tensor(c[name]) for name in COLUMNS if name not in skip}
    kw.update(arena.view)
    return (eng.tensor(c["states"]), c["rows"], None, c["K"]), kw


def launch(eng, c, arena, Q, skip=(), **named):
    args, kw = arguments(eng, c, arena, skip)
    eng.replay_step(args[0], args[1], eng.tensor(Q), args[3], **named, **kw)


@pytest.mark.parametrize("R,K", SHAPES)
def test_collect_and_publish_at_every_kind_of_period(eng, R, K):
    c = case(R, K)
    arena = Arena(eng, c)
    launch(eng, c, arena, c["Q"][-1], prime=True)
    restate(c, arena.expected, c["Q"][-1], 0, prime=True)
    arena.check("prime")
    assert (arena.expected["Q_mean_out"] == GUARD).all() and (arena.expected["Q_all_out"] == GUARD).all()   # prime writes no output row
    for i, period in enumerate(PERIODS):
        arena.view["u_nom_reset"].fill_(3.0)
        launch(eng, c, arena, c["Q"][i], period=period)
        restate(c, arena.expected, c["Q"][i], period)
        arena.check(f"period {period}")
    # the mean is numpy's float64 mean rounded once, exactly (restated above); past every end nothing was collected
    live = np.arange(T)[None, :] < c["rows"][:, None]
    written = arena.expected["Q_mean_out"] != GUARD
    assert (written <= live).all() and written[:, list(p for p in PERIODS if p < T)].sum() == sum(
        int((c["rows"] > p).sum()) for p in PERIODS if p < T)


def test_the_last_period_collects_nothing_and_publishes_last_rows(eng):
    c = case(5, 70)
    arena = Arena(eng, c)
    launch(eng, c, arena, c["Q"][0], period=T + 3)
    for name in ("Q_mean_out", "Q_std_out", "Q_all_out"):
        assert (arena.view[name].cpu().numpy() == GUARD).all(), name
    last = c["states"][np.arange(5), c["rows"] - 1]
    assert np.array_equal(arena.view["s_out"].cpu().numpy(), np.repeat(last, 70, axis=0))
    restate(c, arena.expected, c["Q"][0], T + 3)
    arena.check("past the end")


@pytest.mark.parametrize("R,K", [(5, 3), (5, 70)])
def test_the_device_counter_names_the_period_like_the_host(eng, R, K):
    c = case(R, K)
    by_host, by_dev = Arena(eng, c), Arena(eng, c)
    for i, period in enumerate((0, 4, 6, T + 3)):
        launch(eng, c, by_host, c["Q"][i], period=period)
        counter = torch.full((1,), period + 1, dtype=torch.int64, device=eng.device)
        launch(eng, c, by_dev, c["Q"][i], period=99, period_dev=counter)            # (the host's period is not read)
        assert int(counter.item()) == period + 1                                   # the counter is the step's: only read here
    for name in OUTPUTS:
        assert by_host.full[name].cpu().numpy().tobytes() == by_dev.full[name].cpu().numpy().tobytes(), name
    # a counter that is still 0 names no controller call made: the call behaves as a prime call
    zero, primed = Arena(eng, c), Arena(eng, c)
    launch(eng, c, zero, c["Q"][0], period_dev=torch.zeros(1, dtype=torch.int64, device=eng.device))
    launch(eng, c, primed, c["Q"][0], prime=True)
    for name in OUTPUTS:
        assert zero.full[name].cpu().numpy().tobytes() == primed.full[name].cpu().numpy().tobytes(), name
    restate(c, primed.expected, c["Q"][0], 0, prime=True)
    primed.check("prime")


@pytest.mark.parametrize("absent", OUTPUTS + COLUMNS)
def test_every_optional_pointer_may_be_null(eng, absent):
    c = case(5, 3)
    skip = (absent, absent + "_out") if absent in COLUMNS else (absent,)
    arena = Arena(eng, c, skip=skip)
    for i, period in enumerate((0, 4, 5)):
        launch(eng, c, arena, c["Q"][i], skip=skip, period=period)
        restate(c, arena.expected, c["Q"][i], period)
    arena.check(f"without {absent}")


@pytest.mark.parametrize("h", [7, 50])
def test_the_plans_are_zeroed_and_nothing_beside_them(eng, h):
    c = case(5, 70)
    arena = Arena(eng, c, h=h)
    arena.view["u_nom_reset"].copy_(eng.tensor(np.arange(350 * h, dtype=f32).reshape(350, h) + 1.0))
    launch(eng, c, arena, c["Q"][0], period=2)
    restate(c, arena.expected, c["Q"][0], 2)
    arena.check(f"H = {h}")
    assert not arena.view["u_nom_reset"].any()


def test_two_runs_give_identical_bytes(eng):
    c = case(5, 70)
    Q = np.random.Generator(np.random.SFC64(9)).standard_normal(350).astype(f32)    # (any controls: sums that do round)
    runs = []
    for _ in range(2):
        arena = Arena(eng, c)
        for period in (0, 4, 8):
            launch(eng, c, arena, Q, period=period)
        runs.append({name: full.cpu().numpy().tobytes() for name, full in arena.full.items()})
    assert runs[0] == runs[1]
    # ... and the standard deviation of controls that are no multiples of 2^-20 is within 1 ulp of numpy's two-pass value
    restate(c, arena.expected, Q, 0), restate(c, arena.expected, Q, 4), restate(c, arena.expected, Q, 8)
    got, want = arena.view["Q_std_out"].cpu().numpy(), arena.expected["Q_std_out"]
    assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1
    gm, wm = arena.view["Q_mean_out"].cpu().numpy(), arena.expected["Q_mean_out"]
    assert np.abs(gm.view(np.int32).astype(np.int64) - wm.view(np.int32).astype(np.int64)).max() <= 1


def test_refusals_by_their_text(eng):
    from cartpolesimulation_amd._lib import CpmppiError
    c = case(5, 3)
    arena = Arena(eng, c)
    args, kw = arguments(eng, c, arena)
    Q = eng.tensor(c["Q"][0])

    def refused(text, lengths=None, **fields):
        call = eng.prepare_replay_step(args[0], c["rows"] if lengths is None else lengths, Q, args[3], period=1, **kw)
        for name, value in fields.items():
            setattr(call.args, name, value)
        with pytest.raises(CpmppiError, match=text) as err:
            call.run()
        assert "cpmppi_replay_step: " in str(err.value)
        return err.value

    for name in ("states", "Q", "rows", "rows_host"):
        refused("states, Q, rows and rows_host are required", **{name: None})
    for name in ("R", "T", "K"):
        refused("R, T and K must be at least 1", **{name: 0})
    refused(r"5 recordings x 71 evaluations = 355 envs, the handle has 350", K=71)
    refused(r"rows\[1\] = 0 must lie in 1\.\.9", lengths=np.array([5, 0, 7, 5, 9], np.uint32))
    refused(r"rows\[2\] = 10 must lie in 1\.\.9", lengths=np.array([5, 9, 10, 5, 9], np.uint32))
    refused("no output at all", **{name: None for name in OUTPUTS})
    for name in COLUMNS:
        refused(f"{name}_out without the {name} column", **{name: None})
    refused("u_nom_reset needs H", H=0)
    err = refused("misaligned pointer", Q=Q.data_ptr() + 2)
    assert err.code != refused("no output at all", **{name: None for name in OUTPUTS}).code
    with pytest.raises(ValueError, match="L_out needs the recorded column L"):
        eng.replay_step(args[0], c["rows"], Q, 3, **{**kw, "L": None})
    arena.check("after the refusals")                                              # nothing was launched
