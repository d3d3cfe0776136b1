"""GPU: cpmppi_set_gru and the three weight images it builds (cpmppi_gru_model.hip), read back through the kernels that use them.
Models, tables and inputs: tests/gru_weight_cases.py; their conditions: tests/test_gru_weight_cases_host.py.  E = 2 x N = 96 x H = 8.

A. A refused cpmppi_set_gru changes nothing.  `probe` runs every call that reads the handle's model - gru_predict, gru_advance, the
   fused step, rollout_cost, gru_loss_grad - and keeps the bits; after set_gru(B) is refused (B: another normalisation, one weight out
   of range) the same calls give the same bits, in FAST and in PRECISE; a training run begun before the refusal goes on and stays
   bit-equal to a twin handle that never saw the refused call; a refused FIRST set_gru leaves the handle without a model.
B. The refusal boundary at the 13 places x both signs: the largest accepted float32 magnitude is accepted and a FAST step with it is
   finite, its successor is refused ("f16 range"); NaN, +inf and -inf in each of the 14 tensors are refused ("non-finite").  After
   every refusal the handle still computes with model A, bit for bit.
C. The f16 split cell at the ends of its operands (cases a+ .. e), FAST and PRECISE, against the numpy oracle in float32 and
   float64 under the project's rules as test_gru_long_horizon_with_a_perturbation_buffer applies them: costs through assert_costs with
   flag_rounding_sensitive, u_nom and Q through assert_controls with softmin_allowance.  No tolerance of this module's own.
D. The images after training (gru_adam_repack_kernel rebuilds both float32 images on the device, plain vectors included; the f16
   image is not rebuilt): after gru_train_begin and again after three steps a PRECISE handle's fused step, rollout_cost and
   rollout_cost_grad equal, bit for bit, those of a fresh PRECISE handle given gru_train_get()'s weights; a FAST handle's fused step
   and rollout_cost equal those of a fresh FAST handle holding the INITIAL model.  (FAST rollout_cost_grad is left out: its forward
   sweep reads the f16 image and its reverse sweep the float32 images, so during a run it mixes two models - include/cpmppi.h.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import parity_util as PU  # noqa: E402
import gru_weight_cases as W  # noqa: E402
import gru_train_ref as TR  # noqa: E402
from test_gpu_gru_train import R, T, windows_of  # noqa: E402

f32 = np.float32
E, N, H = W.E, W.N, W.H
WASH, POST, BATCH = 3, 4, 33
MODES = ("fast", "precise")


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-weights] " + text)


def new_engine(math_mode, model=None):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, math_mode=math_mode))
    if model is not None:
        eng.set_gru(model)
    return eng


def raw(t, dtype=np.uint32):
    return np.ascontiguousarray(t.cpu().numpy()).view(dtype).copy()


def fused_step(eng, x=None):
    """The fused MPPI step over the GRU on the probe inputs -> {S, u_nom, Q} as device tensors."""
    x = W.probe_inputs() if x is None else x
    un = eng.tensor(np.array(x["u0"]))
    S = eng.empty(E, N)
    Q, _ = eng.step(np.array(x["s0"]), un, np.array(x["tp"]), np.array(x["te"]), S_out=S, predictor="GRU", h0=np.array(x["h0"]),
                    delta_u=np.array(x["du"]))
    return dict(step_S=S, step_u=un, step_Q=Q)


def given_plans_cost(eng):
    x = W.probe_inputs()
    return eng.rollout_cost(np.array(x["s0"]), np.array(x["plans"]), np.array(x["tp"]), np.array(x["te"]), predictor="GRU", h0=np.array(x["h0"]))


def probe(eng, train=True):
    """Every call that reads the handle's model, on fixed inputs -> {name: bits}."""
    x = W.probe_inputs()
    out = {k: raw(v) for k, v in fused_step(eng).items()}
    traj, hfin = eng.gru_predict(np.array(x["ps0"]), np.array(x["pQ"]), h0=np.array(x["ph0"]), return_hidden=True)
    out["predict"], out["predict_h"] = raw(traj), raw(hfin)
    h = eng.tensor(np.array(x["h0"]))
    eng.gru_advance(eng.tensor(np.array(x["s0"])), eng.tensor(np.array(x["q"])), h)
    out["advance"] = raw(h)
    out["cost"] = raw(given_plans_cost(eng))
    if train:
        states, Q = TR.random_recordings(R, T)
        loss, grad = eng.gru_loss_grad(states, Q, windows_of(BATCH, WASH, POST), WASH, POST)
        out["loss"], out["grad"] = raw(loss, np.uint64), raw(grad)
    return out


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].size} words"


def refused(eng, model, match):
    from cartpolesimulation_amd._lib import CpmppiError
    with pytest.raises(CpmppiError, match=match) as info:
        eng.set_gru(model)
    assert str(info.value).split(": ", 1)[1].startswith("cpmppi_set_gru: "), str(info.value)


# ---------------------------------------------------------------------------------------------- A. a refused set changes nothing
@pytest.mark.parametrize("math_mode", MODES)
def test_a_refused_set_gru_leaves_the_model_as_it_was(math_mode):
    a, b = W.model_a(), W.model_b()
    eng = new_engine(math_mode, a)
    before = probe(eng)
    assert_same(before, probe(eng), "two runs")               # (the calls themselves give the same bits from run to run)
    refused(eng, b, "weights beyond the f16 range")
    assert eng.has_gru
    assert_same(before, probe(eng), "after the refused set_gru")
    # B without its one large weight is another model: the probe does tell models apart
    eng.set_gru(W.random_model(2602))
    other = probe(eng)
    assert all((other[k] != before[k]).any() for k in before)
    eng.close()


def test_a_refused_set_gru_leaves_a_training_run_alive():
    a, b = W.model_a(), W.model_b()
    states, Q = TR.random_recordings(R, T)
    eng, twin = new_engine("precise", a), new_engine("precise", a)
    for e in (eng, twin):
        e.gru_train_begin()
        e.gru_train_step(states, Q, windows_of(BATCH, WASH, POST), WASH, POST, lr=2e-3)
    refused(eng, b, "weights beyond the f16 range")
    assert_same(probe(twin), probe(eng), "the run's model after the refused set_gru")
    losses = []
    for e in (eng, twin):                                     # the step is accepted: the model did not change, the run goes on
        losses.append([raw(e.gru_train_step(states, Q, windows_of(31, WASH, POST), WASH, POST, lr=1e-3), np.uint64) for _ in range(2)])
    assert np.array_equal(np.stack(losses[0]), np.stack(losses[1]))
    mine, theirs = eng.gru_train_get(), twin.gru_train_get()
    for k in W.GRU_KEYS:
        assert np.array_equal(mine[k].view(np.uint32), theirs[k].view(np.uint32)), k
    assert (mine["w_hh1"] != a["w_hh1"]).mean() > 0.99        # (and it is a trained model, not A)
    assert_same(probe(twin), probe(eng), "after two more steps")
    # what the next run starts from is still A (gru_params), not B
    for e in (eng, twin):
        e.gru_train_begin()
    assert_same(probe(twin), probe(eng), "a run begun after the refusal")
    again = eng.gru_train_get()
    for k in W.GRU_KEYS:
        assert np.array_equal(again[k].view(np.uint32), a[k].view(np.uint32)), k
    eng.close()
    twin.close()


def test_a_refused_first_set_gru_leaves_no_model():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = new_engine("fast")
    refused(eng, W.model_b(), "weights beyond the f16 range")
    assert not eng.has_gru
    with pytest.raises(CpmppiError, match="no model set"):
        fused_step(eng)
    bad = W.with_entry(W.model_a(), "in_shift", 2, np.nan)
    refused(eng, bad, "non-finite")
    assert not eng.has_gru
    with pytest.raises(CpmppiError, match="no model set"):
        given_plans_cost(eng)
    eng.set_gru(W.model_a())                                  # ... and a good model is still taken
    assert torch.isfinite(fused_step(eng)["step_S"]).all()
    eng.close()


# ---------------------------------------------------------------------------------------------- B. the refusal boundary
@pytest.fixture(scope="module")
def holder():
    """One FAST handle holding model A and the bits of its cheap call."""
    eng = new_engine("fast", W.model_a())
    yield eng, raw(given_plans_cost(eng))
    eng.close()


@pytest.mark.parametrize("place", W.PLACES, ids=W.PLACE_IDS)
def test_the_limit_is_accepted_and_its_successor_refused(holder, place):
    eng, cheap = holder
    a = W.model_a()
    limit, beyond = W.accept_limit(place[1])
    try:                                                      # (whatever fails, the shared handle goes back to model A)
        for sign in (1.0, -1.0):
            refused(eng, W.at_place(a, place, f32(sign) * beyond), "weights beyond the f16 range")
            assert np.array_equal(raw(given_plans_cost(eng)), cheap), (place, sign)
        for sign in (1.0, -1.0):
            eng.set_gru(W.at_place(a, place, f32(sign) * limit))
            out = fused_step(eng)
            for k, v in out.items():
                assert torch.isfinite(v).all(), (place, sign, k)
            assert (raw(given_plans_cost(eng)) != cheap).any()
    finally:
        eng.set_gru(a)
    assert np.array_equal(raw(given_plans_cost(eng)), cheap)


@pytest.mark.parametrize("key", W.GRU_KEYS + W.NORM_KEYS)
def test_non_finite_values_are_refused(holder, key):
    eng, cheap = holder
    a = W.model_a()
    index = tuple(s // 2 for s in a[key].shape)
    try:
        for value in (np.nan, np.inf, -np.inf):
            refused(eng, W.with_entry(a, key, index, value), "non-finite value in " + key)
            assert np.array_equal(raw(given_plans_cost(eng)), cheap), (key, value)
        # the last entry of the tensor is looked at too
        refused(eng, W.with_entry(a, key, tuple(s - 1 for s in a[key].shape), np.nan), "non-finite value in " + key)
        assert np.array_equal(raw(given_plans_cost(eng)), cheap)
    finally:
        eng.set_gru(a)


# ---------------------------------------------------------------------------------------------- C. the split cell's operand ends
@pytest.mark.parametrize("math_mode", MODES)
@pytest.mark.parametrize("name", W.SPLIT_CASES)
def test_split_cell_at_the_ends_of_its_operands(name, math_mode, capsys):
    c = W.split_case(name)
    refs = W.split_reference(name)
    eng = new_engine(math_mode, c["model"])
    out = {k: v.cpu().numpy() for k, v in fused_step(eng, c).items()}
    eng.close()
    lbd = float(O.MPPIConfig(N=N, H=H).LBD)
    lines = []
    for e, (r32, r64) in enumerate(refs):
        b = PU.cost_buckets(out["step_S"][e], r32["S"], r64["S"], PU.flag_rounding_sensitive(r32["S"], r64["S"]))
        clear = ~b["flagged"]
        lines.append(f"env {e}: worst cost deviation {b['rel'].max():.2e} relative; of its allowance {b['excess'][clear].max():.2f} "
                     f"(clear), {b['excess'][~clear].max() if (~clear).any() else 0.0:.2f} ({int((~clear).sum())} flagged); "
                     f"|u - ref| {np.abs(out['step_u'][e] - r32['u_new']).max():.2e}")
    report(capsys, f"case {name} {math_mode}: " + "; ".join(lines))
    for e, (r32, r64) in enumerate(refs):
        what = f"case {name} {math_mode} env {e}"
        assert np.isfinite(out["step_S"][e]).all() and np.isfinite(out["step_u"][e]).all(), what
        PU.assert_costs(out["step_S"][e], r32["S"], r64["S"], PU.flag_rounding_sensitive(r32["S"], r64["S"]), what + " costs")
        allow = PU.softmin_allowance(r32["S"], r64["S"], c["du"][e], LBD=lbd)
        PU.assert_controls(out["step_u"][e], r32["u_new"], r64["u_new"], what + " u_nom", allowance=allow)
        PU.assert_controls(out["step_Q"][e], r32["Q"], r64["Q"], what + " Q", allowance=allow[0])


# ---------------------------------------------------------------------------------------------- D. the images after training
def model_reads(eng, grad):
    out = {k: raw(v) for k, v in fused_step(eng).items()}
    out["cost"] = raw(given_plans_cost(eng))
    if grad:
        x = W.probe_inputs()
        S, G = eng.rollout_cost_grad(np.array(x["s0"]), np.array(x["plans"]), np.array(x["tp"]), np.array(x["te"]), predictor="GRU",
                                     h0=np.array(x["h0"]))
        out["grad_S"], out["grad_G"] = raw(S), raw(G)
    return out


@pytest.mark.parametrize("math_mode", MODES)
def test_images_after_training(math_mode):
    a = W.model_a()
    norm = {k: a[k] for k in W.NORM_KEYS}
    precise = math_mode == "precise"
    states, Q = TR.random_recordings(R, T)
    eng, first = new_engine(math_mode, a), new_engine(math_mode, a)
    initial = model_reads(first, precise)                     # a handle that never trains
    first.close()
    eng.gru_train_begin()
    begun = eng.gru_train_get()
    for k in W.GRU_KEYS:
        assert np.array_equal(begun[k].view(np.uint32), a[k].view(np.uint32)), k
    assert_same(initial, model_reads(eng, precise), "right after gru_train_begin")
    for i, B in enumerate((33, 31, 129)):
        eng.gru_train_step(states, Q, windows_of(B, WASH, POST), WASH, POST, lr=2e-3 * (i + 1))
    trained = eng.gru_train_get()
    assert (trained["b_ih0"] != a["b_ih0"]).mean() > 0.99 and (trained["w_out"] != a["w_out"]).mean() > 0.99
    mine = model_reads(eng, precise)
    if precise:                                               # the float32 images, plain vectors included, are the trained model's
        fresh = new_engine(math_mode, {**trained, **norm})
        assert_same(model_reads(fresh, True), mine, "PRECISE after three steps against a fresh handle with the trained weights")
        assert all((mine[k] != initial[k]).any() for k in mine)
        fresh.close()
    else:                                                     # the f16 image is the initial model's
        assert_same(initial, mine, "FAST after three steps against a fresh handle with the initial model")
    eng.close()
