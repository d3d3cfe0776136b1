"""GPU: the fused CEM control step over the GRU predictor (gru_cem_step_kernel, cpmppi_cem_step_gru, MPPIEngine.cem_step_gru,
optimizer_cem(gru_model=..., gru_fused=True)) - against the entry points it fuses composed in the test, against the numpy oracles
one iteration at a time, the order at its edges, its device step counter, its refusals, the optimizer and the closed loop.

Shapes: N = 24 (inside one 32-rollout tile), 33 (one rollout in the second tile), 129 (the first rollout past the staged kernel's
128-rollout workgroup and past four waves), 200 (shipped), 256 (full); H = 7 (odd: the Philox pair's tail) and 8, 200 x 35 once;
E = 1 and 3; best_k = 1, N and in between; 1 and 3 iterations; shift 0, 1, 2; both costs, both math modes, h0 NULL and a non-zero
memory, the golden model (tests/golden/gru_c5.npz) and one set of random weights (test_gpu_gru_edges.model_of).

Bounds.  Against the composition (cem_sample -> rollout_cost(predictor="GRU", h0) -> cem_update, `iterations` times, then the shift)
everything is compared on its bits: the kernel's statements are the staged kernels', and the rollout is the GruRollout the
cost-only kernel runs (the precedent: test_gpu_gru_cost_only.py asserts S bit-equal between two kernels that share it).  Against
the oracles: the sampler's bound of test_gpu_cem.py, the cost allowance of test_gpu_gru_cost_only.py (parity_util.assert_costs
with its flags), the whole order exactly as oracle_np.bitonic_topk orders the kernel's OWN costs, and mean / stdev within
test_gpu_cem.py's refit bounds (1e-6 / 2e-6: float32 sums of at most 256 terms in [-1, 1] against float64) of a float64 refit of the
kernel's own samples over its own elite."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from oracle import philox_np as PH  # noqa: E402
from test_gpu_cem import sampler_bound  # noqa: E402
from test_gpu_gru_cost_only import check_costs, oracle_costs  # noqa: E402
from test_gpu_gru_edges import bits, draw_env, engine, model_of  # noqa: E402

f32 = np.float32
SEED, ENV_OFFSET = 2 ** 40 + 7, 1000
QBGM, DEFAULT = "quadratic_boundary_grad_minimal", "default"


def report(capsys, text):
    with capsys.disabled():
        print("\n[cem-gru] " + text)


def problem(E, H, seed, h_scale=0.2):
    """Per env: state, target position and memory as draw_env draws them, and a sampling distribution that clips a few samples."""
    rng = np.random.Generator(np.random.SFC64(seed))
    envs = [draw_env(rng, H, 0.2, h_scale) for _ in range(E)]
    s0, tp, h0 = (np.stack([e[i] for e in envs]).astype(f32) for i in (0, 1, 3))
    mean = rng.uniform(-0.3, 0.3, (E, H)).astype(f32)
    stdev = rng.uniform(0.2, 0.6, (E, H)).astype(f32)
    return s0, tp, np.ones(E, f32), h0, mean, stdev


def fused(eng, s0, mean0, stdev0, tp, te, h0, iterations, best_k, stdev_min, shift, offset, mid=0.0, **kw):
    E, H = mean0.shape
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    S, plan, smp = eng.empty(E, eng.N), eng.empty(E, H), eng.empty(E, eng.N, H)
    order = torch.empty(E, eng.N, dtype=torch.int32, device=mean.device)
    u = eng.cem_step_gru(s0, mean, stdev, tp, te, h0, iterations=iterations, best_k=best_k, stdev_min=stdev_min, shift=shift,
                         mean_fill=mid, stdev_fill=math.sqrt(0.5), seed=SEED, offset=offset, env_offset=ENV_OFFSET, S_out=S,
                         plan_out=plan, samples_out=smp, order_out=order, **kw)[0]
    torch.cuda.synchronize()
    return dict(mean=mean.cpu().numpy(), stdev=stdev.cpu().numpy(), control=u.cpu().numpy(), plan=plan.cpu().numpy(),
                S=S.cpu().numpy(), samples=smp.cpu().numpy(), order=order.cpu().numpy())


def composed(eng, s0, mean0, stdev0, tp, te, h0, iterations, best_k, stdev_min, shift, offset, mid=0.0):
    """The same step from the existing entry points, and the shift as optimizer_cem._shift makes it, by `shift` columns.  The
    whole order: cem_update with best_k = N on the last iteration's costs (its first best_k entries are the elite)."""
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    for i in range(iterations):
        Q = eng.cem_sample(mean, stdev, SEED, offset=offset + i, env_offset=ENV_OFFSET)
        if i == 0:
            first = Q.cpu().numpy()
        S = eng.rollout_cost(s0, Q, tp, te, predictor="GRU", h0=h0)
        mean, stdev = eng.cem_update(S, Q, best_k, stdev_min)
    order = eng.cem_update(S, Q, eng.N, stdev_min, return_elites=True)[2]
    out = dict(control=mean[:, 0].cpu().numpy(), plan=mean.cpu().numpy(), S=S.cpu().numpy(), samples=Q.cpu().numpy(),
               order=order.cpu().numpy(), first=first)
    if shift:
        mean = torch.cat([mean[:, shift:], torch.full_like(mean[:, :shift], mid)], dim=1).contiguous()
        stdev = torch.cat([stdev[:, shift:], torch.full_like(stdev[:, :shift], math.sqrt(0.5))], dim=1).contiguous()
    out.update(mean=mean.cpu().numpy(), stdev=stdev.cpu().numpy())
    return out


# ---- 1. equals the composition, bit for bit -------------------------------------------------------------------------------------
# (N, H, E, best_k, iterations, shift, cost, math mode, a memory?, model)
COMPOSED_CASES = [
    (24, 7, 1, 1, 1, 0, QBGM, "fast", False, "golden"),
    (24, 8, 3, 24, 3, 1, DEFAULT, "precise", True, "random"),
    (33, 8, 3, 10, 3, 2, DEFAULT, "fast", True, "golden"),
    (33, 7, 1, 33, 1, 1, QBGM, "precise", False, "random"),
    (129, 7, 3, 20, 3, 1, QBGM, "precise", True, "golden"),
    (129, 8, 1, 1, 3, 0, DEFAULT, "fast", False, "random"),
    (200, 7, 3, 40, 3, 1, DEFAULT, "precise", True, "golden"),
    (200, 8, 3, 200, 1, 2, QBGM, "fast", True, "random"),
    (256, 8, 3, 64, 3, 0, QBGM, "fast", True, "golden"),
    (256, 7, 1, 256, 1, 2, DEFAULT, "precise", False, "golden"),
    (256, 7, 3, 1, 3, 1, QBGM, "precise", True, "random"),
    (200, 35, 3, 40, 3, 1, QBGM, "fast", True, "golden"),                   # the shipped cem-tf shape
    (200, 35, 1, 40, 3, 1, DEFAULT, "precise", True, "golden"),
]


@pytest.mark.parametrize("N,H,E,best_k,iterations,shift,cost,math_mode,memory,model", COMPOSED_CASES)
def test_fused_equals_the_composed_entry_points(N, H, E, best_k, iterations, shift, cost, math_mode, memory, model, capsys):
    eng = engine(E, N, H, model, cost_function_specification=cost, math_mode=math_mode, action_low=-0.9, action_high=0.8)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 300 + N + H)
    args = (eng, s0, mean0, stdev0, tp, te, h0 if memory else None, iterations, best_k, 0.05, shift, 2 ** 33 + 5)
    ref = composed(*args, mid=-0.05)
    got = fused(*args, mid=-0.05)
    eng.close()
    keys = ("samples", "S", "mean", "stdev", "control", "plan")
    report(capsys, f"fused vs composed {model} {cost} {math_mode} N {N} H {H} E {E} k {best_k} it {iterations} shift {shift} h0 {memory}: "
                   + ", ".join(f"{k} {int((bits(got[k]) != bits(ref[k])).sum())}" for k in keys) + " words differ")
    assert np.isfinite(ref["S"]).all()
    if N * E >= 129:                                                         # the first draw clips at either limit
        assert (ref["first"] == f32(-0.9)).any() and (ref["first"] == f32(0.8)).any()
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.array_equal(got["order"], ref["order"])
    assert np.array_equal(np.sort(got["order"], axis=1), np.tile(np.arange(N), (E, 1)))    # a permutation of the rows
    if shift:
        assert (got["mean"][:, H - shift:] == f32(-0.05)).all() and (got["stdev"][:, H - shift:] == f32(math.sqrt(0.5))).all()
    assert np.array_equal(got["control"], got["plan"][:, 0])


def test_the_memory_is_read_and_not_written():
    E, N, H = 3, 33, 7
    eng = engine(E, N, H)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 77)
    h = eng.tensor(h0.copy())
    with_h = fused(eng, s0, mean0, stdev0, tp, te, h, 2, 8, 0.05, 1, 3)
    assert np.array_equal(bits(h.cpu().numpy()), bits(h0))
    without = fused(eng, s0, mean0, stdev0, tp, te, None, 2, 8, 0.05, 1, 3)
    zeros = fused(eng, s0, mean0, stdev0, tp, te, np.zeros_like(h0), 2, 8, 0.05, 1, 3)
    eng.close()
    assert not np.array_equal(with_h["S"], without["S"])
    assert np.array_equal(bits(without["S"]), bits(zeros["S"])) and np.array_equal(bits(without["mean"]), bits(zeros["mean"]))


# ---- 2. against the oracles, one iteration per call -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,E,best_k,model,math_mode", [(200, 7, 2, 40, "golden", "fast"), (33, 8, 1, 1, "random", "precise")])
def test_one_iteration_per_call_against_the_oracles(N, H, E, best_k, model, math_mode, capsys):
    """Three calls of one iteration each (shift 0, host offsets o, o + 1, o + 2), every one checked on its own, so that no check
    depends on which side of an elite boundary a rounding falls: samples_out against philox_np from the distribution the call started
    with; S_out against the float32 / float64 oracle pair on the device's own samples; order_out against oracle_np.bitonic_topk's
    order of the device's own S_out, all N places; mean / stdev against a float64 refit of samples_out over order_out[:best_k].
    Then one call of three iterations from the same start equals the chain bit for bit."""
    lo, hi, o, stdev_min = -0.5, 0.8, 2 ** 33 + 11, 0.01
    eng = engine(E, N, H, model, action_low=lo, action_high=hi, math_mode=math_mode)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 17 + N)
    mean, stdev = mean0, stdev0
    for i in range(3):
        got = fused(eng, s0, mean, stdev, tp, te, h0, 1, best_k, stdev_min, 0, o + i)
        ref = PH.cem_samples(mean, stdev, SEED, o + i, ENV_OFFSET, N, lo, hi)
        err = np.abs(got["samples"].astype(np.float64) - ref)
        assert np.all(err <= sampler_bound(stdev)), (i, err.max())
        if i == 0:                                                           # (the refit narrows the later draws)
            assert got["samples"].min() == f32(lo) and got["samples"].max() == f32(hi)
        refs = [oracle_costs(model, QBGM, s0[e], got["samples"][e], tp[e], h0[e]) for e in range(E)]
        worst = check_costs(got["S"], refs, QBGM, tp, f"call {i}")
        report(capsys, f"call {i} {model} {math_mode} {E}x{N}x{H}: |samples - philox| / bound {np.max(err / sampler_bound(stdev)):.3f}, "
                       f"cost excess {worst:.3f}")
        for e in range(E):
            assert np.array_equal(got["order"][e], O.bitonic_topk(got["S"][e], N)), (i, e)
            elite = got["samples"][e][got["order"][e, :best_k]].astype(np.float64)
            np.testing.assert_allclose(got["mean"][e], elite.mean(0), atol=1e-6, rtol=0)
            np.testing.assert_allclose(got["stdev"][e], np.maximum(elite.std(0), stdev_min), atol=2e-6, rtol=0)
        assert np.array_equal(got["control"], got["mean"][:, 0]) and np.array_equal(got["plan"], got["mean"])
        mean, stdev = got["mean"], got["stdev"]
    once = fused(eng, s0, mean0, stdev0, tp, te, h0, 3, best_k, stdev_min, 0, o)
    for k in ("mean", "stdev", "control", "plan", "S", "samples", "order"):
        assert np.array_equal(bits(once[k].astype(f32)), bits(got[k].astype(f32))), k
    assert not np.array_equal(once["mean"], mean0)
    eng.close()


# ---- 3. the order at its edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,best_k", [(65, 65), (200, 40)])
@pytest.mark.parametrize("kind,weights,limit", [("+inf", dict(cc_weight_up=3e38), 1.0), ("-inf", dict(cc_weight_up=-3e38), 1.0),
                                                ("nan", dict(R=3e38, cc_weight_up=0.0), 2.0)])
def test_order_with_nan_inf_and_ties(kind, weights, limit, N, best_k):
    """Costs a ranking can get wrong, forced through the inputs as test_gpu_cem_fused.test_order_with_nan_inf_and_ties forces them.
    Env 0, by a cost weight at the edge of float32: the control cost u^2 R cc_weight summed over the horizon overflows for the larger
    plans (+inf, or -inf with the weight negative); with R = 3e38, cc_weight = 0 and limits of +-2 a plan with a control beyond 1.07
    costs inf * 0 = NaN and the others stay finite.  Env 1 starts from a NaN state (every cost NaN: all ties), env 2 samples with
    stdev 0 (every cost equal).  The order is the stable argsort of the device's own costs: NaN last, ties by index, no index >= N."""
    E, H = 3, 7
    eng = engine(E, N, H, cost_weights=weights, action_low=-limit, action_high=limit)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 61)
    s0[1, O.ANGLED_IDX] = np.nan
    stdev0[2] = 0.0
    got = fused(eng, s0, mean0, stdev0, tp, te, h0, 1, best_k, 0.01, 1, 3)
    eng.close()
    S = got["S"]
    assert 0.05 < np.isfinite(S[0]).mean() < 0.95                            # a mix in env 0 ...
    assert {"+inf": np.isposinf, "-inf": np.isneginf, "nan": np.isnan}[kind](S[0][~np.isfinite(S[0])]).all()
    assert np.isnan(S[1]).all() and np.isfinite(S[2, 0]) and np.all(bits(S[2]) == bits(S[2])[0])
    assert got["order"].min() >= 0 and got["order"].max() < N
    for e in range(E):
        assert np.array_equal(got["order"][e], np.argsort(S[e], kind="stable")), e
        assert np.array_equal(got["order"][e], O.bitonic_topk(S[e], N)), e
    assert np.array_equal(got["order"][1], np.arange(N)) and np.array_equal(got["order"][2], np.arange(N))
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["stdev"]).all()        # (the samples are finite whatever they cost)
    if kind == "nan":
        assert np.isnan(S[0, got["order"][0, -1]])                           # NaN is last


# ---- 4. the device counter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_device_counter_equals_the_host_offsets(math_mode):
    """Five control steps with the step counter on the device against the same steps with the host's offset c * iterations: mean,
    stdev and control bitwise equal after every step; the word ends at 5.  Between the steps the memory and the state move on."""
    E, N, H, iters, best_k = 3, 65, 7, 3, 12
    eng = engine(E, N, H, math_mode=math_mode)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 51)
    kw = dict(iterations=iters, best_k=best_k, stdev_min=0.02, shift=1, stdev_fill=math.sqrt(0.5), seed=SEED)
    bufs = [[eng.tensor(mean0.copy()), eng.tensor(stdev0.copy()), eng.zeros(E)] for _ in range(2)]
    counter = torch.zeros(1, dtype=torch.int64, device=bufs[0][0].device)
    s, h = eng.tensor(s0), eng.tensor(h0.copy())
    for c in range(5):
        mh, sh, uh = bufs[0]
        eng.cem_step_gru(s, mh, sh, tp, te, h, offset=4 + c * iters, Q_out=uh, **kw)
        md, sd, ud = bufs[1]
        eng.cem_step_gru(s, md, sd, tp, te, h, offset=4, count_dev=counter, Q_out=ud, **kw)
        for a, b in zip(bufs[0], bufs[1]):
            assert torch.equal(a, b), f"step {c}"
        assert int(counter.item()) == c + 1
        eng.gru_advance(s, uh, h)
        eng.plant_advance(s, uh, n_substeps=10)                              # the next step sees another state
    assert int(counter.item()) == 5 and not torch.equal(bufs[0][0], eng.tensor(mean0))
    eng.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
R_E, R_N, R_H = 3, 40, 7
R_OK = dict(iterations=2, best_k=10, stdev_min=0.01, shift=1, seed=SEED, offset=3)


def _fresh_result():
    eng = engine(R_E, R_N, R_H)
    s0, tp, te, h0, mean0, stdev0 = problem(R_E, R_H, 10)
    got = fused(eng, s0, mean0, stdev0, tp, te, h0, R_OK["iterations"], R_OK["best_k"], R_OK["stdev_min"], 1, 3)
    eng.close()
    return got


def _good_call_equals_fresh(eng):
    s0, tp, te, h0, mean0, stdev0 = problem(R_E, R_H, 10)
    got = fused(eng, s0, mean0, stdev0, tp, te, h0, R_OK["iterations"], R_OK["best_k"], R_OK["stdev_min"], 1, 3)
    ref = _fresh_result()
    for k in ref:
        assert np.array_equal(bits(got[k].astype(f32)), bits(ref[k].astype(f32))), k


class _Outputs:
    """Sentinel-filled buffers of one call: `untouched()` after a refusal."""

    def __init__(self, eng, mean0, stdev0, E=R_E):
        self.mean0, self.stdev0 = mean0, stdev0
        self.mean, self.stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
        self.out = dict(Q_out=eng.empty(E).fill_(-7.25), S_out=eng.empty(E, eng.N).fill_(-7.25), plan_out=eng.empty(E, eng.H).fill_(-7.25),
                        samples_out=eng.empty(E, eng.N, eng.H).fill_(-7.25),
                        order_out=torch.full((E, eng.N), -7, dtype=torch.int32, device=self.mean.device))

    def untouched(self):
        torch.cuda.synchronize()
        return (np.array_equal(self.mean.cpu().numpy(), self.mean0) and np.array_equal(self.stdev.cpu().numpy(), self.stdev0)
                and all(bool((t == (-7 if t.dtype == torch.int32 else -7.25)).all()) for t in self.out.values()))


@pytest.mark.parametrize("case", ["no model", "legacy cost", "quadratic_boundary cost", "N beyond one workgroup", "tuning rows"])
def test_refusals_about_the_handle(case):
    from cartpolesimulation_amd._lib import CpmppiError
    from cartpolesimulation_amd.configs import MPPIConfig, tuning_rows
    from cartpolesimulation_amd.engine import MPPIEngine
    cost = {"legacy cost": "legacy_mppi_cartpole", "quadratic_boundary cost": "quadratic_boundary"}.get(case, QBGM)
    N = 320 if case == "N beyond one workgroup" else R_N
    cfg = MPPIConfig(num_rollouts=N, mpc_horizon=R_H, cost_function_specification=cost)
    eng = MPPIEngine(R_E, cfg)
    if case != "no model":
        eng.set_gru(model_of("golden"))
    if case == "tuning rows":
        eng.set_tuning_rows(tuning_rows(cfg, R_E))
    s0, tp, te, h0, mean0, stdev0 = problem(R_E, R_H, 10)
    bufs = _Outputs(eng, mean0, stdev0)
    want = {"no model": "no model set", "legacy cost": "supports quadratic_boundary_grad_minimal and default",
            "quadratic_boundary cost": "supports quadratic_boundary_grad_minimal and default",
            "N beyond one workgroup": "at most 256 samples", "tuning rows": "tuning rows are registered"}[case]
    for _ in range(2):
        with pytest.raises(CpmppiError, match="libcpmppi error -1: cpmppi_cem_step_gru: .*" + want):
            eng.cem_step_gru(s0, bufs.mean, bufs.stdev, tp, te, h0, **R_OK, **bufs.out)
    assert bufs.untouched()
    # the handle goes on serving: what it supports, and - once the obstacle is gone - the step itself, as a fresh handle's
    assert np.isfinite(eng.cem_sample(bufs.mean, bufs.stdev, 1).cpu().numpy()).all()
    if case == "no model":
        eng.set_gru(model_of("golden"))
    elif case == "tuning rows":
        eng.set_tuning_rows(None)
    if case in ("no model", "tuning rows"):
        _good_call_equals_fresh(eng)
    elif case != "N beyond one workgroup":                                   # (another cost: the handle's other settings are its own)
        eng.set_cost(QBGM)
        got = fused(eng, s0, mean0, stdev0, tp, te, h0, 2, 10, 0.01, 1, 3)
        assert np.isfinite(got["S"]).all() and not np.array_equal(got["mean"], mean0)
    eng.close()


def test_refusals_about_the_arguments_leave_the_handle_usable():
    from cartpolesimulation_amd._lib import CpmppiError
    eng = engine(R_E, R_N, R_H)
    s0, tp, te, h0, mean0, stdev0 = problem(R_E, R_H, 10)
    bufs = _Outputs(eng, mean0, stdev0)

    def call(**over):
        return eng.cem_step_gru(s0, bufs.mean, bufs.stdev, tp, te, h0, **dict(R_OK, **over), **bufs.out)

    for over, text in ((dict(best_k=0), "best_k"), (dict(best_k=R_N + 1), "best_k"), (dict(iterations=0), "iterations"),
                       (dict(shift=R_H + 1), "shift")):
        with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: .*" + text):
            call(**over)
    assert bufs.untouched()
    # a NULL among the required pointers, a misaligned one, E out of range: through the argument block itself
    prep = eng.prepare_cem_step_gru(s0, bufs.mean, bufs.stdev, tp, te, h0, **R_OK, **bufs.out)
    for field in ("s0", "target_position", "target_equilibrium", "mean", "stdev", "Q_out"):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, None)
        with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: null pointer"):
            prep.run()
        setattr(prep.args, field, keep + 2)
        with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: misaligned pointer"):
            prep.run()
        setattr(prep.args, field, keep)
    keep = prep.args.h0
    prep.args.h0 = keep + 1
    with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: misaligned pointer"):
        prep.run()
    prep.args.h0 = keep
    counter = torch.zeros(2, dtype=torch.int64, device=bufs.mean.device)
    prep.args.count_dev = counter.data_ptr() + 4
    with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: misaligned pointer"):
        prep.run()
    prep.args.count_dev = None
    for bad_E in (0, R_E + 1):
        prep.args.E = bad_E
        with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: bad argument .0 < E <= config.E."):
            prep.run()
    prep.args.E = R_E
    assert eng.lib.cpmppi_cem_step_gru(eng._h, None, eng._stream()) == -1
    assert eng.lib.cpmppi_last_error(eng._h).decode().startswith("cpmppi_cem_step_gru: null argument block")
    assert bufs.untouched() and int(counter.sum().item()) == 0
    _good_call_equals_fresh(eng)
    eng.close()


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_capture_without_a_reserved_workspace_is_refused_and_the_capture_survives(math_mode):
    """On a capturing stream the step must not allocate: without cpmppi_cem_reserve it is refused with a text before any HIP call
    that a capture forbids - the capture goes on, ends and replays; after the reserve (which a handle with a model takes in either
    math mode) the same step + cpmppi_gru_advance are captured, and two replays equal two launched periods."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 40, 7
    eng = engine(E, N, H, math_mode=math_mode)
    s0, tp, te, h0, mean0, stdev0 = problem(E, H, 12)
    s, tpd, ted = eng.tensor(s0), eng.tensor(tp), eng.tensor(te)
    mean, stdev, u, h = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy()), eng.zeros(E), eng.tensor(h0.copy())
    counter = torch.zeros(1, dtype=torch.int64, device=mean.device)
    marker = eng.zeros(4)
    step = dict(iterations=2, best_k=10, stdev_min=0.01, shift=1, stdev_fill=math.sqrt(0.5), seed=SEED, offset=3)
    prep = eng.prepare_cem_step_gru(s, mean, stdev, tpd, ted, h, count_dev=counter, Q_out=u, **step)
    side = torch.cuda.Stream(device=mean.device)
    side.wait_stream(torch.cuda.current_stream(mean.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_cem_step_gru: the stream is being captured"):
                prep.run()
            marker.add_(1.0)
    torch.cuda.current_stream(mean.device).wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.array_equal(mean.cpu().numpy(), mean0) and int(counter.item()) == 0
    eng.cem_reserve()
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(mean.device))
    fixed = eng.use_stream(side)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            prep.run()
            eng.gru_advance(s, u, h)
    eng.use_stream(fixed)
    torch.cuda.current_stream(mean.device).wait_stream(side)
    g2.replay()
    g2.replay()
    torch.cuda.synchronize()
    mr, sr, hr = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy()), eng.tensor(h0.copy())
    for c in range(2):
        ur = eng.cem_step_gru(s, mr, sr, tpd, ted, hr, **dict(step, offset=3 + 2 * c))[0]
        eng.gru_advance(s, ur, hr)
    torch.cuda.synchronize()
    assert int(counter.item()) == 2 and torch.equal(mean, mr) and torch.equal(stdev, sr) and torch.equal(u, ur) and torch.equal(h, hr)
    eng.close()


# ---- 6. the optimizer -----------------------------------------------------------------------------------------------------------
OPT = dict(num_rollouts=40, mpc_horizon=7, cem_outer_it=3, cem_best_k=8, cem_stdev_min=0.01, seed=9)


def _states(E):
    return np.stack([O.create_cartpole_state(0.3, -0.5, 0.02, 0.1), O.create_cartpole_state(-0.4, 1.0, -0.05, -0.1),
                     O.create_cartpole_state(0.1, 0.3, 0.08, 0.15)])[:E]


@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_fused_optimizer_equals_the_staged_one(math_mode):
    """optimizer_cem(gru_model, gru_fused=True) against optimizer_cem(gru_model) staged over 4 control steps at E = 3, N = 40,
    H = 7, three outer iterations: the controls, dist_mue, stdev and the memory h bitwise after every step - and the same through
    controller_mpc(config=dict(gru_model=..., gru_fused=True))."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    from cartpolesimulation_amd.harness import FusedOptimizer, HostPacedOptimizer, optimizer_controller
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    E = 3
    target = np.array([-0.05, 0.0, 0.04], f32)
    limits = (np.array([-1.0]), np.array([1.0]))

    def make(**kw):
        vp = SimpleNamespace(target_position=target.copy(), target_equilibrium=np.ones(E, f32))
        opt = optimizer_cem(control_limits=limits, num_envs=E, gru_model=model_of("golden"), variable_parameters=vp,
                            math_mode=math_mode, optimizer_logging=True, **OPT, **kw)
        opt.configure()
        return opt

    staged, fused_opt = make(), make(gru_fused=True)
    ctrl = controller_mpc("CartPole", {"target_position": target.copy(), "target_equilibrium": np.ones(E, f32)}, limits, num_envs=E,
                          config=dict(gru_model=model_of("golden"), gru_fused=True, math_mode=math_mode, **OPT))
    ctrl.configure("cem")
    seam = ctrl.optimizer
    assert fused_opt.fused and fused_opt.gru_fused and seam.fused and seam.gru_fused and not staged.fused
    assert optimizer_controller(fused_opt) is FusedOptimizer and optimizer_controller(staged) is HostPacedOptimizer
    s = _states(E)
    for step in range(4):
        u_s, u_f, u_c = staged.step(s), fused_opt.step(s), ctrl.step(s, time=0.02 * step)
        for name, other, u_o in (("optimizer", fused_opt, u_f), ("controller_mpc", seam, u_c)):
            assert u_o.shape == (E, 1) and np.array_equal(bits(u_o), bits(u_s)), f"step {step} {name}: controls"
            for attr in ("dist_mue", "stdev", "h"):
                assert np.array_equal(bits(getattr(other, attr).cpu().numpy()), bits(getattr(staged, attr).cpu().numpy())), \
                    f"step {step} {name}: {attr}"
            assert other.step_counter == staged.step_counter
        assert np.array_equal(bits(fused_opt.logging_values["J_logged"]), bits(staged.logging_values["J_logged"]))
        s = np.stack([O.ode_v0_step(s[e][None], u_s[e].astype(f32))[0] for e in range(E)])
    assert np.abs(staged.h.cpu().numpy()).max() > 1e-3 and np.abs(u_s).max() > 1e-3
    fused_opt.optimizer_reset()
    assert float(fused_opt.h.abs().max()) == 0.0 and fused_opt.step_counter == 0
    for opt in (staged, fused_opt, seam):
        opt.engine.close()


# ---- 7. the closed loop ---------------------------------------------------------------------------------------------------------
def _schedule_batch(E, parameters=None):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=31, length_of_experiment=0.2, keep_target_equilibrium_x_seconds_up=0.1, turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    if parameters is None:
        return SC.RandomExperimentSetter(cfg).draw(E, 83)
    return SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(E, 83, stride=1), parameters, seed=84)


def _loop_optimizer(E, predictor_type=None, **kw):
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    opt = optimizer_cem(control_limits=(np.array([-1.0]), np.array([1.0])), num_envs=E, gru_model=model_of("golden"), **OPT, **kw)
    if predictor_type is not None:
        opt.cfg.predictor_type = predictor_type           # (the equations the handle would integrate: the network's step never does)
    opt.configure()
    return opt


def _run(E, graph, batch=None, **kw):
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    b = _schedule_batch(E) if batch is None else batch
    opt = _loop_optimizer(E, **kw)
    res = BatchedCartPoleExperiment(opt.engine, b.dt_simulation, b.dt_control, seed=0).run_schedule(b, graph=graph, steps_per_graph=5, optimizer=opt)
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state")}
    out["memory"] = opt.h.cpu().numpy()
    opt.engine.close()
    return b, out


def test_captured_loop_equals_the_launched_loop_and_the_staged_optimizer():
    """run_schedule with the fused GRU optimizer, two experiments of 0.2 s at 40 x 7: captured (graph=True) equals launched - states,
    controls, recording rows and the final memory, bitwise -, and launched equals the same batch under the staged optimizer object
    (HostPacedOptimizer), which still cannot be captured."""
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    E = 2
    b, launched = _run(E, False, gru_fused=True)
    _, captured = _run(E, True, gru_fused=True)
    _, staged = _run(E, False)
    assert b.n_periods == 10 and launched["Q"].shape == (11, E) and np.abs(launched["Q"]).max() > 0.02
    assert np.isfinite(launched["states"]).all() and np.abs(launched["memory"]).max() > 1e-3
    for k in launched:
        assert np.array_equal(bits(launched[k]), bits(captured[k])), ("captured", k)
        assert np.array_equal(bits(launched[k]), bits(staged[k])), ("staged", k)
    staged_opt = _loop_optimizer(E)
    with pytest.raises(ValueError, match="paced by the host"):
        BatchedCartPoleExperiment(staged_opt.engine, seed=0).run_schedule(_schedule_batch(E), graph=True, optimizer=staged_opt)
    staged_opt.engine.close()


def test_a_varying_pole_mass_table_is_still_captured():
    """A batch whose pole mass changes during the experiments, on a handle configured for predictor "ODE" (whose controller would be
    told the mass call by call, which no graph replays): the network reads no pole mass, so the run is captured and equals the
    launched one."""
    from cartpolesimulation_amd.harness import ControllerMass
    E = 2
    prm = dict(m_pole=dict(init_value=0.087, change_every_x_seconds=0.03, mode="bounce", range_random=[0.05, 0.12], range_clip=[0.05, 0.12],
                           increment=0.004, reset_every_x_seconds="inf"))
    b = _schedule_batch(E, prm)
    assert b.m_pole_table is not None and len(np.unique(b.m_pole_table)) > 2
    probe = _loop_optimizer(E, predictor_type="ODE", gru_fused=True)
    assert ControllerMass(b, probe.engine.mppi).varies and ControllerMass(b, probe.engine.mppi, network=True).kind == "none"
    probe.engine.close()
    _, launched = _run(E, False, batch=b, predictor_type="ODE", gru_fused=True)
    _, captured = _run(E, True, batch=b, predictor_type="ODE", gru_fused=True)
    assert np.abs(launched["Q"]).max() > 0.02
    for k in launched:
        assert np.array_equal(bits(launched[k]), bits(captured[k])), k
