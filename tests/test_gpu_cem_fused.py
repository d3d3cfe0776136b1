"""GPU: the fused CEM control step (cpmppi_cem_step: cem, cem-naive-grad, cem-grad-bharadhwaj) - against the entry points it fuses
composed in the test, against the numpy oracles one iteration at a time, its device step counter, the order at its edges, its
refusals, the captured closed loop and the controller seam.

Shapes: N = 40 (under one wave), 65 (one lane in the second wave), 200 (shipped: three waves and eight lanes), 256 (the full block);
H = 7 (odd: the Philox pair's tail) and 8, the shipped 200 x 35 once; E = 1 and 3; best_k = 1, N and in between; 1 and 3 iterations;
shift 0, 1, 2.

Bounds.  Against the composition everything is expected bit for bit (the kernel's statements are the staged kernels'), S_out
included: the composition's cost is cpmppi_rollout_cost_grad's S_out, the same plain forward sweep.  Against the oracles: the
sampler's bound of test_gpu_cem.py (the hardware normal's error scaled by stdev, plus the rounding of the fma), parity_util's cost
band, the elite set exactly, and mean / stdev at test_gpu_cem.py's refit bounds (1e-6 / 2e-6: float32 sums of at most 256 terms in
[-1, 1] against float64)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from oracle import philox_np as PH  # noqa: E402
import parity_util as PU  # noqa: E402
from test_gpu_cem import sampler_bound  # noqa: E402

f32 = np.float32
QBG_W = dict(ccrc_weight_up=3.0, ccrc_weight_down=3.0, dd_linear_weight_up=2.0, dd_linear_weight_down=2.0)
ADAM = dict(learning_rate=0.05, beta1=0.9, beta2=0.999, epsilon=1e-8, gradmax_clip=5.0)
SGD = dict(learning_rate=0.1, gradmax_clip=10.0)
SEED, ENV_OFFSET = 2 ** 40 + 7, 1000


def report(capsys, text):
    with capsys.disabled():
        print("\n[cem] " + text)


def make(E, N, H, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    cost = kw.get("cost_function_specification", "")
    if cost.endswith("_grad"):
        kw.setdefault("cost_weights", QBG_W)
    return MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, shift_mode="none", **kw))


def problem(E, H, seed):
    """States well inside the track, per-env target / L / previous input, a sampling distribution that clips a few samples."""
    rng = np.random.Generator(np.random.SFC64(seed))
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.6, 0.6), rng.uniform(-1.5, 1.5), rng.uniform(-0.04, 0.04),
                                           rng.uniform(-0.1, 0.1)) for _ in range(E)]).astype(f32)
    tp = rng.uniform(-0.03, 0.03, E).astype(f32)
    Lv = rng.uniform(0.3, 0.45, E).astype(f32)
    prev = rng.uniform(-0.3, 0.3, E).astype(f32)
    mean = rng.uniform(-0.3, 0.3, (E, H)).astype(f32)
    stdev = rng.uniform(0.2, 0.6, (E, H)).astype(f32)
    return s0, tp, np.ones(E, f32), Lv, prev, mean, stdev


def refine_kw(refine):
    return {} if refine is None else dict(refine=refine, **(SGD if refine == "sgd" else ADAM))


def fused(eng, s0, mean0, stdev0, tp, te, Lv, prev, iterations, best_k, stdev_min, refine, shift, offset, mid=0.0, **kw):
    E, H = mean0.shape
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    S, plan, smp = eng.empty(E, eng.N), eng.empty(E, H), eng.empty(E, eng.N, H)
    order = torch.empty(E, eng.N, dtype=torch.int32, device=mean.device)
    u, _, _, _, _ = eng.cem_step(s0, mean, stdev, tp, te, L=Lv, previous_input=prev, iterations=iterations, best_k=best_k,
                                 stdev_min=stdev_min, shift=shift, mean_fill=mid, stdev_fill=math.sqrt(0.5), seed=SEED, offset=offset,
                                 env_offset=ENV_OFFSET, S_out=S, plan_out=plan, samples_out=smp, order_out=order, **refine_kw(refine), **kw)
    torch.cuda.synchronize()
    return dict(mean=mean.cpu().numpy(), stdev=stdev.cpu().numpy(), control=u.cpu().numpy(), plan=plan.cpu().numpy(),
                S=S.cpu().numpy(), samples=smp.cpu().numpy(), order=order.cpu().numpy())


def composed(eng, s0, mean0, stdev0, tp, te, Lv, prev, iterations, best_k, stdev_min, refine, shift, offset, mid=0.0):
    """The same step from the existing entry points: cem_sample, (rollout_cost_grad + sgd_step / adam_step,) the cost from
    rollout_cost_grad, cem_update - `iterations` times - and the shift as optimizer_cem._shift makes it, by `shift` columns."""
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    m = v = None
    for i in range(iterations):
        Q = eng.cem_sample(mean, stdev, SEED, offset=offset + i, env_offset=ENV_OFFSET)
        if i == 0:
            first = Q.cpu().numpy()
        if refine is not None:
            _, G = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)
            if refine == "sgd":
                eng.sgd_step(Q, G, SGD["learning_rate"], SGD["gradmax_clip"])
            else:
                if m is None:
                    m, v = torch.zeros_like(Q), torch.zeros_like(Q)
                eng.adam_step(Q, G, m, v, i + 1, ADAM["learning_rate"], ADAM["beta1"], ADAM["beta2"], ADAM["epsilon"], ADAM["gradmax_clip"])
        S, _ = eng.rollout_cost_grad(s0, Q, tp, te, L=Lv, previous_input=prev)
        mean, stdev, el = eng.cem_update(S, Q, best_k, stdev_min, return_elites=True)
    out = dict(control=mean[:, 0].cpu().numpy(), plan=mean.cpu().numpy(), S=S.cpu().numpy(), samples=Q.cpu().numpy(),
               elites=el.cpu().numpy(), first=first)
    if shift:
        mean = torch.cat([mean[:, shift:], torch.full_like(mean[:, :shift], mid)], dim=1).contiguous()
        stdev = torch.cat([stdev[:, shift:], torch.full_like(stdev[:, :shift], math.sqrt(0.5))], dim=1).contiguous()
    out.update(mean=mean.cpu().numpy(), stdev=stdev.cpu().numpy())
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# (N, H, E, best_k, iterations, shift, cost, predictor, refine)
COMPOSED_CASES = [
    (40, 7, 1, 1, 1, 0, "quadratic_boundary_grad_minimal", "ODE_v0", None),
    (40, 7, 3, 40, 3, 1, "default", "ODE", None),
    (65, 8, 3, 20, 3, 2, "quadratic_boundary_grad", "ODE_v0", None),
    (200, 7, 3, 40, 3, 1, "quadratic_boundary_grad_minimal", "ODE", None),
    (256, 8, 1, 256, 1, 1, "default", "ODE_v0", None),
    (256, 7, 3, 64, 3, 0, "quadratic_boundary_grad", "ODE", None),
    (200, 35, 3, 40, 3, 1, "quadratic_boundary_grad_minimal", "ODE_v0", None),       # the shipped cem-tf shape
    (40, 7, 3, 10, 3, 1, "quadratic_boundary_grad_minimal", "ODE_v0", "sgd"),
    (65, 8, 3, 1, 3, 2, "default", "ODE", "sgd"),
    (200, 7, 1, 200, 1, 0, "quadratic_boundary_grad", "ODE", "sgd"),
    (40, 8, 3, 8, 3, 1, "quadratic_boundary_grad_minimal", "ODE", "adam"),
    (65, 7, 1, 65, 3, 0, "default", "ODE_v0", "adam"),
    (256, 8, 3, 32, 3, 2, "quadratic_boundary_grad", "ODE_v0", "adam"),
]


@pytest.mark.parametrize("N,H,E,best_k,iterations,shift,cost,predictor,refine", COMPOSED_CASES)
def test_fused_equals_the_composed_entry_points(N, H, E, best_k, iterations, shift, cost, predictor, refine, capsys):
    """Same state, distribution, per-env L, target and previous input (and per-env pole masses under ODE): mean, stdev, control,
    plan, samples_out, S_out and the elite order of the one call against the existing entry points run in sequence - bit for bit."""
    eng = make(E, N, H, cost_function_specification=cost, predictor_type=predictor, action_low=-0.9, action_high=0.8)
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 100 + N + H)
    if predictor == "ODE":
        eng.set_pole_mass_rows(np.asarray([0.080, 0.087, 0.095], f32)[:E])
    args = (eng, s0, mean0, stdev0, tp, te, Lv, prev, iterations, best_k, 0.05, refine, shift, 2 ** 33 + 5)
    ref = composed(*args, mid=-0.05)
    got = fused(*args, mid=-0.05)
    eng.close()
    dS = float(np.max(np.abs(got["S"] - ref["S"]) / np.abs(ref["S"])))
    report(capsys, f"fused vs composed {cost} / {predictor} / {refine} N {N} H {H} E {E} k {best_k} it {iterations} shift {shift}: "
                   f"S max rel {dS:.2e}; " + ", ".join(f"{k} {int((bits(got[k]) != bits(ref[k])).sum())} words differ"
                                                       for k in ("samples", "mean", "stdev", "control", "plan")))
    assert (ref["first"] == f32(-0.9)).any() and (ref["first"] == f32(0.8)).any()          # the first draw clips at either limit
    assert np.array_equal(got["order"][:, :best_k], ref["elites"])
    assert np.array_equal(np.sort(got["order"], axis=1), np.tile(np.arange(N), (E, 1)))    # a permutation of the rows
    for k in ("samples", "S", "mean", "stdev", "control", "plan"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    if shift:
        assert (got["mean"][:, H - shift:] == f32(-0.05)).all() and (got["stdev"][:, H - shift:] == f32(math.sqrt(0.5))).all()
    assert np.array_equal(got["control"], got["plan"][:, 0])


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,E,best_k", [(200, 7, 3, 40), (65, 8, 1, 1)])
def test_one_iteration_per_call_against_the_oracles(N, H, E, best_k, capsys):
    """Three calls of one iteration each (shift 0, host offsets o, o + 1, o + 2), every one checked on its own: samples_out against
    philox_np from the distribution the call started with, S_out against the numpy predictor + cost on the device's own samples, the
    elite set exactly and mean / stdev to rounding from oracle_np.cem_update on the device's own S_out and samples_out.  Then one
    call of three iterations from the same start equals the chain bit for bit."""
    lo, hi, o, stdev_min = -0.5, 0.8, 2 ** 33 + 11, 0.01
    eng = make(E, N, H, action_low=lo, action_high=hi)
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 7 + N)
    mean, stdev = mean0, stdev0
    for i in range(3):
        got = fused(eng, s0, mean, stdev, tp, te, Lv, None, 1, best_k, stdev_min, None, 0, o + i)
        ref = PH.cem_samples(mean, stdev, SEED, o + i, ENV_OFFSET, N, lo, hi)
        err = np.abs(got["samples"].astype(np.float64) - ref)
        report(capsys, f"call {i} {E}x{N}x{H}: worst |samples - philox| / bound {np.max(err / sampler_bound(stdev)):.3f}")
        assert np.all(err <= sampler_bound(stdev)), (i, err.max())
        if i == 0:                                                           # (the refit narrows the later draws)
            assert got["samples"].min() == f32(lo) and got["samples"].max() == f32(hi)
        for e in range(E):
            Qe = got["samples"][e]
            traj = O.predict_core(s0[e], Qe, L=Lv[e])
            ref_a = O.trajectory_cost(O.COST_QBGM, traj, Qe, tp[e], f32(1.0))
            ref_b = O.trajectory_cost(O.COST_QBGM, O.predict_core(s0[e], Qe, L=Lv[e], mode="f64sub"), Qe, tp[e], f32(1.0))
            PU.assert_costs(got["S"][e], ref_a, ref_b, PU.flag_discontinuities(traj), f"call {i} env {e} costs")
            mr, sr, idx = O.cem_update(got["S"][e], Qe, best_k, stdev_min)
            assert np.array_equal(got["order"][e, :best_k], idx), (i, e)
            np.testing.assert_allclose(got["mean"][e], mr, atol=1e-6, rtol=0)
            np.testing.assert_allclose(got["stdev"][e], sr, atol=2e-6, rtol=0)
        assert np.array_equal(got["control"], got["mean"][:, 0]) and np.array_equal(got["plan"], got["mean"])
        mean, stdev = got["mean"], got["stdev"]
    once = fused(eng, s0, mean0, stdev0, tp, te, Lv, None, 3, best_k, stdev_min, None, 0, o)
    for k in ("mean", "stdev", "control", "plan", "S", "samples", "order"):
        assert np.array_equal(bits(once[k]), bits(got[k])), k
    assert not np.array_equal(once["mean"], mean0)
    eng.close()


@pytest.mark.parametrize("refine", [None, "adam"])
def test_device_counter_equals_the_host_offsets(refine):
    """Five control steps with the step counter on the device against the same steps with the host's offset c * iterations: mean,
    stdev and control bitwise equal after every step; the word ends at 5."""
    E, N, H, iters, best_k = 3, 65, 7, 3, 12
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 51)
    kw = dict(iterations=iters, best_k=best_k, stdev_min=0.02, shift=1, stdev_fill=math.sqrt(0.5), seed=SEED, **refine_kw(refine))
    bufs = [[eng.tensor(mean0.copy()), eng.tensor(stdev0.copy()), eng.zeros(E)] for _ in range(2)]
    counter = torch.zeros(1, dtype=torch.int64, device=bufs[0][0].device)
    s = eng.tensor(s0)
    for c in range(5):
        mh, sh, uh = bufs[0]
        eng.cem_step(s, mh, sh, tp, te, L=Lv, previous_input=uh, offset=4 + c * iters, Q_out=uh, **kw)
        md, sd, ud = bufs[1]
        eng.cem_step(s, md, sd, tp, te, L=Lv, previous_input=ud, offset=4, count_dev=counter, Q_out=ud, **kw)
        for h, d in zip(bufs[0], bufs[1]):
            assert torch.equal(h, d), f"step {c}"
        assert int(counter.item()) == c + 1
        eng.plant_advance(s, uh, L=Lv, n_substeps=10)                        # the next step sees another state
    assert int(counter.item()) == 5 and not torch.equal(bufs[0][0], eng.tensor(mean0))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,best_k", [(65, 65), (200, 40)])
@pytest.mark.parametrize("kind,weights,limit", [("+inf", dict(cc_weight_up=3e38), 1.0), ("-inf", dict(cc_weight_up=-3e38), 1.0),
                                                ("nan", dict(R=3e38, cc_weight_up=0.0), 2.0)])
def test_order_with_nan_inf_and_ties(kind, weights, limit, N, best_k):
    """Costs a ranking can get wrong, forced through the inputs.  Env 0, by a cost weight at the edge of float32: the control cost
    u^2 R cc_weight summed over the horizon overflows for the larger plans (+inf, or -inf with the weight negative); with R = 3e38,
    cc_weight = 0 and limits of +-2 a plan with a control beyond 1.07 costs inf * 0 = NaN and the others stay finite.  Env 1 starts
    from a NaN state (every cost NaN: all ties), env 2 samples with stdev 0 (every cost equal).  The order is the stable argsort of
    the device's own costs - oracle_np.cem_update's: NaN last, ties by index - and no elite indexes a row >= N."""
    E, H = 3, 7
    eng = make(E, N, H, cost_weights=weights, action_low=-limit, action_high=limit)
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 61)
    s0[1, O.ANGLED_IDX] = np.nan
    stdev0[2] = 0.0
    got = fused(eng, s0, mean0, stdev0, tp, te, Lv, None, 1, best_k, 0.01, None, 1, 3)
    eng.close()
    S = got["S"]
    assert 0.05 < np.isfinite(S[0]).mean() < 0.95                            # a mix in env 0 ...
    assert {"+inf": np.isposinf, "-inf": np.isneginf, "nan": np.isnan}[kind](S[0][~np.isfinite(S[0])]).all()
    assert np.isnan(S[1]).all() and np.isfinite(S[2, 0]) and np.all(bits(S[2]) == bits(S[2])[0])
    assert got["order"].min() >= 0 and got["order"].max() < N
    for e in range(E):
        assert np.array_equal(got["order"][e], np.argsort(S[e], kind="stable")), e
        assert np.array_equal(got["order"][e, :best_k], O.cem_update(S[e], got["samples"][e], best_k, 0.01)[2]), e
    assert np.array_equal(got["order"][1], np.arange(N)) and np.array_equal(got["order"][2], np.arange(N))
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["stdev"]).all()        # (the samples are finite whatever they cost)
    if kind != "-inf" and best_k < N:
        assert np.isfinite(S[0, got["order"][0, :best_k]]).all() or np.isfinite(S[0]).sum() < best_k


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kw,refine", [
    ("legacy cost", dict(cost_function_specification="legacy_mppi_cartpole"), None),
    ("quadratic_boundary", dict(cost_function_specification="quadratic_boundary"), None),
    ("PRECISE math", dict(math_mode="precise"), None),
    ("S beyond the LDS budget, refining", dict(intermediate_steps=101), "sgd"),
    ("N beyond one workgroup", dict(num_rollouts=320), None)])
def test_refusals_about_the_handle(what, kw, refine):
    """sweep_check_handle's and sweep_check_shape's lists: refused with a text, by the step and by the reserve, and the handle goes on serving what it
    supports.  Without refinement there is no sub-state buffer: the same S is accepted."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, H = 2, 5
    N = kw.pop("num_rollouts", 24)
    eng = make(E, N, H, **kw)
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 9)
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    step = dict(iterations=2, best_k=4, stdev_min=0.01, **refine_kw(refine))
    for _ in range(2):
        with pytest.raises(CpmppiError, match="cpmppi_cem_step: "):
            eng.cem_step(s0, mean, stdev, tp, te, L=Lv, **step)
        with pytest.raises(CpmppiError, match="cpmppi_cem_reserve: "):
            eng.cem_reserve(refine=refine)
    assert np.array_equal(mean.cpu().numpy(), mean0) and np.array_equal(stdev.cpu().numpy(), stdev0)
    assert np.isfinite(eng.cem_sample(mean, stdev, 1).cpu().numpy()).all()
    if refine is not None:
        eng.cem_reserve()
        u = eng.cem_step(s0, mean, stdev, tp, te, L=Lv, iterations=2, best_k=4, stdev_min=0.01)[0]
        torch.cuda.synchronize()
        assert np.isfinite(u.cpu().numpy()).all() and not np.array_equal(mean.cpu().numpy(), mean0)
    eng.close()


def test_refusals_about_the_arguments_leave_the_handle_usable():
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 3, 40, 7
    eng = make(E, N, H, predictor_type="ODE")
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 10)
    mean, stdev = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    ok = dict(iterations=2, best_k=10, stdev_min=0.01, shift=1, **refine_kw("adam"))

    def call(**over):
        return eng.cem_step(s0, mean, stdev, tp, te, L=Lv, previous_input=prev, **dict(ok, **over))

    for over, text in ((dict(best_k=0), "best_k"), (dict(best_k=N + 1), "best_k"), (dict(iterations=0), "iterations"),
                       (dict(shift=H + 1), "shift")):
        with pytest.raises(CpmppiError, match="cpmppi_cem_step: .*" + text):
            call(**over)
    with pytest.raises(ValueError, match="refine"):
        call(refine="newton")
    # a NULL among the required pointers, a misaligned one, an unknown refine kind: through the argument block itself
    prep = eng.prepare_cem_step(s0, mean, stdev, tp, te, L=Lv, previous_input=prev, **ok)
    for field in ("s0", "target_position", "target_equilibrium", "mean", "stdev", "Q_out"):
        keep = getattr(prep.args, field)
        setattr(prep.args, field, None)
        with pytest.raises(CpmppiError, match="cpmppi_cem_step: null pointer"):
            prep.run()
        setattr(prep.args, field, keep + 2)
        with pytest.raises(CpmppiError, match="cpmppi_cem_step: misaligned pointer"):
            prep.run()
        setattr(prep.args, field, keep)
    prep.args.refine = 3
    with pytest.raises(CpmppiError, match="cpmppi_cem_step: unknown refine kind"):
        prep.run()
    prep.args.refine = 2
    counter = torch.zeros(2, dtype=torch.int64, device=mean.device)
    prep.args.count_dev = counter.data_ptr() + 4
    with pytest.raises(CpmppiError, match="cpmppi_cem_step: misaligned pointer"):
        prep.run()
    prep.args.count_dev = None
    assert np.array_equal(mean.cpu().numpy(), mean0)
    # fewer pole masses registered than envs in the call
    eng.set_pole_mass_rows(eng.tensor(np.full(2, 0.09, f32)))
    with pytest.raises(CpmppiError, match="cpmppi_cem_step: 3 rows"):
        call()
    eng.set_pole_mass_rows(None)
    # ... and a valid call afterwards succeeds
    u = call()[0]
    torch.cuda.synchronize()
    assert np.isfinite(u.cpu().numpy()).all() and not np.array_equal(mean.cpu().numpy(), mean0)
    eng.close()


@pytest.mark.parametrize("refine", [None, "sgd"])
def test_capture_without_a_reserved_workspace_is_refused_and_the_capture_survives(refine):
    """On a capturing stream the step must not allocate: without cpmppi_cem_reserve it is refused with a text before any HIP call
    that a capture forbids - the capture goes on, ends and replays; after the reserve the same step is captured and replayed."""
    from cartpolesimulation_amd._lib import CpmppiError
    E, N, H = 2, 40, 7
    eng = make(E, N, H)
    s0, tp, te, Lv, prev, mean0, stdev0 = problem(E, H, 12)
    s, tpd, ted, Ld = eng.tensor(s0), eng.tensor(tp), eng.tensor(te), eng.tensor(Lv)
    mean, stdev, u = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy()), eng.zeros(E)
    counter = torch.zeros(1, dtype=torch.int64, device=mean.device)
    marker = eng.zeros(4)
    step = dict(iterations=2, best_k=10, stdev_min=0.01, shift=1, stdev_fill=math.sqrt(0.5), seed=SEED, offset=3, **refine_kw(refine))
    prep = eng.prepare_cem_step(s, mean, stdev, tpd, ted, L=Ld, count_dev=counter, Q_out=u, **step)
    side = torch.cuda.Stream(device=mean.device)
    side.wait_stream(torch.cuda.current_stream(mean.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(CpmppiError, match="cpmppi_cem_step: the stream is being captured"):
                prep.run()
            marker.add_(1.0)
    torch.cuda.current_stream(mean.device).wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert marker.cpu().numpy().tolist() == [1.0] * 4 and np.array_equal(mean.cpu().numpy(), mean0) and int(counter.item()) == 0
    # reserved: captured, replayed twice = two launched steps
    eng.cem_reserve(refine=refine)
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(mean.device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            prep.run()
    torch.cuda.current_stream(mean.device).wait_stream(side)
    g2.replay()
    g2.replay()
    torch.cuda.synchronize()
    mr, sr = eng.tensor(mean0.copy()), eng.tensor(stdev0.copy())
    for c in range(2):
        ur = eng.cem_step(s, mr, sr, tpd, ted, L=Ld, **dict(step, offset=3 + 2 * c))[0]
    torch.cuda.synchronize()
    assert int(counter.item()) == 2 and torch.equal(mean, mr) and torch.equal(stdev, sr) and torch.equal(u, ur)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _schedule_batch(E):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=31, length_of_experiment=0.2, keep_target_equilibrium_x_seconds_up=0.1, turning_points=dict(track_relative_complexity=12),
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    return SC.RandomExperimentSetter(cfg).draw(E, 83, L=np.linspace(0.3, 0.45, E).astype(f32))


def _cem(name, E, fused, **over):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    c = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), num_envs=E,
                       config=dict(seed=9, fused=fused, num_rollouts=40, mpc_horizon=7, cem_best_k=8, **over))
    c.configure(name, predictor_specification="ODE")
    return c.optimizer


@pytest.mark.parametrize("name", ["cem", "cem-naive-grad", "cem-grad-bharadhwaj"])
def test_captured_loop_equals_the_launched_loop(name):
    """run_schedule(graph=True, steps_per_graph=5) with a fused CEM optimizer against graph=False with the same configuration: three
    experiments of 0.2 s at 40 x 7 - recorded states, controls and recording rows bitwise equal.  A staged one is still refused."""
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    E, outs = 3, []
    for graph in (False, True):
        b = _schedule_batch(E)
        opt = _cem(name, E, True)
        assert opt.fused and opt.num_rollouts == 40 and opt.mpc_horizon == 7
        res = BatchedCartPoleExperiment(opt.engine, seed=0).run_schedule(b, graph=graph, steps_per_graph=5, optimizer=opt)
        torch.cuda.synchronize()
        outs.append({k: res[k].cpu().numpy() for k in ("states", "dd", "Q", "final_state")})
        opt.engine.close()
    assert b.n_periods == 10 and outs[0]["Q"].shape == (11, E) and np.abs(outs[0]["Q"]).max() > 0.02
    assert np.isfinite(outs[0]["states"]).all()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    if name == "cem":
        staged_opt = _cem(name, E, False)
        with pytest.raises(ValueError, match="paced by the host"):
            BatchedCartPoleExperiment(staged_opt.engine, seed=0).run_schedule(_schedule_batch(E), graph=True, optimizer=staged_opt)
        staged_opt.engine.close()


def test_fused_cem_through_the_controller_seam():
    """controller_mpc(config=dict(fused=True)).configure("cem") in closed loop with the device plant holds a pole upright for 60 steps
    (the configuration and the bound of test_optimizer_cem_improves_and_controls); one library call per step."""
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0},
                          (np.array([-1.0], f32), np.array([1.0], f32)),
                          config=dict(num_rollouts=256, mpc_horizon=35, seed=1, cost_function_specification="default", fused=True))
    ctrl.configure("cem")
    opt = ctrl.optimizer
    assert opt.optimizer_name == "cem" and opt.fused
    eng = opt.engine
    st = eng.tensor(O.create_cartpole_state(0.1, 0.0, 0.0, 0.0)[None].copy())
    for t in range(60):
        q = ctrl.step(st.cpu().numpy()[0], time=0.02 * t)
        assert q.shape == (1,) and abs(float(q[0])) <= 1.0
        eng.plant_advance(st, q.astype(f32), n_substeps=10, dt_sim=0.002)
    fin = st.cpu().numpy()[0]
    assert abs(fin[0]) < 0.3 and abs(fin[4]) < 0.198
    assert opt.step_counter == 60 * opt.cem_outer_it
    assert float(opt.stdev[0, -1]) == pytest.approx(np.sqrt(0.5)) and float(opt.dist_mue[0, -1]) == 0.0
    eng.close()
