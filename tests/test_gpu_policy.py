"""GPU: fine-tuning the neural imitator on the task cost - cpmppi_dense_policy_loss_grad (dense_policy_kernel, dense_finalize_kernel):
loss, per-state costs and the gradient with respect to the 1345 parameters against tests/policy_ref.py (float64 torch autograd of
the closed loop; pinned in tests/test_policy_host.py), the branches, the pins to the existing kernels, the bits, the refusals.

Bands, the project's own from tests/test_gpu_grad.py: loss and cost_out rtol 5e-4; gradient max |g - g_ref| / max |g_ref| <= 2e-3,
the band of entries that cannot be separated from a branch - the batch sum mixes all samples.  PRECONDITION, asserted before the
device result is looked at: the reference gradient with every start state scaled by 1 + 1e-6 (a float32 rounding) moves by at most
2e-4 of its scale, a tenth of the band - a case whose gradient is not determined to that by its inputs says nothing about the
kernel.  The sensitivity grows fast with the horizon, so H <= 8; the seeds were chosen on the CPU so that the precondition holds.

Shapes: B = 1, 63, 65, 130 (lane tail, tile edge, more than one workgroup = partial row), H = 1, 3, 8, both predictors x both costs,
S = 10 and 2, sum and mean."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402
import policy_ref as P  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

f32 = np.float32
LOSS_RTOL, GRAD_BAND, PRECONDITION = 5e-4, 2e-3, 2e-4
COSTS = {"quadratic_boundary_grad_minimal": O.COST_QBGM, "default": O.COST_DEFAULT}
Q, DF = "quadratic_boundary_grad_minimal", "default"
# (B, H, predictor, cost, S, reduce, model)
CASES = [(130, 8, "ODE_v0", Q, 10, "sum", "random"), (130, 8, "ODE", Q, 10, "sum", "random"),
         (130, 8, "ODE_v0", DF, 10, "sum", "golden"), (130, 8, "ODE", DF, 10, "mean", "golden"),
         (130, 8, "ODE_v0", Q, 10, "mean", "golden"), (130, 8, "ODE", DF, 10, "sum", "random"),
         (1, 1, "ODE_v0", Q, 10, "sum", "random"), (63, 3, "ODE", Q, 10, "mean", "golden"), (65, 8, "ODE_v0", DF, 2, "sum", "random"),
         (130, 3, "ODE_v0", Q, 2, "mean", "golden"), (65, 1, "ODE", DF, 2, "sum", "golden"), (1, 8, "ODE", Q, 2, "sum", "random"),
         (63, 3, "ODE_v0", DF, 10, "sum", "random")]


def report(capsys, text):
    with capsys.disabled():
        print("\n[policy] " + text)


def bits(x, dtype=f32):
    return np.ascontiguousarray(np.asarray(x, dtype)).view(np.uint32 if dtype == f32 else np.uint64)


def np_(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "golden":
        return D.golden_model()
    if name == "clipping":                                          # weights at scale 0.3 and out_scale 3: about two steps in three clip
        return {**D.random_model(33, scale=0.3, norm=True), "out_scale": np.array([3.0], f32)}
    return D.random_model(31, norm=True)


def new_engine(m=None, H=8, predictor="ODE_v0", cost=Q, S=10, reduce="sum", E=1, N=32, **kw):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, predictor_type=predictor, cost_function_specification=cost,
                                   intermediate_steps=S, horizon_reduce=reduce, shift_mode="none", **kw))
    if m is not None:
        eng.set_dense(m)
    return eng


@functools.lru_cache(maxsize=None)
def problem(B, seed=5, edge=False):
    """B start states as ONE recording of B rows [1,B,6] with per-row targets, a window per row - in a shuffled order."""
    s0, tp, te = P.start_states(seed, B)
    if edge:                                                        # near the track's end, moving outward: the bounce, the boundary term
        sgn = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(f32)
        s0[:, 4], s0[:, 5] = sgn * f32(0.19) + f32(0.003) * s0[:, 4], sgn * (f32(0.3) + np.abs(s0[:, 5]))
    order = np.random.default_rng(seed).permutation(B)
    windows = np.stack([np.zeros(B, np.int64), order], axis=1)
    return s0, tp, te, windows, order


@functools.lru_cache(maxsize=None)
def reference(B, H, predictor, cost, S, reduce, name, edge=False):
    """-> (loss, gradient, J [B], u [B,H], q [B,H]) of the float64 reference in the windows' order, and the precondition's figure."""
    s0, tp, te, _, order = problem(B, edge=edge)
    kw = dict(cost_id=COSTS[cost], integrator=predictor, S=S, horizon_reduce=reduce)
    s, a, b = s0[order], tp[order], te[order]
    loss, g, J, u, q = P.loss_and_grad(model(name), s, a, b, H, **kw)
    _, g2, _, _, _ = P.loss_and_grad(model(name), s.astype(np.float64) * (1.0 + 1e-6), a, b, H, **kw)
    return loss, g, J, u, q, float(np.abs(g2 - g).max() / np.abs(g).max())


def device_call(eng, B, H, edge=False, grad=True, **out):
    s0, tp, te, windows, _ = problem(B, edge=edge)
    return eng.dense_policy_loss_grad(eng.tensor(s0[None]), eng.tensor(tp[None]), eng.tensor(te[None]), windows, H, grad=grad, **out)


def check_against_reference(capsys, B, H, predictor, cost, S, reduce, name, edge=False):
    loss64, g64, J64, u64, q64, moved = reference(B, H, predictor, cost, S, reduce, name, edge)
    assert moved <= PRECONDITION, f"the case does not determine its gradient: {moved:.2e}"
    eng = new_engine(model(name), H, predictor, cost, S, reduce)
    cost_out, Q_out = eng.empty(B), eng.empty(B, H)
    loss, grad = device_call(eng, B, H, edge, cost_out=cost_out, Q_out=Q_out)
    loss, grad, J, u = float(np_(loss)[0]), np_(grad).astype(np.float64), np_(cost_out), np_(Q_out)
    eng.close()
    g_err = float(np.abs(grad - g64).max() / np.abs(g64).max())
    report(capsys, f"B={B} H={H} {predictor} {cost} S={S} {reduce} {name}{' edge' if edge else ''}: loss rel {abs(loss - loss64) / abs(loss64):.2e}, "
                   f"cost_out rel {np.abs(J / J64 - 1).max():.2e}, gradient {g_err:.2e} of max|g| = {np.abs(g64).max():.3e} "
                   f"(precondition {moved:.1e}); clipped {np.mean(np.abs(q64) > 1):.2f}")
    inside = np.abs(q64) < 1 - 1e-5
    assert np.abs(u - u64)[inside].max(initial=0.0) <= 1e-4 and (np.abs(u) <= 1).all()
    np.testing.assert_allclose(J, J64, rtol=LOSS_RTOL)
    assert abs(loss - loss64) <= LOSS_RTOL * abs(loss64)
    assert g_err <= GRAD_BAND
    return u, q64


# ---------------------------------------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("B,H,predictor,cost,S,reduce,name", CASES)
def test_loss_and_gradient_against_float64_autograd(B, H, predictor, cost, S, reduce, name, capsys):
    check_against_reference(capsys, B, H, predictor, cost, S, reduce, name)


@pytest.mark.parametrize("cost", [Q, DF])
def test_the_bounce_inside_the_horizon(cost, capsys):
    """predictor_ODE_v0 from |position| ~ 0.19 moving outward: every state bounces inside the horizon (judged on the reference's
    own trajectory first), and quadratic_boundary_grad_minimal's boundary term is active."""
    B, H = 65, 8
    s0, tp, te, _, _ = problem(B, edge=True)
    assert (np.abs(s0[:, 4]) > 0.85 * float(O.DEFAULT_PARAMS.TrackHalfLength)).all() and (s0[:, 4] * s0[:, 5] > 0).all()
    t_hit = (float(O.DEFAULT_PARAMS.TrackHalfLength) - np.abs(s0[:, 4])) / np.abs(s0[:, 5])
    assert (t_hit < 0.5 * H * 0.02).all()                           # (at the start speed; the control's share of u_max moves it little)
    check_against_reference(capsys, B, H, "ODE_v0", cost, 10, "sum", "random", edge=True)


def test_a_stated_share_of_the_steps_clip(capsys):
    """out_scale = 3: at least a tenth of the steps clip and not all (asserted from Q_out, so the case cannot go vacuous); a
    clipped step passes nothing back through the net, the others do."""
    u, q64 = check_against_reference(capsys, 130, 8, "ODE", Q, 10, "sum", "clipping")
    share = float(np.mean(np.abs(u) == 1.0))
    assert 0.1 <= share < 1.0, share
    assert abs(share - float(np.mean(np.abs(q64) > 1))) < 0.02


# ---------------------------------------------------------------------------------------------- pinned to the existing kernels
@pytest.mark.parametrize("predictor,cost,reduce", [("ODE_v0", Q, "sum"), ("ODE", DF, "mean"), ("ODE", Q, "sum"), ("ODE_v0", DF, "sum")])
def test_costs_and_first_controls_are_the_existing_kernels_bits(predictor, cost, reduce):
    """cost_out = what cpmppi_rollout_cost_grad returns for the plan Q_out[b,:] from s_0, bit for bit: one forward body (the plan is
    already inside the limits, so that kernel's clamp changes nothing).  Q_out[:,0] = cpmppi_dense_control on the start states, bit
    for bit."""
    B, H = 130, 8
    s0, tp, te, windows, order = problem(B)
    eng = new_engine(model("random"), H, predictor, cost, 10, reduce, E=B, N=32)
    cost_out, Q_out = eng.empty(B), eng.empty(B, H)
    device_call(eng, B, H, grad=False, cost_out=cost_out, Q_out=Q_out)
    s, a, b = s0[order], tp[order], te[order]
    plans = Q_out[:, None, :].expand(B, 32, H).contiguous()
    S, _ = eng.rollout_cost_grad(s, plans, a, b)
    assert np.array_equal(bits(np_(S)[:, 0]), bits(np_(cost_out)))
    first, _ = eng.dense_control(eng.tensor(s), eng.tensor(a), eng.tensor(b))
    assert np.array_equal(bits(np_(first)), bits(np_(Q_out)[:, 0]))
    eng.close()


def test_with_w1_zero_the_bias_gradient_is_the_plan_gradient_s_sum(capsys):
    """w1 = 0: the policy ignores the state, every control is the same number, and d loss / d b3 = (out_scale / B) sum_b sum_k G[b,k]
    with G from cpmppi_rollout_cost_grad for those plans.  Band: every G[b,k] carries up to 2e-3 of its plan's gradient scale
    (tests/test_gpu_grad.py), so the sum is held to 2e-3 of (out_scale / B) sum_b H max_k |G[b,k]|.  d loss / d w1 is NOT zero (the
    reference pins it in the cases above); here only: it is finite and some of it is not zero."""
    B, H = 65, 8
    m = {**model("random"), "w1": np.zeros((32, 7), f32)}
    s0, tp, te, windows, order = problem(B)
    eng = new_engine(m, H, "ODE_v0", Q, 10, "sum", E=B, N=32)
    Q_out = eng.empty(B, H)
    _, grad = device_call(eng, B, H, Q_out=Q_out)
    u = np_(Q_out)
    assert (u == u[0, 0]).all() and abs(u[0, 0]) < 1
    _, G = eng.rollout_cost_grad(s0[order], Q_out[:, None, :].expand(B, 32, H).contiguous(), tp[order], te[order])
    G = np_(G)[:, 0, :].astype(np.float64)
    A = float(m["out_scale"][0])
    want, scale = A / B * G.sum(), A / B * H * np.abs(G).max(axis=1).sum()
    g = D.unflatten(np_(grad))
    report(capsys, f"w1 = 0: d loss / d b3 {g['b3'][0]:.6e}, from the plan gradients {want:.6e} ({abs(g['b3'][0] - want) / scale:.1e} of scale)")
    assert abs(g["b3"][0] - want) <= GRAD_BAND * scale
    assert np.isfinite(g["w1"]).all() and g["w1"].any()
    eng.close()


# ---------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("predictor,cost", [("ODE", Q), ("ODE_v0", Q), ("ODE", DF), ("ODE_v0", DF)])
def test_bits_loss_only_repeat_and_canaries(predictor, cost):
    """Every predictor x cost pair is two instantiations of the forward loop (with and without the gradient): their losses agree
    bit for bit in each."""
    B, H = 130, 8
    eng = new_engine(model("random"), H, predictor, cost)
    PAD = 16
    bufs = {k: torch.full((n + 2 * PAD,), -7.0, device=eng.device) for k, n in (("grad", D.NPAR), ("cost", B), ("Q", B * H))}
    view = lambda k, *shape: bufs[k][PAD:-PAD].view(*shape)  # noqa: E731
    loss, grad = device_call(eng, B, H, grad_out=view("grad", D.NPAR), cost_out=view("cost", B), Q_out=view("Q", B, H))
    loss, grad = np_(loss).copy(), np_(grad).copy()
    for k, b in bufs.items():
        b = np_(b)
        assert (b[:PAD] == -7.0).all() and (b[-PAD:] == -7.0).all() and not (b[PAD:-PAD] == -7.0).any(), k
    only, none = device_call(eng, B, H, grad=False)
    assert none is None and np.array_equal(bits(np_(only), np.float64), bits(loss, np.float64))
    loss2, grad2 = device_call(eng, B, H)
    assert np.array_equal(bits(np_(loss2), np.float64), bits(loss, np.float64)) and np.array_equal(bits(np_(grad2)), bits(grad))
    eng.close()


def test_canaries_behind_the_check_points():
    """The check-points are the handle's own workspace: reserved for more start states and steps than the call has (194 and 9
    against 130 and 8: another row of lanes, another control step), filled with a canary through the test aid.  The call writes
    exactly its own [8][6][3 x 64] floats - every lane of its three waves, the 62 beyond the batch included - and nothing behind."""
    from cartpolesimulation_amd._lib import CpmppiError
    B, H = 130, 8
    eng = new_engine(model("random"), H, "ODE_v0", Q)
    assert eng.dense_policy_ckpt().size == 0
    eng.dense_policy_reserve(194, 9)
    assert eng.dense_policy_ckpt(fill=-7.0).size == 9 * 6 * 4 * 64
    used = H * 6 * 3 * 64
    only, _ = device_call(eng, B, H, grad=False)                    # the loss alone writes no check-point
    assert (eng.dense_policy_ckpt() == -7.0).all()
    loss, _ = device_call(eng, B, H)
    ckpt = eng.dense_policy_ckpt()
    assert not (ckpt[:used] == -7.0).any() and np.isfinite(ckpt[:used]).all() and (ckpt[used:] == -7.0).all()
    s0, _, _, _, order = problem(B)
    assert np.array_equal(bits(ckpt[:6 * 192].reshape(6, 192)[:, :B].T), bits(s0[order]))      # step 0's are the start states
    assert np.array_equal(bits(np_(only), np.float64), bits(np_(loss), np.float64))
    with pytest.raises(CpmppiError, match="cpmppi_dense_policy_ckpt_copy: .* are reserved"):
        eng._check(eng.lib.cpmppi_dense_policy_ckpt_copy(eng._h, ckpt.ctypes.data_as(C.POINTER(C.c_float)), ckpt.size + 1, 0))
    eng.close()


def test_a_small_call_after_a_larger_one_equals_a_fresh_handle():
    eng, fresh = new_engine(model("random"), 8, "ODE_v0", DF), new_engine(model("random"), 8, "ODE_v0", DF)
    device_call(eng, 130, 8)
    a, b = device_call(eng, 63, 3), device_call(fresh, 63, 3)
    assert np.array_equal(bits(np_(a[0]), np.float64), bits(np_(b[0]), np.float64)) and np.array_equal(bits(np_(a[1])), bits(np_(b[1])))
    eng.close()
    fresh.close()


def capture(eng, call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    fixed = eng.use_stream(side)
    try:
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            call.run()
    finally:
        eng.use_stream(fixed)
    torch.cuda.current_stream().wait_stream(side)
    return graph


def test_captured_equals_launched_and_a_capture_that_would_allocate_is_refused():
    from cartpolesimulation_amd._lib import CpmppiError
    B, H = 130, 8
    s0, tp, te, windows, _ = problem(B)
    results = []
    for captured in (False, True):
        eng = new_engine(model("random"), H, "ODE_v0", Q)
        dev = (eng.tensor(s0[None]), eng.tensor(tp[None]), eng.tensor(te[None]))
        call = eng.prepare_dense_policy_loss_grad(*dev, windows, H)
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            fixed = eng.use_stream(side)
            try:
                with torch.cuda.stream(side), torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                    with pytest.raises(CpmppiError, match="cpmppi_dense_policy_loss_grad: the stream is being captured.*cpmppi_dense_policy_reserve"):
                        call.run()
            finally:
                eng.use_stream(fixed)
            torch.cuda.current_stream().wait_stream(side)
            eng.dense_policy_reserve(B, H)
            capture(eng, call).replay()
        else:
            call.run()
        results.append((np_(call.result[0]).copy(), np_(call.result[1]).copy()))
        eng.close()
    (la, ga), (lb, gb) = results
    assert np.array_equal(bits(la, np.float64), bits(lb, np.float64)) and np.array_equal(bits(ga), bits(gb))


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_refusals_by_name_launch_nothing_and_change_nothing(golden_dir):
    from cartpolesimulation_amd import _lib as L
    B, H = 13, 3
    s0, tp, te, windows, _ = problem(B)
    w_host = np.ascontiguousarray(windows, np.uint32)

    def setup(eng):
        t = dict(s=eng.tensor(s0[None]), tp=eng.tensor(tp[None]), te=eng.tensor(te[None]),
                 w=torch.as_tensor(w_host.astype(np.int32)).to(eng.device),
                 loss=torch.full((1,), -7.0, dtype=torch.float64, device=eng.device), grad=torch.full((D.NPAR,), -7.0, device=eng.device),
                 cost=torch.full((B,), -7.0, device=eng.device), Q=torch.full((B, H), -7.0, device=eng.device))

        def args(**kw):
            a = L.cpmppi_dense_policy_args()
            a.B, a.R, a.T, a.horizon = B, 1, B, H
            a.states, a.target_position, a.target_equilibrium = t["s"].data_ptr(), t["tp"].data_ptr(), t["te"].data_ptr()
            a.windows, a.windows_host, a.loss_out, a.grad_out = t["w"].data_ptr(), w_host.ctypes.data, t["loss"].data_ptr(), t["grad"].data_ptr()
            a.cost_out, a.Q_out = t["cost"].data_ptr(), t["Q"].data_ptr()
            for k, v in kw.items():
                setattr(a, k, v)
            return a

        def refused(text, fn, *rest):
            assert fn(eng._h, *rest) != 0
            err = eng.lib.cpmppi_last_error(eng._h).decode()
            assert re.search(text, err), err

        def untouched():
            torch.cuda.synchronize()
            return all((np_(t[k]) == -7.0).all() for k in ("loss", "grad", "cost", "Q"))
        return t, args, refused, untouched

    eng = new_engine()
    t, args, refused, untouched = setup(eng)
    lib = eng.lib
    step = lambda a: (C.byref(a), 1e-3, 0.9, 0.999, 1e-8, 0.0, None)  # noqa: E731
    refused("cpmppi_dense_policy_loss_grad: no model set", lib.cpmppi_dense_policy_loss_grad, C.byref(args()), None)
    refused("cpmppi_dense_policy_train_step: no model set", lib.cpmppi_dense_policy_train_step, *step(args()))
    eng.set_dense(model("random"))
    refused("cpmppi_dense_policy_train_step: call cpmppi_dense_train_begin first", lib.cpmppi_dense_policy_train_step, *step(args()))
    for text, kw in (("states, target_position, target_equilibrium, windows, windows_host and loss_out are required", dict(states=None)),
                     (".*are required", dict(target_position=None)), (".*are required", dict(target_equilibrium=None)),
                     (".*are required", dict(windows=None)), (".*are required", dict(windows_host=None)), (".*are required", dict(loss_out=None)),
                     ("B, R, T and horizon must be at least 1", dict(B=0)), (".*at least 1", dict(R=0)), (".*at least 1", dict(T=0)),
                     (".*at least 1", dict(horizon=0)),
                     (r"window \d+ = \(0, 12\) lies outside r < R, t0 <= T - 1", dict(T=B - 1)),
                     ("misaligned pointer", dict(states=t["s"].data_ptr() + 2)), ("misaligned pointer", dict(loss_out=t["loss"].data_ptr() + 4)),
                     ("misaligned pointer", dict(Q_out=t["Q"].data_ptr() + 1)), ("misaligned pointer", dict(L=t["tp"].data_ptr() + 2))):
        refused("cpmppi_dense_policy_loss_grad: " + text, lib.cpmppi_dense_policy_loss_grad, C.byref(args(**kw)), None)
    assert lib.cpmppi_dense_policy_loss_grad(eng._h, C.byref(args(loss_out=t["loss"].data_ptr() + 4)), None) == -5       # CPMPPI_ERR_ALIGN
    refused("cpmppi_dense_policy_reserve: B and horizon must be at least 1", lib.cpmppi_dense_policy_reserve, 0, 3)
    refused("cpmppi_dense_policy_reserve: B and horizon must be at least 1", lib.cpmppi_dense_policy_reserve, 3, 0)
    # per-env tuning rows, pole-mass rows
    from cartpolesimulation_amd.configs import tuning_rows
    eng.set_tuning_rows(tuning_rows(eng.mppi, 1))
    refused("cpmppi_dense_policy_loss_grad: per-env tuning rows are registered", lib.cpmppi_dense_policy_loss_grad, C.byref(args()), None)
    eng.set_tuning_rows(None)
    assert untouched()
    before = eng.dense_control(t["s"][0], t["tp"][0], t["te"][0])[0].clone()
    eng.close()
    for kw, text in ((dict(predictor="ODE", per_env_pole_mass=True), "per-row pole masses are registered"),
                     (dict(cost="quadratic_boundary_grad"), "the cost is differentiated for quadratic_boundary_grad_minimal and default alone"),
                     (dict(cost="quadratic_boundary"), "the cost is differentiated for"),
                     (dict(math_mode="precise"), "the adjoint is written for the FAST arithmetic"),
                     (dict(S=30), r"S too large for the LDS sub-state buffer \(<= 19\)"),
                     (dict(gru=True), "the handle's predictor is the GRU")):
        gru = kw.pop("gru", False)
        eng = new_engine(model("random"), **kw)
        t, args, refused, untouched = setup(eng)
        if gru:
            g = np.load(os.path.join(golden_dir, "gru_c5.npz"))
            eng.set_gru({k: g[k] for k in g.files if k not in ("s0", "Q", "h0", "traj", "h_final")})
        if kw.get("per_env_pole_mass"):
            eng.set_pole_mass_rows(torch.full((1,), 0.09, device=eng.device))
        eng.dense_train_begin()
        refused("cpmppi_dense_policy_loss_grad: " + text, eng.lib.cpmppi_dense_policy_loss_grad, C.byref(args()), None)
        refused("cpmppi_dense_policy_train_step: " + text, eng.lib.cpmppi_dense_policy_train_step, *step(args()))
        assert untouched()
        assert np.array_equal(bits(np_(eng.dense_control(t["s"][0], t["tp"][0], t["te"][0])[0])), bits(np_(before)))
        if gru:
            with pytest.raises(ValueError, match="the GRU as the differentiated plant is not built"):
                device_call(eng, B, H)
        eng.close()
