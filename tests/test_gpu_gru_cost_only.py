"""GPU: the cost-only GRU rollout (gru_cost_only_kernel, cpmppi_rollout_cost_gru, MPPIEngine.rollout_cost(predictor="GRU")) and
the three sampling optimizers built on it (cem, cem-gmm, random-action with gru_model=).

Helpers, models ("golden" = tests/golden/gru_c5.npz, "random" = SFC64(30) at scale 0.3) and bounds are those of
tests/test_gpu_gru_edges.py, imported from there.

Reference: O.gru_mppi_step(model, s, zeros(H), inputs, tp, 1.0, MPPIConfig(N, H, cost, cc_weight=0, shift_mode="none"), h0)["S"] in
float32 and float64 - a zero nominal sequence, no correction term, no shift: the cost of the given plans and nothing else.
Bound: parity_util.assert_costs with flag_rounding_sensitive (and flag_indicators for `default`); nothing new.  State, target
position and h0 per env as draw_env draws them; inputs clip(0.5 N(0,1), -1, 1) or U(-1, 1), alternating with the case.  Every
compared env has at most 5 % of its rollouts flagged (asserted); the random model meets `default` only at H in {1, 7} (its float32
and float64 oracles part on 5-10 % of the rollouts at H = 35).

The same statements, the same bits: on a handle with cc_weight = 0 and shift_mode "none" the fused step's S_out for delta_u =
inputs and a zero nominal sequence is asserted bit-identical to the cost-only launch in both math modes - the two kernels share
the cell, the cost statements and their order, and the fused kernel's additions (u_nom = 0 + du, + a correction term of 0) change
no bit of a finite cost.

Measured on the MI355X (this module's first run, 170 cases in 4 s): worst clear rollout of test_costs_vs_oracle_across_tails at 0.395
of its assert_costs allowance; the bit comparison with the fused step: no word differs in any of the 8 cells; the optimizers'
memory within 9.31e-08 (cem), 7.45e-08 (cem-gmm), 8.94e-08 (random-action) of the float32 oracle's.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
import parity_util as PU  # noqa: E402
from test_gpu_gru_edges import COSTS, bits, cost_flags, draw_env, engine, model_of, report  # noqa: E402

f32 = np.float32
E3 = 3
TAILS_N = [1, 31, 33, 128, 129, 200, 257]       # lane tail, wave tail, block tail, CEM's shipped 200, three blocks
TAILS_H = [1, 7, 35]
SENT = f32(-7.25)


# (the random model under `default` beyond H = 7: its float32 and float64 oracles part on more than 5 % of the rollouts - no case)
TAIL_CASES = [(model, cost, N, H) for model in ("golden", "random") for cost in COSTS for N in TAILS_N for H in TAILS_H
              if not (model == "random" and cost == "default" and H > 7)]


def draw_inputs(rng, N, H, kind):
    if kind == "normal":
        return np.clip(0.5 * rng.standard_normal((N, H)), -1.0, 1.0).astype(f32)
    return rng.uniform(-1.0, 1.0, (N, H)).astype(f32)


@functools.lru_cache(maxsize=None)
def case_inputs(N, H, E=E3):
    """-> s0 [E,6], tp [E], h0 [E,2,32], inputs [E,N,H]; the draw of the inputs alternates with the case."""
    rng = np.random.Generator(np.random.SFC64(7000 + 40 * N + H))
    kind = ("normal", "uniform")[(TAILS_N.index(N) + TAILS_H.index(H)) % 2] if (N in TAILS_N and H in TAILS_H) else "normal"
    envs = []
    for _ in range(E):
        s, tp, _, h0 = draw_env(rng, H, 0.2)
        envs.append((s, tp, h0, draw_inputs(rng, N, H, kind)))
    return tuple(np.stack([e[i] for e in envs]) for i in range(4))


def oracle_costs(model, cost, s, inputs, tp, h0):
    """The reference for one env in float32 and float64."""
    N, H = inputs.shape
    cfg = O.MPPIConfig(N=N, H=H, cost_id=COSTS[cost], cc_weight=0.0, shift_mode="none")
    a = O.gru_mppi_step(model_of(model), s, np.zeros(H, f32), inputs, f32(tp), f32(1.0), cfg, h0=h0)
    b = O.gru_mppi_step(model_of(model), s, np.zeros(H, f32), inputs, f32(tp), f32(1.0), cfg, h0=h0, dtype=np.float64)
    return a, b


@functools.lru_cache(maxsize=None)
def case_reference(model, cost, N, H, with_h0):
    """Computed once per case, shared by the math modes, never written to."""
    s0, tp, h0, inputs = case_inputs(N, H)
    return [oracle_costs(model, cost, s0[e], inputs[e], tp[e], h0[e] if with_h0 else None) for e in range(E3)]


def check_costs(S, refs, cost, tp, what):
    worst = 0.0
    for e, (r32, r64) in enumerate(refs):
        fl = cost_flags(r32, r64, cost, tp[e])
        assert fl.mean() <= 0.05, f"{what} env {e}: {int(fl.sum())} of {fl.size} rollouts flagged"
        b = PU.assert_costs(S[e], r32["S"], r64["S"], fl, f"{what} env {e} costs")
        clear = ~b["flagged"]
        worst = max(worst, float(b["excess"][clear].max()) if clear.any() else 0.0)
    return worst


def call_gru(eng, E, s0, inputs, tp, te, h0, S):
    """The C entry point itself, on device tensors (None = NULL)."""
    from cartpolesimulation_amd.engine import _ptr
    return eng.lib.cpmppi_rollout_cost_gru(eng._h, E, _ptr(s0), _ptr(inputs), _ptr(tp), _ptr(te), _ptr(h0), _ptr(S), eng._stream())


# ---- 1. costs against the oracle across tails
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("model,cost,N,H", TAIL_CASES)
def test_costs_vs_oracle_across_tails(model, cost, N, H, math_mode, capsys):
    """Three envs that differ in state, target, memory and plans, through the C entry point of a handle built for FOUR envs into a
    caller-owned buffer [5, N] of sentinels: rows 0..2 against the oracle, the fourth env's row (which a launch of cfg.E envs would
    write) and the row behind it untouched.  N = 129 once more without a memory (h0 = NULL)."""
    s0, tp, h0, inputs = case_inputs(N, H)
    eng = engine(E3 + 1, N, H, model, cost_function_specification=cost, math_mode=math_mode)
    s_t, in_t, tp_t, te_t, h_t = eng.tensor(s0), eng.tensor(inputs), eng.tensor(tp), eng.tensor(np.ones(E3, f32)), eng.tensor(h0)
    worst = 0.0
    for with_h0 in ((True, False) if N == 129 else (True,)):
        buf = torch.full((E3 + 2, N), float(SENT), dtype=torch.float32, device=eng.device)
        assert call_gru(eng, E3, s_t, in_t, tp_t, te_t, h_t if with_h0 else None, buf) == 0, eng.lib.cpmppi_last_error(eng._h)
        out = buf.cpu().numpy()
        assert np.all(out[E3:] == SENT), "rows behind the three envs were written"
        what = f"{model} {cost} N {N} H {H} {math_mode} h0 {with_h0}"
        worst = max(worst, check_costs(out[:E3], case_reference(model, cost, N, H, with_h0), cost, tp, what))
        # the engine method is the same launch
        S = eng.rollout_cost(s0, inputs, tp, np.ones(E3, f32), predictor="GRU", h0=h0 if with_h0 else None)
        assert np.array_equal(bits(S.cpu().numpy()), bits(out[:E3]))
    report(capsys, f"item1 {model} {cost} N {N} H {H} {math_mode}: excess {worst:.3f}")
    eng.close()


# ---- 2. same statements, same bits
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
@pytest.mark.parametrize("cost", list(COSTS))
def test_bit_identical_to_the_fused_step_with_a_zero_nominal(cost, math_mode):
    E, N, H = 2, 129, 26
    s0, tp, h0, inputs = case_inputs(N, H, E)
    eng = engine(E, N, H, cost_function_specification=cost, math_mode=math_mode, cc_weight=0.0, shift_mode="none")
    te = np.ones(E, f32)
    for h in (h0, None):
        S_cost = eng.rollout_cost(s0, inputs, tp, te, predictor="GRU", h0=h).cpu().numpy()
        S_step = eng.empty(E, N)
        eng.step(s0, eng.zeros(E, H), tp, te, S_out=S_step, predictor="GRU", h0=h, delta_u=inputs)
        S_step = S_step.cpu().numpy()
        assert np.isfinite(S_cost).all()
        differing = int((bits(S_cost) != bits(S_step)).sum())
        assert differing == 0, f"{differing} of {S_cost.size} costs differ, worst {np.abs(S_cost - S_step).max():.3e}"
    eng.close()


# ---- 3. refusals through ctypes
@pytest.mark.parametrize("case", ["no model", "legacy cost", "quadratic_boundary cost", "E beyond cfg.E", "E zero", "NULL inputs",
                                  "NULL S_out"])
def test_refusals_launch_nothing(case):
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    E, N, H = 2, 33, 5
    cost = {"legacy cost": "legacy_mppi_cartpole", "quadratic_boundary cost": "quadratic_boundary"}.get(case, "default")
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, cost_function_specification=cost))
    if case != "no model":
        eng.set_gru(model_of("golden"))
    s0, tp, _, inputs = case_inputs(N, H, E)
    s_t, in_t, tp_t, te_t = eng.tensor(s0), eng.tensor(inputs), eng.tensor(tp), eng.tensor(np.ones(E, f32))
    S = torch.full((E + 1, N), float(SENT), dtype=torch.float32, device=eng.device)
    args = dict(E=E, s0=s_t, inputs=in_t, tp=tp_t, te=te_t, h0=None, S=S)
    args.update({"E beyond cfg.E": dict(E=E + 1), "E zero": dict(E=0), "NULL inputs": dict(inputs=None),
                 "NULL S_out": dict(S=None)}.get(case, {}))
    rc = call_gru(eng, args["E"], args["s0"], args["inputs"], args["tp"], args["te"], args["h0"], args["S"])
    torch.cuda.synchronize()
    assert rc == -1
    msg = eng.lib.cpmppi_last_error(eng._h).decode()
    assert msg.startswith("cpmppi_rollout_cost_gru: "), msg
    want = {"no model": "no model set", "legacy cost": "supports quadratic_boundary_grad_minimal and default",
            "quadratic_boundary cost": "supports quadratic_boundary_grad_minimal and default", "E beyond cfg.E": "E out of range",
            "E zero": "E out of range"}.get(case, "are required")
    assert want in msg, msg
    assert np.all(S.cpu().numpy() == SENT), "a refused call wrote costs"
    # the engine method words its own refusals before any library call
    if case == "no model":
        with pytest.raises(ValueError, match="takes no L"):
            eng.rollout_cost(s0, inputs, tp, np.ones(E, f32), L=np.full(E, 0.4, f32), predictor="GRU")
        with pytest.raises(ValueError, match="memory of the GRU"):
            eng.rollout_cost(s0, inputs, tp, np.ones(E, f32), h0=np.zeros((E, 2, 32), f32))
        from cartpolesimulation_amd._lib import CpmppiError
        with pytest.raises(CpmppiError, match="cpmppi_rollout_cost_gru: no model set"):
            eng.rollout_cost(s0, inputs, tp, np.ones(E, f32), predictor="GRU")
    eng.close()


# ---- 4. the optimizers
def _shift(x, fill, dim):
    tail = torch.full_like(x.narrow(dim, 0, 1), fill)
    return torch.cat([x.narrow(dim, 1, x.shape[dim] - 1), tail], dim=dim).contiguous()


def staged_step(name, eng, st, s_t, tp_t, te_t, hp):
    """One control step of optimizer `name` written out in engine calls on the state dict `st` -> (controls [E], costs [E,N])."""
    E = s_t.shape[0]
    if name == "random-action":
        mid, half = 0.5 * (hp["lo"] + hp["hi"]), 0.5 * (hp["hi"] - hp["lo"])
        wide = eng.zeros(E, eng.H)
        x = eng.cem_sample(wide + mid, wide + 0.01 * half, hp["seed"], offset=st["counter"])
        z = (x - mid) / (0.01 * half)
        Q = (hp["lo"] + (hp["hi"] - hp["lo"]) * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))).clamp_(hp["lo"], hp["hi"]).contiguous()
        st["counter"] += 1
        S = eng.rollout_cost(s_t, Q, tp_t, te_t, predictor="GRU", h0=st["h"])
        u = Q[torch.arange(E, device=S.device), torch.argmin(S, dim=1), 0].clone()
    else:
        ar = torch.arange(E, device=s_t.device)[:, None]
        for _ in range(hp["outer"]):
            if name == "cem":
                Q = eng.cem_sample(st["mean"], st["stdev"], hp["seed"], offset=st["counter"])
            else:
                Q = eng.cem_gmm_sample(st["centres"], st["stdev"], hp["seed"], offset=st["counter"])
            S = eng.rollout_cost(s_t, Q, tp_t, te_t, predictor="GRU", h0=st["h"])
            st["mean"], st["stdev"], el = eng.cem_update(S, Q, hp["best_k"], hp["stdev_min"], return_elites=True)
            if name == "cem-gmm":
                st["centres"] = Q[ar, el.long()].contiguous()
            st["counter"] += 1
        u = (st["mean"][:, 0] if name == "cem" else st["centres"][:, 0, 0]).clone()
        mid = 0.5 * (hp["lo"] + hp["hi"])
        st["mean"], st["stdev"] = _shift(st["mean"], mid, 1), _shift(st["stdev"], math.sqrt(0.5), 1)
        if name == "cem-gmm":
            st["centres"] = _shift(st["centres"], mid, 2)
    _, h_new = eng.gru_predict(s_t, u.reshape(E, 1), h0=st["h"].transpose(0, 1).contiguous(), return_hidden=True)
    st["h"] = h_new.transpose(0, 1).contiguous()
    return u, S


@pytest.mark.parametrize("name", ["cem", "cem-gmm", "random-action"])
def test_optimizers_over_the_gru(name, capsys):
    """Two control steps of three envs, golden model: controls, distribution and J_logged bit-equal to the staged composition of
    engine calls above (its own engine); the optimizer's memory against the oracle's for (state, applied control); and a twin whose
    memory is zeroed before step 2 costs its plans differently."""
    from types import SimpleNamespace
    from cartpolesimulation_amd import optimizer_cem as OC
    from cartpolesimulation_amd.engine import MPPIEngine
    cls = {"cem": OC.optimizer_cem, "cem-gmm": OC.optimizer_cem_gmm, "random-action": OC.optimizer_random_action}[name]
    E, H, seed = E3, 12, 9
    N = 64 if name == "random-action" else 200
    model = model_of("golden")
    target = np.array([-0.05, 0.0, 0.04], f32)
    kw = dict(control_limits=(np.array([-1.0]), np.array([1.0])), num_envs=E, gru_model=model, num_rollouts=N, mpc_horizon=H,
              seed=seed, optimizer_logging=True)
    if name != "random-action":
        kw.update(cem_outer_it=3, cem_best_k=40, cem_stdev_min=0.01, cem_initial_action_stdev=0.5)

    def make():
        vp = SimpleNamespace(target_position=target.copy(), target_equilibrium=np.ones(E, f32))
        opt = cls(variable_parameters=vp, **kw)
        opt.configure(predictor_specification="GRU-6IN-32H1-32H2-5OUT-0")
        return opt

    opt, twin = make(), make()
    eng = MPPIEngine(E, opt.cfg, opt.phys)
    eng.set_gru(model)
    hp = dict(lo=-1.0, hi=1.0, seed=seed, outer=3, best_k=40, stdev_min=0.01)
    st = dict(counter=0, h=eng.zeros(E, 2, 32), mean=eng.zeros(E, H), stdev=eng.zeros(E, H) + 0.5)
    st["centres"] = st["mean"][:, None, :].contiguous()
    tp_t, te_t = eng.tensor(target), eng.tensor(np.ones(E, f32))
    s = np.stack([O.create_cartpole_state(0.3, -0.5, 0.02, 0.1), O.create_cartpole_state(-0.4, 1.0, -0.05, -0.1),
                  O.create_cartpole_state(0.1, 0.3, 0.08, 0.15)])
    h_ref = np.zeros((E, 2, 32), f32)
    worst_h = 0.0
    for it in range(2):
        if it == 1:
            assert twin.h.abs().max().item() > 1e-3
            twin.h.zero_()
        u, u_twin = opt.step(s), twin.step(s)
        u_ref, S_ref = staged_step(name, eng, st, eng.tensor(s), tp_t, te_t, hp)
        assert u.shape == (E, 1)
        assert np.array_equal(bits(u[:, 0]), bits(u_ref.cpu().numpy())), f"step {it}: controls"
        assert np.array_equal(bits(opt.logging_values["J_logged"]), bits(S_ref.cpu().numpy())), f"step {it}: J_logged"
        if name != "random-action":
            assert np.array_equal(bits(opt.dist_mue.cpu().numpy()), bits(st["mean"].cpu().numpy())), f"step {it}: mean"
            assert np.array_equal(bits(opt.stdev.cpu().numpy()), bits(st["stdev"].cpu().numpy())), f"step {it}: stdev"
        if name == "cem-gmm":
            assert np.array_equal(bits(opt.centres.cpu().numpy()), bits(st["centres"].cpu().numpy())), f"step {it}: centres"
        assert np.array_equal(bits(opt.h.cpu().numpy()), bits(st["h"].cpu().numpy())), f"step {it}: memory"
        if it == 0:
            assert np.array_equal(bits(u_twin), bits(u)) and np.array_equal(bits(twin.logging_values["J_logged"]),
                                                                              bits(opt.logging_values["J_logged"]))
        else:                                                   # the same plans from a zeroed memory: other costs
            assert not np.array_equal(twin.logging_values["J_logged"], opt.logging_values["J_logged"])
            rel = np.abs(twin.logging_values["J_logged"] - opt.logging_values["J_logged"]) / np.abs(opt.logging_values["J_logged"])
            assert np.median(rel) > 1e-6, f"the memory moves the costs by {np.median(rel):.2e} only"
        hd = opt.h.cpu().numpy()
        assert hd.shape == (E, 2, 32)
        for e in range(E):
            q = np.array([[u[e, 0]]], f32)                      # the memory advances under the control the optimizer applied
            h32 = O.gru_predict(model, s[e][None], q, h_ref[e][:, None, :])[1][:, 0]
            h64 = O.gru_predict(model, s[e][None], q, h_ref[e][:, None, :], dtype=np.float64)[1][:, 0]
            dh = np.abs(hd[e] - h32)
            assert np.all(dh <= 1e-4 + np.abs(h32 - h64)), f"step {it} env {e}: memory off by {dh.max():.2e}"
            worst_h = max(worst_h, float(dh.max()))
            h_ref[e] = h32
        s = np.stack([O.ode_v0_step(s[e][None], u[e].astype(f32))[0] for e in range(E)])
    report(capsys, f"item4 {name}: memory {worst_h:.2e}")
    eng.close()


# ---- 5. capture
@pytest.mark.parametrize("math_mode", ["fast", "precise"])
def test_captured_launch_replays_bit_identically(math_mode):
    """One cpmppi_rollout_cost_gru launch captured on a side stream (a single kernel node) and replayed twice with new plans,
    states and memories written into the same buffers: each replay equals the eager launch on those values bit for bit."""
    E, N, H = 2, 129, 7
    eng = engine(E, N, H, math_mode=math_mode)
    draws = [case_inputs(N, H, E)]
    for seed in (1, 2):
        rng = np.random.Generator(np.random.SFC64(8000 + seed))
        envs = []
        for _ in range(E):
            s, tp, _, h0 = draw_env(rng, H, 0.2)
            envs.append((s, tp, h0, draw_inputs(rng, N, H, "uniform")))
        draws.append(tuple(np.stack([e[i] for e in envs]) for i in range(4)))
    te = np.ones(E, f32)
    eager = [eng.rollout_cost(s0, inputs, tp, te, predictor="GRU", h0=h0).cpu().numpy() for s0, tp, h0, inputs in draws]
    assert not np.array_equal(eager[1], eager[2])
    s0, tp, h0, inputs = draws[0]
    s_t, in_t, tp_t, te_t, h_t = (eng.tensor(x.copy()) for x in (s0, inputs, tp, te, h0))
    S = torch.full((E, N), float(SENT), dtype=torch.float32, device=eng.device)
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert call_gru(eng, E, s_t, in_t, tp_t, te_t, h_t, S) == 0
    torch.cuda.current_stream(eng.device).wait_stream(side)
    torch.cuda.synchronize()
    assert np.all(S.cpu().numpy() == SENT)                       # captured, not run
    for k in (1, 2, 0):
        for dst, src in zip((s_t, tp_t, h_t, in_t), draws[k]):
            dst.copy_(torch.as_tensor(src))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(S.cpu().numpy()), bits(eager[k])), f"replay with draw {k}"
    eng.close()
