"""The reference of the cost fine-tuning tests (cpmppi_dense_policy_*): the closed loop net -> clip -> ODE plant -> plugin cost in
torch float64 on the CPU, vectorised over the batch, differentiated by autograd.  Written from include/cpmppi.h; nothing of the
library under test is used.

It composes tests/dense_ref.py (``forward``, ``_norm``, ``features``: the net) with the substep and the cost formulas of
oracle/oracle_torch.py (``_ode``, ``_wrap``: imported; the integrator loop of its ``predict_core`` and the two stage costs of its
``trajectory_cost``, restated here with a target PER START STATE - test_policy_host.py pins the restatement to
``OT.trajectory_cost`` / ``OT.predict_core`` for a uniform target).  Non-smooth pieces as autograd takes them, which is how
cpmppi_grad.hpp documents its own: the branch taken at the bounce (``torch.where``), derivative 1 through the wrap, 0 through
indicators and through ``clamp`` where it clips.

A batch is B start states s0 [B,6] with targets tp, te [B] (the row of the window) and pole lengths L [B] or None."""
import numpy as np
import torch

import dense_ref as D
from oracle import oracle_np as O
from oracle import oracle_torch as OT

f64 = torch.float64
KEYS = D.KEYS


def t64(x, dtype=f64):
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype)


def substeps(st, u, L, t, S, integrator, p):
    """S substeps from the state tuple ``st`` (six [B] tensors) under the force ``u`` [B]: oracle_torch.predict_core's loop body."""
    a, ad, ca, sa, x, xd = st
    THL = float(p.TrackHalfLength)
    for _ in range(S):
        aDD, xDD = OT._ode(ca, sa, ad, xd, u, L, p)
        if integrator == "ODE":
            ad, xd = ad + aDD * t, xd + xDD * t
            a, x = a + ad * t, x + xd * t
            ca, sa = torch.cos(a), torch.sin(a)
            a = torch.atan2(sa, ca)
            continue
        a, ad, x, xd = a + ad * t, ad + aDD * t, x + xd * t, xd + xDD * t
        cb = torch.cos(a)
        hit = (x >= THL) | (-x >= THL)
        ad_b = ad - 2 * (xd * cb) / (0.5 * L)
        a_b = a + ad_b * t
        xd_b = -xd
        x_b = x + xd_b * t
        a, ad = torch.where(hit, a_b, a), torch.where(hit, ad_b, ad)
        x, xd = torch.where(hit, x_b, x), torch.where(hit, xd_b, xd)
        a = OT._wrap(a)
        ca, sa = torch.cos(a), torch.sin(a)
    return (a, ad, ca, sa, x, xd)


def stage_cost(cost_id, st, u, x_t, te, p, c):
    """The stage cost [B] of the states ``st`` and the controls ``u`` [B]: the formulas of oracle_torch.trajectory_cost, the
    targets per start state."""
    THL = float(p.TrackHalfLength)
    ang, angD, x = st[0], st[1], st[4]
    cosang = torch.cos(ang)
    if cost_id == O.COST_QBGM:
        ptf = float(np.float32(c.qbgm_permissible_track_fraction))
        dd = c.qbgm_dd_quadratic_weight * ((x - x_t) / (2 * THL)) ** 2
        near = (x.abs() > ptf * THL).to(x.dtype)
        db = c.qbgm_db_weight * (near * ((x.abs() - ptf * THL) / ((1 - ptf) * THL)) ** 2)
        ep = c.qbgm_ep_weight * (1.0 - te * cosang) ** 2
        ekp = c.qbgm_ekp_weight * angD ** 2
        cc = c.qbgm_cc_weight * (c.qbgm_R * u ** 2)
        return dd + db + ep + ekp + cc
    if cost_id == O.COST_DEFAULT:
        dd = c.def_dd_weight * (((x - x_t) / (2.0 * THL)) ** 2 + (x.abs() > 0.90 * THL).to(x.dtype) * 1.0e7)
        ep = c.def_ep_weight * (te * 0.25 * (1.0 - cosang) ** 2)
        cc = c.def_cc_weight * (c.def_R * u ** 2)
        return dd + ep + cc
    raise ValueError(cost_id)


def terminal_cost(cost_id, st, x_t, p):
    if cost_id != O.COST_DEFAULT:
        return torch.zeros_like(st[0])
    THL = float(p.TrackHalfLength)
    return 10000.0 * ((st[0].abs() > 0.2) | ((st[4] - x_t).abs() > 0.1 * THL)).to(st[0].dtype)


def closed_loop(weights, norm, s0, tp, te, horizon, cost_id=O.COST_QBGM, integrator="ODE_v0", L=None, dt=0.02, S=10,
                horizon_reduce="sum", p=O.DEFAULT_PARAMS, c=O.DEFAULT_COST):
    """``weights``: float64 tensors by key (they may require grad); ``norm`` = dense_ref._norm(model, float64); s0 [B,6], tp, te [B]
    tensors.  -> (J [B], the controls u [B,horizon], the unclipped q [B,horizon])."""
    a_in, b_in, A, Bo = norm
    B = s0.shape[0]
    dtype = s0.dtype
    Lt = torch.full((B,), float(p.L), dtype=dtype) if L is None else t64(L, dtype)
    t = float(dt / float(S))
    st = tuple(s0[:, i] for i in range(6))
    total, us, qs = torch.zeros(B, dtype=dtype), [], []
    for _ in range(horizon):
        x = torch.stack([st[1], st[2], st[3], st[4], st[5], te, tp], dim=1)          # dense_ref.features' order
        q = D.forward(weights, x * a_in + b_in) * A + Bo
        u = torch.clamp(q, -1.0, 1.0)
        us.append(u)
        qs.append(q)
        total = total + stage_cost(cost_id, st, u, tp, te, p, c)
        st = substeps(st, float(p.u_max) * u, Lt, t, S, integrator, p)
    total = total + terminal_cost(cost_id, st, tp, p)
    if horizon_reduce == "mean":
        total = total / (horizon + 1)
    return total, torch.stack(us, dim=1), torch.stack(qs, dim=1)


def loss_and_grad(model, s0, tp, te, horizon, grad=True, dtype=f64, **kw):
    """numpy in / float64 numpy out.  ``dtype`` torch.float32: the same formulas evaluated plainly in float32 - what that loses against
    float64 is the yardstick of the trajectory test, as in tests/test_gpu_imitator.py.
    -> (loss = mean J, gradient [1345] in the flat order (None without ``grad``), J [B], u [B,horizon], q [B,horizon])."""
    w = D._tensors(model, dtype, grad=grad)
    J, u, q = closed_loop(w, D._norm(model, dtype), t64(s0, dtype), t64(tp, dtype), t64(te, dtype), horizon, **kw)
    loss = J.mean()
    g = None
    if grad:
        loss.backward()
        g = np.concatenate([w[k].grad.double().numpy().reshape(-1) for k in KEYS])
    return float(loss.detach()), g, J.detach().double().numpy(), u.detach().double().numpy(), q.detach().double().numpy()


def start_states(seed, B, angle=3.0, angleD=4.0, position=0.15, positionD=0.5, target=0.1):
    """B random start states (float32, angle_cos / angle_sin of the float32 angle) and targets: -> (s0 [B,6], tp [B], te [B] mixed
    +-1)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    ang = rng.uniform(-angle, angle, B).astype(f32)
    s0 = np.stack([ang, rng.uniform(-angleD, angleD, B).astype(f32), np.cos(ang.astype(np.float64)).astype(f32),
                   np.sin(ang.astype(np.float64)).astype(f32), rng.uniform(-position, position, B).astype(f32),
                   rng.uniform(-positionD, positionD, B).astype(f32)], axis=1).astype(f32)
    tp = rng.uniform(-target, target, B).astype(f32)
    te = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(f32)
    return s0, tp, te


def clip_and_adam(opt, grad, clip_norm):
    """One step of dense_ref.Adam ``opt`` with the gradient scaled to the global norm ``clip_norm`` (<= 0: off) in float64, as
    include/cpmppi.h states cpmppi_dense_policy_train_step; a non-finite gradient leaves ``opt`` alone.  -> the parameters."""
    g = np.asarray(grad, np.float64)
    norm = float(np.sqrt((g * g).sum()))
    if not np.isfinite(norm):
        return opt.p
    if clip_norm > 0 and norm > clip_norm:
        g = g * (clip_norm / norm)
    return opt.step(g)
