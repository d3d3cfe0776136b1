"""The reference of the GRU gradient tests: a float64 torch restatement of oracle_np.gru_predict that feeds
oracle_torch.trajectory_cost, differentiated by torch.autograd - d get_trajectory_cost(predict_core_GRU(s, Q), Q) / d Q.

tests/test_gru_grad_ref_host.py pins the restatement to the numpy oracle (trajectory to 1e-12, cost); tests/test_gpu_gru_grad.py
compares the kernel against it.  The cost takes cos(angle) with angle = atan2(sin, cos) of the network's outputs, so autograd
differentiates c / sqrt(c^2 + s^2) through both; the stage-0 angle is the given state's and carries no gradient; indicator terms
(`default`: track edge, terminal cost) and a clipped control contribute zero, as in oracle_torch.cost_and_grad."""
import functools

import numpy as np
import torch

from oracle import oracle_np as O
from oracle import oracle_torch as OT

f32, f64 = np.float32, torch.float64
COSTS = {"quadratic_boundary_grad_minimal": O.COST_QBGM, "default": O.COST_DEFAULT}
COST_FLAG_NAMES = {"quadratic_boundary_grad_minimal": "qbgm", "default": "default"}


def _cell(x, h, w_ih, w_hh, b_ih, b_hh):
    Hd = h.shape[1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[:, :Hd] + gh[:, :Hd])
    z = torch.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
    n = torch.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
    return (1.0 - z) * n + z * h


def gru_predict(model, s0, Q, h0=None, dtype=f64):
    """oracle_np.gru_predict on float64 torch tensors: s0 [6], Q [N,H] (tensor), h0 [2,32] or None ->
    traj[k][component] (k = 0..H, each a tensor [N]; the form oracle_torch.trajectory_cost takes).  ``dtype=torch.float32``: the
    same statements on float32 tensors (Q float32 too) - a float32 realisation of the reference, to judge its conditioning."""
    N, H = Q.shape
    npd = np.float64 if dtype == f64 else np.float32
    m = {k: torch.tensor(np.asarray(v, dtype=npd)) for k, v in model.items()}
    s = torch.tensor(np.asarray(s0, dtype=f32).astype(npd))
    h = [torch.zeros(N, 32, dtype=dtype) if h0 is None else torch.tensor(np.asarray(h0, f32)[layer].astype(npd)).repeat(N, 1)
         for layer in range(2)]
    feat0 = torch.stack([s[O.ANGLED_IDX], s[O.ANGLE_COS_IDX], s[O.ANGLE_SIN_IDX], s[O.POSITION_IDX], s[O.POSITIOND_IDX]])
    feat = (feat0 * m["in_scale"][1:] + m["in_shift"][1:]).repeat(N, 1)
    traj = [[s[i].repeat(N) for i in range(6)]]
    for k in range(H):
        qn = Q[:, k] * m["in_scale"][0] + m["in_shift"][0]
        x = torch.cat([qn[:, None], feat], dim=1)
        h[0] = _cell(x, h[0], m["w_ih0"], m["w_hh0"], m["b_ih0"], m["b_hh0"])
        h[1] = _cell(h[0], h[1], m["w_ih1"], m["w_hh1"], m["b_ih1"], m["b_hh1"])
        feat = h[1] @ m["w_out"].T + m["b_out"]
        y = feat * m["out_scale"] + m["out_shift"]
        st = [None] * 6
        st[O.ANGLED_IDX], st[O.ANGLE_COS_IDX], st[O.ANGLE_SIN_IDX] = y[:, 0], y[:, 1], y[:, 2]
        st[O.POSITION_IDX], st[O.POSITIOND_IDX] = y[:, 3], y[:, 4]
        st[O.ANGLE_IDX] = torch.atan2(y[:, 2], y[:, 1])
        traj.append(st)
    return traj


def cost_and_grad(model, cost, s0, Q, target_position, target_equilibrium=1.0, h0=None, horizon_reduce="sum", clip=(-1.0, 1.0),
                  dtype=np.float64, eval_dtype=f64):
    """numpy in / numpy out: (cost [N], grad [N,H], traj [N,H+1,6]) of one env in float64; ``dtype=np.float32`` only rounds the
    results (the evaluation stays double); ``eval_dtype=torch.float32`` evaluates the network and its adjoint in float32."""
    Qt = torch.tensor(np.asarray(Q, dtype=np.float64 if eval_dtype == f64 else np.float32), requires_grad=True)
    Qa = Qt.clamp(clip[0], clip[1]) if clip is not None else Qt
    traj = gru_predict(model, s0, Qa, h0, eval_dtype)
    J = OT.trajectory_cost(COSTS[cost], traj, Qa, target_position, target_equilibrium, horizon_reduce)
    (g,) = torch.autograd.grad(J.sum(), Qt)
    tr = torch.stack([torch.stack(st, dim=1) for st in traj], dim=1).detach().numpy()
    return J.detach().numpy().astype(dtype), g.numpy().astype(dtype), tr


# ---- the cases of tests/test_gpu_gru_grad.py (inputs and float64 references, computed once and left unchanged)
SHAPES = [(3, 40, 35), (2, 16, 35), (2, 1, 2), (2, 31, 7), (2, 33, 7), (1, 129, 2), (1, 300, 1)]
PAIRS = [("golden", "quadratic_boundary_grad_minimal"), ("golden", "default"), ("random", "quadratic_boundary_grad_minimal")]


@functools.lru_cache(maxsize=None)
def case_inputs(E, N, H):
    """SFC64(1000 + N + H): per env draw_env(rng, H, 0.3), then Q = 0.5 N(0,1) with the first four rollouts x 3 (beyond the
    limits: their gradient is exactly 0 there in both results)."""
    from test_gpu_gru_edges import draw_env
    rng = np.random.Generator(np.random.SFC64(1000 + N + H))
    s0, tp, h0, Q = [], [], [], []
    for _ in range(E):
        s, t, _, h = draw_env(rng, H, 0.3)
        q = (0.5 * rng.standard_normal((N, H))).astype(f32)
        q[:4] *= 3.0
        s0.append(s); tp.append(t); h0.append(h); Q.append(q)
    out = tuple(np.stack(x) for x in (s0, tp, h0, Q))
    for x in out:
        x.setflags(write=False)
    return out


def reference_of(model_name, cost, s0, tp, te, h0, Q, reduce, clip=(-1.0, 1.0)):
    """One env -> (J [N], g [N,H], flagged [N]) in float64 under target equilibrium `te` and control limits `clip` (None: the
    inputs are not clipped, control_mode "penalise").  Flagged: PU.flag_indicators on the oracle's trajectory, or an input within
    1e-3 of a control limit."""
    import parity_util as PU
    from test_gpu_gru_edges import model_of
    N = Q.shape[0]
    J, g, _ = cost_and_grad(model_of(model_name), cost, s0, Q, tp, te, h0, reduce, clip)
    h0b = np.repeat(h0[:, None, :], N, axis=1) if h0 is not None else None
    Qa = Q if clip is None else np.clip(Q, f32(clip[0]), f32(clip[1]))
    traj = O.gru_predict(model_of(model_name), s0, Qa, h0b, dtype=np.float64)[0]
    f = PU.flag_indicators(traj, COST_FLAG_NAMES[cost], tp)
    if clip is not None:
        f = f | ((np.abs(Q - f32(clip[0])) < 1e-3) | (np.abs(Q - f32(clip[1])) < 1e-3)).any(axis=1)
    return J, g, f


@functools.lru_cache(maxsize=None)
def case_reference(model_name, cost, E, N, H, with_h0, reduce, te=1.0):
    """-> (J [E,N], g [E,N,H], flagged [E,N]) in float64 (reference_of per env of case_inputs; `te`: every env's target equilibrium)."""
    s0, tp, h0, Q = case_inputs(E, N, H)
    per_env = [reference_of(model_name, cost, s0[e], tp[e], te, h0[e] if with_h0 else None, Q[e], reduce) for e in range(E)]
    out = tuple(np.stack(x) for x in zip(*per_env))
    for x in out:
        x.setflags(write=False)
    return out
