"""Inputs and references of the GRU target tests (test_gru_target_cases_host.py judges them on the host, test_gpu_gru_targets.py runs
them against the four kernels that cost rollouts under the GRU predictor).  Pure numpy + torch on the CPU + the oracle: no GPU.

Every kernel of that family reads two scalars per env, the target position and the target equilibrium.  The cases here give every
env its own pair: both signs of the target equilibrium in every case (env 0 hangs in STEP, "a" and "c" and is upright in "b"),
target positions that are distinct, of both signs and as far apart as +-0.5 THL allows.

An env is drawn like test_gpu_gru_edges.draw_env (the same order of draws) with two differences:
  * an env with te = -1 starts near the hanging pole: angle pi + U(-1, 1), wrapped into (-pi, pi];
  * the target position is sign * U(TP_LO, TP_HI), the sign alternating from env to env.  draw_env's +-0.05 is too narrow for the
    teeth conditions of the host test (the position term is the smallest of the costs' terms); [0.3, 0.5] THL stays inside
    +-0.5 THL and meets them for the costs under every model / cost pair, for the gradient under one pair per case - more the
    limit does not allow (test_gru_target_cases_host.py).
The seeds are chosen with the host test, which states what they have to deliver.

STEP: the fused step and the cost-only launch, 3 envs x 130 rollouts (a second block with two live columns), H = 11, knot period 5.
GRAD: the gradient launch at the smallest shapes that reach its addressing - see the table in test_gpu_gru_targets.py.  Inputs as
gru_grad_ref.case_inputs draws them, 0.5 N(0,1) with the first SCALED_ROWS rollouts x 3; the (3, 130, 4) case also runs under the
limits LIMITS with clipping and under control_mode "penalise" (MODES)."""
import functools

import numpy as np

from oracle import oracle_np as O
import gru_grad_ref as R

f32 = np.float32
THL = float(O.DEFAULT_PARAMS.TrackHalfLength)
TP_LO, TP_HI = 0.3 * THL, 0.5 * THL
LIMITS = (float(f32(-0.7)), float(f32(0.9)))
SCALED_ROWS = 16                         # of 130: enough inputs beyond each of LIMITS and between them and +-1 (host test)
PAIRS = R.PAIRS
# control limits of the gradient launch by mode: (control_mode, action_low, action_high, the reference's `clip`)
MODES = {"clip": ("clip", -1.0, 1.0, (-1.0, 1.0)), "limits": ("clip", LIMITS[0], LIMITS[1], LIMITS), "penalise": ("penalise", -1.0, 1.0, None)}

STEP = dict(E=3, N=130, H=11, period=5, te=(-1.0, 1.0, -1.0), seed=9329)
GRAD = {"a": dict(E=3, N=130, H=4, te=(-1.0, 1.0, -1.0), seed=9330, handle_envs=3),
        "b": dict(E=2, N=257, H=3, te=(1.0, -1.0), seed=9356, handle_envs=2),
        "c": dict(E=2, N=129, H=9, te=(-1.0, 1.0), seed=9319, handle_envs=3)}


def wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def draw_target_env(rng, H, u_scale, te, sign, h_scale=0.2):
    """draw_env with the env's target equilibrium and the sign of its target position -> state, target position, nominal sequence, memory."""
    ang = rng.uniform(-1, 1)
    if te < 0:
        ang = wrap(np.pi + ang)
    s = O.create_cartpole_state(ang, rng.uniform(-2, 2), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2))
    tp = f32(sign * rng.uniform(TP_LO, TP_HI))
    u0 = (u_scale * rng.standard_normal(H)).astype(f32)
    h0 = (h_scale * rng.standard_normal((2, 32))).astype(f32)
    return s, tp, u0, h0


def _frozen(arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def step_inputs():
    """-> dict(s0 [E,6], tp [E], te [E], u0 [E,H], h0 [E,2,32], du [E,N,H] (host perturbations of the configured spread),
    plans [E,N,H] (clip(0.5 N(0,1), -1, 1): the given plans of the cost-only launch))."""
    c = STEP
    rng = np.random.Generator(np.random.SFC64(c["seed"]))
    stdev = O.MPPIConfig(N=c["N"], H=c["H"]).stdev
    envs = []
    for e in range(c["E"]):
        s, tp, u0, h0 = draw_target_env(rng, c["H"], 0.3, c["te"][e], 1.0 if e % 2 == 0 else -1.0)
        du = O.sample_delta_u(rng, c["N"], c["H"], stdev, c["period"])
        plans = np.clip(0.5 * rng.standard_normal((c["N"], c["H"])), -1.0, 1.0).astype(f32)
        envs.append((s, tp, u0, h0, du, plans))
    s0, tp, u0, h0, du, plans = _frozen([np.stack([e[i] for e in envs]) for i in range(6)])
    return dict(s0=s0, tp=tp, te=np.array(c["te"], f32), u0=u0, h0=h0, du=du, plans=plans)


def _oracle_cfg(N, H, period, cost, **kw):
    return O.MPPIConfig(N=N, H=H, period=period, cost_id=R.COSTS[cost], **kw)


@functools.lru_cache(maxsize=None)
def step_reference(model, cost, te=None, tp=None):
    """The oracle pair (float32, float64) of every env of the fused step; `te` / `tp` (tuples) replace the envs' own - the host
    test's teeth."""
    from test_gpu_gru_edges import oracle_pair
    c, x = STEP, step_inputs()
    te, tp = x["te"] if te is None else te, x["tp"] if tp is None else tp
    cfg = _oracle_cfg(c["N"], c["H"], c["period"], cost)
    return [oracle_pair(model, x["s0"][e], x["u0"][e], x["du"][e], tp[e], cfg, x["h0"][e], te=te[e]) for e in range(c["E"])]


@functools.lru_cache(maxsize=None)
def plans_reference(model, cost, te=None, tp=None):
    """The oracle pair of every env's given plans: a zero nominal sequence, no correction term, no shift (the reference of
    test_gpu_gru_cost_only.py)."""
    from test_gpu_gru_edges import oracle_pair
    c, x = STEP, step_inputs()
    te, tp = x["te"] if te is None else te, x["tp"] if tp is None else tp
    cfg = _oracle_cfg(c["N"], c["H"], c["period"], cost, cc_weight=0.0, shift_mode="none")
    return [oracle_pair(model, x["s0"][e], np.zeros(c["H"], f32), x["plans"][e], tp[e], cfg, x["h0"][e], te=te[e]) for e in range(c["E"])]


@functools.lru_cache(maxsize=None)
def grad_inputs(key):
    """-> dict(s0 [E,6], tp [E], te [E], h0 [E,2,32], Q [E,N,H])."""
    c = GRAD[key]
    rng = np.random.Generator(np.random.SFC64(c["seed"]))
    envs = []
    for e in range(c["E"]):
        s, tp, _, h0 = draw_target_env(rng, c["H"], 0.3, c["te"][e], 1.0 if e % 2 == 0 else -1.0)
        q = (0.5 * rng.standard_normal((c["N"], c["H"]))).astype(f32)
        q[:SCALED_ROWS] *= 3.0
        envs.append((s, tp, h0, q))
    s0, tp, h0, Q = _frozen([np.stack([e[i] for e in envs]) for i in range(4)])
    return dict(s0=s0, tp=tp, te=np.array(c["te"], f32), h0=h0, Q=Q)


@functools.lru_cache(maxsize=None)
def grad_reference(key, model, cost, with_h0, reduce, mode="clip", te=None, tp=None, clip="mode"):
    """-> (J [E,N], g [E,N,H], flagged [E,N]) in float64: gru_grad_ref.reference_of per env under that env's target equilibrium and
    target position and the limits of `mode`.  `te` / `tp` (tuples) and `clip` replace them - the host test's teeth."""
    x = grad_inputs(key)
    te, tp = x["te"] if te is None else te, x["tp"] if tp is None else tp
    clip = MODES[mode][3] if clip == "mode" else clip
    per_env = [R.reference_of(model, cost, x["s0"][e], tp[e], float(te[e]), x["h0"][e] if with_h0 else None, x["Q"][e], reduce, clip)
               for e in range(GRAD[key]["E"])]
    return tuple(_frozen([np.stack(a) for a in zip(*per_env)]))


@functools.lru_cache(maxsize=None)
def grad_reference_float32(key, model, cost, with_h0, reduce, mode="clip"):
    """The reference's gradient [E,N,H] with the network and its adjoint evaluated by torch in float32: how well float32 pins a
    rollout's gradient at all (a rollout whose inputs are clipped but for one small entry has a max |g| that float32 cannot)."""
    import torch
    from test_gpu_gru_edges import model_of
    x = grad_inputs(key)
    return np.stack([R.cost_and_grad(model_of(model), cost, x["s0"][e], x["Q"][e], x["tp"][e], float(x["te"][e]),
                                     x["h0"][e] if with_h0 else None, reduce, MODES[mode][3], eval_dtype=torch.float32)[1]
                     for e in range(GRAD[key]["E"])]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def grad_costs_float32(key, model, cost, with_h0, reduce, mode="clip"):
    """The float32 numpy oracle's costs of the gradient case's plans [E,N] (what the float64 reference's J is held against)."""
    c, x = GRAD[key], grad_inputs(key)
    control_mode, lo, hi, _ = MODES[mode]
    cfg = _oracle_cfg(c["N"], c["H"], 10, cost, cc_weight=0.0, shift_mode="none", control_mode=control_mode, horizon_reduce=reduce)
    from test_gpu_gru_edges import model_of
    return np.stack([O.gru_mppi_step(model_of(model), x["s0"][e], np.zeros(c["H"], f32), x["Q"][e], x["tp"][e], x["te"][e], cfg,
                                     h0=x["h0"][e] if with_h0 else None, low=lo, high=hi)["S"] for e in range(c["E"])])


def gradient_errors(G, g):
    """The gradient comparison's error per rollout [E,N]: max over the horizon relative to the rollout's max |g| (test_gpu_gru_grad.py)."""
    return np.abs(G - g).max(axis=2) / (np.abs(g).max(axis=2) + 1e-6)
