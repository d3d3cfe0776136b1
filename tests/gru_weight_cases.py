"""Models and tables of the GRU weight-image tests (test_gru_weight_cases_host.py judges them on the host, test_gpu_gru_weights.py
hands them to cpmppi_set_gru and to the kernels that read the three weight images).  Pure numpy + the oracle: no GPU.

What cpmppi_set_gru stores in the f16 split image is, for a gate row, the weight PRE-SCALED - r and z by -log2(e), n by 2 log2(e) -
and for the head the weight itself; it refuses a model in which a stored value v has !(|v| < 60000).  `stored` / `accepted` restate
that predicate in float32 as the host code evaluates it (float32(float64(scale) * float64(w))), `accept_limit` walks to its edge
with nextafter: the largest accepted float32 magnitude of a place and its successor.

PLACES: the 13 places a weight can sit in - {w_ih0, w_hh0, w_ih1, w_hh1} x {r, z, n} and w_out - each with an entry of its own
(rows and columns spread over both lane halves and both k-blocks of the fragments).

The launches are small throughout, E = 2 envs x N = 96 rollouts (three tiles) x H = 8: the models are the edge here, not the shapes.

SPLIT: the cases of the f16 split cell at the ends of its operands.  Every model is `random_model`, the scale-0.3 recipe of
test_gru_random_weights_vs_oracle with its normalisation, changed in one way:
  a+ / a-   one entry of every place of a gate matrix at +-0.9 of that gate's limit (the signs alternate from place to place; a- is a+
            mirrored): stored values of 54 000, the hi part's ulp 32
  b         half of all matrix entries scaled by 10^U(-8, -4): hi and lo are f16 subnormals or vanish
  c         the memory h0 drawn from {1, -1, 0, 1e-6, -1e-6, 0.5}
  d+ / d-   in_shift of the control input (fed at every step; the state features are fed back from the head after the first) at
            +-6.0e4, in_shift of angle_sin at 1.0e3: normalised inputs just inside the +-65504 the split can carry
  e         every in_scale 1e-6
Inputs per case as test_gru_random_weights_vs_oracle draws them, the perturbations from the oracle's sampler."""
import functools

import numpy as np

from oracle import oracle_np as O

f32 = np.float32
E, N, H = 2, 96, 8
LOG2E = 1.4426950408889634
GATES = ("r", "z", "n")
GATE_SCALE = {"r": -LOG2E, "z": -LOG2E, "n": 2.0 * LOG2E, "head": 1.0}
STORE_LIMIT = f32(60000.0)
GRU_KEYS = ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_out", "b_out")
NORM_KEYS = ("in_scale", "in_shift", "out_scale", "out_shift")
MATRICES = ("w_ih0", "w_hh0", "w_ih1", "w_hh1", "w_out")
# the limits written out (60000 / log2(e), 60000 / (2 log2(e)) and 60000, each rounded towards acceptance)
STATED_LIMITS = {"r": f32(41588.83), "z": f32(41588.83), "n": f32(20794.414), "head": f32(59999.996)}


def stored(kind, w):
    """What put16 is handed for a weight `w` of a gate row of `kind` (or of the head)."""
    return f32(np.float64(GATE_SCALE[kind]) * np.float64(f32(w)))


def accepted(kind, w):
    return bool(np.abs(stored(kind, w)) < STORE_LIMIT)


@functools.lru_cache(maxsize=None)
def accept_limit(kind):
    """-> (the largest float32 magnitude `accepted`, its float32 successor, which is not)."""
    w = f32(np.float64(STORE_LIMIT) / abs(GATE_SCALE[kind]))
    while not accepted(kind, w):
        w = np.nextafter(w, f32(0.0))
    while accepted(kind, np.nextafter(w, f32(np.inf))):
        w = np.nextafter(w, f32(np.inf))
    return f32(w), f32(np.nextafter(w, f32(np.inf)))


def _places():
    out = []
    for i, key in enumerate(("w_ih0", "w_hh0", "w_ih1", "w_hh1")):
        cols = 6 if key == "w_ih0" else 32
        for g, gate in enumerate(GATES):
            j = 3 * i + g
            out.append((key, gate, 32 * g + (5 + 7 * j) % 32, (3 + 11 * j) % cols))
    out.append(("w_out", "head", 2, 19))
    return tuple(out)


PLACES = _places()                       # (key, kind, row, column)
PLACE_IDS = tuple(f"{k}-{kind}" for k, kind, _, _ in PLACES)


def random_model(seed):
    """The recipe of test_gru_random_weights_vs_oracle at scale 0.3, normalisation included."""
    scale = 0.3
    rng = np.random.Generator(np.random.SFC64(seed))
    u = lambda *s: (scale * rng.uniform(-1, 1, s)).astype(f32)  # noqa: E731
    return dict(w_ih0=u(96, 6), w_hh0=u(96, 32), b_ih0=u(96), b_hh0=u(96), w_ih1=u(96, 32), w_hh1=u(96, 32), b_ih1=u(96),
                b_hh1=u(96), w_out=(0.3 * rng.uniform(-1, 1, (5, 32))).astype(f32), b_out=(0.1 * rng.uniform(-1, 1, 5)).astype(f32),
                in_scale=rng.uniform(0.5, 2.0, 6).astype(f32), in_shift=(0.1 * rng.uniform(-1, 1, 6)).astype(f32),
                out_scale=rng.uniform(0.5, 1.5, 5).astype(f32), out_shift=(0.05 * rng.uniform(-1, 1, 5)).astype(f32))


def with_entry(model, key, index, value):
    """A copy of `model` with model[key][index] = value."""
    m = {k: np.array(v, f32) for k, v in model.items()}
    m[key][index] = f32(value)
    return m


def at_place(model, place, value):
    key, _, row, col = place
    return with_entry(model, key, (row, col), value)


def model_a():
    return random_model(2601)


def model_b():
    """Another model, another normalisation, and one weight of a z row beyond what the f16 image takes."""
    return with_entry(random_model(2602), "w_hh1", (40, 9), 5.0e4)


# ---------------------------------------------------------------------------------------------- the split cell's cases
SPLIT_CASES = ("a+", "a-", "b", "c", "d+", "d-", "e")
H0_VALUES = np.array([1.0, -1.0, 0.0, 1e-6, -1e-6, 0.5], f32)


@functools.lru_cache(maxsize=None)
def split_case(name):
    """-> dict(model, s0 [E,6], tp [E], te [E], u0 [E,H], h0 [E,2,32], du [E,N,H]); arrays read-only."""
    seed = 2610 + SPLIT_CASES.index(name)
    m = random_model(seed)
    rng = np.random.Generator(np.random.SFC64(seed + 100))
    if name in ("a+", "a-"):
        for j, place in enumerate(PLACES[:12]):
            sign = (1.0 if j % 2 == 0 else -1.0) * (1.0 if name == "a+" else -1.0)
            m = at_place(m, place, f32(sign * 0.9) * accept_limit(place[1])[0])
    elif name == "b":
        for k in MATRICES:
            tiny = rng.uniform(0, 1, m[k].shape) < 0.5
            factor = 10.0 ** rng.uniform(-8, -4, m[k].shape)
            m[k] = np.where(tiny, m[k].astype(np.float64) * factor, m[k]).astype(f32)
    elif name in ("d+", "d-"):
        m["in_shift"] = m["in_shift"].copy()
        m["in_shift"][0] = f32(6.0e4 if name == "d+" else -6.0e4)         # Q
        m["in_shift"][3] = f32(1.0e3)                                     # angle_sin
    elif name == "e":
        m["in_scale"] = np.full(6, 1e-6, f32)
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1), 0.0) for _ in range(E)])
    u0 = (0.2 * rng.standard_normal((E, H))).astype(f32)
    h0 = (0.3 * rng.standard_normal((E, 2, 32))).astype(f32)
    if name == "c":
        h0 = H0_VALUES[rng.integers(0, len(H0_VALUES), (E, 2, 32))]
    stdev = O.MPPIConfig(N=N, H=H).stdev
    du = np.stack([O.sample_delta_u(rng, N, H, np.float64(stdev)) for _ in range(E)]).astype(f32)
    case = dict(model=m, s0=s0.astype(f32), tp=np.zeros(E, f32), te=np.ones(E, f32), u0=u0, h0=h0, du=du)
    for v in list(case.values()) + list(m.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def split_reference(name):
    """The numpy oracle's MPPI step of every env in float32 and float64 -> [(ref32, ref64)] * E.  (A saturated gate overflows exp in
    the oracle's sigmoid: 1 / (1 + inf) = 0 is the value meant.)"""
    c = split_case(name)
    cfg = O.MPPIConfig(N=N, H=H)
    out = []
    with np.errstate(over="ignore"):
        for e in range(E):
            a = O.gru_mppi_step(c["model"], c["s0"][e], c["u0"][e], c["du"][e], c["tp"][e], c["te"][e], cfg, h0=c["h0"][e])
            b = O.gru_mppi_step(c["model"], c["s0"][e], c["u0"][e], c["du"][e], c["tp"][e], c["te"][e], cfg, h0=c["h0"][e],
                                dtype=np.float64)
            out.append((a, b))
    return out


# ---------------------------------------------------------------------------------------------- what a handle is probed with
PREDICT_B = 37                           # the predict seam's batch: a ragged second tile


@functools.lru_cache(maxsize=None)
def probe_inputs():
    """The inputs of every call a handle's model is read back through, bit for bit: dict(s0 [E,6], tp, te [E], u0 [E,H], h0 [E,2,32],
    du [E,N,H], plans [E,N,H] (given control sequences), q [E] (one control per env), ps0 [B,6], pQ [B,H], ph0 [2,B,32] (the predict
    seam, B = PREDICT_B)); arrays read-only."""
    rng = np.random.Generator(np.random.SFC64(2600))
    draw = lambda n: np.stack([O.create_cartpole_state(rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1),  # noqa: E731
                                                       rng.uniform(-0.2, 0.2)) for _ in range(n)]).astype(f32)
    stdev = O.MPPIConfig(N=N, H=H).stdev
    x = dict(s0=draw(E), tp=rng.uniform(-0.05, 0.05, E).astype(f32), te=np.ones(E, f32),
             u0=(0.2 * rng.standard_normal((E, H))).astype(f32), h0=(0.3 * rng.standard_normal((E, 2, 32))).astype(f32),
             du=np.stack([O.sample_delta_u(rng, N, H, np.float64(stdev)) for _ in range(E)]).astype(f32),
             plans=np.clip(0.5 * rng.standard_normal((E, N, H)), -1.0, 1.0).astype(f32), q=rng.uniform(-1, 1, E).astype(f32),
             ps0=draw(PREDICT_B), pQ=rng.uniform(-1, 1, (PREDICT_B, H)).astype(f32),
             ph0=(0.3 * rng.standard_normal((2, PREDICT_B, 32))).astype(f32))
    for v in x.values():
        v.setflags(write=False)
    return x
