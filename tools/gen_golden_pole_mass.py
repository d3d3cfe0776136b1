"""Golden vectors for predictor_type "ODE" with a pole mass PER ROW: tests/golden/ode_pole_mass.npz, produced by the reference's own
next_state_predictor_ODE (SI_Toolkit_ASF/ToolkitCustomization/predictors_customization.py:25-69) under the import stand-ins of
oracle/ref_shims.py, called with variable_parameters.L[B] and variable_parameters.m_pole[B] - both of which it broadcasts per row
(:51-64).  TEST INFRASTRUCTURE, our own code; usage, from a CartPoleSimulation checkout (as oracle/gen_golden_ode.py):
    cd <reference checkout> && python -B <this repository>/tools/gen_golden_pole_mass.py
It also checks, on the CPU, that the rollout fixture stays inside the flagged-row cap of the GPU test's rule on the oracle's own
rounding-level realisations alone (no rounding-sensitive row at all), and that oracle_np.ode_step reproduces every value bit for bit."""
import hashlib
import os
import sys
from dataclasses import replace
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()
os.chdir(ref_shims.REFERENCE_ROOT)
from SI_Toolkit_ASF.ToolkitCustomization.predictors_customization import next_state_predictor_ODE  # noqa: E402
from CartPole.state_utilities import create_cartpole_state as _ccs  # noqa: E402

f32 = np.float32
OUT = os.path.join(ROOT, "tests", "golden")
DT, S_SUB = 0.02, 10
M_RANGE, L_RANGE = (0.015, 0.15), (0.2, 0.5)          # cartpole_physical_parameters.yml `m_pole:` updater range; pole lengths
lib = ref_shims.NumpyLibrary()
rng = np.random.Generator(np.random.SFC64(2024))


def state(a, ad, x, xd):
    return _ccs({"angle": a, "angleD": ad, "position": x, "positionD": xd}).astype(f32)


def stepper(L, m_pole):
    return next_state_predictor_ODE(DT, S_SUB, lib, batch_size=1, variable_parameters=SimpleNamespace(L=L, m_pole=m_pole),
                                    disable_individual_compilation=True)


out = {}
# single control steps from random states, every row with its own length and mass
B = 64
s = np.stack([state(a, ad, x, xd) for a, ad, x, xd in zip(rng.uniform(-np.pi, np.pi, B), rng.uniform(-12, 12, B),
                                                            rng.uniform(-0.19, 0.19, B), rng.uniform(-1.5, 1.5, B))])
Q = rng.uniform(-1, 1, (B, 1)).astype(f32)
L, m = rng.uniform(*L_RANGE, B).astype(f32), rng.uniform(*M_RANGE, B).astype(f32)
out.update({"kat/s": s, "kat/Q": Q[:, 0], "kat/L": L, "kat/m_pole": m, "kat/s_next": stepper(L, m).step(s, Q)})

# rollouts: half the rows near upright, half hanging (no fast-spin regime: the rounding-sensitive rows are ode_predictor.npz's)
n, H = 32, 20
s0 = np.stack([state(a, ad, x, xd) for a, ad, x, xd in zip(
    np.concatenate([rng.uniform(-0.3, 0.3, n // 2), np.pi + rng.uniform(-0.3, 0.3, n // 2)]), rng.uniform(-1.0, 1.0, n),
    rng.uniform(-0.1, 0.1, n), rng.uniform(-0.3, 0.3, n))])
Qr = np.clip(0.6 * rng.standard_normal((n, H)), -1, 1).astype(f32)
Lr, mr = rng.uniform(*L_RANGE, n).astype(f32), rng.uniform(*M_RANGE, n).astype(f32)
ns = stepper(Lr, mr)
traj = np.zeros((n, H + 1, 6), f32)
traj[:, 0] = s0
for k in range(H):                                     # predict_core as ODE_module.py:46-50 drives it
    traj[:, k + 1] = ns.step(traj[:, k], Qr[:, k, np.newaxis])
out.update({"roll/s0": s0, "roll/Q": Qr, "roll/L": Lr, "roll/m_pole": mr, "roll/traj": traj})

# ---- checks on the CPU -------------------------------------------------------------------------------------------------
from oracle import oracle_np as O  # noqa: E402
from oracle import oracle_c as OC  # noqa: E402
from oracle import parity as PU  # noqa: E402

assert np.array_equal(O.ode_step(s, Q[:, 0], L=L, m_pole=m), out["kat/s_next"]), "oracle_np.ode_step (arrays) != the reference"
rows = np.stack([O.ode_step(s[i:i + 1], Q[i], L=L[i], m_pole=m[i])[0] for i in range(B)])
assert np.array_equal(rows, out["kat/s_next"]), "oracle_np.ode_step (row by row) != the reference"
t = s0
for k in range(H):
    t = O.ode_step(t, Qr[:, k], L=Lr, m_pole=mr)
    assert np.array_equal(t, traj[:, k + 1]), f"oracle_np.ode_step != the reference at control step {k}"
default = O.ode_step(s, Q[:, 0], L=L)
print("one control step: the mass moves states by up to", float(np.abs(default - out["kat/s_next"]).max()))
# the flagged-row cap: rows on which the C oracle's own rounding-level realisations (the set of tests/test_gpu_pole_mass_rows.py)
# scatter by more than a quarter of the band
def circular(d):
    d = np.asarray(d, np.float64)
    d[..., O.ANGLE_IDX] = np.angle(np.exp(1j * d[..., O.ANGLE_IDX]))
    return d


ocfg = O.MPPIConfig(N=1, H=H, integrator="ODE")
gap = np.zeros(traj.shape)
for i in range(n):
    p_i = replace(O.DEFAULT_PARAMS, m_pole=mr[i])
    cfg, row = OC.make_config(ocfg, p_i), dict(Q=Qr[i:i + 1], L=Lr[i:i + 1])
    base = OC.predict(cfg, s0[i:i + 1], **row)
    assert (np.abs(circular(base - traj[i:i + 1])) <= PU.band(traj[i:i + 1])).all(), f"the C oracle leaves the band on row {i}"
    alts = [OC.predict(OC.make_config(ocfg, p_i, mode="f64sub"), s0[i:i + 1], **row)]
    if OC.fma_lib() is not None:
        alts.append(OC.predict(cfg, s0[i:i + 1], use_lib=OC.fma_lib(), **row))
    for col in (O.ANGLED_IDX, O.POSITIOND_IDX, O.POSITION_IDX, O.ANGLE_COS_IDX, O.ANGLE_SIN_IDX):
        sp = s0[i:i + 1].copy()
        sp[:, col] = np.nextafter(sp[:, col], f32(np.inf))
        alts.append(OC.predict(cfg, sp, **row))
    alts.append(OC.predict(cfg, s0[i:i + 1], Q=np.nextafter(Qr[i:i + 1], f32(np.inf)), L=Lr[i:i + 1]))
    try:
        for seed in (1, 2, 3):
            OC.set_trig_jitter(seed)
            alts.append(OC.predict(cfg, s0[i:i + 1], **row))
    finally:
        OC.set_trig_jitter(0)
    for a in alts:
        gap[i] = np.maximum(gap[i], np.abs(circular(a - traj[i:i + 1])[0]))
sensitive = (gap > 0.25 * PU.band(traj)).reshape(n, -1).any(axis=1)
print("rounding-sensitive rollout rows:", int(sensitive.sum()), "of", n, "; largest scatter / band:", float((gap / PU.band(traj)).max()))
assert not sensitive.any(), "the rollout fixture must stay clear of the flagged bucket on the oracle's realisations alone"

path = os.path.join(OUT, "ode_pole_mass.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
for rel in ("SI_Toolkit_ASF/ToolkitCustomization/predictors_customization.py", "CartPole/cartpole_equations.py",
            "CartPole/state_utilities.py", "CartPole/cartpole_parameters.py", "cartpole_physical_parameters.yml"):
    print(hashlib.sha256(open(os.path.join(ref_shims.REFERENCE_ROOT, rel), "rb").read()).hexdigest(), "", rel)
print("numpy", np.__version__)
