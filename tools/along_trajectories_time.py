#!/usr/bin/env python3
"""Control along recorded trajectories, timed: `--recordings` x `--rows` synthetic recordings, `--num-evals` copies of each, as ONE
device loop (harness.ReplayRun: the fused MPPI step + one cpmppi_replay_step per row), launched and captured, against the way the
package did the same thing before the loop existed - paced by the host with its public calls: per row the recorded rows expanded
K-fold with torch on the device, one `engine.step`, the mean over the copies and the row's bookkeeping with small torch launches.
Host clock around work that ends in a synchronise; one warm-up run of every form, then `--reps` timed ones; the bare step alone
(`--reps` x `--rows` launches of the same engine) for the loop's floor.

Usage: python tools/along_trajectories_time.py [--recordings 120] [--rows 500] [--num-evals 64] [--rollouts 1024] [--horizon 50]
                                               [--predictor ODE] [--reps 3] [--only launched|captured|host|step]
Development tool (not part of the product).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.harness import ReplayBuffers, ReplayRun  # noqa: E402

f32 = np.float32
SEED = 3


def synthetic(R, T, seed=1):
    rng = np.random.Generator(np.random.SFC64(seed))
    angle = rng.uniform(-0.5, 0.5, (R, T)).astype(f32)
    states = np.stack([angle, rng.uniform(-1, 1, (R, T)).astype(f32), np.cos(angle), np.sin(angle),
                       rng.uniform(-0.1, 0.1, (R, T)).astype(f32), rng.uniform(-0.3, 0.3, (R, T)).astype(f32)], axis=-1).astype(f32)
    return dict(states=states, rows=np.full(R, T, np.uint32), tp=rng.uniform(-0.1, 0.1, (R, T)).astype(f32),
                te=np.ones((R, T), f32), L=np.full((R, T), 0.395, f32))


def device_loop(eng, rec, K, graph):
    buf = ReplayBuffers(eng, rec["states"], rec["rows"], K, rec["tp"], rec["te"], L=rec["L"])
    return ReplayRun(eng, buf, SEED).run(graph=graph, steps_per_graph=10)["Q"]


def host_paced(eng, rec, K):
    """What a caller of the public entry points did per row before: index, expand, step, reduce."""
    R, T = rec["states"].shape[:2]
    states, tp, te, L = (eng.tensor(rec[k]) for k in ("states", "tp", "te", "L"))
    u_nom, out = eng.zeros(R * K, eng.H), eng.empty(R, T)
    for c in range(T):
        s = states[:, c].repeat_interleave(K, dim=0)
        Q, _ = eng.step(s, u_nom, tp[:, c].repeat_interleave(K), te[:, c].repeat_interleave(K), L=L[:, c].repeat_interleave(K),
                        seed=SEED, offset=c, env_offset=0)
        out[:, c] = Q.reshape(R, K).double().mean(dim=1).float()
    return out


def bare_steps(eng, rec, K, n):
    R = rec["states"].shape[0]
    E = R * K
    s = eng.tensor(np.repeat(rec["states"][:, 0], K, axis=0))
    call = eng.prepare_step(s, eng.zeros(E, eng.H), eng.zeros(E), eng.zeros(E) + 1.0, L=eng.zeros(E) + 0.395, seed=SEED, offset=0,
                            env_offset=0)
    for c in range(n):
        call.run(offset=c)


def timed(fn, reps):
    fn()                                                       # warm-up: allocations, the first launch of every kernel
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=120)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--num-evals", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--predictor", default="ODE", choices=["ODE", "ODE_v0"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["launched", "captured", "host", "step"])
    args = ap.parse_args()
    R, T, K = args.recordings, args.rows, args.num_evals
    rec = synthetic(R, T)
    eng = MPPIEngine(R * K, MPPIConfig(num_rollouts=args.rollouts, mpc_horizon=args.horizon, predictor_type=args.predictor))
    forms = dict(launched=lambda: device_loop(eng, rec, K, False), captured=lambda: device_loop(eng, rec, K, True),
                 host=lambda: host_paced(eng, rec, K), step=lambda: bare_steps(eng, rec, K, T))
    out = dict(recordings=R, rows=T, num_evals=K, envs=R * K, rollouts=args.rollouts, horizon=args.horizon, predictor=args.predictor)
    for name, fn in forms.items():
        if args.only in (None, name):
            times = timed(fn, args.reps)
            out[name + "_s"] = [round(t, 4) for t in times]
            out[name + "_us_per_period"] = round(min(times) / T * 1e6, 1)
    if args.only is None:
        a, b = device_loop(eng, rec, K, True).cpu().numpy(), host_paced(eng, rec, K).cpu().numpy()
        out["captured_vs_host_paced_max_abs"] = float(np.abs(a - b).max())     # (the two means may round apart by an ulp)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
