#!/usr/bin/env python3
"""Development tool (GPU): the time of one cpmppi_ode_fit_step (loss, forward-mode gradient, Adam: two launches) at B = 4096 windows x
horizon 20, for 1 trained parameter (u_max, the reference's shipped choice) and for all 8, beside cpmppi_brunton over the SAME 4096
starts - the forward-only sibling (rotation flavours of the substep, per-step statistics) - and the loss-only call.

All forms run in ONE process, alternating, `--rounds` times (default 7); a round times `--reps` calls between two device
synchronisations after a warm-up of each form.  lr = 0: the steps do not move the parameters, every call does the same work.
-> one JSON line per (predictor, math mode) (and --out FILE)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cartpolesimulation_amd._lib import ODE_FIT_NAMES  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from brunton_bench import make_recordings, timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    H, R, count = 20, 16, 256                              # 16 recordings x 256 starts = 4096 windows
    T = count + H + 4
    lines = []
    for predictor in ("ODE", "ODE_v0"):
        for math_mode in ("fast", "precise"):
            eng = MPPIEngine(1, MPPIConfig(num_rollouts=64, mpc_horizon=H, predictor_type=predictor, math_mode=math_mode))
            states, Q = make_recordings(eng, R, T)
            windows = np.array([(r, t) for r in range(R) for t in range(count)])
            scale = np.ones(5, np.float32)
            eng.ode_fit_begin()
            calls = {"step_1": eng.prepare_ode_fit_step(states, Q, windows, H, ("u_max",), scale, lr=0.0),
                     "step_8": eng.prepare_ode_fit_step(states, Q, windows, H, ODE_FIT_NAMES, scale, lr=0.0),
                     "loss_only_1": eng.prepare_ode_fit_loss_grad(states, Q, windows, H, ("u_max",), scale, grad=False),
                     "brunton": eng.prepare_brunton(states, Q, horizon=H, count=count)}
            ms = {k: [] for k in calls}
            for c in calls.values():
                c.run()
            for _ in range(args.rounds):
                for k, c in calls.items():
                    c.run()
                    ms[k].append(timed(c.run, args.reps))
            rec = dict(predictor=predictor, math_mode=math_mode, windows=len(windows), horizon=H, rounds=args.rounds, reps=args.reps,
                       **{k + "_median_us": float(np.median(v)) * 1e3 for k, v in ms.items()},
                       **{k + "_min_max_us": [min(v) * 1e3, max(v) * 1e3] for k, v in ms.items()})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
    return lines


if __name__ == "__main__":
    main()
