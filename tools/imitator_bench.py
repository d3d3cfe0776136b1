#!/usr/bin/env python3
"""Development tool (GPU): the times of the neural imitator (cpmppi_dense_*), each beside a baseline that is not the code under test.

  --part train     wall time of one cpmppi_dense_train_step (two launches) at (B = 64, P = 1) and (B = 4096, P = 1), beside the same
                   training step written in eager PyTorch-ROCm on the same device: torch.nn.Linear x 3 with tanh, the mean squared
                   error, backward, torch.optim.Adam - and the loss-only call
  --part control   cpmppi_dense_control at E = 256 and 8192
  --part loop      one control period of the CAPTURED device loop at E = 256 (harness.ScheduleRun, 10 periods per graph) with the
                   imitator as the controller, beside the fused MPPI period at the shipped 3500 rollouts x 35 steps

The forms of a part run in ONE process, alternating, `--rounds` times (default 7); a round times `--reps` calls between two device
synchronisations after a warm-up of each form; the median over the rounds is reported.  lr = 0 in the library's steps: every call
does the same work.  A job script runs each part under its own time limit.  -> one JSON line per part (and --out FILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.train_imitator import initial_weights  # noqa: E402
from brunton_bench import timed  # noqa: E402

f32 = np.float32


def medians(forms, rounds, reps):
    """{name: a callable that enqueues one call} -> {name_median_us, name_min_max_us}."""
    ms = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    for _ in range(rounds):
        for k, fn in forms.items():
            fn()
            ms[k].append(timed(fn, reps))
    out = {k + "_median_us": float(np.median(v)) * 1e3 for k, v in ms.items()}
    out.update({k + "_min_max_us": [min(v) * 1e3, max(v) * 1e3] for k, v in ms.items()})
    return out


def random_recordings(rng, R, T):
    angle = rng.uniform(-np.pi, np.pi, (R, T))
    s = np.stack([angle, rng.normal(0, 4.0, (R, T)), np.cos(angle), np.sin(angle), rng.uniform(-0.19, 0.19, (R, T)),
                  rng.normal(0, 0.5, (R, T))], axis=-1).astype(f32)
    return s, rng.uniform(-0.15, 0.15, (R, T)).astype(f32), np.ones((R, T), f32), rng.uniform(-1, 1, (R, T)).astype(f32)


def part_train(args):
    eng = MPPIEngine(1, MPPIConfig(num_rollouts=64, mpc_horizon=2))
    model = initial_weights(1)
    eng.set_dense(model)
    eng.dense_train_begin()
    rng = np.random.default_rng(0)
    rec = dict(part="train", rounds=args.rounds, reps=args.reps)
    for B in (64, 4096):
        s, tp, te, lab = (eng.tensor(x) for x in random_recordings(rng, 16, 256))
        windows = np.stack([rng.integers(0, 16, B), rng.integers(0, 256, B)], axis=1)
        step = eng.prepare_dense_train_step(s, tp, te, lab, windows, 1, 0, lr=0.0)
        loss = eng.prepare_dense_loss_grad(s, tp, te, lab, windows, 1, 0, grad=False)
        # the same step in eager PyTorch on the same samples
        net = torch.nn.Sequential(torch.nn.Linear(7, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                                  torch.nn.Linear(32, 1)).to(eng.device)
        opt = torch.optim.Adam(net.parameters(), lr=0.0)
        r, t = torch.as_tensor(windows[:, 0]).to(eng.device), torch.as_tensor(windows[:, 1]).to(eng.device)
        x = torch.cat([s[r, t, 1:6], te[r, t, None], tp[r, t, None]], dim=1).contiguous()
        y = lab[r, t].contiguous()

        def eager():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(net(x)[:, 0], y).backward()
            opt.step()

        m = medians({"dense_train_step": step.run, "dense_loss_only": loss.run, "eager_pytorch_step": eager}, args.rounds, args.reps)
        rec[f"B{B}"] = m
    eng.close()
    return rec


def part_control(args):
    rec = dict(part="control", rounds=args.rounds, reps=args.reps)
    rng = np.random.default_rng(1)
    for E in (256, 8192):
        eng = MPPIEngine(1, MPPIConfig(num_rollouts=64, mpc_horizon=2))
        eng.set_dense(initial_weights(1))
        s, tp, te, _ = random_recordings(rng, 1, E)
        call = eng.prepare_dense_control(eng.tensor(s[0]), eng.tensor(tp[0]), eng.tensor(te[0]))
        rec[f"E{E}"] = medians({"dense_control": call.run}, args.rounds, args.reps)
        eng.close()
    return rec


def part_loop(args):
    """Wall time per control period of the captured loop (controller + plant step, 10 periods per graph replay), E = 256."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import ScheduleRun
    E, periods = 256, 200
    cfg = dict(seed=5, length_of_experiment=periods * 0.02, dt=dict(saving=0.02))
    batch = SC.RandomExperimentSetter(cfg).draw(E, 6)
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=3500, mpc_horizon=35))
    rec = dict(part="loop", E=E, periods=periods, rounds=args.rounds, rollouts=3500, horizon=35)
    ms = {"imitator_period": [], "fused_mppi_period": []}
    for _ in range(args.rounds + 1):                           # (the first round is the warm-up)
        for name, kw in (("imitator_period", dict(imitator=initial_weights(1))), ("fused_mppi_period", {})):
            run = ScheduleRun(eng, batch, 3, **kw)
            run.capture(10)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while run.periods_left:
                run.enqueue_next()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / run.T * 1e6)
            run.finish()
            torch.cuda.synchronize()
    for k, v in ms.items():
        rec[k + "_median_us"], rec[k + "_min_max_us"] = float(np.median(v[1:])), [min(v[1:]), max(v[1:])]
    eng.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=["train", "control", "loop", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    parts = dict(train=part_train, control=part_control, loop=part_loop)
    lines = []
    for name in (parts if args.part == "all" else [args.part]):
        rec = parts[name](args)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
