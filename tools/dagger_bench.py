#!/usr/bin/env python3
"""Development tool (GPU): the times of DAgger for the neural imitator (cpmppi_dagger_step, harness.DaggerController,
train_imitator.dagger), each beside a baseline that is not the code under test.  E = 256 experiments, MPPI 3500 rollouts x 35 steps.

  --part period     one control period of the CAPTURED device loop (harness.ScheduleRun, 10 periods per graph) with DAgger
                    (expert step + dagger step + plant), beside the two loops it is made of, whose code this feature does not
                    touch: the fused MPPI period and the imitator period.  Reported: the three, and DAgger as a multiple of MPPI.
  --part iteration  wall time of ONE whole DAgger iteration on the device (run with beta = 0 + the Adam steps of one epoch), beside
                    the route through the host that it replaces: generate_dataset(imitator=) -> control_along_trajectories ->
                    train_imitator (one epoch), at the same sizes.  Report only.
  --part run        a real run with the shipped schedule (beta = 1, 0.5, 0.25, 0): the on-policy disagreement and the mean of
                    score_runs per iteration.  Whatever comes out is reported; nothing is claimed.

The forms of a part run in ONE process, alternating, `--rounds` times (default 7) after a warm-up round; the median over the rounds
is reported.  A job script runs each part under its own time limit.  -> one JSON line per part (and --out FILE)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cartpolesimulation_amd import _lib as L  # noqa: E402
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.train_imitator import dagger, identity_normalization, initial_weights  # noqa: E402

f32 = np.float32
E, ROLLOUTS, HORIZON = 256, 3500, 35


def median_and_range(v):
    return float(np.median(v)), [float(min(v)), float(max(v))]


def part_period(args):
    """Wall time per control period of the captured loop, 10 periods per graph replay."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import DaggerDataset, ScheduleRun
    periods = 200
    cfg = dict(seed=5, length_of_experiment=periods * 0.02, dt=dict(saving=0.02))
    batch = SC.RandomExperimentSetter(cfg).draw(E, 6)
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=ROLLOUTS, mpc_horizon=HORIZON))
    model = initial_weights(1)
    rec = dict(part="period", E=E, periods=periods, rounds=args.rounds, rollouts=ROLLOUTS, horizon=HORIZON)
    beta = np.full(E, 0.5, f32)
    forms = {"dagger_period": lambda: dict(imitator=model, dagger=(model, DaggerDataset(eng, E, batch.n_periods + 1), beta, 7)),
             "fused_mppi_period": dict, "imitator_period": lambda: dict(imitator=model)}
    us = {k: [] for k in forms}
    for _ in range(args.rounds + 1):                           # (the first round is the warm-up)
        for name, kw in forms.items():
            run = ScheduleRun(eng, batch, 3, **kw())
            run.capture(10)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while run.periods_left:
                run.enqueue_next()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / run.T * 1e6)
            run.finish()
            torch.cuda.synchronize()
    for k, v in us.items():
        rec[k + "_median_us"], rec[k + "_min_max_us"] = median_and_range(v[1:])
    rec["dagger_over_mppi"] = rec["dagger_period_median_us"] / rec["fused_mppi_period_median_us"]
    rec["dagger_minus_mppi_us"] = rec["dagger_period_median_us"] - rec["fused_mppi_period_median_us"]
    eng.close()
    return rec


def part_iteration(args):
    """One DAgger iteration (beta = 0: the imitator drives, the MPC labels; then one epoch of Adam steps) on the device and through
    the host.  Both start from the same model with a fixed normalisation; they draw different batches and are not compared in value."""
    from cartpolesimulation_amd import recording as REC
    from cartpolesimulation_amd.along_trajectories import control_along_trajectories, stack_recordings
    from cartpolesimulation_amd.train_imitator import train_imitator
    periods, B = 100, 64
    cfg = dict(seed=5, length_of_experiment=periods * 0.02, dt=dict(saving=0.02))
    mppi = MPPIConfig(num_rollouts=ROLLOUTS, mpc_horizon=HORIZON)
    steps = -(-(E * (periods + 1)) // B)                       # the steps of one epoch over E recordings of periods + 1 rows
    model = {**initial_weights(1), **identity_normalization()}
    rec = dict(part="iteration", E=E, periods=periods, batch_size=B, steps=steps, rounds=args.rounds, rollouts=ROLLOUTS, horizon=HORIZON)
    s = {"device_dagger_iteration": [], "host_route": [], "host_generate": [], "host_relabel": [], "host_train": []}
    eng = MPPIEngine(E, mppi)
    for r in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dagger(eng, cfg, experiments=E, iterations=1, beta=0.0, steps_per_iteration=steps, batch_size=B, lr=2e-3, seed=r, init=model, graph=True)
        torch.cuda.synchronize()
        s["device_dagger_iteration"].append(time.perf_counter() - t0)
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            paths = REC.generate_dataset(eng, E, os.path.join(tmp, "recordings"), config=cfg, seed=r, imitator=model, graph=True)
            t1 = time.perf_counter()
            relabelled = control_along_trajectories(paths, config=mppi, num_evals=1, seed=r)
            states, rows, attrs = stack_recordings(paths)
            t2 = time.perf_counter()
            train_imitator(eng, states, attrs["target_position"], attrs["target_equilibrium"], relabelled["Q"], rows, epochs=1, batch_size=B,
                           lr=2e-3, seed=r, init=model)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
        for k, v in (("host_route", t3 - t0), ("host_generate", t1 - t0), ("host_relabel", t2 - t1), ("host_train", t3 - t2)):
            s[k].append(v)
    for k, v in s.items():
        rec[k + "_median_s"], rec[k + "_min_max_s"] = median_and_range(v[1:])
    rec["host_over_device"] = rec["host_route_median_s"] / rec["device_dagger_iteration_median_s"]
    eng.close()
    return rec


def part_run(args):
    """The shipped schedule once, at the data generator's experiment length: what comes out."""
    cfg = dict(seed=11, length_of_experiment=args.length, dt=dict(saving=0.02))
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=ROLLOUTS, mpc_horizon=HORIZON))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model, h = dagger(eng, cfg, experiments=E, iterations=len(args.beta.split(",")), beta=args.beta, steps_per_iteration=args.steps,
                      batch_size=64, lr=2e-3, seed=1873, graph=True, log=print)
    torch.cuda.synchronize()
    rec = dict(part="run", E=E, length_s=args.length, rollouts=ROLLOUTS, horizon=HORIZON, steps_per_iteration=args.steps, batch_size=64,
               lr=2e-3, wall_s=time.perf_counter() - t0, beta=h["beta"], disagreement=h["disagreement"], expert_share=h["expert_share"],
               first_and_last_batch_loss=[[x[0], x[-1]] for x in h["batch_loss"]], score_columns=list(L.SCORE_COLUMNS),
               score_mean=[[float(x) for x in s.mean(axis=0)] for s in h["scores"]])
    # the trained net alone in the loop, on a batch it has not seen
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    batch = SC.RandomExperimentSetter(cfg).draw(E, 99)
    exp = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=5)
    for name, kw in (("imitator_alone", dict(imitator=model)), ("mppi_alone", {})):
        res = exp.run_schedule(batch, graph=True, **kw)
        sc = eng.score_runs(res["states"], res["Q"], target_position_table=batch.target_position, save_every=batch.n_save,
                            sched_stride=batch.stride, period_steps=batch.n_ctrl).cpu().numpy()
        rec[name + "_score_mean"] = [float(x) for x in sc.mean(axis=0)]
    eng.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=["period", "iteration", "run", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--beta", default="1,0.5,0.25,0", help="--part run: the schedule (default: the shipped one)")
    ap.add_argument("--steps", type=int, default=2000, help="--part run: Adam steps per iteration")
    ap.add_argument("--length", type=float, default=10.0, help="--part run: seconds per experiment")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    parts = dict(period=part_period, iteration=part_iteration, run=part_run)
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
