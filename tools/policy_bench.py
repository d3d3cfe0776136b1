#!/usr/bin/env python3
"""Development tool (GPU): fine-tuning the neural imitator on the task cost (cpmppi_dense_policy_*, train_imitator.finetune_on_cost).
Report only: nothing here is a threshold.

  --part step   wall time of one cpmppi_dense_policy_train_step at B = 4096 start states x 35 control steps (ODE_v0,
                quadratic_boundary_grad_minimal, S = 10) beside one cpmppi_dense_train_step (the MSE step, whose code this feature
                shares the tile contraction with) at the same sample count 4096 x 35, and at 4096 x 1 - the shape
                tools/imitator_bench.py records.  lr = 0: every call does the same work.
  --part run    a DAgger-trained model (the shipped schedule, E = 256, MPPI 3500 x 35) fine-tuned on the cost from the states of its
                own DAgger dataset; MPPIEngine.score_runs of the net alone on 256 fresh experiments before and after, beside the
                MPC's.  Whatever comes out is reported; nothing is claimed.

The forms of --part step run in ONE process, alternating, `--rounds` times (default 7) after a warm-up of each; a round times
`--reps` calls between two device synchronisations; the median over the rounds is reported.  -> one JSON line per part (and --out)."""
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
from cartpolesimulation_amd import _lib as L  # noqa: E402
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.train_imitator import dagger, finetune_on_cost, identity_normalization, initial_weights  # noqa: E402
from imitator_bench import medians, random_recordings  # noqa: E402

f32 = np.float32
E, ROLLOUTS, HORIZON = 256, 3500, 35


def part_step(args):
    B, H = 4096, HORIZON
    eng = MPPIEngine(1, MPPIConfig(num_rollouts=64, mpc_horizon=H))
    eng.set_dense({**initial_weights(1), **identity_normalization()})
    eng.dense_train_begin()
    rng = np.random.default_rng(0)
    s, tp, te, lab = random_recordings(rng, 64, B // 64 * H)
    s[..., 0] = rng.uniform(-0.3, 0.3, s.shape[:2])                 # near upright: the closed loop stays finite over 35 steps
    s[..., 1], s[..., 2], s[..., 3] = rng.normal(0, 1.0, s.shape[:2]), np.cos(s[..., 0]), np.sin(s[..., 0])
    dev = [eng.tensor(x) for x in (s, tp, te, lab)]
    R, T = s.shape[:2]
    starts = np.stack([rng.integers(0, R, B), rng.integers(0, T, B)], axis=1)
    rows = np.stack([np.repeat(np.arange(R), T), np.tile(np.arange(T), R)], axis=1)          # R T = B H samples, one row each
    eng.dense_policy_reserve(B, H)
    eng.dense_train_reserve(len(rows))
    forms = {"policy_train_step": eng.prepare_dense_policy_train_step(*dev[:3], starts, H, lr=0.0, clip_norm=10.0).run,
             "policy_loss_only": eng.prepare_dense_policy_loss_grad(*dev[:3], starts, H, grad=False).run,
             "mse_train_step_same_samples": eng.prepare_dense_train_step(*dev, rows, 1, 0, lr=0.0).run,
             "mse_train_step_B4096": eng.prepare_dense_train_step(*dev, starts, 1, 0, lr=0.0).run}
    rec = dict(part="step", B=B, horizon=H, substeps=10, samples=int(len(rows)), rounds=args.rounds, reps=args.reps)
    rec.update(medians(forms, args.rounds, args.reps))
    loss = float(forms["policy_loss_only"]()[0].item())
    rec["policy_loss_is_finite"] = bool(np.isfinite(loss))
    rec["policy_over_mse_same_samples"] = rec["policy_train_step_median_us"] / rec["mse_train_step_same_samples_median_us"]
    eng.close()
    return rec


def part_run(args):
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    cfg = dict(seed=11, length_of_experiment=args.length, dt=dict(saving=0.02))
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=ROLLOUTS, mpc_horizon=HORIZON))
    t0 = time.perf_counter()
    model, h = dagger(eng, cfg, experiments=E, iterations=len(args.beta.split(",")), beta=args.beta, steps_per_iteration=args.steps,
                      batch_size=64, lr=2e-3, seed=1873, graph=True, log=print)
    torch.cuda.synchronize()
    rec = dict(part="run", E=E, length_s=args.length, rollouts=ROLLOUTS, horizon=HORIZON, dagger_beta=h["beta"], dagger_steps=args.steps,
               dagger_wall_s=time.perf_counter() - t0, finetune=dict(horizon=args.horizon, epochs=args.epochs, batch_size=args.batch_size,
                                                                     lr=args.lr, clip_norm=args.clip_norm),
               score_columns=list(L.SCORE_COLUMNS))
    batch = SC.RandomExperimentSetter(cfg).draw(E, 99)              # 256 fresh experiments, the same for the three controllers
    exp = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=5)

    def score(name, **kw):
        res = exp.run_schedule(batch, graph=True, **kw)
        sc = eng.score_runs(res["states"], res["Q"], target_position_table=batch.target_position, save_every=batch.n_save,
                            sched_stride=batch.stride, period_steps=batch.n_ctrl).cpu().numpy()
        rec[name + "_score_mean"] = [float(x) for x in sc.mean(axis=0)]

    score("mppi_alone")
    score("imitator_after_dagger", imitator=model)
    data = h["dataset"]
    t0 = time.perf_counter()
    tuned, hist = finetune_on_cost(eng, data.states, data.target_position, data.target_equilibrium, horizon=args.horizon,
                                   epochs=args.epochs, batch_size=args.batch_size, lr=args.lr, clip_norm=args.clip_norm, seed=3, init=model,
                                   log=print)
    torch.cuda.synchronize()
    rec["finetune_wall_s"] = time.perf_counter() - t0
    rec["finetune_epoch_loss"] = hist["loss"]
    rec["finetune_non_finite_batches"] = int((~np.isfinite(np.array(hist["batch_loss"]))).sum())
    score("imitator_after_finetune", imitator=tuned)
    eng.close()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=["step", "run", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--beta", default="1,0.5,0.25,0", help="--part run: DAgger's schedule (default: the shipped one)")
    ap.add_argument("--steps", type=int, default=2000, help="--part run: DAgger's Adam steps per iteration")
    ap.add_argument("--length", type=float, default=10.0, help="--part run: seconds per experiment")
    ap.add_argument("--horizon", type=int, default=8, help="--part run: control steps of the differentiated closed loop")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--clip-norm", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    parts = dict(step=part_step, run=part_run)
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
