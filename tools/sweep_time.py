#!/usr/bin/env python3
"""One controller sweep's wall time: `sweep.run_sweep` - every setting of a grid x the same experiments as ONE device loop with per-env
tuning rows and one score launch - against the same settings run one handle at a time (an engine of `--experiments` envs per
setting, its own device loop and score launch).  Host clock around work that ends in a synchronise, engine creation and the score
included; the sweep `--reps` times, launched and captured.  The two sides' scores are not compared here: the launch plan picks the
build of the rollout kernel by the launch's size, and the builds do not round alike, so a 10 s closed loop of 4 envs is not the one of
4 x settings envs bit for bit; tests/test_gpu_sweep.py compares a setting with its plain run at a size where both get the same build.

``--optimizer rpgd`` (or ``gradient``): the same for the fused rpgd / gradient optimizer on predictor ODE at its shipped sizes - one
loop with a row per env (run_sweep(optimizer=...)) against one scalar fused optimizer of `--experiments` envs per setting, one after
another; the grid is learning_rate x ep_weight_up.

Usage: python tools/sweep_time.py [--settings 8x8] [--experiments 4] [--length 10] [--reps 2] [--skip-single-captured]
                                  [--optimizer mppi|rpgd|gradient]
Development tool (not part of the product).  Prints one JSON line."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cartpolesimulation_amd import schedule as SC  # noqa: E402
from cartpolesimulation_amd import sweep as SW  # noqa: E402
from cartpolesimulation_amd.configs import TUNING_COLUMNS, MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.harness import BatchedCartPoleExperiment  # noqa: E402


def one_handle_at_a_time(cfg, settings, batch, seed, graph):
    """-> scores [settings, experiments, 5]: a handle, a device loop and a score launch per setting."""
    X, out = batch.E, []
    for k, s in enumerate(settings):
        fields = {n: v for n, v in s.items() if n not in TUNING_COLUMNS[:7]}          # LBD, SQRTRHOINV
        weights = {n: v for n, v in s.items() if n in TUNING_COLUMNS[:7]}             # the cost vector's entries
        eng = MPPIEngine(X, dataclasses.replace(cfg, cost_weights=dict(cfg.cost_weights or {}, **weights), **fields))
        res = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=seed).run_schedule(
            batch, env_offset=X * k, graph=graph)
        out.append(eng.score_runs(res["states"], res["Q"], target_position_table=eng.tensor(batch.target_position.astype(np.float32)),
                                  save_every=batch.n_save, sched_stride=batch.stride, period_steps=batch.n_ctrl).cpu().numpy())
        eng.close()
    return np.stack(out)


def one_optimizer_at_a_time(name, settings, batch, seed, graph):
    """-> scores [settings, experiments, 5]: a scalar fused optimizer, a device loop and a score launch per setting."""
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    cls = {"rpgd": optimizer_rpgd, "gradient": optimizer_gradient}[name]
    out = []
    for s in settings:
        opt = cls(seed=seed, num_envs=batch.E, fused=True, learning_rate=s["learning_rate"], cost_weights=dict(ep_weight_up=s["ep_weight_up"]))
        opt.configure(predictor_specification="ODE")
        eng = opt.engine
        res = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=seed).run_schedule(
            batch, graph=graph, optimizer=opt)
        out.append(eng.score_runs(res["states"], res["Q"], target_position_table=eng.tensor(batch.target_position.astype(np.float32)),
                                  save_every=batch.n_save, sched_stride=batch.stride, period_steps=batch.n_ctrl).cpu().numpy())
        eng.close()
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="8x8", help="values of LBD (rpgd / gradient: of learning_rate) x values of ep_weight_up")
    ap.add_argument("--optimizer", choices=SW.OPTIMIZERS, default="mppi")
    ap.add_argument("--experiments", type=int, default=4)
    ap.add_argument("--length", type=float, default=10.0, help="seconds per experiment")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-single-captured", action="store_true")
    args = ap.parse_args()
    a, b = (int(x) for x in args.settings.split("x"))
    grid = dict(LBD=np.geomspace(25.0, 400.0, a), ep_weight_up=np.linspace(10.0, 90.0, b))
    cfg = MPPIConfig()                                         # the shipped controller
    batch = SC.RandomExperimentSetter(dict(seed=1, length_of_experiment=args.length)).draw(args.experiments, 1)
    out = dict(settings=a * b, experiments=args.experiments, seconds=args.length, rollouts=cfg.num_rollouts, horizon=cfg.mpc_horizon)
    kw = {}
    if args.optimizer != "mppi":                               # the optimizer's own shipped sizes, on the predictor it ships with
        grid = dict(learning_rate=np.geomspace(0.01, 0.2, a), ep_weight_up=np.linspace(10.0, 90.0, b))
        cfg, kw = MPPIConfig(predictor_type="ODE"), dict(optimizer=args.optimizer)
        out.update(optimizer=args.optimizer, rollouts=16 if args.optimizer == "rpgd" else 40)
    swept = None
    for graph in (False, True):
        for rep in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            swept = SW.run_sweep(cfg, grid, batch, seed=3, graph=graph, **kw)
            torch.cuda.synchronize()
            out[f"sweep_graph{int(graph)}_rep{rep}_s"] = round(time.perf_counter() - t0, 3)
    for graph in (False,) if args.skip_single_captured else (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        single = one_handle_at_a_time(cfg, swept["settings"], batch, 3, graph) if args.optimizer == "mppi" else \
            one_optimizer_at_a_time(args.optimizer, swept["settings"], batch, 3, graph)
        torch.cuda.synchronize()
        out[f"one_handle_at_a_time_graph{int(graph)}_s"] = round(time.perf_counter() - t0, 3)
        assert single.shape == swept["scores"].shape and np.isfinite(single).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
