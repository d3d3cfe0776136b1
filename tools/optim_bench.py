#!/usr/bin/env python3
"""Timing of one controller step per optimizer section of config_optimizers.yml at its shipped hyper-parameters, through
the controller seam (controller_mpc.configure(name) / .step), for E problem instances at once (GPU box).

  python tools/optim_bench.py [--envs 64] [--steps 30] [--predictor-specification ODE]
(ODE = the shipped config_controllers.yml's predictor: Euler-Cromer, no edge bounce; default ODE_v0)
Prints one JSON object per optimizer: ms per controller step (all envs), candidate plans evaluated per second.

  python tools/optim_bench.py --fused [--envs 64] [--predictor-specification ODE] [--datagen 256,10]
                              [--optimizers cem-tf,cem-naive-grad-tf,cem-grad-bharadhwaj-tf] [--staged-repeats 3]
The optimizers with a fused control step (default: gradient-tf and rpgd; the three CEM sections by name), staged and fused
(cpmppi_rpgd_step / cpmppi_cem_step) in the SAME process: one record each through the controller seam ("staged", "fused":
controller.step, the control read back every step) and one for the fused step on device tensors with the step counter on the device
("fused_device": optimizer.step_device, no read-back).  ``--staged-repeats R``: the staged record R times over (its max - min
spread is the margin a comparison allows).  ``--datagen E,seconds``: E experiments of that length through the closed loop
(harness.run_schedule), launched + staged against captured + fused (the first of --optimizers, shipped sizes).

  python tools/optim_bench.py --gru [--envs 64] [--steps 30] [--cost-only-shapes 1x200x35,64x200x35,256x200x35,256x1024x50]
The neural predictor (GRU-6IN-32H1-32H2-5OUT, synthetic weights drawn as bench.py's C5_gru line draws them) under the three
optimizers that run on it - cem-tf, cem-gmm-tf, random-action-tf - through the controller seam, one record each; then, per
E x N x H of --cost-only-shapes, the cost-only launch (cpmppi_rollout_cost_gru) against the fused GRU step handed the same
[E,N,H] as delta_u with a zero nominal sequence (cpmppi_step: the same rollouts plus the MPPI update and its finalize launch) in
ONE process, the two alternating: device time from events around batches of back-to-back launches, the median over the rounds and
each column's min - max scatter.  Last, per E x N x H of --cem-shapes and math mode, the cem control step over the network, staged
(optimizer_cem(gru_model=...).step: cem_outer_it x (cem_sample, cpmppi_rollout_cost_gru, cem_update), the shift, the memory through
the predict seam) against fused (gru_fused=True: cpmppi_cem_step_gru + cpmppi_gru_advance), alternating in this one process:
"fused" through the same ``step`` on the same device state, "fused_device" through ``step_device`` with the step counter on the
device; per control step the device time between two events around a batch of steps and the wall time of the batch, medians over
the rounds with min and max, and whether the fused step stays within the staged median + the staged runs' own min - max spread.

  python tools/optim_bench.py --gru-rpgd [--rpgd-shapes 1x16x35x4,64x16x35x4,256x16x35x4,1x40x35x5,64x40x35x5,256x40x35x5]
The same comparison for rpgd (N = 16) and gradient-tf over the network, per E x N x H x iterations and math mode: staged
(``gru_adjoint=True``: iterations x (cpmppi_rollout_cost_grad_gru = two launches, cpmppi_adam_step), cpmppi_rollout_cost_gru, top-k
and torch glue, the memory through the predict seam) against fused (``gru_fused=True``: cpmppi_rpgd_step_gru + cpmppi_gru_advance),
the same three columns and the same verdict.

  python tools/optim_bench.py --rows [--rows-shapes 1x16x35x4,64x16x35x4,256x16x35x4,1x40x35x5,64x40x35x5,256x40x35x5]
The fused ODE step with a row per env (cpmppi_rpgd_step_rows) against the plain fused step (cpmppi_rpgd_step), per E x N x H x
iterations (N = 16: rpgd, otherwise gradient-tf) and predictor: two optimizers of one seed, the rows equal to the scalars so that the
work is the same, ``step_device`` with the step counter on the device, the two alternating in this one process - and with them a
second plain optimizer ("plain_again": the plain step on another engine's buffers, the control of the comparison); device time per
control step from events around batches of steps, medians over the rounds with min and max, and whether the rows step stays within
the plain median + the plain runs' own min - max spread.

  python tools/optim_bench.py --gru-grad [--steps 30] [--grad-shapes 1x16x35,64x16x35,1x40x35,64x40x35]
The GRU adjoint (same synthetic weights).  Per E x N x H of --grad-shapes (default: the rpgd and gradient-tf sizes at 1 and 64
envs) and math mode, cpmppi_rollout_cost_grad_gru against cpmppi_rollout_cost_gru on the same plans, alternating in one process as
above (ms per launch, the ratio); then rpgd and gradient-tf through the controller seam over the GRU (``gru_adjoint=True``) and over
the ODE, alternating, at 1 and 64 envs and both math modes of the GRU kernels.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cartpolesimulation_amd.controller_mpc import controller_mpc  # noqa: E402
from oracle import oracle_np as O  # noqa: E402  (initial states only)

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--predictor-specification", default="ODE_v0")
ap.add_argument("--fused", action="store_true", help="rpgd and gradient-tf, staged against fused, in this one process")
ap.add_argument("--optimizers", default="gradient-tf,rpgd", help="with --fused: comma-separated optimizer names")
ap.add_argument("--staged-repeats", type=int, default=1, help="with --fused: how many times the staged record is measured")
ap.add_argument("--gru", action="store_true", help="the GRU predictor under cem-tf, cem-gmm-tf and random-action-tf; cost-only launch vs fused step")
ap.add_argument("--cost-only-shapes", default="1x200x35,64x200x35,256x200x35,256x1024x50", help="with --gru: ExNxH,... (the last default: bench.py's C5)")
ap.add_argument("--cem-shapes", default="1x200x35,64x200x35,256x200x35", help="with --gru: ExNxH,... of the staged / fused cem step (3 iterations)")
ap.add_argument("--gru-rpgd", action="store_true", help="rpgd and gradient-tf over the GRU predictor: the staged step (gru_adjoint) against the fused one (gru_fused)")
ap.add_argument("--rpgd-shapes", default="1x16x35x4,64x16x35x4,256x16x35x4,1x40x35x5,64x40x35x5,256x40x35x5",
                help="with --gru-rpgd: ExNxHxiterations,... (N = 16: rpgd, otherwise gradient-tf)")
ap.add_argument("--rows", action="store_true", help="the fused ODE rpgd / gradient step: a row per env (cpmppi_rpgd_step_rows) against the plain step")
ap.add_argument("--rows-shapes", default="1x16x35x4,64x16x35x4,256x16x35x4,1x40x35x5,64x40x35x5,256x40x35x5",
                help="with --rows: ExNxHxiterations,... (N = 16: rpgd, otherwise gradient-tf)")
ap.add_argument("--gru-grad", action="store_true", help="the GRU adjoint: gradient launch vs cost-only launch; rpgd and gradient-tf over the GRU vs the ODE")
ap.add_argument("--grad-shapes", default="1x16x35,64x16x35,1x40x35,64x40x35", help="with --gru-grad: ExNxH,...")
ap.add_argument("--datagen", default=None, help="with --fused: E,seconds of the closed-loop data generator, e.g. 256,10")
args = ap.parse_args()
E = args.envs
rng = np.random.Generator(np.random.SFC64(3))
s_host = np.stack([O.create_cartpole_state(rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5), rng.uniform(-0.05, 0.05), 0.0)
                   for _ in range(E)])


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def fused_bench():
    spec = args.predictor_specification
    names = [n for n in args.optimizers.split(",") if n]
    for name in names:
        for mode in ("staged",) * max(1, args.staged_repeats) + ("fused", "fused_device"):
            ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                                  control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=1, fused=mode != "staged"))
            ctrl.configure(name, predictor_specification=spec)
            opt = ctrl.optimizer
            eng = opt.engine
            s = eng.tensor(s_host)
            if mode == "fused_device":
                tp, te, L = eng.zeros(E), eng.zeros(E) + 1.0, eng.zeros(E) + 0.395
                counter = torch.zeros(1, dtype=torch.int64, device=s.device)
                dt = timed(lambda: opt.step_device(s, tp, te, L=L, previous_input=opt.controls, count_dev=counter), args.steps)
            else:
                dt = timed(lambda: ctrl.step(s, 0.0, {}), args.steps)
            print(json.dumps({"bench": "controller_step", "optimizer": name, "mode": mode, "predictor": opt.cfg.predictor_type, "envs": E,
                              "num_rollouts": opt.num_rollouts, "mpc_horizon": opt.mpc_horizon,
                              "iterations": getattr(opt, "outer_its", getattr(opt, "gradient_steps", getattr(opt, "cem_outer_it", None))),
                              "ms_per_controller_step": round(dt * 1e3, 4)}), flush=True)
            eng.close()
    if args.datagen:
        from cartpolesimulation_amd import schedule as SC
        from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
        n, seconds = int(args.datagen.split(",")[0]), float(args.datagen.split(",")[1])
        cfg = dict(seed=5, length_of_experiment=seconds)
        for mode, graph in (("launched_staged", False), ("launched_fused", False), ("captured_fused", True)):
            ctrl = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), num_envs=n, config=dict(seed=1, fused=mode != "launched_staged"))
            ctrl.configure(names[0], predictor_specification=spec)
            opt = ctrl.optimizer
            best = None
            for _ in range(2):                                  # (the first run pays the one-time costs)
                opt.optimizer_reset()
                b = SC.RandomExperimentSetter(cfg).draw(n, 6)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                BatchedCartPoleExperiment(opt.engine, b.dt_simulation, b.dt_control, seed=0).run_schedule(b, graph=graph, optimizer=opt)
                torch.cuda.synchronize()
                best = time.perf_counter() - t0
            print(json.dumps({"bench": "data_generator", "optimizer": names[0], "mode": mode, "predictor": opt.cfg.predictor_type,
                              "experiments": n, "length_s": seconds, "control_periods": int(b.n_periods), "seconds": round(best, 4),
                              "ms_per_control_period": round(best / (b.n_periods + 1) * 1e3, 4)}), flush=True)
            opt.engine.close()


def synthetic_gru():
    """bench.py's C5_gru weights: SFC64(5), U(-1, 1) / sqrt(32), no normalisation vectors."""
    g = np.random.Generator(np.random.SFC64(5))
    u = lambda *shape: g.uniform(-1, 1, shape).astype(np.float32) / np.sqrt(32.0, dtype=np.float32)  # noqa: E731
    return dict(w_ih0=u(96, 6), w_hh0=u(96, 32), b_ih0=u(96), b_hh0=u(96), w_ih1=u(96, 32), w_hh1=u(96, 32), b_ih1=u(96),
                b_hh1=u(96), w_out=u(5, 32), b_out=u(5))


def gru_bench():
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine
    model = synthetic_gru()
    for name in ("cem-tf", "cem-gmm-tf", "random-action-tf"):
        ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0}, control_limits=([-1.0], [1.0]),
                              num_envs=E, config=dict(seed=1, gru_model=model))
        ctrl.configure(name)
        opt = ctrl.optimizer
        s = opt.engine.tensor(s_host)
        dt = timed(lambda: ctrl.step(s, 0.0, {}), args.steps)
        print(json.dumps({"bench": "controller_step", "optimizer": name, "predictor": "GRU", "envs": E, "num_rollouts": opt.num_rollouts,
                          "mpc_horizon": opt.mpc_horizon, "iterations": opt.cem_outer_it,
                          "ms_per_controller_step": round(dt * 1e3, 4)}), flush=True)
        opt.engine.close()
    rounds, batch = 12, 10
    for shape in filter(None, args.cost_only_shapes.split(",")):
        e, n, h = (int(x) for x in shape.split("x"))
        g = np.random.Generator(np.random.SFC64(11))
        s0 = np.stack([O.create_cartpole_state(g.uniform(-0.3, 0.3), g.uniform(-0.5, 0.5), g.uniform(-0.05, 0.05), 0.0) for _ in range(e)])
        for math_mode in ("fast", "precise"):
            eng = MPPIEngine(e, MPPIConfig(num_rollouts=n, mpc_horizon=h, math_mode=math_mode, cc_weight=0.0, shift_mode="none"))
            eng.set_gru(model)
            s, tp, te, h0 = eng.tensor(s0), eng.zeros(e), eng.zeros(e) + 1.0, eng.zeros(e, 2, 32)
            plans = torch.clamp(0.5 * torch.randn(e, n, h, device=s.device, generator=torch.Generator(s.device).manual_seed(1)), -1.0, 1.0)
            S, u_out = eng.empty(e, n), eng.empty(e, h)
            fused = eng.prepare_step(s, eng.zeros(e, h), tp, te, S_out=S, predictor="GRU", h0=h0, delta_u=plans, u_nom_out=u_out)
            launches = {"cost_only": lambda: eng.rollout_cost(s, plans, tp, te, predictor="GRU", h0=h0), "fused_step": fused.run}
            ms = {k: [] for k in launches}
            for r in range(rounds + 2):                           # (the first two rounds warm up)
                for k, fn in launches.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(batch):
                        fn()
                    b.record()
                    b.synchronize()
                    if r >= 2:
                        ms[k].append(a.elapsed_time(b) / batch)
            rec = {"bench": "gru_cost_only", "envs": e, "num_rollouts": n, "mpc_horizon": h, "math_mode": math_mode, "rounds": rounds,
                   "launches_per_round": batch}
            for k, v in ms.items():
                rec[k + "_ms"] = round(float(np.median(v)), 5)
                rec[k + "_min_max_ms"] = [round(float(min(v)), 5), round(float(max(v)), 5)]
            rec["cost_only_over_fused"] = round(rec["cost_only_ms"] / rec["fused_step_ms"], 4)
            print(json.dumps(rec), flush=True)
            eng.close()


def gru_cem_bench():
    """The cem control step over the network, staged against fused, alternating in one process (the module docstring)."""
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    model = synthetic_gru()

    def make(mode, e, n, h, math_mode, vp):
        return optimizer_cem(control_limits=([-1.0], [1.0]), seed=1, num_envs=e, num_rollouts=n, mpc_horizon=h, cem_outer_it=3,
                             math_mode=math_mode, gru_model=model, gru_fused=mode != "staged", variable_parameters=vp)

    gru_step_bench("gru_cem_step", filter(None, args.cem_shapes.split(",")), make)


def gru_rpgd_bench():
    """The rpgd / gradient control step over the network, staged (gru_adjoint=True) against fused (gru_fused=True: cpmppi_rpgd_step_gru
    + cpmppi_gru_advance), alternating in one process as the cem step above; a shape E x N x H x iterations with N = 16 is rpgd's
    (resamp_per 10, three quarters kept), any other gradient-tf's."""
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    model = synthetic_gru()

    def make(mode, e, n, h, math_mode, vp, iterations):
        flag = dict(gru_adjoint=True) if mode == "staged" else dict(gru_fused=True)
        common = dict(control_limits=([-1.0], [1.0]), seed=1, num_envs=e, num_rollouts=n, mpc_horizon=h, gru_model=model,
                      variable_parameters=vp, **flag)
        opt = optimizer_rpgd(outer_its=iterations, **common) if n == 16 else optimizer_gradient(gradient_steps=iterations, **common)
        opt.cfg.math_mode = math_mode                         # (the GRU kernels' math mode is the handle's)
        return opt

    gru_step_bench("gru_rpgd_step", filter(None, args.rpgd_shapes.split(",")), make)


def gru_step_bench(bench, shapes, make):
    """A control step over the network, staged against fused, alternating in one process (the module docstring): `make(mode, E, N,
    H, math mode, variable parameters[, iterations])` builds the optimizer of a mode; a shape is E x N x H[x iterations]."""
    from types import SimpleNamespace
    rounds, batch = 12, 10
    for shape in shapes:
        e, n, h, *more = (int(x) for x in shape.split("x"))
        g = np.random.Generator(np.random.SFC64(11))
        s0 = np.stack([O.create_cartpole_state(g.uniform(-0.3, 0.3), g.uniform(-0.5, 0.5), g.uniform(-0.05, 0.05), 0.0) for _ in range(e)])
        for math_mode in ("fast", "precise"):
            opts = {}
            for mode in ("staged", "fused", "fused_device"):
                vp = SimpleNamespace(target_position=np.zeros(e, np.float32), target_equilibrium=np.ones(e, np.float32))
                opts[mode] = make(mode, e, n, h, math_mode, vp, *more)
                opts[mode].configure()
            states = {k: o.engine.tensor(s0) for k, o in opts.items()}
            dev = opts["fused_device"]
            tp, te = dev.engine.zeros(e), dev.engine.zeros(e) + 1.0
            counter = torch.zeros(1, dtype=torch.int64, device=tp.device)
            steps = {"staged": lambda: opts["staged"].step(states["staged"], as_tensor=True),
                     "fused": lambda: opts["fused"].step(states["fused"], as_tensor=True),
                     "fused_device": lambda: dev.step_device(states["fused_device"], tp, te, count_dev=counter)}
            device_ms, wall_ms = {k: [] for k in steps}, {k: [] for k in steps}
            for r in range(rounds + 2):                           # (the first two rounds warm up)
                for k, fn in steps.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    a.record()
                    for _ in range(batch):
                        fn()
                    b.record()
                    b.synchronize()
                    if r >= 2:
                        wall_ms[k].append((time.perf_counter() - t0) / batch * 1e3)
                        device_ms[k].append(a.elapsed_time(b) / batch)
            rec = {"bench": bench, "optimizer": dev.optimizer_name, "envs": e, "num_rollouts": n, "mpc_horizon": h,
                   "iterations": more[0] if more else 3, "math_mode": math_mode, "rounds": rounds, "steps_per_round": batch}
            for k in steps:
                for what, v in (("device", device_ms[k]), ("wall", wall_ms[k])):
                    rec[f"{k}_{what}_ms"] = round(float(np.median(v)), 5)
                    rec[f"{k}_{what}_min_max_ms"] = [round(float(min(v)), 5), round(float(max(v)), 5)]
            for what in ("device", "wall"):
                lo, hi = rec[f"staged_{what}_min_max_ms"]
                for k in ("fused", "fused_device"):
                    rec[f"{k}_over_staged_{what}"] = round(rec[f"{k}_{what}_ms"] / rec[f"staged_{what}_ms"], 4)
                    rec[f"{k}_within_staged_spread_{what}"] = bool(rec[f"{k}_{what}_ms"] <= rec[f"staged_{what}_ms"] + (hi - lo))
            print(json.dumps(rec), flush=True)
            for o in opts.values():
                o.engine.close()


def rows_bench():
    """The fused ODE step, plain against a row per env (the module docstring)."""
    from cartpolesimulation_amd.configs import rpgd_rows
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    rounds, batch = 12, 10
    for shape in filter(None, args.rows_shapes.split(",")):
        e, n, h, iterations = (int(x) for x in shape.split("x"))
        g = np.random.Generator(np.random.SFC64(11))
        s0 = np.stack([O.create_cartpole_state(g.uniform(-0.3, 0.3), g.uniform(-0.5, 0.5), g.uniform(-0.05, 0.05), 0.0) for _ in range(e)])
        for spec in ("ODE_v0", "ODE"):
            opts = {}
            for mode in ("plain", "rows", "plain_again"):        # (a second plain optimizer: what another set of buffers costs)
                common = dict(control_limits=([-1.0], [1.0]), seed=1, num_envs=e, num_rollouts=n, mpc_horizon=h, fused=True)
                if mode == "rows":                               # the plain optimizer's scalars, per env: the same work
                    plain = opts["plain"]
                    common["rows"] = rpgd_rows(plain.cfg, e, plain.learning_rate, plain.gradmax_clip)
                opt = optimizer_rpgd(outer_its=iterations, **common) if n == 16 else optimizer_gradient(gradient_steps=iterations, **common)
                opt.configure(predictor_specification=spec)
                opt.reserve_fused()
                opts[mode] = opt
            steps = {}
            for mode, opt in opts.items():
                eng = opt.engine
                s, tp, te, L = eng.tensor(s0), eng.zeros(e), eng.zeros(e) + 1.0, eng.zeros(e) + 0.395
                counter = torch.zeros(1, dtype=torch.int64, device=s.device)
                steps[mode] = (lambda opt=opt, s=s, tp=tp, te=te, L=L, counter=counter:
                               opt.step_device(s, tp, te, L=L, previous_input=opt.controls, count_dev=counter))
            ms = alternating(steps, rounds, batch)
            torch.cuda.synchronize()
            assert torch.equal(opts["plain"].Q, opts["rows"].Q) and torch.equal(opts["plain"].Q, opts["plain_again"].Q)   # (the same steps, to the bit)
            rec = {"bench": "rpgd_step_rows", "optimizer": opts["rows"].optimizer_name, "predictor": spec, "envs": e, "num_rollouts": n,
                   "mpc_horizon": h, "iterations": iterations, "rounds": rounds, "steps_per_round": batch}
            for k, v in ms.items():
                rec[k + "_ms"] = round(float(np.median(v)), 5)
                rec[k + "_min_max_ms"] = [round(float(min(v)), 5), round(float(max(v)), 5)]
            lo, hi = rec["plain_min_max_ms"]
            rec["rows_over_plain"] = round(rec["rows_ms"] / rec["plain_ms"], 4)
            rec["rows_within_plain_spread"] = bool(rec["rows_ms"] <= rec["plain_ms"] + (hi - lo))
            rec["plain_again_over_plain"] = round(rec["plain_again_ms"] / rec["plain_ms"], 4)
            print(json.dumps(rec), flush=True)
            for o in opts.values():
                o.engine.close()


def alternating(launches, rounds=12, batch=10):
    """Device ms per launch of each entry of `launches`, the entries alternating: {name: [ms per round]} (two warm-up rounds)."""
    ms = {k: [] for k in launches}
    for r in range(rounds + 2):
        for k, fn in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            if r >= 2:
                ms[k].append(a.elapsed_time(b) / batch)
    return ms


def gru_grad_bench():
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine
    model = synthetic_gru()
    rounds, batch = 12, 10
    for shape in args.grad_shapes.split(","):
        e, n, h = (int(x) for x in shape.split("x"))
        g = np.random.Generator(np.random.SFC64(11))
        s0 = np.stack([O.create_cartpole_state(g.uniform(-0.3, 0.3), g.uniform(-0.5, 0.5), g.uniform(-0.05, 0.05), 0.0) for _ in range(e)])
        for math_mode in ("fast", "precise"):
            eng = MPPIEngine(e, MPPIConfig(num_rollouts=n, mpc_horizon=h, math_mode=math_mode, cc_weight=0.0, shift_mode="none"))
            eng.set_gru(model)
            s, tp, te, h0 = eng.tensor(s0), eng.zeros(e), eng.zeros(e) + 1.0, eng.zeros(e, 2, 32)
            plans = torch.clamp(0.5 * torch.randn(e, n, h, device=s.device, generator=torch.Generator(s.device).manual_seed(1)), -1.0, 1.0)
            ms = alternating({"cost_only": lambda: eng.rollout_cost(s, plans, tp, te, predictor="GRU", h0=h0),
                              "cost_grad": lambda: eng.rollout_cost_grad(s, plans, tp, te, predictor="GRU", h0=h0)}, rounds, batch)
            rec = {"bench": "gru_cost_grad", "envs": e, "num_rollouts": n, "mpc_horizon": h, "math_mode": math_mode, "rounds": rounds,
                   "launches_per_round": batch}
            for k, v in ms.items():
                rec[k + "_ms"] = round(float(np.median(v)), 5)
                rec[k + "_min_max_ms"] = [round(float(min(v)), 5), round(float(max(v)), 5)]
            rec["cost_grad_over_cost_only"] = round(rec["cost_grad_ms"] / rec["cost_only_ms"], 4)
            print(json.dumps(rec), flush=True)
            eng.close()
    for name in ("rpgd", "gradient-tf"):
        for e in (1, 64):
            s_e = s_host[np.arange(e) % s_host.shape[0]]
            for math_mode in ("fast", "precise"):
                ctrls = {}
                for predictor, extra in (("GRU", dict(gru_model=model, gru_adjoint=True)), ("ODE", {})):
                    # (the ODE adjoint is written for the FAST arithmetic: its column is the same in both rows of a pair)
                    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                                          control_limits=([-1.0], [1.0]), num_envs=e, config=dict(seed=1, **extra))
                    ctrl.configure(name, predictor_specification=None if predictor == "GRU" else "ODE")
                    if predictor == "GRU":                       # the GRU kernels' math mode is the handle's
                        opt = ctrl.optimizer
                        opt.engine.close()
                        opt.cfg.math_mode = math_mode
                        opt.configure()
                    ctrls[predictor] = ctrl
                states = {k: c.optimizer.engine.tensor(s_e) for k, c in ctrls.items()}
                wall = {k: [] for k in ctrls}
                for r in range(rounds + 2):
                    for k, c in ctrls.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(batch):
                            c.step(states[k], 0.0, {})
                        torch.cuda.synchronize()
                        if r >= 2:
                            wall[k].append((time.perf_counter() - t0) / batch * 1e3)
                opt = ctrls["GRU"].optimizer
                rec = {"bench": "controller_step_gru_adjoint", "optimizer": name, "envs": e, "num_rollouts": opt.num_rollouts,
                       "mpc_horizon": opt.mpc_horizon, "math_mode": opt.cfg.math_mode,
                       "iterations": getattr(opt, "outer_its", getattr(opt, "gradient_steps", None))}
                for k, v in wall.items():
                    rec[k.lower() + "_ms_per_controller_step"] = round(float(np.median(v)), 4)
                    rec[k.lower() + "_min_max_ms"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
                rec["gru_over_ode"] = round(rec["gru_ms_per_controller_step"] / rec["ode_ms_per_controller_step"], 4)
                print(json.dumps(rec), flush=True)
                for c in ctrls.values():
                    c.optimizer.engine.close()


if args.fused:
    fused_bench()
    sys.exit(0)
if args.rows:
    rows_bench()
    sys.exit(0)
if args.gru_grad:
    gru_grad_bench()
    sys.exit(0)
if args.gru_rpgd:
    gru_rpgd_bench()
    sys.exit(0)
if args.gru:
    gru_bench()
    gru_cem_bench()
    sys.exit(0)
for name in ("mppi", "cem-tf", "cem-gmm-tf", "cem-naive-grad-tf", "cem-grad-bharadhwaj-tf", "gradient-tf", "rpgd", "random-action-tf"):
    ctrl = controller_mpc("CartPole", {"target_position": 0.0, "target_equilibrium": 1.0, "L": 0.395},
                          control_limits=([-1.0], [1.0]), num_envs=E, config=dict(seed=1))
    ctrl.configure(name, predictor_specification=args.predictor_specification)
    opt = ctrl.optimizer
    s = opt.engine.tensor(s_host)
    for _ in range(3):
        ctrl.step(s, 0.0, {})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctrl.step(s, 0.0, {})
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    rec = {"optimizer": name, "predictor": opt.cfg.predictor_type, "envs": E, "num_rollouts": int(getattr(opt, "num_rollouts", 0)), "mpc_horizon": int(getattr(opt, "mpc_horizon", 0)),
           "ms_per_controller_step": round(dt * 1e3, 3)}
    for k in ("outer_its", "cem_outer_it", "gradient_steps", "opt_iters", "num_iterations"):
        if hasattr(opt, k):
            rec[k] = getattr(opt, k)
    print(json.dumps(rec), flush=True)
