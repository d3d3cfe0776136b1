#!/usr/bin/env python3
"""Timing of one training step of the GRU predictor (GPU box): MPPIEngine.gru_train_step (cpmppi_gru_train_step: forward sweep,
loss, reverse sweep, weight-gradient contraction, Adam and the image rebuild - six launches) against torch.nn.GRU + Linear +
torch.optim.Adam in float32 on the same device and shape.

  python tools/train_bench.py [--batches 64,4096] [--wash-out 10] [--post-wash-out 50] [--steps 20] [--rounds 5] [--out FILE.json]
  python tools/train_bench.py --rollout ...     the step through the open-loop rollout (cpmppi_gru_rollout_train_step) against the
                                                teacher-forced step, alternating round by round in one process: the ratio of the
                                                medians against the bar 352 / 304 (the reverse sweeps' MFMAs per row) plus the
                                                teacher-forced rounds' own min - max scatter; for information a float32 torch loop
                                                doing the same rollout training (the cell called row by row)

Both forms run in ONE process and alternate round by round; a round is ``--steps`` back-to-back steps between two device events
(device time per step) inside a host clock that ends in a synchronise (wall time per step: what a training loop pays, the
engine's per-step upload of the batch's windows included).  One warm-up round per form and shape, then ``--rounds`` timed ones;
reported: the median and the min - max scatter.  The torch form is handed its batch already gathered and normalised on the device
([B,W+P,6] and [B,P,5]) - the gather the library does inside its forward kernel is not charged to torch - and runs with torch's
defaults for the device (MIOpen's RNN where torch selects it; ``--native-rnn`` disables that and times torch's own cell kernels).
Data: recordings of the oracle's plant model under smooth random controls, min-max normalised; weights uniform +-1/sqrt(32).
Prints one JSON object per shape and writes all of them to ``--out``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32


def recordings(R, T, seed=5):
    from oracle import oracle_np as O
    rng = np.random.Generator(np.random.SFC64(seed))
    t = np.arange(T - 1)
    amp, freq, phase = rng.uniform(0.1, 0.3, (R, 3, 1)), rng.uniform(0.02, 0.2, (R, 3, 1)), rng.uniform(0, 2 * np.pi, (R, 3, 1))
    Q = np.clip((amp * np.sin(freq * t + phase)).sum(axis=1), -0.9, 0.9).astype(f32)
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.5, 0.5), rng.uniform(-1, 1), rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2))
                   for _ in range(R)])
    states = O.predict_core(s0, Q, integrator="ODE_v0").astype(f32)
    return states, np.concatenate([Q, Q[:, -1:]], axis=1)


class TorchNet(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.gru = torch.nn.GRU(6, 32, num_layers=2, batch_first=True)
        self.head = torch.nn.Linear(32, 5)
        with torch.no_grad():
            for l in range(2):
                getattr(self.gru, f"weight_ih_l{l}").copy_(torch.as_tensor(model[f"w_ih{l}"]))
                getattr(self.gru, f"weight_hh_l{l}").copy_(torch.as_tensor(model[f"w_hh{l}"]))
                getattr(self.gru, f"bias_ih_l{l}").copy_(torch.as_tensor(model[f"b_ih{l}"]))
                getattr(self.gru, f"bias_hh_l{l}").copy_(torch.as_tensor(model[f"b_hh{l}"]))
            self.head.weight.copy_(torch.as_tensor(model["w_out"]))
            self.head.bias.copy_(torch.as_tensor(model["b_out"]))

    def forward(self, x):
        return self.head(self.gru(x)[0])


def timed(run, steps, device):
    """-> (device ms per step, wall ms per step) of `steps` back-to-back calls of run()."""
    torch.cuda.synchronize(device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        run()
    b.record()
    torch.cuda.synchronize(device)
    return a.elapsed_time(b) / steps, (time.perf_counter() - t0) * 1e3 / steps


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def rollout_record(args, eng, s_dev, q_dev, w, W, P, lr, net, opt, x, lab):
    """One shape of --rollout: the rollout step and the teacher-forced step of the library alternating, then the torch loop."""
    dev = eng.device
    loss_out = torch.empty(1, dtype=torch.float64, device=dev)
    forced = lambda: eng.gru_train_step(s_dev, q_dev, w, W, P, lr=lr, loss_out=loss_out)                  # noqa: E731
    rolled = lambda: eng.gru_train_step(s_dev, q_dev, w, W, P, lr=lr, loss_out=loss_out, rollout=True)    # noqa: E731

    def theirs():
        opt.zero_grad(set_to_none=True)
        out, h = net.gru(x[:, :W + 1])
        y = net.head(out)[:, W:]
        ys = [y]
        for j in range(W + 1, W + P):
            out, h = net.gru(torch.cat([x[:, j:j + 1, :1], y], dim=2), h)
            y = net.head(out)
            ys.append(y)
        loss = ((torch.cat(ys, dim=1) - lab) ** 2).mean()
        loss.backward()
        opt.step()
        return loss

    first = (float(rolled().cpu()[0]), float(forced().cpu()[0]))
    timed(rolled, args.steps, dev)
    timed(forced, args.steps, dev)
    t_rolled, t_forced = [], []
    for _ in range(args.rounds):
        t_rolled.append(timed(rolled, args.steps, dev))
        t_forced.append(timed(forced, args.steps, dev))
    timed(theirs, 2, dev)
    t_theirs = [timed(theirs, args.steps, dev) for _ in range(2)]
    rec = dict(B=len(w), wash_out=W, post_wash_out=P, steps_per_round=args.steps, rounds=args.rounds, first_loss_rollout=first[0],
               first_loss_teacher_forced=first[1],
               rollout_device_ms=stats([t[0] for t in t_rolled]), rollout_wall_ms=stats([t[1] for t in t_rolled]),
               teacher_forced_device_ms=stats([t[0] for t in t_forced]), teacher_forced_wall_ms=stats([t[1] for t in t_forced]),
               torch_rollout_wall_ms=stats([t[1] for t in t_theirs]))
    tf = rec["teacher_forced_device_ms"]
    rec["rollout_over_teacher_forced_device"] = rec["rollout_device_ms"]["median"] / tf["median"]
    rec["bar"] = 352.0 / 304.0 + (tf["max"] - tf["min"]) / tf["median"]
    rec["within_bar"] = bool(rec["rollout_over_teacher_forced_device"] <= rec["bar"])
    rec["torch_over_library_wall"] = rec["torch_rollout_wall_ms"]["median"] / rec["rollout_wall_ms"]["median"]
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="64,4096")
    ap.add_argument("--wash-out", type=int, default=10)
    ap.add_argument("--post-wash-out", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rollout", action="store_true", help="time the rollout step against the teacher-forced step")
    ap.add_argument("--native-rnn", action="store_true", help="torch.backends.cudnn.enabled = False: torch's own cell kernels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_bench needs the MI355X: there is no CPU path to time")
    if args.native_rnn:
        torch.backends.cudnn.enabled = False
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.train_gru import initial_weights, make_windows, normalization_from_recordings
    W, P, lr = args.wash_out, args.post_wash_out, 2e-3
    states, Q = recordings(64, 256)
    model = {**initial_weights(1873), **normalization_from_recordings(states, Q)}
    legal = make_windows([states.shape[1]] * states.shape[0], W, P, 1)
    eng = MPPIEngine(1, MPPIConfig(num_rollouts=1, mpc_horizon=2))
    dev = eng.device
    s_dev, q_dev = eng.tensor(states), eng.tensor(Q)
    results = []
    for B in (int(x) for x in args.batches.split(",")):
        w = legal[np.random.default_rng(B).integers(0, len(legal), B)]
        eng.set_gru(model)
        eng.gru_train_begin()
        eng.gru_train_reserve(B, W + P)
        loss_out = torch.empty(1, dtype=torch.float64, device=dev)
        ours = lambda: eng.gru_train_step(s_dev, q_dev, w, W, P, lr=lr, loss_out=loss_out)          # noqa: E731
        # the torch form on the same batch, gathered and normalised once
        rows = w[:, 1:2] + np.arange(W + P)[None, :]
        raw = np.concatenate([Q[w[:, 0:1], rows][..., None], states[w[:, 0:1], rows][..., 1:]], axis=-1)
        x = torch.as_tensor(raw * model["in_scale"] + model["in_shift"]).to(dev)
        lab = torch.as_tensor((states[w[:, 0:1], rows[:, W:] + 1][..., 1:] - model["out_shift"]) / model["out_scale"]).to(dev)
        net = TorchNet(model).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=lr)

        def theirs():
            opt.zero_grad(set_to_none=True)
            loss = ((net(x)[:, W:] - lab) ** 2).mean()
            loss.backward()
            opt.step()
            return loss

        if args.rollout:
            results.append(rollout_record(args, eng, s_dev, q_dev, w, W, P, lr, net, opt, x, lab))
            continue
        first = (float(ours().cpu()[0]), float(theirs().detach().cpu()))                              # the same loss, to start with
        timed(ours, args.steps, dev)
        timed(theirs, args.steps, dev)
        t_ours, t_theirs = [], []
        for _ in range(args.rounds):
            t_ours.append(timed(ours, args.steps, dev))
            t_theirs.append(timed(theirs, args.steps, dev))
        rec = dict(B=B, wash_out=W, post_wash_out=P, steps_per_round=args.steps, rounds=args.rounds,
                   torch_rnn="native" if args.native_rnn else "default", first_loss_library=first[0], first_loss_torch=first[1],
                   library_device_ms=stats([t[0] for t in t_ours]), library_wall_ms=stats([t[1] for t in t_ours]),
                   torch_device_ms=stats([t[0] for t in t_theirs]), torch_wall_ms=stats([t[1] for t in t_theirs]))
        rec["torch_over_library_wall"] = rec["torch_wall_ms"]["median"] / rec["library_wall_ms"]["median"]
        rec["windows_per_second_library"] = B / (rec["library_wall_ms"]["median"] * 1e-3)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return results


if __name__ == "__main__":
    main()
