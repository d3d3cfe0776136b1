"""GPU, end to end: a 3 x 2 grid x 2 experiments in one device loop (N=256, H=20, 1 s) - the table's rows are in grid order, a
setting's scores are those of a plain run of that configuration on the same experiments (bit for bit through the log: the same Philox
env indices, the same build), and the command line prints the table."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from cartpolesimulation_amd import schedule as SC  # noqa: E402
from cartpolesimulation_amd import sweep as SW  # noqa: E402
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402

GRID = dict(LBD=[50.0, 100.0, 200.0], ep_weight_up=[20.0, 80.0])


def test_sweep_table_and_one_setting_against_a_plain_run():
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.harness import BatchedCartPoleExperiment
    cfg = MPPIConfig(num_rollouts=256, mpc_horizon=20)
    batch = SC.RandomExperimentSetter(dict(seed=4, length_of_experiment=1.0)).draw(2, 12)
    sw = SW.run_sweep(cfg, GRID, batch, seed=6, first_row=5)
    assert [(s["LBD"], s["ep_weight_up"]) for s in sw["settings"]] == [(l, w) for l in GRID["LBD"] for w in GRID["ep_weight_up"]]
    assert sw["scores"].shape == (6, 2, 5) and sw["mean"].shape == sw["worst"].shape == (6, 5) and np.isfinite(sw["scores"]).all()
    assert np.array_equal(sw["mean"], sw["scores"].mean(axis=1)) and np.all(sw["worst"][:, :3] >= sw["mean"][:, :3])
    assert len({tuple(r) for r in sw["mean"].round(9)}) == 6                              # the settings differ
    table = sw["result"]["states"]
    for k in (0, 3, 5):
        s = sw["settings"][k]
        eng = MPPIEngine(2, dataclasses.replace(cfg, LBD=s["LBD"], cost_weights=dict(ep_weight_up=s["ep_weight_up"])))
        plain = BatchedCartPoleExperiment(eng, dt_simulation=batch.dt_simulation, dt_control=batch.dt_control, seed=6).run_schedule(
            batch, env_offset=2 * k)
        assert torch.equal(plain["states"], table[:, 2 * k:2 * k + 2]) and torch.equal(plain["Q"], sw["result"]["Q"][:, 2 * k:2 * k + 2])
        got = eng.score_runs(plain["states"], plain["Q"], target_position_table=eng.tensor(batch.target_position.astype(np.float32)),
                             save_every=batch.n_save, sched_stride=batch.stride, period_steps=batch.n_ctrl, first_row=5).cpu().numpy()
        assert np.array_equal(got, sw["scores"][k])
        eng.close()


def test_command_line_prints_the_table(capsys):
    SW.main(["--grid", "LBD=50,200", "--grid", "SQRTRHOINV=0.02,0.04", "--experiments", "2", "--length", "0.5", "--num-rollouts", "256",
             "--mpc-horizon", "20", "--graph"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0].split()[:3] == ["LBD", "SQRTRHOINV", "mean_abs_distance:mean"] and len(lines) == 5
    assert [tuple(float(x) for x in ln.split()[:2]) for ln in lines[1:]] == [(50, 0.02), (50, 0.04), (200, 0.02), (200, 0.04)]
    assert all(len(ln.split()) == 12 and np.isfinite([float(x) for x in ln.split()]).all() for ln in lines[1:])
