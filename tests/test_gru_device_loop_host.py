"""CPU: the learned model in the device loop - what can be checked without a GPU.  The new entry point cpmppi_gru_advance is
declared in the header and bound (the ABI number stays 5: no layout and no existing semantics change); the harness and the data
generator refuse, each with its reason, what the loop cannot run with predictor="GRU".  Stand-in engines: the refusals come before
anything touches a device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gru_advance_is_declared_and_bound_and_the_abi_stays_5():
    from cartpolesimulation_amd import _lib
    header = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert "cpmppi_gru_advance" in _lib.EXPORTS
    proto = re.search(r"^int cpmppi_gru_advance\(([^;]*)\);", header, re.M | re.S)
    assert proto, "include/cpmppi.h declares no cpmppi_gru_advance"
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert args == ["cpmppi_handle* h", "uint32_t E", "const float* s", "const float* Q", "float* h_io", "void* stream"]
    assert re.search(r"^#define CPMPPI_ABI_VERSION 5u\b", header, re.M) and _lib.ABI_VERSION == 5
    comment = header[header.index("#define CPMPPI_ABI_VERSION"):header.index("#define CPMPPI_STATE_DIM")]
    assert "cpmppi_gru_advance" in comment
    # no field was added for it: the step's argument block is what it was
    assert [n for n, _ in _lib.cpmppi_step_args._fields_][-4:] == ["h0", "previous_input", "offset_dev", "u_nom_out"]


def _batch(E=2):
    from cartpolesimulation_amd import schedule as SC
    cfg = dict(seed=31, length_of_experiment=0.1,
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    return cfg, SC.RandomExperimentSetter(cfg).draw(E, 83)


def test_harness_refuses_what_the_network_cannot_run():
    from cartpolesimulation_amd import harness as HA
    cfg, b = _batch()
    bare, with_net = SimpleNamespace(has_gru=False), SimpleNamespace(has_gru=True)
    s0 = np.zeros((2, 6), np.float32)
    for eng in (bare, with_net):
        exp = HA.BatchedCartPoleExperiment(eng, b.dt_simulation, b.dt_control)
        with pytest.raises(ValueError, match="predictor must be one of"):
            exp.run(s0, 2, predictor="Dense")
        with pytest.raises(ValueError, match="predictor must be one of"):
            exp.run_schedule(b, predictor="ODE")
        with pytest.raises(ValueError, match="h0 is the memory of the GRU predictor"):
            exp.run(s0, 2, h0=np.zeros((2, 2, 32), np.float32))
        with pytest.raises(ValueError, match="h0 is the memory of the GRU predictor"):
            exp.run_schedule(b, h0=np.zeros((2, 2, 32), np.float32))
    exp = HA.BatchedCartPoleExperiment(bare, b.dt_simulation, b.dt_control)
    with pytest.raises(ValueError, match="the engine has no model"):
        exp.run(s0, 2, predictor="GRU")
    with pytest.raises(ValueError, match="the engine has no model"):
        exp.run_schedule(b, predictor="GRU")
    with pytest.raises(ValueError, match="the engine has no model"):
        HA.ScheduleRun(SimpleNamespace(), b, 0, predictor="GRU")                # (an engine object that never heard of a network)
    exp = HA.BatchedCartPoleExperiment(with_net, b.dt_simulation, b.dt_control)
    with pytest.raises(ValueError, match="optimizer= object carries its own predictor"):
        exp.run_schedule(b, predictor="GRU", optimizer=SimpleNamespace(num_envs=2))
    with pytest.raises(ValueError, match="knots_fn is not supported"):
        exp.run_schedule(b, predictor="GRU", knots_fn=lambda c: None)


def test_controller_mass_is_none_with_the_network():
    """A GRU step reads no pole mass: a pole-mass table that varies does not make the host pace the run (or forbid its capture)."""
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.harness import ControllerMass
    cfg = dict(seed=35, length_of_experiment=0.2,
               random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    prm = dict(m_pole=dict(init_value=0.087, change_every_x_seconds=0.02, mode="increase", range_random=[0.015, 0.3],
                           range_clip=[0.015, 0.3], increment=0.02, reset_every_x_seconds="inf"))
    b = SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(2, 79, stride=1), prm)
    ode = MPPIConfig(predictor_type="ODE")
    told = ControllerMass(b, ode)
    assert (told.kind, told.varies) == ("value", True)
    net = ControllerMass(b, ode, network=True)
    assert (net.kind, net.varies) == ("none", False)


def test_generate_dataset_refuses_groups_and_optimizer_objects_with_a_network():
    from cartpolesimulation_amd.recording import generate_dataset
    cfg, _ = _batch()
    with pytest.raises(ValueError, match="gru_model: env groups"):
        generate_dataset(SimpleNamespace(), 2, "/nonexistent", config=cfg, seed=1, groups=2, gru_model={})
    with pytest.raises(ValueError, match="gru_model goes with the fused MPPI step"):
        generate_dataset(None, 2, "/nonexistent", config=cfg, seed=1, optimizer=SimpleNamespace(fused=True), gru_model={})
