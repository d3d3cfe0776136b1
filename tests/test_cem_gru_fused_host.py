"""CPU: the host side of the fused CEM control step over the GRU predictor - the export and the ctypes mirror of
cpmppi_cem_gru_args against the header text, the rules of ``gru_fused=True`` (what it needs, what it refuses, that ``fused=True``
beside a model is still refused in the old words), the bookkeeping of the fused object on a stand-in engine (one
cpmppi_cem_step_gru and one cpmppi_gru_advance per control step, on the optimizer's own memory), the controller kind and pole-mass
rule of the device loop, and the data generator's command line."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_cem_fused_host import C_TYPES, FusedFake  # noqa: E402
from test_gru_sampling_optimizers_host import SPEC, golden_model  # noqa: E402
from test_optimizers_host_logic import _states  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(seed=5, mpc_horizon=6, num_rollouts=12, cem_outer_it=3, cem_best_k=4, cem_stdev_min=0.02, num_envs=2)


def test_export_and_abi_version():
    from cartpolesimulation_amd import _lib
    assert "cpmppi_cem_step_gru" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert re.search(r"#define CPMPPI_ABI_VERSION 5u", text)
    assert re.search(r"int cpmppi_cem_step_gru\(cpmppi_handle\* h, const cpmppi_cem_gru_args\* args, void\* stream\);", text)
    # no existing struct changed: the ODE step's block is what it was
    assert len(_lib.cpmppi_cem_args._fields_) == 29


def header_fields(struct):
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    body = text[text.index(f"typedef struct {{\n  uint32_t E;                       /* active envs in this call ({struct}) */"):
                text.index(f"}} {struct};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        mt = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        assert mt, decl
        fields.append((mt.group(4), C.c_void_p if mt.group(3) else C_TYPES[mt.group(2)]))
    return fields


def test_cem_gru_args_mirror_matches_the_header():
    """Field order, names and types of the ctypes mirror against the struct's text in include/cpmppi.h; and the struct is
    cpmppi_cem_args without L, previous_input, refine and the Adam fields, plus h0."""
    from cartpolesimulation_amd import _lib
    fields = header_fields("cpmppi_cem_gru_args")
    assert fields == list(_lib.cpmppi_cem_gru_args._fields_)
    A = _lib.cpmppi_cem_gru_args
    for name, ctype in fields:
        if ctype in (C.c_void_p, C.c_uint64):
            assert getattr(A, name).offset % 8 == 0, name
    dropped = {"L", "previous_input", "refine", "learning_rate", "beta1", "beta2", "epsilon", "gradmax_clip"}
    ode = [n for n, _ in header_fields("cpmppi_cem_args")]
    assert [n for n, _ in fields if n != "h0"] == [n for n in ode if n not in dropped]
    assert dict(fields)["h0"] is C.c_void_p and len(fields) == 29 - len(dropped) + 1


class GruFusedFake(FusedFake):
    """FusedFake plus the fused GRU step and the memory's hand-over, recorded."""

    def __init__(self, E, cfg, phys=None, device=0):
        super().__init__(E, cfg, phys, device)
        self.gru_launches, self.advances, self.gru = [], [], None

    def prepare_cem_step_gru(self, s0, mean, stdev, tp, te, h0=None, **kw):
        eng, args = self, SimpleNamespace(**kw)

        class Prepared:
            def run(self, offset=None, iterations=None):
                for name, x in (("offset", offset), ("iterations", iterations)):
                    if x is not None:
                        setattr(args, name, x)
                eng.gru_launches.append(dict(vars(args), s0=s0, mean=mean, stdev=stdev, h0=h0))
                args.Q_out.fill_(100.0 if args.count_dev is not None else 1.0 + args.offset)
                args.S_out.copy_(torch.arange(eng.N, dtype=torch.float32).expand(eng.E, eng.N))
                args.plan_out.copy_(args.Q_out[:, None].expand(eng.E, eng.H))

        return Prepared()

    def gru_advance(self, s, Q, h):
        self.advances.append(dict(s=s, Q=Q, h=h, launches_before=len(self.gru_launches)))
        h.add_(1.0)
        return h


@pytest.fixture()
def gru_fused_engine(monkeypatch):
    import cartpolesimulation_amd.engine as EN
    monkeypatch.setattr(EN, "MPPIEngine", GruFusedFake)
    return GruFusedFake


def test_flag_rules(gru_fused_engine):
    from cartpolesimulation_amd import optimizer_cem as OC
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    from cartpolesimulation_amd.harness import FusedOptimizer, HostPacedOptimizer, optimizer_controller
    model = golden_model()
    # the opt-in makes a fused object over the network; by a model, by a model and a specification
    for spec in (None, SPEC):
        opt = OC.optimizer_cem(gru_model=model, gru_fused=True, **KW)
        assert opt.fused is True and opt.gru_fused is True
        opt.configure(predictor_specification=spec)
        assert opt.engine.gru is model and tuple(opt.h.shape) == (2, 2, 32) and optimizer_controller(opt) is FusedOptimizer
    staged = OC.optimizer_cem(gru_model=model, **KW)
    assert staged.fused is False and staged.gru_fused is False and optimizer_controller(staged) is HostPacedOptimizer
    # it needs the network, under the base's rules
    bare = OC.optimizer_cem(gru_fused=True, **KW)
    with pytest.raises(ValueError, match="gru_fused=True is the fused step over the GRU predictor: it needs gru_model="):
        bare.configure()
    with pytest.raises(ValueError, match="a GRU predictor_specification needs gru_model="):
        OC.optimizer_cem(gru_fused=True, **KW).configure(predictor_specification=SPEC)
    with pytest.raises(ValueError, match="selects the ODE predictor"):
        OC.optimizer_cem(gru_model=model, gru_fused=True, **KW).configure(predictor_specification="ODE")
    # fused=True beside a model: the old sentence, word for word; both flags: refused by name
    with pytest.raises(ValueError, match="fused=True integrates the ODE") as ei:
        OC.optimizer_cem(gru_model=model, fused=True, **KW)
    assert str(ei.value) == OC.GRU_NOT_FUSED and "cpmppi_cem_step" in str(ei.value)
    late = OC.optimizer_cem(fused=True, **KW)
    with pytest.raises(ValueError, match="fused=True integrates the ODE"):
        late.configure(predictor_specification=SPEC)
    with pytest.raises(ValueError, match="gru_fused=True and fused=True"):
        OC.optimizer_cem(gru_model=model, fused=True, gru_fused=True, **KW)
    # not fusable, and no fused GRU adjoint: refused by name
    for cls, why in ((OC.optimizer_cem_gmm, "cem-gmm is not fusable"), (OC.optimizer_random_action, "random-action is not fusable"),
                     (OC.optimizer_cem_naive_grad, "no fused GRU adjoint"), (OC.optimizer_cem_grad_bharadhwaj, "no fused GRU adjoint")):
        kw = {k: v for k, v in KW.items() if not (cls is OC.optimizer_random_action and k.startswith("cem_"))}
        for given in (dict(gru_model=model), dict(gru_model=model, gru_adjoint=True), {}):
            with pytest.raises(ValueError, match=r"gru_fused=True: .*cpmppi_cem_step_gru.* is built for cem, not for "
                                                 + cls.optimizer_name + ": .*" + why):
                cls(gru_fused=True, **given, **kw)
    # ... and _check_gru_adjoint's refusal stays
    with pytest.raises(ValueError, match="gru_adjoint=True with fused=True"):
        OC.optimizer_cem_naive_grad(gru_model=model, gru_adjoint=True, fused=True, **KW)
    # controller_mpc hands the flag on from its config, as it hands gru_model on
    ctrl = controller_mpc(config=dict(gru_model=model, gru_fused=True, num_rollouts=12, mpc_horizon=6, seed=3), num_envs=2)
    ctrl.configure("cem")
    assert type(ctrl.optimizer) is OC.optimizer_cem and ctrl.optimizer.gru_fused and ctrl.optimizer.fused and ctrl.predictor is None
    with pytest.raises(ValueError, match="not for cem-gmm"):
        ctrl.configure("cem-gmm")
    ctrl = controller_mpc(config=dict(gru_model=model, num_rollouts=12, mpc_horizon=6, seed=3), num_envs=2)
    ctrl.configure("cem")
    assert ctrl.optimizer.gru_fused is False and ctrl.optimizer.fused is False             # opt-in


def test_one_step_and_one_advance_per_control_step(gru_fused_engine):
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    E, s = 2, _states(2)
    opt = optimizer_cem(gru_model=golden_model(), gru_fused=True, optimizer_logging=True, **KW)
    opt.configure()
    eng, h_id = opt.engine, opt.h.data_ptr()
    for step in range(3):
        u = opt.step(s)
        launch, adv = eng.gru_launches[-1], eng.advances[-1]
        assert len(eng.gru_launches) == len(eng.advances) == step + 1 and adv["launches_before"] == step + 1     # step, then advance
        assert launch["offset"] == 3 * step and launch["iterations"] == 3 and launch["best_k"] == 4 and launch["shift"] == 1
        assert launch["stdev_min"] == 0.02 and launch["mean_fill"] == 0.0 and launch["stdev_fill"] == math.sqrt(0.5)
        assert launch["seed"] == 5 and launch["count_dev"] is None
        assert launch["h0"] is opt.h and launch["mean"] is opt.dist_mue and launch["stdev"] is opt.stdev
        assert adv["h"] is opt.h and adv["Q"] is opt.controls and adv["s"].data_ptr() == launch["s0"].data_ptr()
        assert opt.h.data_ptr() == h_id and float(opt.h.min()) == step + 1.0                 # in place, once per step
        assert u.shape == (E, 1) and np.all(u == 1.0 + 3 * step)
        assert opt.logging_values["J_logged"].shape == (E, 12)
    assert opt.step_counter == 9 and eng.fused_launches == []                                # never the ODE step
    assert eng.calls == dict(eng.calls, grad=0, cost=0, cem_sample=0)
    # the device form: the same two calls, nothing counted on the host; L and previous_input go unread
    s_t, tp, te = torch.as_tensor(s, dtype=torch.float32), torch.zeros(E), torch.ones(E)
    counter = torch.zeros(1, dtype=torch.int64)
    out = opt.step_device(s_t, tp, te, L=torch.full((E,), 0.4), previous_input=opt.controls, count_dev=counter)
    assert out is opt.controls and eng.gru_launches[-1]["count_dev"] is counter and len(eng.advances) == 4
    assert eng.advances[-1]["s"] is s_t and opt.step_counter == 9
    opt.optimizer_reset()
    assert not opt.h.any() and opt.h.data_ptr() == h_id and opt.step_counter == 0
    called = []
    eng.cem_reserve = lambda E=None, refine=None: called.append(refine)
    opt.reserve_fused()
    assert called == [None]


def test_the_device_loop_tells_a_network_optimizer_no_pole_mass(gru_fused_engine, monkeypatch):
    from cartpolesimulation_amd import harness as HA
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    E = 2
    cfg = dict(seed=31, length_of_experiment=0.1, random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    prm = dict(m_pole=dict(init_value=0.087, change_every_x_seconds=0.03, mode="bounce", range_random=[0.05, 0.12], range_clip=[0.05, 0.12],
                           increment=0.004, reset_every_x_seconds="inf"))
    b = SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(E, 83, stride=1), prm, seed=84)
    monkeypatch.setattr(FusedFake, "mppi", property(lambda self: self.cfg), raising=False)
    runs = {}
    for name, kw in (("network", dict(gru_model=golden_model(), gru_fused=True)), ("equations", dict(fused=True))):
        opt = optimizer_cem(**kw, **KW)
        opt.cfg.predictor_type = "ODE"                      # the handle's integrator is told the mass call by call - the network is not
        opt.configure()
        runs[name] = HA.ScheduleRun(opt.engine, b, 0, optimizer=opt)
        assert runs[name].fused and runs[name].Q is opt.controls
    assert runs["equations"].mass.kind == "value" and runs["equations"].mass.varies
    assert runs["network"].mass.kind == "none" and not runs["network"].mass.varies
    assert HA.ControllerMass(b, runs["network"].eng.mppi, network=True).kind == "none"
    with pytest.raises(ValueError, match="ONE pole mass"):
        runs["equations"].capture(5)

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached

    monkeypatch.setattr(torch.cuda, "Stream", stop)          # the first thing capture() does once nothing forbids it
    with pytest.raises(Reached):
        runs["network"].capture(5)
    assert runs["network"].controller.opt.engine.reserved == [("cem", None)]
    # control along recordings over the network stays out of scope, named
    rb = SimpleNamespace(E=E, T=3)
    with pytest.raises(ValueError, match="does not serve the GRU predictor"):
        HA.ReplayRun(runs["network"].eng, rb, 0, optimizer=runs["network"].controller.opt)


def test_command_line_builds_the_fused_gru_optimizer(gru_fused_engine, monkeypatch, tmp_path):
    from cartpolesimulation_amd import recording as R
    from cartpolesimulation_amd import _optimizer_base as OB
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    seen = {}

    def gen(engine, n, out, **kw):
        seen.update(engine=engine, n=n, out=out, **kw)
        return [os.path.join(out, "Experiment.csv")]

    monkeypatch.setattr(R, "generate_dataset", gen)
    import cartpolesimulation_amd.model_folder as MF
    monkeypatch.setattr(MF, "load_gru_model", lambda folder: dict(golden_model(), folder=folder))
    folder = str(tmp_path / "GRU-6IN-32H1-32H2-5OUT-0")
    R.main(["--optimizer", "cem", "--fused", "--gru-model", folder, "--experiments", "3", "--rollouts", "12", "--horizon", "6",
            "--seed", "4", "--out", str(tmp_path)])
    opt = seen["optimizer"]
    assert type(opt) is optimizer_cem and opt.gru_fused and opt.fused and opt.num_envs == 3 and opt.num_rollouts == 12
    assert opt.gru_model["folder"] == folder and opt.engine.gru is opt.gru_model and opt.h is not None
    assert seen["engine"] is None and seen["gru_model"] is None and seen["graph"] is True
    # the other optimizers keep the exit message, and so does cem without --fused
    for argv in (["--optimizer", "cem-gmm"], ["--optimizer", "rpgd", "--fused"], ["--optimizer", "cem-naive-grad", "--fused"],
                 ["--optimizer", "cem"]):
        with pytest.raises(SystemExit, match="built for the fused MPPI step"):
            R.main(argv + ["--gru-model", folder, "--experiments", "2", "--rollouts", "12", "--horizon", "6", "--seed", "4"])
    assert OB.GRU_SPECIFICATION == "GRU-6IN-32H1-32H2-5OUT"
