"""CPU: the host side of the fused rpgd / gradient control step over the GRU predictor - the exports and the ctypes mirror of
cpmppi_rpgd_gru_args against the header text and against cpmppi_rpgd_args, the rules of ``gru_fused=True`` on optimizer_rpgd and
optimizer_gradient (what it needs, what it refuses, which refusals stay word for word), the bookkeeping of the fused object on a
stand-in engine (one cpmppi_rpgd_step_gru and one cpmppi_gru_advance per control step, on the optimizer's own memory), the
controller kind and pole-mass rule of the device loop, and the data generator's command line."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_cem_fused_host import FusedFake  # noqa: E402
from test_cem_gru_fused_host import header_fields  # noqa: E402
from test_gru_sampling_optimizers_host import SPEC, golden_model  # noqa: E402
from test_optimizers_host_logic import CHECKOUT, _states  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(seed=5, mpc_horizon=6, num_rollouts=12, num_envs=2)
RPGD = dict(outer_its=3, resamp_per=2, opt_keep_k_ratio=0.5, shift_previous=1, sample_mean=0.05)


def test_exports_and_abi_version():
    from cartpolesimulation_amd import _lib
    assert "cpmppi_rpgd_step_gru" in _lib.EXPORTS and "cpmppi_rpgd_gru_reserve" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert re.search(r"#define CPMPPI_ABI_VERSION 5u", text)
    assert re.search(r"int cpmppi_rpgd_step_gru\(cpmppi_handle\* h, const cpmppi_rpgd_gru_args\* args, void\* stream\);", text)
    assert re.search(r"int cpmppi_rpgd_gru_reserve\(cpmppi_handle\* h, uint32_t E\);", text)
    # no existing struct changed: the ODE step's block and the CEM blocks are what they were
    assert len(_lib.cpmppi_rpgd_args._fields_) == 32 and len(_lib.cpmppi_cem_args._fields_) == 29
    assert len(_lib.cpmppi_cem_gru_args._fields_) == 22
    lib = _lib.load()
    assert lib.cpmppi_abi_version() == 5 and hasattr(lib, "cpmppi_rpgd_step_gru") and hasattr(lib, "cpmppi_rpgd_gru_reserve")


def _rpgd_args_header_fields():
    """cpmppi_rpgd_args' fields from the header text (its first comment does not name the struct, as the newer blocks' do)."""
    from test_cem_fused_host import C_TYPES
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    end = text.index("} cpmppi_rpgd_args;")
    body = re.sub(r"/\*.*?\*/", "", text[text.rindex("typedef struct {", 0, end):end], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if decl:
            mt = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
            assert mt, decl
            fields.append((mt.group(4), C.c_void_p if mt.group(3) else C_TYPES[mt.group(2)]))
    return fields


def test_rpgd_gru_args_mirror_matches_the_header():
    """Field order, names and types of the ctypes mirror against the struct's text in include/cpmppi.h; and the struct is
    cpmppi_rpgd_args without L and previous_input, plus h0 in their place."""
    from cartpolesimulation_amd import _lib
    fields = header_fields("cpmppi_rpgd_gru_args")
    assert fields == list(_lib.cpmppi_rpgd_gru_args._fields_)
    A = _lib.cpmppi_rpgd_gru_args
    for name, ctype in fields:
        if ctype in (C.c_void_p, C.c_uint64):
            assert getattr(A, name).offset % 8 == 0, name
    ode = _rpgd_args_header_fields()
    assert ode == list(_lib.cpmppi_rpgd_args._fields_)
    assert [f for f in fields if f[0] != "h0"] == [f for f in ode if f[0] not in ("L", "previous_input")]
    names = [n for n, _ in fields]
    assert dict(fields)["h0"] is C.c_void_p and len(fields) == len(ode) - 1 and names.index("h0") == names.index("Q") - 1
    assert C.sizeof(A) == C.sizeof(_lib.cpmppi_rpgd_args) - 8


class GruRpgdFake(FusedFake):
    """FusedFake plus the fused GRU rpgd step, its reserve and the memory's hand-over, recorded."""

    def __init__(self, E, cfg, phys=None, device=0):
        super().__init__(E, cfg, phys, device)
        self.gru_launches, self.advances, self.ode_launches, self.gru = [], [], [], None

    def rpgd_gru_reserve(self, E=None):
        self.reserved.append("rpgd_gru")

    def prepare_rpgd_step(self, *a, **kw):
        self.ode_launches.append(kw)
        return super().prepare_rpgd_step(*a, **kw)

    def prepare_rpgd_step_gru(self, s0, Q, m, v, tp, te, h0=None, **kw):
        eng, args = self, SimpleNamespace(**kw)

        class Prepared:
            def run(self, **host):
                for name, x in host.items():
                    assert name in ("count", "adam_iteration", "draw_offset", "iterations")
                    setattr(args, name, x)
                eng.gru_launches.append(dict(vars(args), s0=s0, Q=Q, m=m, v=v, h0=h0, host=dict(host)))
                args.Q_out.fill_(100.0 if args.count_dev is not None else 1.0 + host["count"])
                args.S_out.copy_(torch.arange(eng.N, dtype=torch.float32).expand(eng.E, eng.N))
                args.plan_out.copy_(args.Q_out[:, None].expand(eng.E, eng.H))

        return Prepared()

    def gru_advance(self, s, Q, h):
        self.advances.append(dict(s=s, Q=Q, h=h, launches_before=len(self.gru_launches)))
        h.add_(1.0)
        return h


@pytest.fixture()
def gru_rpgd_engine(monkeypatch):
    import cartpolesimulation_amd.engine as EN
    monkeypatch.setattr(EN, "MPPIEngine", GruRpgdFake)
    return GruRpgdFake


def _classes():
    from cartpolesimulation_amd import optimizer_gradient as OG
    return ((OG.optimizer_rpgd, dict(KW, **RPGD)), (OG.optimizer_gradient, dict(KW, gradient_steps=3)))


def test_flag_rules(gru_rpgd_engine):
    from cartpolesimulation_amd import optimizer_cem as OC
    from cartpolesimulation_amd import optimizer_gradient as OG
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    from cartpolesimulation_amd.harness import FusedOptimizer, HostPacedOptimizer, optimizer_controller
    model = golden_model()
    for cls, kw in _classes():
        # the opt-in makes a fused object over the network; by a model, by a model and a specification; gru_adjoint beside it is accepted
        for spec, more in ((None, {}), (SPEC, {}), (None, dict(gru_adjoint=True))):
            opt = cls(gru_model=model, gru_fused=True, **more, **kw)
            assert opt.fused is True and opt.gru_fused is True and opt.gru_adjoint is True
            opt.configure(predictor_specification=spec)
            assert opt.engine.gru is model and tuple(opt.h.shape) == (2, 2, 32) and optimizer_controller(opt) is FusedOptimizer
        staged = cls(gru_model=model, gru_adjoint=True, **kw)
        assert staged.fused is False and staged.gru_fused is False and optimizer_controller(staged) is HostPacedOptimizer
        plain = cls(**kw)
        assert plain.fused is False and plain.gru_fused is False and plain.gru_adjoint is False
        # it needs the network, in optimizer_cem's sentence, under the base's rules
        with pytest.raises(ValueError) as ei:
            cls(gru_fused=True, **kw).configure()
        assert str(ei.value) == OC.GRU_FUSED_NEEDS_MODEL
        with pytest.raises(ValueError, match="a GRU predictor_specification needs gru_model="):
            cls(gru_fused=True, **kw).configure(predictor_specification=SPEC)
        with pytest.raises(ValueError, match="selects the ODE predictor"):
            cls(gru_model=model, gru_fused=True, **kw).configure(predictor_specification="ODE")
        # both flags: refused by name, with this family's entry points
        with pytest.raises(ValueError, match="gru_fused=True and fused=True") as ei:
            cls(gru_model=model, fused=True, gru_fused=True, **kw)
        assert str(ei.value) == OG.GRU_FUSED_OR_FUSED and "cpmppi_rpgd_step_gru" in str(ei.value)
        assert OG.GRU_FUSED_OR_FUSED == OC.GRU_FUSED_OR_FUSED.replace("cpmppi_cem_step", "cpmppi_rpgd_step")
        # no such cost in the GRU kernels
        with pytest.raises(ValueError, match="gru_adjoint=True with quadratic_boundary_grad"):
            cls(gru_model=model, gru_fused=True, cost_function_specification="quadratic_boundary_grad", **kw)
        # what stays word for word
        with pytest.raises(ValueError, match="gru_adjoint=True with fused=True: cpmppi_rpgd_step and cpmppi_cem_step integrate the ODE"):
            cls(gru_model=model, gru_adjoint=True, fused=True, **kw)
        with pytest.raises(NotImplementedError) as ei:
            cls(gru_model=model, fused=True, **kw)
        assert str(ei.value) == cls._gru_refusal and "pass gru_adjoint=True" in str(ei.value)
        with pytest.raises(NotImplementedError):
            cls(gru_model=model, **kw)
        late = cls(fused=True, **kw)
        with pytest.raises(NotImplementedError):
            late.configure(predictor_specification=SPEC)
    # the two CEM hybrids still have no fused GRU adjoint
    for cls in (OC.optimizer_cem_naive_grad, OC.optimizer_cem_grad_bharadhwaj):
        with pytest.raises(ValueError, match="no fused GRU adjoint"):
            cls(gru_model=model, gru_fused=True, seed=5, mpc_horizon=6, num_rollouts=12, num_envs=2)
    # controller_mpc hands the flag on from its config, as it hands gru_model on
    for name, cls in (("rpgd", OG.optimizer_rpgd), ("gradient", OG.optimizer_gradient)):
        ctrl = controller_mpc(config=dict(gru_model=model, gru_fused=True, num_rollouts=12, mpc_horizon=6, seed=3), num_envs=2)
        ctrl.configure(name)
        assert type(ctrl.optimizer) is cls and ctrl.optimizer.gru_fused and ctrl.optimizer.fused and ctrl.predictor is None
        ctrl = controller_mpc(config=dict(gru_model=model, gru_adjoint=True, num_rollouts=12, mpc_horizon=6, seed=3), num_envs=2)
        ctrl.configure(name)
        assert ctrl.optimizer.gru_fused is False and ctrl.optimizer.fused is False             # opt-in


@pytest.mark.parametrize("which", [0, 1])
def test_one_step_and_one_advance_per_control_step(gru_rpgd_engine, which):
    cls, kw = _classes()[which]
    rpgd = which == 0
    E, s = 2, _states(2)
    opt = cls(gru_model=golden_model(), gru_fused=True, optimizer_logging=True, **kw)
    opt.configure()
    eng, h_id, draws0 = opt.engine, opt.h.data_ptr(), opt.draws
    assert draws0 == 1
    for step in range(4):
        u = opt.step(s)
        launch, adv = eng.gru_launches[-1], eng.advances[-1]
        assert len(eng.gru_launches) == len(eng.advances) == step + 1 and adv["launches_before"] == step + 1     # step, then advance
        resampled = sum(1 for c in range(1, step + 1) if c % 2 == 0) if rpgd else 0      # resamp_per = 2: after steps 2, 4, ...
        assert launch["host"] == dict(count=step, adam_iteration=3 * step, draw_offset=draws0 + resampled, iterations=3)
        assert launch["keep_k"] == (6 if rpgd else 12) and launch["resamp_per"] == (2 if rpgd else 0) and launch["shift"] == 1
        assert launch["seed"] == 5 and launch["count_dev"] is None and launch["learning_rate"] == 0.05
        if rpgd:
            assert launch["distribution"] == "normal" and launch["sample_mean"] == 0.05
        assert launch["h0"] is opt.h and launch["Q"] is opt.Q and launch["m"] is opt.m and launch["v"] is opt.v
        assert adv["h"] is opt.h and adv["Q"] is opt.controls and adv["s"].data_ptr() == launch["s0"].data_ptr()
        assert opt.h.data_ptr() == h_id and float(opt.h.min()) == step + 1.0                 # in place, once per step
        assert u.shape == (E, 1) and np.all(u == 1.0 + step)
        assert opt.logging_values["J_logged"].shape == (E, 12)
    assert opt.count == 4 and opt.adam_it == 12 and opt.draws == draws0 + (2 if rpgd else 0)
    assert eng.ode_launches == [] and eng.calls == dict(eng.calls, grad=0, cost=0, adam=0)   # never the ODE step, never staged
    # the device form: the same two calls, nothing counted on the host; L and previous_input go unread
    s_t, tp, te = torch.as_tensor(s, dtype=torch.float32), torch.zeros(E), torch.ones(E)
    counter = torch.zeros(1, dtype=torch.int64)
    out = opt.step_device(s_t, tp, te, L=torch.full((E,), 0.4), previous_input=opt.controls, count_dev=counter)
    assert out is opt.controls and eng.gru_launches[-1]["count_dev"] is counter and eng.gru_launches[-1]["host"] == {}
    assert len(eng.advances) == 5 and eng.advances[-1]["s"] is s_t and opt.count == 4 and opt.adam_it == 12
    opt.optimizer_reset()
    assert not opt.h.any() and opt.h.data_ptr() == h_id and opt.count == 0
    opt.reserve_fused()
    assert eng.reserved == ["rpgd_gru"]
    # warmup=True keeps the host counters: the first step runs warmup_iterations, a device counter is refused
    warm = cls(gru_model=golden_model(), gru_fused=True, warmup=True, warmup_iterations=7, **kw)
    warm.configure()
    warm.step(s)
    warm.step(s)
    assert [x["host"]["iterations"] for x in warm.engine.gru_launches] == [7, 3] and warm.adam_it == 10
    with pytest.raises(ValueError, match="warmup=True"):
        warm.step_device(s_t, tp, te, count_dev=counter)


def test_the_device_loop_tells_a_network_optimizer_no_pole_mass(gru_rpgd_engine, monkeypatch):
    from cartpolesimulation_amd import harness as HA
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.optimizer_gradient import optimizer_rpgd
    E = 2
    cfg = dict(seed=31, length_of_experiment=0.1, random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    prm = dict(m_pole=dict(init_value=0.087, change_every_x_seconds=0.03, mode="bounce", range_random=[0.05, 0.12], range_clip=[0.05, 0.12],
                           increment=0.004, reset_every_x_seconds="inf"))
    b = SC.apply_parameter_schedule(SC.RandomExperimentSetter(cfg).draw(E, 83, stride=1), prm, seed=84)
    monkeypatch.setattr(FusedFake, "mppi", property(lambda self: self.cfg), raising=False)
    runs = {}
    for name, kw in (("network", dict(gru_model=golden_model(), gru_fused=True)), ("equations", dict(fused=True))):
        opt = optimizer_rpgd(**kw, **KW, **RPGD)
        opt.cfg.predictor_type = "ODE"                      # the handle's integrator is told the mass call by call - the network is not
        opt.configure()
        runs[name] = HA.ScheduleRun(opt.engine, b, 0, optimizer=opt)
        assert runs[name].fused and runs[name].Q is opt.controls and isinstance(runs[name].controller, HA.FusedOptimizer)
    assert runs["equations"].mass.kind == "value" and runs["equations"].mass.varies
    assert runs["network"].mass.kind == "none" and not runs["network"].mass.varies
    with pytest.raises(ValueError, match="ONE pole mass"):
        runs["equations"].capture(5)

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached

    monkeypatch.setattr(torch.cuda, "Stream", stop)          # the first thing capture() does once nothing forbids it
    with pytest.raises(Reached):
        runs["network"].capture(5)
    assert runs["network"].controller.opt.engine.reserved == ["rpgd_gru"]
    # control along recordings over the network stays out of scope, named
    with pytest.raises(ValueError, match="does not serve the GRU predictor"):
        HA.ReplayRun(runs["network"].eng, SimpleNamespace(E=E, T=3), 0, optimizer=runs["network"].controller.opt)


def test_command_line_builds_the_fused_gru_optimizer(gru_rpgd_engine, monkeypatch, tmp_path):
    """`recording --optimizer rpgd|gradient --gru-fused --gru-model FOLDER` builds the fused optimizer over the network and runs it
    captured; with --config-root the checkout's own optimizer (rpgd).  (`--fused --gru-model` beside rpgd keeps its exit message:
    --fused is the step that integrates the ODE.)"""
    from cartpolesimulation_amd import recording as R
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    from cartpolesimulation_amd.optimizer_gradient import optimizer_gradient, optimizer_rpgd
    seen = {}

    def gen(engine, n, out, **kw):
        seen.clear()
        seen.update(engine=engine, n=n, out=out, **kw)
        return [os.path.join(out, "Experiment.csv")]

    monkeypatch.setattr(R, "generate_dataset", gen)
    import cartpolesimulation_amd.model_folder as MF
    monkeypatch.setattr(MF, "load_gru_model", lambda folder: dict(golden_model(), folder=folder))
    folder = str(tmp_path / "GRU-6IN-32H1-32H2-5OUT-0")
    common = ["--gru-model", folder, "--experiments", "3", "--rollouts", "12", "--horizon", "6", "--seed", "4", "--out", str(tmp_path)]
    for name, cls in (("rpgd", optimizer_rpgd), ("gradient", optimizer_gradient), ("cem", optimizer_cem)):
        R.main(["--optimizer", name, "--gru-fused"] + common)
        opt = seen["optimizer"]
        assert type(opt) is cls and opt.gru_fused and opt.fused and opt.num_envs == 3 and opt.num_rollouts == 12
        assert opt.gru_model["folder"] == folder and opt.engine.gru is opt.gru_model and opt.h is not None
        assert seen["engine"] is None and seen["gru_model"] is None and seen["graph"] is True
    # the checkout's settings (tests/golden/reference_checkout: config_controllers.yml names rpgd, as shipped) choose the optimizer
    R.main(["--config-root", CHECKOUT, "--gru-fused"] + common)
    opt = seen["optimizer"]
    assert type(opt) is optimizer_rpgd and opt.gru_fused and opt.fused and opt.h is not None and seen["graph"] is True
    assert opt.outer_its == 4 and opt.resamp_per == 10                       # (config_optimizers.yml: rpgd)
    # what the flag refuses, by name
    for argv, text in ((["--optimizer", "rpgd", "--gru-fused"], "needs --gru-model"),
                       (["--optimizer", "rpgd", "--gru-fused", "--fused", "--gru-model", folder], "give one of them"),
                       (["--optimizer", "cem-gmm", "--gru-fused", "--gru-model", folder], "built for rpgd, gradient and cem, not 'cem-gmm'"),
                       (["--gru-fused", "--gru-model", folder], "built for rpgd, gradient and cem, not 'mppi'"),
                       (["--optimizer", "rpgd", "--gru-fused", "--groups", "2", "--gru-model", folder], "--groups 1")):
        with pytest.raises(SystemExit, match=text):
            R.main(argv + ["--experiments", "2", "--rollouts", "12", "--horizon", "6", "--seed", "4"])
