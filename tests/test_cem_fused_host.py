"""CPU: the host side of the fused CEM control step - exports and the ctypes mirror of cpmppi_cem_args against the header text,
and the bookkeeping of `fused=True` on cem / cem-naive-grad / cem-grad-bharadhwaj (one library call per control step, the Philox
offset and iteration count it is handed, warm-up, reset, the refusals of optimizer and harness) on the checker-backed stand-in
for the device engine of test_optimizers_host_logic.py."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_optimizers_host_logic import FakeEngine, _states  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}


def test_exports_and_abi_version():
    from cartpolesimulation_amd import _lib
    assert "cpmppi_cem_step" in _lib.EXPORTS and "cpmppi_cem_reserve" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert re.search(r"#define CPMPPI_ABI_VERSION 5u", text)
    assert re.search(r"int cpmppi_cem_step\(cpmppi_handle\* h, const cpmppi_cem_args\* args, void\* stream\);", text)
    assert re.search(r"int cpmppi_cem_reserve\(cpmppi_handle\* h, uint32_t E, uint32_t refine\);", text)
    assert (_lib.CEM_REFINE_NONE, _lib.CEM_REFINE_SGD, _lib.CEM_REFINE_ADAM) == (0, 1, 2)
    assert re.search(r"CPMPPI_CEM_REFINE_NONE = 0, CPMPPI_CEM_REFINE_SGD = 1, CPMPPI_CEM_REFINE_ADAM = 2", text)


def test_cem_args_mirror_matches_the_header():
    """Field order, names and types of the ctypes mirror, machine-checked against the struct's text in include/cpmppi.h."""
    from cartpolesimulation_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    body = text[text.index("typedef struct {\n  uint32_t E;                       /* active envs in this call (cpmppi_cem_args) */"):
                text.index("} cpmppi_cem_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        mt = re.match(r"^(const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        assert mt, decl
        fields.append((mt.group(4), C.c_void_p if mt.group(3) else C_TYPES[mt.group(2)]))
    assert fields == list(_lib.cpmppi_cem_args._fields_)
    assert len(fields) == 29
    # natural alignment of the C struct = ctypes' default: pointers and the 64-bit words on 8-byte offsets
    A = _lib.cpmppi_cem_args
    for name, ctype in fields:
        if ctype in (C.c_void_p, C.c_uint64):
            assert getattr(A, name).offset % 8 == 0, name
    # every group of the contract is there
    names = [n for n, _ in fields]
    for group in (("E", "s0", "target_position", "target_equilibrium", "L", "previous_input"), ("mean", "stdev"),
                  ("iterations", "best_k", "stdev_min"), ("refine", "learning_rate", "beta1", "beta2", "epsilon", "gradmax_clip"),
                  ("shift", "mean_fill", "stdev_fill"), ("seed", "offset", "env_offset", "count_dev"),
                  ("Q_out", "S_out", "plan_out", "samples_out", "order_out")):
        assert all(n in names for n in group), group


class FusedFake(FakeEngine):
    """FakeEngine plus the fused entry points: every launch is recorded with what it was handed; it writes the control
    1 + offset (or 100 in device mode) so that the optimizer's outputs can be told apart."""

    def __init__(self, E, cfg, phys=None, device=0):
        super().__init__(E, cfg, phys, device)
        self.fused_launches, self.reserved = [], []

    def apply_pole_mass_of(self, variable_parameters, **kw):
        pass

    def rpgd_reserve(self, E=None):
        self.reserved.append("rpgd")

    def cem_reserve(self, E=None, refine=None):
        self.reserved.append(("cem", refine))

    def prepare_rpgd_step(self, *a, **kw):
        return SimpleNamespace(run=lambda **k: None)

    def prepare_cem_step(self, s0, mean, stdev, tp, te, L=None, previous_input=None, **kw):
        eng, args = self, SimpleNamespace(**kw)

        class Prepared:
            def run(self, offset=None, iterations=None):
                for name, x in (("offset", offset), ("iterations", iterations)):
                    if x is not None:
                        setattr(args, name, x)
                eng.fused_launches.append(dict(vars(args), previous_input=previous_input, mean=mean, stdev=stdev))
                args.Q_out.fill_(100.0 if args.count_dev is not None else 1.0 + args.offset)
                args.S_out.copy_(torch.arange(eng.N, dtype=torch.float32).expand(eng.E, eng.N))
                args.plan_out.copy_(args.Q_out[:, None].expand(eng.E, eng.H))

        p = Prepared()
        p.args = args
        return p


@pytest.fixture()
def fused_engine(monkeypatch):
    import cartpolesimulation_amd.engine as EN
    monkeypatch.setattr(EN, "MPPIEngine", FusedFake)
    return FusedFake


CEM = dict(seed=2, mpc_horizon=8, num_rollouts=8, cem_outer_it=3, cem_best_k=3, cem_stdev_min=0.02, num_envs=2)


def _classes():
    from cartpolesimulation_amd import optimizer_cem as OC
    return {"cem": (OC.optimizer_cem, None), "cem-naive-grad": (OC.optimizer_cem_naive_grad, "sgd"),
            "cem-grad-bharadhwaj": (OC.optimizer_cem_grad_bharadhwaj, "adam")}


@pytest.mark.parametrize("name", ["cem", "cem-naive-grad", "cem-grad-bharadhwaj"])
def test_one_library_call_per_control_step_with_the_offsets_of_the_staged_path(fused_engine, name):
    cls, refine = _classes()[name]
    s = _states(2)
    staged, fused = cls(**CEM), cls(fused=True, optimizer_logging=True, **CEM)
    staged.configure()
    fused.configure()
    assert not staged.fused and fused.fused
    mean_id, stdev_id = fused.dist_mue.data_ptr(), fused.stdev.data_ptr()
    for step in range(4):
        before = staged.step_counter
        assert fused.step_counter == before
        staged.step(s)
        u = fused.step(s)
        launch = fused.engine.fused_launches[-1]
        assert len(fused.engine.fused_launches) == step + 1                 # exactly one fused launch per control step ...
        assert launch["offset"] == before and launch["iterations"] == 3
        assert launch["best_k"] == 3 and launch["stdev_min"] == 0.02 and launch["shift"] == 1
        assert launch["mean_fill"] == 0.0 and launch["stdev_fill"] == math.sqrt(0.5) and launch["seed"] == 2
        assert launch["count_dev"] is None and launch.get("refine") == refine
        assert launch["mean"].data_ptr() == mean_id and launch["stdev"].data_ptr() == stdev_id
        assert u.shape == (2, 1) and np.all(u == 1.0 + before)
        assert np.array_equal(fused.logging_values["Q_logged"], u[:, 0]) and fused.logging_values["J_logged"].shape == (2, 8)
        assert fused.logging_values["u_logged"].shape == (2, 8)
    assert staged.step_counter == 12 and fused.step_counter == 12
    # ... and nothing else: no staged launch at all, mean and stdev stay the buffers they were
    assert fused.engine.calls == dict(fused.engine.calls, grad=0, cost=0, adam=0, sgd=0, cem_sample=0)
    assert fused.dist_mue.data_ptr() == mean_id and fused.stdev.data_ptr() == stdev_id
    if refine == "sgd":
        assert launch["learning_rate"] == fused.learning_rate and launch["gradmax_clip"] == fused.gradmax_clip
    if refine == "adam":
        assert (launch["beta1"], launch["beta2"], launch["epsilon"]) == (fused.adam_beta_1, fused.adam_beta_2, fused.adam_epsilon)
    # the control of the step before is the next step's previous input (none before the first)
    assert fused.engine.fused_launches[0]["previous_input"] is None
    for later in fused.engine.fused_launches[1:]:
        assert later["previous_input"] is fused.controls
    # as_tensor: a tensor of the caller's own, not the buffer the next step overwrites
    t = fused.step(s, as_tensor=True)
    assert torch.is_tensor(t) and t.data_ptr() != fused.controls.data_ptr() and torch.equal(t, fused.controls)


def test_warmup_first_step_and_reset(fused_engine):
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    s = _states(2)
    staged = optimizer_cem(warmup=True, warmup_iterations=11, **CEM)
    g = optimizer_cem(fused=True, warmup=True, warmup_iterations=11, **CEM)
    staged.configure()
    g.configure()
    for _ in range(2):
        staged.step(s)
        g.step(s)
    first, second = g.engine.fused_launches
    assert (first["iterations"], first["offset"]) == (11, 0)                     # warm-up on the first step only
    assert (second["iterations"], second["offset"]) == (3, 11)
    assert g.step_counter == staged.step_counter == 14
    assert first["previous_input"] is None and second["previous_input"] is g.controls
    # after a reset the first step warms up again, from offset 0 and with no previous input
    g.optimizer_reset()
    staged.optimizer_reset()
    staged.step(s)
    g.step(s)
    last = g.engine.fused_launches[-1]
    assert (last["iterations"], last["offset"]) == (11, 0) and last["previous_input"] is None
    assert g.step_counter == staged.step_counter == 11
    g.step(s)
    assert g.engine.fused_launches[-1]["previous_input"] is g.controls and g.engine.fused_launches[-1]["offset"] == 11


def test_gmm_and_random_action_refuse_fused(fused_engine):
    from cartpolesimulation_amd import optimizer_cem as OC
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    for cls in (OC.optimizer_cem_gmm, OC.optimizer_random_action):
        with pytest.raises(ValueError, match="built for cem, cem-naive-grad and cem-grad-bharadhwaj, not for " + cls.optimizer_name):
            cls(fused=True, seed=1, num_envs=2)
        assert cls(seed=1, num_envs=2).fused is False
    c = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), config=dict(seed=3, fused=True), num_envs=2)
    with pytest.raises(ValueError, match="not for cem-gmm"):
        c.configure("cem-gmm")
    for name in ("cem", "cem-naive-grad-tf", "cem-grad-bharadhwaj"):
        c.configure(name)
        assert c.optimizer.fused is True
    c = controller_mpc("CartPole", {}, control_limits=([-1.0], [1.0]), config=dict(seed=3), num_envs=2)
    c.configure("cem")
    assert c.optimizer.fused is False                                            # opt-in


def test_step_device_and_its_refusals(fused_engine):
    from cartpolesimulation_amd.optimizer_cem import optimizer_cem
    E = 2
    s = torch.as_tensor(_states(E), dtype=torch.float32)
    tp, te, L = torch.zeros(E), torch.ones(E), torch.full((E,), 0.395)
    counter = torch.zeros(1, dtype=torch.int64)
    r = optimizer_cem(fused=True, **CEM)
    r.configure()
    u = r.step_device(s, tp, te, L=L, count_dev=counter)
    assert u is r.controls and torch.all(u == 100.0)
    launch = r.engine.fused_launches[-1]
    assert launch["count_dev"] is counter and launch["offset"] == 0 and launch["iterations"] == 3
    assert r.step_counter == 0                                                   # device mode: the host counts nothing
    r.step_device(s, tp, te, L=L, count_dev=counter)
    assert len(r.engine.fused_launches) == 2
    # without a device counter the host counter advances as in step()
    r.step_device(s, tp, te, L=L)
    assert r.engine.fused_launches[-1]["count_dev"] is None and r.step_counter == 3
    with pytest.raises(ValueError, match="target_position must be a contiguous float32 tensor"):
        r.step_device(s, torch.zeros(E, dtype=torch.float64), te)
    with pytest.raises(ValueError, match="s must be"):
        r.step_device(s[:1], tp, te)
    # a device counter cannot tell a warm-up step from the others
    w = optimizer_cem(fused=True, warmup=True, **CEM)
    w.configure()
    with pytest.raises(ValueError, match="warmup"):
        w.step_device(s, tp, te, count_dev=counter)
    w.step_device(s, tp, te)                                                     # (host counter: allowed)
    assert w.engine.fused_launches[-1]["iterations"] == 250
    # step_device without fused
    staged = optimizer_cem(**CEM)
    staged.configure()
    with pytest.raises(ValueError, match="fused=True"):
        staged.step_device(s, tp, te)


def test_capture_reserves_through_the_optimizer(fused_engine, monkeypatch):
    """ScheduleRun.capture() asks the OPTIMIZER for its workspace (reserve_fused), whichever fused optimizer it holds: rpgd ->
    cpmppi_rpgd_reserve, the CEM family -> cpmppi_cem_reserve with its refine kind; a staged CEM optimizer is refused."""
    from cartpolesimulation_amd import harness as HA
    from cartpolesimulation_amd import schedule as SC
    from cartpolesimulation_amd.optimizer_gradient import optimizer_rpgd
    E = 2
    cfg = dict(seed=31, length_of_experiment=0.1, random_initial_state=dict(init_limits=dict(angle=[0.0, 10.0], angleD=20.0, position=0.3, positionD=0.1)))
    b = SC.RandomExperimentSetter(cfg).draw(E, 83)
    monkeypatch.setattr(FusedFake, "mppi", property(lambda self: self.cfg), raising=False)

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached

    monkeypatch.setattr(torch.cuda, "Stream", stop)                          # the first thing capture() does after the reserve
    rp = optimizer_rpgd(fused=True, seed=2, mpc_horizon=8, num_rollouts=8, outer_its=2, num_envs=E)
    opts = [(rp, "rpgd")] + [(cls(fused=True, **CEM), ("cem", refine)) for cls, refine in _classes().values()]
    for opt, expected in opts:
        opt.configure()
        called = []
        monkeypatch.setattr(opt, "reserve_fused", lambda opt=opt, called=called: called.append(1) or type(opt).reserve_fused(opt))
        run = HA.ScheduleRun(opt.engine, b, 0, optimizer=opt)
        assert run.fused and run.counter is not None and run.Q is opt.controls
        with pytest.raises(Reached):
            run.capture(5)
        assert called == [1] and opt.engine.reserved == [expected]
    staged = _classes()["cem"][0](**CEM)
    staged.configure()
    with pytest.raises(ValueError, match="paced by the host"):
        HA.BatchedCartPoleExperiment(staged.engine, b.dt_simulation, b.dt_control, seed=0).run_schedule(b, graph=True, optimizer=staged)
