"""CPU: the sampling optimizers over the GRU predictor - the host side.  cem, cem-gmm and random-action configured with a model
hand every cost launch of a control step to the GRU path (``rollout_cost(..., predictor="GRU", h0=h)``) with the env's current
memory, advance that memory once per control step from the control they applied, and zero it on reset; the gradient family and
``fused=True`` refuse the network by name; specification and model select the predictor under optimizer_mppi's rules; and
controller_mpc hands a ``gru_model`` of its config to the optimizer, over a checkout's ``predictor_specification: "ODE"`` default.

The device engine is replaced by GruFake (the checker-backed stand-in of test_optimizers_host_logic.py plus the GRU calls, both
from oracle_np): nothing here needs a device; the real kernels are covered by tests/test_gpu_gru_cost_only.py."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402
from test_optimizers_host_logic import CHECKOUT, FakeEngine, _states  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_c5.npz")
SPEC = "GRU-6IN-32H1-32H2-5OUT-0"


def golden_model():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files if k not in ("s0", "Q", "h0", "traj", "h_final")}


class GruFake(FakeEngine):
    """FakeEngine plus the two GRU calls of the engine, from the oracle; every cost launch is recorded with what it was handed."""

    def __init__(self, E, cfg, phys=None, device=0):
        super().__init__(E, cfg, phys, device)
        self.cost_launches, self.predict_launches, self.gru = [], [], None

    def apply_pole_mass_of(self, variable_parameters, **kw):
        pass

    def cem_gmm_sample(self, centres, stdev, seed, offset=0, env_offset=0):
        g = torch.Generator().manual_seed(int(seed) * 1000003 + int(offset))
        comp = torch.randint(centres.shape[1], (self.E, self.N), generator=g)
        mean = torch.gather(centres, 1, comp[:, :, None].expand(-1, -1, self.H))
        return (mean + stdev[:, None, :] * torch.randn(self.E, self.N, self.H, generator=g)).clamp(self.lo, self.hi).contiguous()

    def rollout_cost(self, s0, inputs, tp, te, L=None, predictor="ODE_v0", h0=None):
        self.cost_launches.append(dict(predictor=predictor, L=L, h0=None if h0 is None else h0.clone(), inputs=inputs.clone()))
        if predictor != "GRU":
            return super().rollout_cost(s0, inputs, tp, te, L=L)
        assert self.gru is not None and L is None and tuple(h0.shape) == (self.E, 2, 32)
        cfg = O.MPPIConfig(N=self.N, H=self.H, cost_id=O.COST_QBGM, cc_weight=0.0, shift_mode="none")
        s0, Q, h = np.asarray(s0, f32), inputs.numpy(), h0.numpy()
        S = [O.gru_mppi_step(self.gru, s0[e], np.zeros(self.H, f32), Q[e], f32(np.asarray(tp).reshape(-1)[e]),
                             f32(np.asarray(te).reshape(-1)[e]), cfg, h0=h[e], low=self.lo, high=self.hi)["S"] for e in range(self.E)]
        return torch.as_tensor(np.stack(S), dtype=torch.float32)

    def gru_predict(self, s0, Q, h0=None, return_hidden=False):
        assert tuple(h0.shape) == (2, self.E, 32) and tuple(Q.shape) == (self.E, 1) and return_hidden
        self.predict_launches.append(dict(s0=np.asarray(s0, f32).copy(), Q=Q.clone(), h0=h0.clone()))
        traj, h = O.gru_predict(self.gru, np.asarray(s0, f32), Q.numpy(), h0.numpy())
        return torch.as_tensor(traj, dtype=torch.float32), torch.as_tensor(h, dtype=torch.float32)


@pytest.fixture()
def gru_engine(monkeypatch):
    import cartpolesimulation_amd.engine as EN
    monkeypatch.setattr(EN, "MPPIEngine", GruFake)
    return GruFake


def _sampling_classes():
    from cartpolesimulation_amd import optimizer_cem as OC
    return {"cem": OC.optimizer_cem, "cem-gmm": OC.optimizer_cem_gmm, "random-action": OC.optimizer_random_action}


def _gradient_classes():
    from cartpolesimulation_amd import optimizer_cem as OC
    from cartpolesimulation_amd import optimizer_gradient as OG
    return {"cem-naive-grad": OC.optimizer_cem_naive_grad, "cem-grad-bharadhwaj": OC.optimizer_cem_grad_bharadhwaj,
            "gradient": OG.optimizer_gradient, "rpgd": OG.optimizer_rpgd}


KW = dict(seed=5, mpc_horizon=6, num_rollouts=12, cem_outer_it=3, cem_best_k=4, num_envs=2)


def _kw(name):
    """random-action has no distribution to refit: it takes no cem_* keyword."""
    return {k: v for k, v in KW.items() if not (name == "random-action" and k.startswith("cem_"))}


@pytest.mark.parametrize("name", ["cem", "cem-gmm", "random-action"])
@pytest.mark.parametrize("how", ["model alone", "model and specification"])
def test_every_cost_launch_takes_the_gru_path_and_the_memory_moves_once_per_step(gru_engine, name, how):
    E = KW["num_envs"]
    model = golden_model()
    opt = _sampling_classes()[name](gru_model=model, **_kw(name))
    opt.configure(predictor_specification=SPEC if how == "model and specification" else None)
    eng = opt.engine
    assert eng.gru is model and opt.cfg.predictor_type == "ODE_v0"       # (the constructor's integrator is left alone)
    assert tuple(opt.h.shape) == (E, 2, 32) and not opt.h.any()
    iters = 1 if name == "random-action" else KW["cem_outer_it"]
    s = _states(E)
    h_ref = np.zeros((E, 2, 32), f32)
    for step in range(3):
        before = opt.h.clone()
        u = opt.step(s)
        assert u.shape == (E, 1)
        launches, eng.cost_launches = eng.cost_launches, []
        # every outer iteration: one launch, the GRU path, no pole length, the memory the step began with
        assert len(launches) == iters
        for launch in launches:
            assert launch["predictor"] == "GRU" and launch["L"] is None
            assert torch.equal(launch["h0"], before)
        if iters > 1:
            assert not torch.equal(launches[0]["inputs"], launches[-1]["inputs"])
        # once per control step: from the state seen and the control applied, [E,2,32] -> [2,E,32] and back
        assert len(eng.predict_launches) == step + 1
        p = eng.predict_launches[-1]
        assert np.array_equal(p["s0"], s) and np.array_equal(p["Q"].numpy()[:, 0], u[:, 0])
        assert torch.equal(p["h0"], before.transpose(0, 1))
        want = O.gru_predict(model, s, u.astype(f32), np.ascontiguousarray(h_ref.transpose(1, 0, 2)))[1].transpose(1, 0, 2)
        assert np.array_equal(opt.h.numpy(), want) and opt.h.is_contiguous()
        assert np.abs(want - h_ref).max() > 1e-4                         # (it moved)
        h_ref = want
        s = np.stack([O.ode_v0_step(s[e][None], u[e].astype(f32))[0] for e in range(E)])
    assert np.abs(h_ref[0] - h_ref[1]).max() > 1e-4                      # (envs that agreed would hide a transpose slip)
    opt.optimizer_reset()
    assert tuple(opt.h.shape) == (E, 2, 32) and not opt.h.any()
    opt.step(s)
    assert not eng.cost_launches[0]["h0"].any()


@pytest.mark.parametrize("name", ["cem", "cem-gmm", "random-action"])
def test_without_a_model_the_ode_path_is_what_it_was(gru_engine, name):
    opt = _sampling_classes()[name](**_kw(name))
    opt.configure(predictor_specification="ODE")
    assert opt.h is None and opt.engine.gru is None and opt.cfg.predictor_type == "ODE"
    opt.step(_states(KW["num_envs"]))
    assert opt.h is None and not opt.engine.predict_launches
    assert all(l["predictor"] == "ODE_v0" and l["h0"] is None and l["L"] is not None for l in opt.engine.cost_launches)


@pytest.mark.parametrize("name", ["cem", "cem-gmm", "random-action"])
def test_specification_and_model_rules(gru_engine, name, tmp_path):
    cls, KW = _sampling_classes()[name], _kw(name)
    # a specification without a model
    opt = cls(**KW)
    with pytest.raises(ValueError, match="needs gru_model"):
        opt.configure(predictor_specification=SPEC)
    assert opt.engine is None
    # a model beside an ODE specification
    for spec in ("ODE", "ODE_v0", "ODE_v0_default"):
        opt = cls(gru_model=golden_model(), **KW)
        with pytest.raises(ValueError, match="the model would be ignored"):
            opt.configure(predictor_specification=spec)
        assert opt.engine is None
    # an unknown specification stays what it was, with a model or without
    with pytest.raises(NotImplementedError, match="sampling optimizers"):
        cls(gru_model=golden_model(), **KW).configure(predictor_specification="SGP_10")
    # a model alone selects the network; so does a model folder's path
    opt = cls(gru_model=golden_model(), **KW)
    opt.configure()
    assert opt.h is not None and opt.engine.gru is opt.gru_model
    with pytest.raises(Exception) as ei:                                  # a folder that holds no model: the loader's own error
        cls(gru_model=str(tmp_path), **KW).configure()
    assert not isinstance(ei.value, (TypeError, AttributeError)), ei.value


@pytest.mark.parametrize("name", ["cem-naive-grad", "cem-grad-bharadhwaj", "gradient", "rpgd"])
def test_the_gradient_family_refuses_the_gru_by_name(gru_engine, name):
    cls = _gradient_classes()[name]
    kw = dict(seed=1, mpc_horizon=6, num_rollouts=8, num_envs=2)

    def check(ei):
        msg = str(ei.value)
        assert "no adjoint kernel" in msg and "GRU" in msg
        for runs_on_it in ("cem", "cem-gmm", "random-action"):
            assert runs_on_it in msg

    with pytest.raises(NotImplementedError) as ei:                        # the model is not swallowed by **kwargs
        cls(gru_model=golden_model(), **kw)
    check(ei)
    opt = cls(**kw)
    with pytest.raises(NotImplementedError) as ei:                        # nor does the specification fall to the ODE's sentence
        opt.configure(predictor_specification=SPEC)
    check(ei)
    assert opt.engine is None
    opt.configure(predictor_specification="ODE")                          # the ODE path is what it was
    assert opt.engine is not None and opt.h is None


@pytest.mark.parametrize("name", ["cem"])
def test_fused_refuses_the_gru(gru_engine, name):
    cls = _sampling_classes()[name]
    with pytest.raises(ValueError, match="fused=True integrates the ODE") as ei:
        cls(gru_model=golden_model(), fused=True, **KW)
    assert "cpmppi_cem_step" in str(ei.value)
    opt = cls(fused=True, **KW)
    with pytest.raises(ValueError, match="fused=True integrates the ODE"):
        opt.configure(predictor_specification=SPEC)
    assert opt.engine is None


@pytest.mark.parametrize("config_root", [None, CHECKOUT])
@pytest.mark.parametrize("name", ["cem", "cem-gmm", "random-action"])
def test_controller_hands_the_model_to_the_optimizer(gru_engine, name, config_root):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    model = golden_model()
    ctrl = controller_mpc(config=dict(gru_model=model, num_rollouts=12, mpc_horizon=6, seed=3), config_root=config_root)
    if config_root is not None:                                           # the checkout's default names the ODE predictor
        assert ctrl.config_optimizer.get("predictor_type") == "ODE"
    ctrl.configure(name)
    opt = ctrl.optimizer
    assert type(opt) is _sampling_classes()[name]
    assert opt.gru_model is model and opt.engine.gru is model and opt.h is not None
    assert opt.cfg.predictor_type == "ODE_v0" and ctrl.predictor is None
    u = ctrl.step(_states(1)[0])
    assert np.shape(u) == (1,)
    assert opt.engine.cost_launches and all(l["predictor"] == "GRU" for l in opt.engine.cost_launches)
    # an ODE specification beside the model is an error, wherever the specification comes from
    with pytest.raises(ValueError, match="gru_model was given"):
        ctrl.configure(name, predictor_specification="ODE")
    with pytest.raises(ValueError, match="gru_model was given"):
        controller_mpc(config=dict(gru_model=model, predictor_specification="ODE_v0", num_rollouts=12, mpc_horizon=6),
                       config_root=config_root).configure(name)
    # and the explicit GRU specification is the same controller
    ctrl.configure(name, predictor_specification=SPEC)
    assert ctrl.optimizer.h is not None and ctrl.predictor is None


@pytest.mark.parametrize("name", ["gradient", "rpgd", "cem-naive-grad", "cem-grad-bharadhwaj"])
def test_controller_does_not_swallow_the_model_for_the_gradient_family(gru_engine, name):
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    ctrl = controller_mpc(config=dict(gru_model=golden_model(), num_rollouts=8, mpc_horizon=6, seed=3))
    with pytest.raises(NotImplementedError, match="no adjoint kernel"):
        ctrl.configure(name)


def test_mppi_shares_the_hand_over(gru_engine):
    """optimizer_mppi's selection rules and memory now come from _OptimizerBase: one definition for the four optimizers."""
    from cartpolesimulation_amd._optimizer_base import _OptimizerBase
    from cartpolesimulation_amd.optimizer_mppi import optimizer_mppi
    for cls in (optimizer_mppi, *_sampling_classes().values()):
        assert cls._advance_memory is _OptimizerBase._advance_memory
        assert cls._attach_gru is _OptimizerBase._attach_gru
    assert optimizer_mppi._gru_selected is _OptimizerBase._gru_selected
    with pytest.raises(ValueError, match="needs gru_model"):
        optimizer_mppi(num_rollouts=8, mpc_horizon=4, seed=7).configure(predictor_specification=SPEC)
    with pytest.raises(ValueError, match="the model would be ignored"):
        optimizer_mppi(num_rollouts=8, mpc_horizon=4, seed=7, gru_model=golden_model()).configure(predictor_specification="ODE")
