"""Closed-loop harness on the device: E simulated cartpoles, each driven by its own MPPI problem instance.

This is the build's counterpart of the reference's experiment loop (run_data_generator.py:9-10 ->
CartPole/data_generator.py:259-367 -> CartPole.run_cartpole_random_experiment, CartPole/__init__.py:659-735, whose
inner update_state loop is :283-324): every control period the controller sees the state and holds Q for
dt_control / dt_simulation plant steps.  Plant (cpmppi_plant_advance) and controller (cpmppi_step) both run on the
GPU and no value crosses PCIe inside the loop.  With ``predictor="GRU"`` the controller's plant model is the network of
``engine.set_gru`` and a third launch sits between the two: cpmppi_gru_advance moves each env's memory on with the state the controller
saw and the control it chose (update_internal_state, controller_mppi_cartpole.py:566-567).  The simulator's measurement chain (latency, measurement noise, vertical angle offset:
cartpole_physical_parameters.yml:18-28, all off as shipped), its additive control disturbance (:13-15, amplitude 0 as shipped) and its
parameter updaters / controller informer (:29-52) come as tables of the batch (schedule.apply_parameter_schedule).

`run` holds target position, target equilibrium and pole length constant per env; `run_schedule` runs a batch of the data
generator's random experiments (schedule.ExperimentBatch): the target position follows each experiment's random trace and the
target equilibrium flips on its dwell times, tabulated on the host and read by the device loop at its own step counter
(cpmppi_plant_step), with rows saved every dt_save whatever the control period.
"""
import os

import numpy as np
import torch

from .state_utilities import ANGLE_IDX, ANGLED_IDX, ANGLE_COS_IDX, ANGLE_SIN_IDX, POSITION_IDX, POSITIOND_IDX


def generate_random_initial_states(E, rng, track_half_length=0.198, init_limits=None):
    """CartPole/data_generator.py:221-256 with the limits of config_data_gen.yml:14-18, for E envs at once."""
    lim = dict(angle=(0.0, 180.0), angleD=1200.0, position=0.8, positionD=0.5)
    lim.update(init_limits or {})
    s = np.zeros((E, 6), dtype=np.float32)
    s[:, POSITION_IDX] = rng.uniform(-1.0, 1.0, E) * track_half_length * lim["position"]
    s[:, POSITIOND_IDX] = rng.uniform(-1.0, 1.0, E) * track_half_length * lim["positionD"]
    side = np.where(rng.uniform(size=E) > 0.5, 1.0, -1.0)
    angle = side * rng.uniform(lim["angle"][0], lim["angle"][1], E) * (np.pi / 180.0)
    s[:, ANGLE_IDX] = angle
    s[:, ANGLED_IDX] = rng.uniform(-1.0, 1.0, E) * lim["angleD"] * (np.pi / 180.0)
    s[:, ANGLE_COS_IDX], s[:, ANGLE_SIN_IDX] = np.cos(angle), np.sin(angle)
    return s


PREDICTORS = ("ODE_v0", "GRU")


def check_predictor(engine, predictor, h0=None, optimizer=None, knots_fn=None):
    """The controller's plant model in the device loop: "ODE_v0" (the engine's equations) or "GRU" (the network of set_gru, whose
    memory the loop hands from period to period).  ValueError for what the loop cannot run."""
    if predictor not in PREDICTORS:
        raise ValueError(f"predictor must be one of {PREDICTORS}, got {predictor!r}")
    if predictor != "GRU":
        if h0 is not None:
            raise ValueError("h0 is the memory of the GRU predictor: pass predictor='GRU'")
        return False
    if not getattr(engine, "has_gru", False):
        raise ValueError("predictor='GRU' needs a network: the engine has no model (engine.set_gru)")
    if optimizer is not None:
        raise ValueError("predictor='GRU' is the fused MPPI step over the network; an optimizer= object carries its own predictor "
                         "and memory (gru_model=): give one or the other")
    if knots_fn is not None:
        raise ValueError("predictor='GRU' draws its perturbations in the kernel (Philox): knots_fn is not supported with it")
    return True


def check_tuning(tuning, optimizer=None, predictor="ODE_v0", knots_fn=None):
    """``tuning=`` of run / run_schedule: the per-env rows (configs.tuning_rows) are read by the fused ODE MPPI step with its own
    Philox noise - ValueError, naming the conflict, for anything else that was asked for beside them."""
    if tuning is None:
        return
    if optimizer is not None:
        raise ValueError("tuning= and optimizer=: the tuning rows are read by the fused MPPI step, not by an optimizer object")
    if predictor == "GRU":
        raise ValueError("tuning= and predictor='GRU': the tuning rows are read by the ODE predictors' fused MPPI step")
    if knots_fn is not None:
        raise ValueError("tuning= and knots_fn: a row holds the sampler's sigma, so the step draws its own Philox noise")


def check_imitator(imitator, optimizer=None, predictor="ODE_v0", h0=None, knots_fn=None, tuning=None):
    """``imitator=`` of run_schedule: the neural imitator computes the controls in the MPC's place, so everything that configures the
    MPC is refused beside it by name.  -> the model dict ``MPPIEngine.set_dense`` takes (a folder is read with
    ``model_folder.load_dense_model``), or None."""
    if imitator is None:
        return None
    if optimizer is not None:
        raise ValueError("imitator= and optimizer=: the imitator is the controller; an optimizer object is another one")
    if predictor == "GRU":
        raise ValueError("imitator= and predictor='GRU': the imitator rolls nothing out and has no predictor")
    if h0 is not None:
        raise ValueError("imitator= and h0: the memory belongs to the GRU predictor; a Dense net has none")
    if knots_fn is not None:
        raise ValueError("imitator= and knots_fn: the imitator draws no perturbations")
    if tuning is not None:
        raise ValueError("imitator= and tuning=: the tuning rows are read by the fused MPPI step, not by the imitator")
    if isinstance(imitator, (str, os.PathLike)):
        from .model_folder import load_dense_model
        return load_dense_model(os.fspath(imitator))
    return imitator


ENGINE_MODEL = "engine-model"   # imitator= beside dagger=: the Dense model the engine holds as it stands (a training run goes on)


def check_dagger(dagger, batch, imitator, optimizer=None, predictor="ODE_v0", h0=None, knots_fn=None, tuning=None):
    """``dagger=dict(dataset=, beta=, seed=)`` of run_schedule: an expert of the device loop labels every state and the imitator -
    or the coin of ``beta`` - drives.  Refused by name: everything the loop is not built for.  -> (the model dict for
    ``MPPIEngine.set_dense`` or ENGINE_MODEL, the dataset, beta as float32 [E], the gate's seed)."""
    if imitator is None:
        raise ValueError("dagger= needs imitator=: the model that drives where the expert does not (a model dict, a model folder, or "
                         "harness.ENGINE_MODEL for the one the engine holds)")
    unknown = set(dagger) - {"dataset", "beta", "seed"}
    if unknown or "dataset" not in dagger or "beta" not in dagger:
        raise ValueError(f"dagger= takes dataset=, beta= and seed= (default 0), got {sorted(dagger)}")
    if predictor == "GRU":
        raise ValueError("dagger= and predictor='GRU': the GRU predictor as the expert is not built (its memory would have to follow "
                         "the applied control)")
    if h0 is not None:
        raise ValueError("dagger= and h0: the memory belongs to the GRU predictor, which is not built as the expert")
    if knots_fn is not None:
        raise ValueError("dagger= and knots_fn: the expert draws its own Philox noise on the device")
    if tuning is not None:
        raise ValueError("dagger= and tuning=: per-env tuning rows of the expert are not built")
    if optimizer is not None:
        if getattr(optimizer, "gru_model", None) is not None or getattr(optimizer, "h", None) is not None:
            raise ValueError("dagger= and an optimizer with gru_model=: a GRU-model optimizer as the expert is not built")
        if not getattr(optimizer, "fused", False):
            raise ValueError("dagger= and a host-paced optimizer=: the expert must stay on the device (the fused MPPI step, or rpgd / "
                             "gradient with fused=True)")
    dataset = dagger["dataset"]
    if not isinstance(dataset, DaggerDataset):
        raise ValueError("dagger=: dataset must be a harness.DaggerDataset")
    if dataset.T != batch.n_periods + 1:
        raise ValueError(f"dagger=: the dataset has {dataset.T} rows per recording, the batch makes {batch.n_periods + 1} controller "
                         f"calls (n_periods + 1)")
    beta = np.asarray(dagger["beta"], np.float32)
    if beta.shape not in ((), (batch.E,)):
        raise ValueError(f"dagger=: beta must be a scalar or [{batch.E}], got shape {beta.shape}")
    beta = np.ascontiguousarray(np.broadcast_to(beta, (batch.E,)))
    if isinstance(imitator, str) and imitator == ENGINE_MODEL:
        imitator = ENGINE_MODEL
    elif isinstance(imitator, (str, os.PathLike)):
        from .model_folder import load_dense_model
        imitator = load_dense_model(os.fspath(imitator))
    return imitator, dataset, beta, int(dagger.get("seed", 0))


def gru_memory(engine, E, h0):
    """The network's memory a run starts from: zeros [E,2,32], or a copy of ``h0`` (the run advances its own)."""
    return engine.zeros(E, 2, 32) if h0 is None else engine.tensor(h0, (E, 2, 32)).clone()


class BatchedCartPoleExperiment:
    def __init__(self, engine, dt_simulation=0.002, dt_control=0.02, seed=0):
        self.engine = engine
        self.dt_simulation = float(dt_simulation)
        self.n_sub = int(round(dt_control / dt_simulation))
        self.seed = int(seed)

    def run(self, s0, n_control_steps, target_position=0.0, target_equilibrium=1.0, L=None, record=True,
            env_offset=0, graph=False, steps_per_graph=10, predictor="ODE_v0", h0=None, tuning=None):
        """-> dict(states[T+1,E,6], Q[T,E]) as device tensors (only if ``record``), final state, final u_nom.
        ``tuning`` [E,16] (configs.tuning_rows): the controller's cost weights, LBD and sigma per env (MPPIEngine.set_tuning_rows),
        registered for this run - launched or captured - and taken off the handle afterwards; the result keeps the tensor.
        ``predictor="GRU"``: the controller rolls out with the engine's network from each env's memory ``h0`` [E,2,32] (None: zeros),
        which cpmppi_gru_advance moves on every period with (state seen, control chosen) - three launches per control period; the
        result gains ``memory`` [E,2,32], the memory after the last period.  ``L`` still goes to the plant; the network knows none."""
        eng = self.engine
        check_tuning(tuning, predictor=predictor)
        gru = check_predictor(eng, predictor, h0)
        s = eng.tensor(s0).clone()
        E = s.shape[0]
        if tuning is not None and tuple(np.shape(tuning))[:1] != (E,):
            raise ValueError(f"tuning must hold one row per env ({E}), got shape {tuple(np.shape(tuning))}")
        tp = eng.tensor(np.broadcast_to(np.asarray(target_position, dtype=np.float32), (E,)).copy())
        te = eng.tensor(np.broadcast_to(np.asarray(target_equilibrium, dtype=np.float32), (E,)).copy())
        Lt = None if L is None else eng.tensor(np.broadcast_to(np.asarray(L, dtype=np.float32), (E,)).copy())
        u_nom = eng.zeros(E, eng.H)
        Q = eng.empty(E)
        states = eng.empty(n_control_steps + 1, E, 6) if record else None
        Qs = eng.empty(n_control_steps, E) if record else None
        if record:
            states[0] = s
        h = gru_memory(eng, E, h0) if gru else None
        L_model = None if gru else Lt                          # (the network knows no pole length)
        # captured, the period is named by a counter in device memory (Philox step counter = control step index = recording row;
        # after the step: + 1), so that no launch argument changes between steps; launched, by the host's t
        counter = torch.zeros(1, dtype=torch.int64, device=s.device) if graph else None
        seed, n_sub, dt_sim = self.seed, self.n_sub, self.dt_simulation

        def period(t):                                         # (plain keywords: the host's time per period is the launched loop's pace)
            eng.step(s, u_nom, tp, te, L=L_model, seed=seed, offset=t if counter is None else 0, offset_dev=counter, env_offset=env_offset,
                     Q_out=Q, predictor=predictor, h0=h)
            if gru:
                eng.gru_advance(s, Q, h)                       # before the plant moves s: the state the controller saw
            # plant + this period's row of the recording in ONE launch (two kernels per control step in all)
            eng.plant_advance(s, Q, L=Lt, n_substeps=n_sub, dt_sim=dt_sim, states_log=states, Q_log=Qs,
                              row=t if counter is None else 0, row_dev=counter)

        loop = PeriodLoop(eng, n_control_steps)
        rows = None if tuning is None else eng.set_tuning_rows(tuning)
        try:
            if graph:                                          # the launch-bound case: few envs, ~70 us of GPU work per control step
                loop.capture(period, steps_per_graph, s.device)
            loop.enqueue_rest(period)
        finally:
            if rows is not None:                               # (a launch, and a captured one, keeps the pointer it was enqueued with)
                eng.set_tuning_rows(None)
        res = dict(states=states, Q=Qs, final_state=s, u_nom=u_nom)
        if rows is not None:
            res["tuning"] = rows
        if gru:
            res["memory"] = h
        return res

    # ------------------------------------------------------------------ the data generator's experiments (moving targets)
    def run_schedule(self, batch, env_offset=0, graph=False, steps_per_graph=10, knots_fn=None, u_nom0=None, optimizer=None,
                     predictor="ODE_v0", h0=None, tuning=None, imitator=None, dagger=None):
        """Run the E experiments of a schedule.ExperimentBatch to their end: CartPole.run_cartpole_random_experiment
        (CartPole/__init__.py:659-735) for all of them at once.  Per control period two launches - the fused MPPI step, reading
        the period's target position / equilibrium (/ pole length) from three [E] vectors, and cpmppi_plant_step, which advances
        the plants, records the rows that fall into the period and refills those vectors from the schedule tables for the next
        controller call.  The run ends, as the reference's does, with a controller call on the final state (its control completes
        the last row).  -> dict of device tensors: states [R,E,6], dd [R,E,2] (angleDD, positionDD), Q [periods + 1, E], final
        state and nominal sequences; rows are the simulation steps 0, n_save, 2 n_save, ...
        ``u_nom0`` [E,H]: nominal sequences to start from (a controller that has been stepped before; default zeros).
        ``knots_fn(c)`` (tests): perturbation knots [E,N,P] for controller call c instead of the in-kernel Philox draw.
        ``optimizer``: any of the package's optimizers configured for the batch's E envs (`controller_mpc(..., num_envs=E)
        .configure(...).optimizer`: cem, rpgd, gradient, ...) computes the controls instead of the fused MPPI step - host-paced, one
        `optimizer.step` per control period on device tensors, the plant / schedule / recording launch unchanged.  A FUSED rpgd /
        gradient / cem optimizer (`fused=True`: one cpmppi_rpgd_step / cpmppi_cem_step per period, its step counter on the device) is
        not paced by the host and may be captured (``graph=True``) like the MPPI step; so is cem over the network
        (`optimizer_cem(gru_model=..., gru_fused=True)`: cpmppi_cem_step_gru + cpmppi_gru_advance per period, the memory the
        optimizer's own), and rpgd and gradient over it (`optimizer_rpgd / optimizer_gradient(gru_model=..., gru_fused=True)`:
        cpmppi_rpgd_step_gru + cpmppi_gru_advance).  An optimizer object that runs the network reads no pole mass: a varying mass table paces no such run.
        ``predictor="GRU"``: the fused MPPI step over the engine's network (set_gru) - per control period three launches, the step
        from each experiment's memory ``h0`` [E,2,32] (None: zeros), cpmppi_gru_advance on (the MEASURED state the controller was
        given, the control it chose), the plant; launched or captured.  The result gains ``memory``, the memory after every
        controller call made (the final one included).  Not with ``optimizer=`` (such an object carries its own network and
        memory) and not with ``knots_fn``.
        ``tuning`` [E,16] (configs.tuning_rows): the controller's cost weights, LBD and sigma per experiment, registered with the
        engine for this run (launched or captured) and taken off it afterwards; the result keeps the tensor and, for
        MPPIEngine.score_runs, the loop's device table of target positions (``target_position_table``).  Not with
        ``optimizer=``, ``predictor="GRU"`` or ``knots_fn`` (ValueError).
        ``imitator``: the neural imitator of the MPC - a model dict (``MPPIEngine.set_dense``) or a model folder
        (``model_folder.load_dense_model``) - computes the controls instead: one cpmppi_dense_control per period on the state the
        controller is shown and the period's targets, then the plant; launched or captured; schedule tables, measurement chain,
        disturbance and ``score_runs`` apply unchanged.  Not with ``optimizer=``, ``predictor="GRU"``, ``gru_model=``, ``h0``,
        ``knots_fn`` or ``tuning=`` (ValueError by name).  The engine keeps the model.
        ``dagger=dict(dataset=, beta=, seed=)``, only together with ``imitator=`` (DaggerController): the MPC - the fused MPPI step,
        or a FUSED ``optimizer=`` - is the expert that labels every state the controller is shown, and per experiment and period it
        drives with probability ``beta`` (a scalar or [E]; the coin is Philox of ``seed``), the imitator otherwise; every call's
        sample lands in ``dataset`` (a DaggerDataset with n_periods + 1 rows per recording, E recordings reserved by this run).
        ``imitator=harness.ENGINE_MODEL``: the model the engine holds as it stands (a training run goes on).  The result gains
        ``Q_expert`` [E], the expert's last control, and ``recordings`` = (first, stop) of the dataset.  Not with
        ``predictor="GRU"``, ``h0``, an optimizer with ``gru_model=``, a host-paced optimizer, ``knots_fn`` or ``tuning=``."""
        if dagger is not None:
            dagger = check_dagger(dagger, batch, imitator, optimizer, predictor, h0, knots_fn, tuning)
            imitator = dagger[0]
        else:
            imitator = check_imitator(imitator, optimizer, predictor, h0, knots_fn, tuning)
        check_tuning(tuning, optimizer, predictor, knots_fn)
        if tuning is not None and tuple(np.shape(tuning))[:1] != (batch.E,):
            raise ValueError(f"tuning must hold one row per experiment ({batch.E}), got shape {tuple(np.shape(tuning))}")
        run = ScheduleRun(self.engine, batch, self.seed, env_offset=env_offset, knots_fn=knots_fn, u_nom0=u_nom0, optimizer=optimizer,
                          predictor=predictor, h0=h0, imitator=imitator, dagger=dagger)
        if batch.dt_simulation != self.dt_simulation or batch.n_ctrl != self.n_sub:
            raise ValueError("the batch was drawn for other time scales than this experiment runner's")
        if graph and run.controller.cannot_capture:
            raise ValueError(run.controller.cannot_capture)
        rows = None if tuning is None else self.engine.set_tuning_rows(tuning)
        try:
            if graph and knots_fn is None and run.T > 0:
                run.capture(steps_per_graph)
            run.loop.enqueue_rest(run._period)
            res = run.finish()
        finally:
            if rows is not None:                                # (a launch, and a captured one, keeps the pointer it was enqueued with)
                self.engine.set_tuning_rows(None)
        if rows is not None:
            res["tuning"] = rows
            res["target_position_table"] = run.buffers.plant["target_position_table"]     # (the loop's own table, for score_runs)
        return res


def controller_pole_mass(b, per_env=False):
    """What the simulator's 'm_pole' attribute holds at each of the T + 1 controller calls of a schedule.ExperimentBatch with an
    `m_pole:` updater table: the true mass at that call where the controller informer says told, the experiment's initial mass
    otherwise (CartPole/controller_informer.py).  -> (m_ctrl, m_ctrl_env), at most one of them not None:
      m_ctrl [T+1]        every experiment has the same mass schedule AND the same informer (the deterministic updater modes): one
                          value per call, the handle's scalar (cpmppi_set_pole_mass)
      m_ctrl_env [T+1,E]  ``per_env`` only: schedules or informers that differ between experiments (`mode: random`, `init_value:
                          random`, 'switching_random'), each experiment with its OWN informer column (cpmppi_set_pole_mass_rows)
    Without ``per_env`` such a batch yields (None, None): the controller keeps the handle's mass (with a warning where only the
    informer differs)."""
    mt = np.asarray(b.m_pole_table, np.float32)
    T, E = b.n_periods, mt.shape[1]
    calls = np.minimum(np.arange(T + 1) * b.n_ctrl, mt.shape[0] - 1)
    inf = b.informed_table(E)
    told = np.ones((T + 1, E), bool) if inf is None else inf[np.minimum(calls, len(inf) - 1)]
    shared = inf is None or bool((inf == inf[:, :1]).all())
    if (mt == mt[:, :1]).all() and (shared or not per_env):
        if not shared:
            import warnings
            warnings.warn("the informer differs between experiments ('switching_random'): the controller's one pole mass cannot follow "
                          "it and stays the handle's; the plants follow their own tables (MPPIConfig(per_env_pole_mass=True) follows it "
                          "per experiment)")
            return None, None
        return np.where(told[:, 0], mt[calls, 0], mt[0, 0]).astype(np.float32), None
    if not per_env:
        return None, None
    return None, np.ascontiguousarray(np.where(told, mt[calls], mt[0]), np.float32)


class ControllerMass:
    """The pole MASS the controller of a schedule run is told: predictor_ODE takes it from the simulator's 'm_pole' attribute at every
    call (predictors_customization.py:55-58; predictor_ODE_v0 does not), told or not as the informer says (controller_pole_mass).
    Decided on the host from the batch and the engine's MPPIConfig:
      kind    "none" (the handle's mass stands) | "value" (`values` [T+1]: one per controller call, the handle's scalar) |
              "rows" (`table` [T+1,E]: one row per call, a mass per experiment - MPPIConfig.per_env_pole_mass)
      varies  it changes between calls: the host paces such a run call by call (no captured graph, one cpmppi_groups_run per period)
    `bind` makes the device side, `apply(c)` goes before controller call c, `release` after the last one."""

    def __init__(self, batch, mppi, network=False):
        """``network``: the controller rolls out with the GRU, which reads no pole mass - kind "none" whatever the batch's table."""
        self.values = self.table = None
        if batch.m_pole_table is not None and mppi.predictor_type == "ODE" and not network:
            self.values, self.table = controller_pole_mass(batch, per_env=mppi.per_env_pole_mass)
        self.kind = "value" if self.values is not None else "rows" if self.table is not None else "none"
        per_call = self.values if self.values is not None else self.table
        self.varies = per_call is not None and bool((per_call != per_call[:1]).any())
        self.engines, self.slices, self.registered = [], [], False
        self.rows = self.rows_table = None                      # "rows", bound: the registered vector [E] and `table` on the device

    def bind(self, engines, slices=None, register=True):
        """The engines whose launches read the mass - one over all envs, or env groups with their ``slices`` [(first, stop)].
        "rows": the table stays on the device and every handle reads ITS slice of ONE registered [E] vector (``register`` False:
        the vector is only kept filled, for an optimizer object that registers it with its own engine)."""
        self.engines = list(engines)
        if self.kind != "rows":
            return
        self.slices = list(slices) if slices is not None else [(0, self.table.shape[1])]
        self.rows_table = self.engines[0].tensor(self.table)
        self.rows = self.rows_table[0].clone()
        self.registered = bool(register)
        if register:
            for eng, (e0, e1) in zip(self.engines, self.slices):
                eng.set_pole_mass_rows(self.rows[e0:e1])

    def apply(self, c):
        """Before controller call c: the mass the simulator would hand it.  The scalar goes to every handle (read when the launch
        is enqueued); of a mass per experiment every engine copies its slice of row c into the vector on the stream it launches
        on (rows that are constant in time: once)."""
        if self.kind == "value":
            for eng in self.engines:
                eng.set_pole_mass(float(self.values[c]))
        elif self.kind == "rows" and (c == 0 or self.varies):
            for eng, (e0, e1) in zip(self.engines, self.slices):
                with torch.cuda.stream(eng.launch_stream()):
                    self.rows[e0:e1].copy_(self.rows_table[c, e0:e1])

    def for_optimizer(self, c):
        """-> variable_parameters.m_pole at call c: the float, or the device row (an optimizer with per_env_pole_mass registers it)."""
        if self.kind == "value":
            return float(self.values[c])
        self.apply(c)
        return self.rows

    def release(self):
        """The handles are left as found (the launches enqueued keep the vector)."""
        if self.registered:
            for eng in self.engines:
                eng.set_pole_mass_rows(None)
            self.registered = False


class PeriodLoop:
    """`T` control periods of a device loop, enqueued by one host thread: the caller's ``period(c)`` launches period c; after
    `capture`, `steps_per_graph` periods at a time are replays of ONE HIP graph and only the rest is launched.  The body captured is
    ``period(None)``: it names its period by a counter in device memory, so that no launch argument changes between replays.
    (The body is handed in with every call, not kept: a loop that held a bound method of the run that holds the loop would be a
    reference cycle, and a captured graph must be freed when its run is dropped, not by the cycle collector during a later capture.)"""

    def __init__(self, engine, T):
        self.eng, self.T, self.c = engine, int(T), 0
        self.graph, self.per = None, 0

    def capture(self, period, steps_per_graph, device):
        """On a side stream that waits for what the launch stream holds; the launch stream then waits for the capture."""
        cap = torch.cuda.Stream(device=device)
        launch = self.eng.launch_stream()
        cap.wait_stream(launch)
        cap.wait_stream(torch.cuda.current_stream(device))
        self.graph = torch.cuda.CUDAGraph()
        self.per = max(1, min(int(steps_per_graph), self.T))
        fixed = self.eng.use_stream(cap)
        try:
            with torch.cuda.stream(cap):
                with torch.cuda.graph(self.graph, stream=cap):
                    for _ in range(self.per):
                        period(None)
        finally:
            self.eng.use_stream(fixed)
        launch.wait_stream(cap)

    def _replay(self):
        """One replay of the captured graph, if there is one and a whole one still fits.  -> whether"""
        if self.graph is None or self.T - self.c < self.per:
            return False
        with torch.cuda.stream(self.eng.launch_stream()):
            self.graph.replay()
        self.c += self.per
        return True

    def enqueue_next(self, period):
        """The next control period(s): one replay, else one period launched (a driver that interleaves several runs)."""
        if not self._replay():
            period(self.c)
            self.c += 1

    def enqueue_rest(self, period):
        """All that is left: the replays, then the remainder launched (nothing but the body between two periods)."""
        while self._replay():
            pass
        for c in range(self.c, self.T):
            period(c)
        self.c = self.T


class ScheduleBuffers:
    """What a schedule run derives from its batch alone: the states, the vectors the controller reads and the plant refills, the
    logs, the schedule tables on the device and the plant launch's keyword arguments (`plant`).  It holds no controller and binds no
    pole mass: ScheduleRun steps one, pipeline.run_schedule_groups hands one to the env groups."""

    def __init__(self, engine, batch, u_nom0=None):
        eng, b = engine, batch
        E, T = b.E, b.n_periods
        self.b, self.T = b, T
        R = b.n_sim // b.n_save + 1
        self.s = s = eng.tensor(b.s0).clone()
        tp_tab = eng.tensor(b.target_position.astype(np.float32))                 # the controller computes in float32
        te_tab = eng.tensor(b.target_equilibrium.astype(np.float32))
        L_tab = eng.tensor(b.L_table) if b.L_table is not None else None
        m_tab = eng.tensor(b.m_pole_table) if b.m_pole_table is not None else None
        for tab in (L_tab, m_tab):
            if tab is not None and (b.stride != 1 or tab.shape[0] != b.n_sim + 1):
                raise ValueError("a pole-length / pole-mass table is per simulation step: draw the batch with stride 1 (dt_save = dt_simulation)")
        Lc_tab, told = None, b.informed_table(E)
        if L_tab is not None and told is not None:                                  # what the controller is TOLD: the true length or the initial one
            Lc_tab = eng.tensor(np.where(told, np.asarray(b.L_table, np.float32), np.asarray(b.L_table, np.float32)[0]))
        self.cur_tp, self.cur_te = tp_tab[0].clone(), te_tab[0].clone()
        self.cur_L = (Lc_tab if Lc_tab is not None else L_tab)[0].clone() if L_tab is not None else (eng.tensor(b.L) if b.L is not None else None)
        self.u_nom = eng.zeros(E, eng.H) if u_nom0 is None else eng.tensor(u_nom0, (E, eng.H)).clone()
        self.Q = eng.empty(E)                                      # the controls: the controller writes them, the plant reads them
        self.states, self.dd, self.Qs = eng.zeros(R, E, 6), eng.zeros(R, E, 2), eng.zeros(T + 1, E)
        self.states[0] = s
        self.tail = b.n_sim - T * b.n_ctrl                                        # simulation steps after the last controller call
        self.plant = dict(dt_sim=b.dt_simulation, period_steps=b.n_ctrl, L=None if L_tab is not None else self.cur_L,
                          states_log=self.states, dd_log=self.dd, save_every=b.n_save, Q_log=self.Qs, target_position_table=tp_tab,
                          target_equilibrium_table=te_tab, L_table=L_tab, sched_stride=b.stride, target_position_out=self.cur_tp,
                          target_equilibrium_out=self.cur_te, L_out=self.cur_L if L_tab is not None else None, m_pole_table=m_tab,
                          L_controller_table=Lc_tab)
        if b.Q_disturbance is not None:                                           # the simulator's additive control disturbance
            qd = np.ascontiguousarray(b.Q_disturbance, np.float32)
            if qd.shape != (T + 1, E):
                raise ValueError(f"Q_disturbance is {qd.shape}, expected one row per controller call {(T + 1, E)}")
            self.plant.update(Q_disturbance_table=eng.tensor(qd), Q_bias=float(b.Q_bias))
        # the measurement chain (CartPole.add_noise_and_latency): the controller reads s_meas, which every plant step refills; the
        # t = 0 call sees the true state (:869-870)
        self.s_ctrl = self.s
        if b.latency or b.measurement_noise is not None or b.angle_offset is not None:
            self.s_ctrl = self.s.clone()
            self.plant.update(s_measured=self.s_ctrl, latency=float(b.latency))
            n_back = float(b.latency) / b.dt_simulation
            if n_back > 0:
                hist = np.zeros((int(n_back) + 2, E, 6), np.float32)
                hist[:, :, 2] = 1.0                                               # (CartPole/latency_adder.py:25-26)
                self.plant.update(state_history=eng.tensor(hist))
            if b.measurement_noise is not None:
                nz = np.ascontiguousarray(b.measurement_noise, np.float32)
                if nz.shape != (T + 1, E, 4):
                    raise ValueError(f"measurement_noise is {nz.shape}, expected one row per controller call {(T + 1, E, 4)}")
                self.plant.update(measurement_noise_table=eng.tensor(nz))
            if b.angle_offset is not None:
                if b.stride != 1 or b.angle_offset.shape[0] != b.n_sim + 1:
                    raise ValueError("the angle-offset table is per simulation step: draw the batch with stride 1")
                self.plant.update(angle_offset_table=torch.as_tensor(np.ascontiguousarray(b.angle_offset, np.float64), device=self.s.device))
                if told is not None:
                    self.plant.update(informed_table=torch.as_tensor(np.ascontiguousarray(told, np.uint8), device=self.s.device))
        # the control applied in the last period = the next call's Q_ccrc / "Q_applied_-1" (CartPole/__init__.py:489, 517-518), for the
        # cost plugins that read a previous input (0 before the first update, :838)
        from .optimizer_mppi import PREVIOUS_INPUT_COSTS
        self.previous_input = {}                                   # (a keyword of the controller call)
        if eng.mppi.cost_function_specification in PREVIOUS_INPUT_COSTS:
            self.previous_input = dict(previous_input=eng.zeros(E))
            self.plant.update(Q_applied_out=self.previous_input["previous_input"])

    def prepare_plant(self, engine):
        """-> the plant launch of one control period as a prepared call: `.run(period=c)`; `n_substeps=` for a run's last steps."""
        return engine.prepare_plant_step(self.s, self.Q, self.b.n_ctrl, period=0, **self.plant)

    def result(self):
        return dict(states=self.states, dd=self.dd, Q=self.Qs, final_state=self.s, u_nom=self.u_nom, batch=self.b)


# The controller of a schedule run, one class per kind.  ScheduleRun asks three things of it: `control(c)` enqueues controller call c
# (None under capture: the call is named by `counter`, the device's count of the calls made - None while the host counts),
# `before_capture()` does what must happen once before the loop is captured, and `cannot_capture` says why it cannot be (or None; a
# kind that never can has no `before_capture`).

class FusedMppiStep:
    """The fused MPPI step over the engine's equations or - ``memory`` [E,2,32], advanced in place - over its network.  The
    perturbations come from ``knots_fn(c)`` (tests), from Philox at the host's offset c, or at the device counter."""
    cannot_capture = None

    def __init__(self, engine, buffers, mass, seed, env_offset, knots_fn, memory):
        self.eng, self.buf, self.mass, self.knots_fn, self.memory = engine, buffers, mass, knots_fn, memory
        self.philox = dict(seed=int(seed), env_offset=int(env_offset))
        self.counter = self.step = None

    def _arguments(self):
        """(Read when a call is built: a test may still re-point the vectors of the buffers before the first period.)"""
        buf = self.buf
        model = dict(L=buf.cur_L) if self.memory is None else dict(predictor="GRU", h0=self.memory)
        return (buf.s_ctrl, buf.u_nom, buf.cur_tp, buf.cur_te), dict(Q_out=buf.Q, **model, **buf.previous_input)

    def control(self, c):
        if c is not None:
            self.mass.apply(c)
        if self.step is not None:
            self.step.run(offset=c)
        elif self.knots_fn is None and self.counter is None:
            # the launched loop: the argument block is built once (the Python-side argument handling of step + plant_step is
            # ~30 us per period - more than the GPU needs for a few dozen envs); per period mass.apply, this and the plant's
            args, kw = self._arguments()
            self.step = self.eng.prepare_step(*args, offset=0, **self.philox, **kw)
            self.step.run(offset=c)
        else:
            args, kw = self._arguments()
            noise = dict(knots=self.knots_fn(c)) if self.knots_fn is not None else dict(offset_dev=self.counter, **self.philox)
            self.eng.step(*args, **noise, **kw)
        if self.memory is not None:
            # before the plant launch refills s_ctrl: the memory moves on with what the controller saw and chose
            self.eng.gru_advance(self.buf.s_ctrl, self.buf.Q, self.memory)

    def before_capture(self):
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.buf.s.device)
        self.step = None                                           # (built for the host's offset)


class ImitatorController:
    """The neural imitator (Dense-7IN-32H1-32H2-1OUT, ``MPPIEngine.set_dense``) in the MPC's place: one cpmppi_dense_control per
    control period on the state the controller is shown and the period's targets -> the controls the plant reads.  It reads no pole
    mass, no pole length and no previous input.  Captured, the call carries a device counter, which it advances and the plant launch
    reads as its period."""
    cannot_capture = None

    def __init__(self, engine, buffers):
        self.eng, self.buf = engine, buffers
        self.counter = self.call = None

    def control(self, c):
        if self.call is None:                                      # (built once: the buffers persist; a test may re-point them before)
            buf = self.buf
            self.call = self.eng.prepare_dense_control(buf.s_ctrl, buf.cur_tp, buf.cur_te, Q_out=buf.Q, count_dev=self.counter)
        self.call.run()

    def before_capture(self):
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.buf.s.device)
        self.call = None                                           # (built without the counter)


class DaggerDataset:
    """The aggregated dataset of DAgger on the device, in the layout ``MPPIEngine.dense_train_step`` reads where it lies:
    ``states`` [R,T,6], ``target_position``, ``target_equilibrium``, ``labels`` [R,T] (the expert's controls), and beside them
    ``imitator`` [R,T] (the imitator's controls), ``gate`` [R,T] uint8 (1 where the expert drove) and ``sq_err`` [R] float64 (per
    recording the sum over its rows of (imitator - expert)^2).  ``filled``: the recordings written so far; a run of E experiments
    reserves the next E."""

    def __init__(self, engine, recordings, rows):
        R, T = int(recordings), int(rows)
        if R < 1 or T < 1:
            raise ValueError(f"DaggerDataset needs at least one recording and one row, got {R} x {T}")
        self.R, self.T, self.filled = R, T, 0
        self.states = engine.zeros(R, T, 6)
        self.target_position, self.target_equilibrium = engine.zeros(R, T), engine.zeros(R, T)
        self.labels, self.imitator = engine.zeros(R, T), engine.zeros(R, T)
        self.gate = torch.zeros(R, T, dtype=torch.uint8, device=self.states.device)
        self.sq_err = torch.zeros(R, dtype=torch.float64, device=self.states.device)

    tensors = property(lambda self: (self.states, self.target_position, self.target_equilibrium, self.labels))

    def reserve(self, E):
        """-> the first of the next ``E`` recordings, which are the caller's from now on."""
        E = int(E)
        if E < 1 or self.filled + E > self.R:
            raise ValueError(f"DaggerDataset is full: {self.filled} of its {self.R} recordings are written, {E} more do not fit")
        r0 = self.filled
        self.filled += E
        return r0


class ExpertBuffers:
    """The buffers of a schedule run as the expert of a DAgger run sees them: everything the run's own, but ``Q`` - a private buffer
    for the expert's controls, so that the run's ``Q`` is left to the applied ones."""

    def __init__(self, buffers):
        self._buffers = buffers
        self.Q = buffers.Q.clone()

    def __getattr__(self, name):                                   # (only what the instance itself does not hold)
        return getattr(self.__dict__["_buffers"], name)


class DaggerController:
    """DAgger in the device loop: the ``expert`` - a FusedMppiStep over the engine's equations or a FusedOptimizer, built on
    ExpertBuffers so that its controls go to a private ``Q_expert`` - computes its control of every period, then one
    cpmppi_dagger_step computes the imitator's, tosses the coin of ``beta`` [E], writes the applied control where the plant reads it
    (its ``Q_log`` and ``Q_applied_out`` therefore see the applied control) and the sample - the state shown, the targets, the
    expert's control as the label - into recordings ``r0 .. r0 + E - 1`` of the ``dataset``.
    The expert's plan stays warm-started from ITS OWN previous solution whoever drove, as ``control_along_trajectories(
    warm_start=True)`` does for rows it did not drive; a cost that reads the previous input is handed the applied one.
    Captured if the expert can be: the dagger step reads the period off the expert's device counter."""

    def __init__(self, engine, buffers, expert, expert_buffers, dataset, beta, seed, env_offset=0):
        self.eng, self.buf, self.expert, self.dataset = engine, buffers, expert, dataset
        E = buffers.s.shape[0]
        if buffers.Q is expert_buffers.Q:                          # (never: the expert writes a buffer of its own)
            raise ValueError("the expert must write its own controls buffer")
        self.Q_expert = expert_buffers.Q
        if isinstance(expert, FusedOptimizer):
            buffers.Q.copy_(self.Q_expert)                         # (what the first call reads as the control applied before it)
            expert.previous_input = buffers.Q
        self.beta = engine.tensor(np.ascontiguousarray(beta, np.float32))
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.r0 = dataset.reserve(E)
        self.call = None

    cannot_capture = property(lambda self: self.expert.cannot_capture)
    counter = property(lambda self: self.expert.counter)

    def control(self, c):
        self.expert.control(c)
        if self.call is None:                                      # (built once: the buffers persist)
            buf, d = self.buf, self.dataset
            self.call = self.eng.prepare_dagger_step(
                buf.s_ctrl, buf.cur_tp, buf.cur_te, self.Q_expert, self.beta, buf.Q, *d.tensors, r0=self.r0, seed=self.seed,
                env_offset=self.env_offset, period_dev=self.expert.counter, imitator_out=d.imitator, gate_out=d.gate,
                sq_err=d.sq_err[self.r0:self.r0 + buf.s.shape[0]])
        self.call.run(period=c)                                    # (None under capture: the device counter names it)

    def before_capture(self):
        self.expert.before_capture()
        self.call = None                                           # (built without the counter)


def _tell_optimizer(optimizer, buffers, mass, c):
    """What the simulator hands controller.step (CartPole/__init__.py:509-520), as attributes of the optimizer's variable_parameters
    (the pole mass of call c; None under capture: it stays).  -> them."""
    vp = optimizer.variable_parameters
    vp.target_position, vp.target_equilibrium = buffers.cur_tp, buffers.cur_te
    if buffers.cur_L is not None:
        vp.L = buffers.cur_L
    if mass.kind != "none" and c is not None:
        vp.m_pole = mass.for_optimizer(c)
    for prev_Q in buffers.previous_input.values():
        vp.Q_ccrc = prev_Q
        setattr(vp, "Q_applied_-1", prev_Q)
    return vp


class HostPacedOptimizer:
    """One of the package's optimizer objects: one `optimizer.step` per control period on device tensors, which returns the
    controls as a device tensor."""
    cannot_capture = "an optimizer object is paced by the host: run this batch launched (graph=False)"
    counter = None

    def __init__(self, optimizer, buffers, mass):
        self.opt, self.buf, self.mass = optimizer, buffers, mass

    def control(self, c):
        b = self.buf.b
        _tell_optimizer(self.opt, self.buf, self.mass, c)
        t = float(b.times[min(c * b.n_ctrl, len(b.times) - 1)])
        self.buf.Q.copy_(self.opt.step(self.buf.s_ctrl, t, as_tensor=True).reshape(-1))


class FusedOptimizer:
    """A fused optimizer object (rpgd, gradient, the cem family with `fused=True`): one library call per period, everything on the
    device.  It counts its control steps on the device, launched or captured: the same arithmetic either way - unless it warms up:
    the first step's extra iterations are told by the host, and such an optimizer keeps its host counters."""
    cannot_capture = None

    def __init__(self, optimizer, buffers, mass, previous_input=None):
        """``previous_input`` [E]: where the control applied in the period before stands, if not in the controls buffer itself (a
        loop along recordings: the recorded column)."""
        self.opt, self.buf, self.mass, self.previous_input = optimizer, buffers, mass, previous_input
        if optimizer.engine is None:
            optimizer.configure()
        buffers.Q = optimizer.controls                             # the fused step writes its controls where the plant reads them
        self.counter = None if optimizer.warmup else torch.zeros(1, dtype=torch.int64, device=buffers.s.device)
        if optimizer.warmup:
            self.cannot_capture = "warmup=True needs the host to tell the first step from the others: run this batch launched (graph=False)"

    def control(self, c):
        opt, buf = self.opt, self.buf
        vp = _tell_optimizer(opt, buf, self.mass, c)
        if c is not None:                                          # (captured: applied once before the capture)
            opt.engine.apply_pole_mass_of(vp, **opt._mass_rows)
        # the control of the period before is the one this buffer still holds
        previous = buf.Q if self.previous_input is None else self.previous_input
        opt.step_device(buf.s_ctrl, buf.cur_tp, buf.cur_te, L=buf.cur_L, previous_input=previous, count_dev=self.counter)

    def before_capture(self):
        """The optimizer's own handle: its mass, its workspace."""
        opt, vp = self.opt, self.opt.variable_parameters
        if self.mass.kind != "none":
            vp.m_pole = self.mass.for_optimizer(0)
        opt.engine.apply_pole_mass_of(vp, **opt._mass_rows)
        opt.reserve_fused()


def optimizer_controller(optimizer):
    """-> the controller kind that runs this optimizer object."""
    return FusedOptimizer if getattr(optimizer, "fused", False) else HostPacedOptimizer


class ScheduleRun:
    """The device loop of BatchedCartPoleExperiment.run_schedule as an object that enqueues one piece at a time, so that several
    runs can be interleaved by one host thread: the batch's `buffers`, the `controller` that computes the controls, the `mass` it is
    told, and the `loop` that launches or replays the periods."""

    def __init__(self, engine, batch, seed, env_offset=0, knots_fn=None, u_nom0=None, optimizer=None, predictor="ODE_v0", h0=None,
                 imitator=None, dagger=None):
        """``imitator``: the model dict of the neural imitator (``check_imitator`` has refused what cannot stand beside it); the engine
        takes it (``set_dense``) and it computes the controls.  ``dagger``: what ``check_dagger`` returns - the MPC is the expert of
        a DaggerController, and ``imitator`` may be ENGINE_MODEL (nothing is set)."""
        gru = check_predictor(engine, predictor, h0, optimizer, knots_fn)
        if optimizer is not None:
            if getattr(optimizer, "num_envs", batch.E) != batch.E:
                raise ValueError(f"the optimizer is configured for {optimizer.num_envs} envs, the batch has {batch.E}")
            if getattr(optimizer, "variable_parameters", None) is None:
                from types import SimpleNamespace
                optimizer.variable_parameters = SimpleNamespace()
        self.eng = engine
        self.buffers = buf = ScheduleBuffers(engine, batch, u_nom0)
        self.T, self.tail = buf.T, buf.tail
        # (an optimizer object that runs the network - gru_model=, its memory `h` once configured - reads no pole mass either)
        network = (gru or (imitator is not None and dagger is None) or getattr(optimizer, "h", None) is not None
                   or getattr(optimizer, "gru_model", None) is not None)
        self.mass = ControllerMass(batch, engine.mppi, network=network)
        self.mass.bind([engine], register=optimizer is None)       # (an optimizer object registers the row with its own engine)
        self.memory = gru_memory(engine, batch.E, h0) if gru else None
        mpc = buf if dagger is None else ExpertBuffers(buf)        # what the MPC writes its controls into
        if imitator is not None and imitator is not ENGINE_MODEL:
            engine.set_dense(imitator)
        if imitator is not None and dagger is None:
            self.controller = ImitatorController(engine, buf)
        elif optimizer is None:
            self.controller = FusedMppiStep(engine, mpc, self.mass, seed, env_offset, knots_fn, self.memory)
        else:
            self.controller = optimizer_controller(optimizer)(optimizer, mpc, self.mass)
        if dagger is not None:
            self.controller = DaggerController(engine, buf, self.controller, mpc, *dagger[1:], env_offset=env_offset)
        self.fused = isinstance(self.controller, FusedOptimizer)
        self.loop = PeriodLoop(engine, self.T)
        self._plant = None                                         # the plant launch at the host's period: built once

    Q = property(lambda self: self.buffers.Q)
    counter = property(lambda self: self.controller.counter)
    periods_left = property(lambda self: self.loop.c < self.T)

    def _plant_step(self, c, **last):
        """The plant launch of control period c, named by the host or by the device counter (``n_substeps=``: the run's last steps)."""
        counter = self.controller.counter
        if counter is not None:
            buf = self.buffers
            self.eng.plant_step(buf.s, buf.Q, last.get("n_substeps", buf.b.n_ctrl), period_dev=counter, **buf.plant)
            return
        if self._plant is None:
            self._plant = self.buffers.prepare_plant(self.eng)
        self._plant.run(period=c, **last)

    def _period(self, c):
        self.controller.control(c)
        self._plant_step(c)

    def capture(self, steps_per_graph=10):
        """Capture `steps_per_graph` control periods as ONE HIP graph (device step counter: Philox offset = schedule row =
        recording row, no launch argument changes between periods); enqueue_next then replays it."""
        why = self.controller.cannot_capture
        if why is None and self.mass.varies:
            why = ("a captured graph replays ONE pole mass for the controller: run this batch launched (graph=False)"
                   if self.mass.kind == "value" else
                   "a captured graph cannot step through the controller's per-experiment pole-mass table (the row would "
                   "have to be selected on the device): run this batch launched (graph=False)")
        if why is not None:
            raise ValueError(why)
        # the graph replays the handle's controller mass as it is when CAPTURED: the run's (constant) one, which may differ from
        # the mass the handle was created with (an uninformed controller; advisor, round 5)
        self.mass.apply(0)
        self.controller.before_capture()
        self.loop.capture(self._period, steps_per_graph, self.buffers.s.device)

    def enqueue_next(self):
        """The next control period(s) of the run: one period launched, or one replay of the captured graph."""
        self.loop.enqueue_next(self._period)

    def finish(self):
        """The run's last controller call (+ the trailing simulation steps of a length that is not a whole number of periods)."""
        assert not self.periods_left
        self.controller.control(self.T)
        self.mass.release()
        self._plant_step(self.T, n_substeps=self.tail)
        return self.result()

    def result(self):
        res = self.buffers.result()
        if self.memory is not None:
            res["memory"] = self.memory
        if isinstance(self.controller, DaggerController):
            res["Q_expert"] = self.controller.Q_expert
            res["recordings"] = (self.controller.r0, self.controller.r0 + self.buffers.s.shape[0])
        return res


# ---- control along recorded trajectories: the recorded row stands where the plant's stands -------------------------------------------
REPLAY_REFUSALS = {
    "gru": "control along recordings does not serve the GRU predictor: its memory along a recording needs the washout rows "
           "published per period (predictor must be an ODE one)",
    "host_paced": "control along recordings needs a controller that stays on the device: an optimizer object is paced by the host "
                  "(the fused MPPI step, or rpgd with fused=True)",
    "cold_optimizer": "warm_start=False is served by the fused MPPI step alone: an optimizer object keeps its plans, moments and "
                      "counters between rows",
}


class ReplayBuffers:
    """What a loop along recordings derives from the recordings alone: ``states`` [R,T,6] and the columns [R,T] on the device,
    their true lengths ``rows`` [R], and for the E = R*K envs (env r*K + k: the copies of a recording are contiguous) the vectors
    the controller reads and cpmppi_replay_step refills, the controls, the plans and the results - the mean [R,T] and standard
    deviation [R,T] over a recording's copies, NaN past its end, and with ``keep_evals`` every control [T,E].  It has the
    attributes the controller kinds read off ScheduleBuffers (s, s_ctrl, cur_tp, cur_te, cur_L, Q, u_nom, previous_input).
    ``previous`` [R,T]: the recorded control applied before each row; a cost that reads a previous input needs it."""

    def __init__(self, engine, states, rows, K, target_position, target_equilibrium, L=None, previous=None, keep_evals=False):
        eng = engine
        self.states = eng.tensor(states)
        if self.states.dim() != 3 or self.states.shape[2] != 6:
            raise ValueError(f"states must be [R,T,6], got {tuple(self.states.shape)}")
        R, T = self.states.shape[0], self.states.shape[1]
        self.R, self.T, self.K, self.E = R, T, int(K), R * int(K)
        self.rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), np.uint32)
        if self.rows.shape != (R,) or self.rows.min() < 1 or self.rows.max() > T:
            raise ValueError(f"rows must hold a length in 1..{T} for each of the {R} recordings")
        self.rows_dev = torch.as_tensor(self.rows.astype(np.int32)).to(self.states.device)
        E, nan = self.E, float("nan")
        self.columns = dict(target_position=eng.tensor(target_position, (R, T)), target_equilibrium=eng.tensor(target_equilibrium, (R, T)),
                            L=eng.tensor(L, (R, T)), previous_input=eng.tensor(previous, (R, T)))
        self.s = self.s_ctrl = eng.zeros(E, 6)
        self.cur_tp, self.cur_te = eng.zeros(E), eng.zeros(E)
        self.cur_L = eng.zeros(E) if L is not None else None
        self.previous = eng.zeros(E)                               # (without a recorded column: 0, as before a run's first update)
        self.u_nom, self.Q = eng.zeros(E, eng.H), eng.zeros(E)
        self.Q_mean, self.Q_std = eng.empty(R, T).fill_(nan), eng.empty(R, T).fill_(nan)
        self.Q_all = eng.empty(T, E).fill_(nan) if keep_evals else None
        from .optimizer_mppi import PREVIOUS_INPUT_COSTS
        self.previous_input = {}                                   # (a keyword of the controller call)
        if eng.mppi.cost_function_specification in PREVIOUS_INPUT_COSTS:
            if previous is None:
                raise ValueError(f"the cost {eng.mppi.cost_function_specification!r} reads the control applied before each row: the "
                                 "recordings must carry it (Q_ccrc / Q_applied_-1)")
            self.previous_input = dict(previous_input=self.previous)

    def replay_arguments(self, warm_start=True):
        """-> (positional, keyword) arguments of engine.replay_step for these buffers (read when a call is built: a fused optimizer
        has put its own controls buffer in by then)."""
        c = self.columns
        kw = dict(rows_dev=self.rows_dev, target_position=c["target_position"], target_equilibrium=c["target_equilibrium"], L=c["L"],
                  previous_input=c["previous_input"], Q_mean_out=self.Q_mean, Q_std_out=self.Q_std, Q_all_out=self.Q_all,
                  s_out=self.s, target_position_out=self.cur_tp, target_equilibrium_out=self.cur_te, L_out=self.cur_L,
                  previous_input_out=self.previous if c["previous_input"] is not None else None,
                  u_nom_reset=None if warm_start else self.u_nom)
        return (self.states, self.rows, self.Q, self.K), kw

    def result(self):
        R, T, K = self.R, self.T, self.K
        res = dict(Q=self.Q_mean, Q_std=self.Q_std, rows=self.rows, u_nom=self.u_nom)
        if self.Q_all is not None:
            res["Q_evals"] = self.Q_all.reshape(T, R, K)
        return res


class ReplayRun:
    """The device loop along recordings: prime (row 0 goes to the controller), then per period the controller call and ONE
    cpmppi_replay_step, which collects the row's controls and publishes the next row - launched, or `steps_per_graph` periods at a
    time as replays of one HIP graph.  The controller kinds and PeriodLoop are ScheduleRun's; the semantics are this package's own
    (include/cpmppi.h, cpmppi_replay_args): every copy of a recording is an independent controller instance, its env index feeds
    Philox, the Philox offset of row c is c, and the plan is carried from row to row unless ``warm_start`` is False."""

    def __init__(self, engine, buffers, seed, env_offset=0, optimizer=None, warm_start=True, predictor="ODE_v0"):
        if predictor == "GRU":
            raise ValueError(REPLAY_REFUSALS["gru"])
        check_predictor(engine, predictor, None, optimizer, None)
        if optimizer is not None:
            if getattr(optimizer, "h", None) is not None or getattr(optimizer, "gru_model", None) is not None:
                raise ValueError(REPLAY_REFUSALS["gru"])
            if not getattr(optimizer, "fused", False):
                raise ValueError(REPLAY_REFUSALS["host_paced"])
            if not warm_start:
                raise ValueError(REPLAY_REFUSALS["cold_optimizer"])
            if getattr(optimizer, "num_envs", buffers.E) != buffers.E:
                raise ValueError(f"the optimizer is configured for {optimizer.num_envs} envs, the recordings x evaluations are {buffers.E}")
            if getattr(optimizer, "variable_parameters", None) is None:
                from types import SimpleNamespace
                optimizer.variable_parameters = SimpleNamespace()
        from types import SimpleNamespace
        self.eng, self.buffers, self.warm_start = engine, buffers, bool(warm_start)
        self.T = buffers.T
        self.mass = ControllerMass(SimpleNamespace(m_pole_table=None), engine.mppi)      # (a recording tells no controller-side mass)
        if optimizer is None:
            self.controller = FusedMppiStep(engine, buffers, self.mass, seed, env_offset, None, None)
        else:
            self.controller = FusedOptimizer(optimizer, buffers, self.mass, previous_input=buffers.previous)
        self.loop = PeriodLoop(engine, self.T)
        self._by_host = self._by_counter = None                    # the replay launch, named either way: built once each
        self.primed = False

    periods_left = property(lambda self: self.loop.c < self.T)

    def _prepare(self, **named):
        args, kw = self.buffers.replay_arguments(self.warm_start)
        return self.eng.prepare_replay_step(*args, **named, **kw)

    def prime(self):
        """Row 0 of every recording to the vectors the controller reads: once, before controller call 0."""
        if self._by_host is None:
            self._by_host = self._prepare(period=0)
        self._by_host.run(period=0, prime=1)
        self.primed = True

    def _replay_step(self, c):
        counter = self.controller.counter
        if counter is not None:
            if self._by_counter is None:
                self._by_counter = self._prepare(period_dev=counter)
            self._by_counter.run()
            return
        if self._by_host is None:
            self._by_host = self._prepare(period=0)
        self._by_host.run(period=c, prime=0)

    def _period(self, c):
        self.controller.control(c)
        self._replay_step(c)

    def capture(self, steps_per_graph=10):
        why = self.controller.cannot_capture
        if why is not None:
            raise ValueError(why)
        self.mass.apply(0)
        self.controller.before_capture()
        self.loop.capture(self._period, steps_per_graph, self.buffers.s.device)

    def run(self, graph=False, steps_per_graph=10):
        """All of it -> `result()`."""
        if graph and self.controller.cannot_capture:
            raise ValueError(self.controller.cannot_capture)
        if not self.primed:
            self.prime()
        if graph and self.T > 0:
            self.capture(steps_per_graph)
        self.loop.enqueue_rest(self._period)
        return self.result()

    def result(self):
        return self.buffers.result()
