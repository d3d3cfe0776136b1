"""GPU: a direct call of step / plant_step / rpgd_step / cem_step and the same call prepared once and run are one computation.
Each entry point is called directly, and separately built with prepare_* and run on fresh copies of the same inputs, twice:
the second pass with the counters of the next control step - given to the direct call as arguments, to the prepared one through
``run`` - which pins that ``run`` reaches the block.  Every output and every tensor updated in place is expected bit for bit:
both forms fill one argument block for one kernel.

Shapes: E = 3 envs, N = 33 rollouts (a ragged wave), H = 5 (shorter than a quad of control steps), two knots; rpgd and cem with
2 iterations, keep_k = 17 and best_k = 7 - the smallest at which the per-env indexing and the surplus lanes are live."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O  # noqa: E402

f32 = np.float32
E, N, H, SEED = 3, 33, 5, 2 ** 33 + 5
QBG_W = dict(ccrc_weight_up=3.0, ccrc_weight_down=3.0, dd_linear_weight_up=2.0, dd_linear_weight_down=2.0)


@pytest.fixture(scope="module")
def eng():
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    e = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=H,
                                 cost_function_specification="quadratic_boundary_grad", cost_weights=QBG_W))
    assert e.P == 2
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """Host arrays only: each form uploads copies of its own."""
    rng = np.random.Generator(np.random.SFC64(77))
    s0 = np.stack([O.create_cartpole_state(rng.uniform(-0.6, 0.6), rng.uniform(-1.5, 1.5), rng.uniform(-0.04, 0.04),
                                           rng.uniform(-0.1, 0.1)) for _ in range(E)]).astype(f32)
    return dict(s0=s0, tp=rng.uniform(-0.03, 0.03, E).astype(f32), te=np.ones(E, f32), L=rng.uniform(0.3, 0.45, E).astype(f32),
                prev=rng.uniform(-0.3, 0.3, E).astype(f32), u_nom=rng.uniform(-0.3, 0.3, (E, H)).astype(f32),
                plans=(0.3 * rng.standard_normal((E, N, H))).astype(f32), mean=rng.uniform(-0.3, 0.3, (E, H)).astype(f32),
                stdev=rng.uniform(0.2, 0.6, (E, H)).astype(f32), Q=rng.uniform(-1, 1, (3, E)).astype(f32),
                tp_table=rng.uniform(-0.15, 0.15, (21, E)).astype(f32))


def same(direct, prepared):
    assert direct.keys() == prepared.keys()
    for name in direct:
        assert torch.equal(direct[name], prepared[name]), name


def per_env(eng, x):
    return {k: eng.tensor(x[k].copy()) for k in ("s0", "tp", "te", "L", "prev")}


def test_step(eng, inputs):
    def buffers():
        d = per_env(eng, inputs)
        d.update(u_nom=eng.tensor(inputs["u_nom"].copy()), Q_out=eng.zeros(E), S_out=eng.zeros(E, N))
        return d

    def arguments(d):
        return (d["s0"], d["u_nom"], d["tp"], d["te"]), dict(L=d["L"], previous_input=d["prev"], seed=SEED, env_offset=4,
                                                             Q_out=d["Q_out"], S_out=d["S_out"])

    direct, prepared = buffers(), buffers()
    args, kw = arguments(direct)
    got = [tuple(t.clone() for t in eng.step(*args, offset=offset, **kw)) for offset in (0, 1)]
    args, kw = arguments(prepared)
    call = eng.prepare_step(*args, offset=0, **kw)
    assert call.Q_out is prepared["Q_out"] and call.S_out is prepared["S_out"]
    first = tuple(t.clone() for t in call.run())
    second = call.run(offset=1)
    torch.cuda.synchronize()
    assert second[0] is prepared["Q_out"] and second[1] is prepared["S_out"]
    for a, b in zip(got, (first, second)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(got[0][1], got[1][1])                          # the second pass drew other noise: the counter counted
    same(direct, prepared)


def test_plant_step(eng, inputs):
    n_ctrl, n_save = 10, 5

    def buffers():
        d = dict(s=eng.tensor(inputs["s0"].copy()), states_log=eng.zeros(2 * n_ctrl // n_save + 1, E, 6), Q_log=eng.zeros(3, E),
                 target_position_table=eng.tensor(inputs["tp_table"].copy()), target_position_out=eng.zeros(E),
                 Q_applied_out=eng.zeros(E), L=eng.tensor(inputs["L"].copy()))
        d["states_log"][0] = d["s"]
        return d

    def keywords(d):
        return dict(period_steps=n_ctrl, save_every=n_save, **{k: v for k, v in d.items() if k != "s"})

    Q = [eng.tensor(q.copy()) for q in inputs["Q"]]
    direct, prepared = buffers(), buffers()
    for period in (0, 1):
        assert eng.plant_step(direct["s"], Q[period], n_ctrl, period=period, **keywords(direct)) is direct["s"]
    mid = direct["s"].clone()
    eng.plant_step(direct["s"], Q[2], 0, period=2, **keywords(direct))   # the last controller call: record only
    # one block for the whole run: the control is read from the buffer the block points to
    held = Q[0].clone()
    call = eng.prepare_plant_step(prepared["s"], held, n_ctrl, period=0, **keywords(prepared))
    assert call.run() is prepared["s"]
    held.copy_(Q[1])
    call.run(period=1)
    held.copy_(Q[2])
    call.run(period=2, n_substeps=0)
    torch.cuda.synchronize()
    same(direct, prepared)
    assert torch.equal(direct["s"], mid) and torch.equal(direct["Q_log"], eng.tensor(inputs["Q"]))
    assert torch.equal(direct["states_log"][-1], direct["s"]) and not torch.equal(direct["states_log"][2], direct["states_log"][-1])


def test_rpgd_step(eng, inputs):
    hp = dict(iterations=2, learning_rate=0.05, epsilon=1e-2, gradmax_clip=5.0, keep_k=17, resamp_per=2, shift=1,
              sample_mean=0.0, seed=SEED, env_offset=4)

    def buffers():
        d = per_env(eng, inputs)
        Q = eng.tensor(inputs["plans"].copy())
        d.update(Q=Q, m=torch.zeros_like(Q), v=torch.zeros_like(Q), Q_out=eng.zeros(E), S_out=eng.zeros(E, N),
                 plan_out=eng.zeros(E, H), order_out=torch.zeros(E, N, dtype=torch.int32, device=Q.device))
        return d

    def arguments(d):
        return ((d["s0"], d["Q"], d["m"], d["v"], d["tp"], d["te"]),
                dict(L=d["L"], previous_input=d["prev"], Q_out=d["Q_out"], S_out=d["S_out"], plan_out=d["plan_out"],
                     order_out=d["order_out"], **hp))

    direct, prepared = buffers(), buffers()
    args, kw = arguments(direct)
    first = [t.clone() for t in eng.rpgd_step(*args, **kw)]
    after_first = direct["Q"].clone()
    # the next control step: count 1 resamples (resamp_per 2) at the draw offset given, Adam goes on from iteration 2
    out = eng.rpgd_step(*args, count=1, adam_iteration=2, draw_offset=1, **kw)
    assert [id(t) for t in out] == [id(direct[k]) for k in ("Q_out", "S_out", "plan_out", "order_out")]
    args, kw = arguments(prepared)
    call = eng.prepare_rpgd_step(*args, **kw)
    assert call.out == tuple(prepared[k] for k in ("Q_out", "S_out", "plan_out", "order_out"))
    for a, b in zip(first, call.run()):
        assert torch.equal(a, b)
    assert torch.equal(after_first, prepared["Q"])
    assert call.run(count=1, adam_iteration=2, draw_offset=1) is call.out
    torch.cuda.synchronize()
    same(direct, prepared)
    # ... and the counters counted: the step with them at zero again ends elsewhere
    again = buffers()
    args, kw = arguments(again)
    eng.rpgd_step(*args, **kw)
    eng.rpgd_step(*args, **kw)
    assert not torch.equal(again["Q"], direct["Q"])


def test_cem_step(eng, inputs):
    hp = dict(iterations=2, best_k=7, stdev_min=0.01, shift=1, mean_fill=0.0, stdev_fill=math.sqrt(0.5), seed=SEED, env_offset=4)

    def buffers():
        d = per_env(eng, inputs)
        d.update(mean=eng.tensor(inputs["mean"].copy()), stdev=eng.tensor(inputs["stdev"].copy()), Q_out=eng.zeros(E),
                 S_out=eng.zeros(E, N), plan_out=eng.zeros(E, H), samples_out=eng.zeros(E, N, H),
                 order_out=torch.zeros(E, N, dtype=torch.int32, device=d["s0"].device))
        return d

    def arguments(d):
        return ((d["s0"], d["mean"], d["stdev"], d["tp"], d["te"]),
                dict(L=d["L"], previous_input=d["prev"], **{k: d[k] for k in ("Q_out", "S_out", "plan_out", "samples_out", "order_out")},
                     **hp))

    direct, prepared = buffers(), buffers()
    args, kw = arguments(direct)
    first = [t.clone() for t in eng.cem_step(*args, **kw)]
    eng.cem_step(*args, offset=2, **kw)
    second_samples = direct["samples_out"].clone()
    args, kw = arguments(prepared)
    call = eng.prepare_cem_step(*args, **kw)
    for a, b in zip(first, call.run()):
        assert torch.equal(a, b)
    assert call.run(offset=2) is call.out
    torch.cuda.synchronize()
    same(direct, prepared)
    assert not torch.equal(first[3], second_samples)                      # other draws in the second pass: the offset counted
