"""Host: DAgger for the neural imitator - the gate's reference (tests/dagger_ref.py) pinned against a scalar restatement and known
answers, the beta schedule and the command line, every refusal of the Python layer that needs no device, and the code-object
metadata of dagger_step_kernel."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dagger_ref as G  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- 1. the gate
def philox_scalar(counter, key):
    """Philox4x32-10 on Python integers (Salmon et al. 2011), written out once more, without numpy."""
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def u24(seed, env, c):
    """The gate's 24 bits: word 1 of the block (0xFFFFFFFF, env, 0, c_lo) under key (seed_lo ^ 0x51ed270b, seed_hi ^ c_hi)."""
    return philox_scalar([M32, env & M32, 0, c & M32], ((seed & M32) ^ 0x51ED270B, ((seed >> 32) ^ (c >> 32)) & M32))[1] >> 8


# (seed, env_offset, c) -> the 24-bit integers of envs 0..3: c either side of 2^32, an env offset, one that wraps, a 64-bit seed
KNOWN = {(7, 0, 0): [10953806, 3632200, 12721032, 1508095],
         (7, 0, 2 ** 32 - 1): [1580649, 6407802, 14729281, 15886701],
         (7, 0, 2 ** 32): [16754288, 9291554, 2532125, 13091429],
         (7, 0, 2 ** 32 + 1): [11594979, 10502565, 3207513, 2426632],
         (0x123456789ABCDEF0, 1000, 5): [676785, 1988521, 14269049, 13172866],
         (7, 2 ** 32 - 2, 3): [11821882, 8816742, 8143187, 11830661]}


@pytest.mark.parametrize("case", list(KNOWN), ids=lambda k: f"seed{k[0]:x}-off{k[1]}-c{k[2]}")
def test_the_gate_uniform_is_pinned(case):
    seed, off, c = case
    ub = G.gate_uniform(seed, off, 4, c)
    assert ub.dtype == f32 and ((0 <= ub) & (ub < 1)).all()
    got = (ub.astype(np.float64) * 2.0 ** 24).astype(np.int64).tolist()
    assert got == KNOWN[case] == [u24(seed, off + e, c) for e in range(4)]


def test_the_period_high_word_goes_into_the_key_and_the_block_is_no_samplers():
    from oracle import philox_np as P
    a, b = G.gate_uniform(7, 0, 64, 3), G.gate_uniform(7, 0, 64, 3 + 2 ** 32)
    assert not np.array_equal(a, b)                                  # the same low word: only the key differs
    assert not np.array_equal(G.gate_uniform(7, 0, 64, 3), G.gate_uniform(7, 64, 64, 3))
    assert np.array_equal(G.gate_uniform(7, 5, 59, 3), G.gate_uniform(7, 0, 64, 3)[5:])     # an env keeps its draw wherever it is launched
    # it IS the sampler's quad block of rollout 0xFFFFFFFF, which no launch has (N is a uint32 count: its rollouts end at N - 1)
    words = P.quad_words(7, 3, np.arange(64), G.GATE_ROLLOUT, 0)
    assert np.array_equal((words[:, 1] >> 8).astype(np.float64) * 2.0 ** -24, a.astype(np.float64))


def test_beta_edges():
    seed, off, E, c = 11, 3, 4096, 17
    ub = G.gate_uniform(seed, off, E, c)
    step = f32(2.0 ** -24)
    assert not G.gate(seed, off, E, c, 0.0).any() and not G.gate(seed, off, E, c, -1.0).any()
    assert G.gate(seed, off, E, c, 1.0).all() and G.gate(seed, off, E, c, 2.0).all()
    assert not G.gate(seed, off, E, c, np.nan).any()
    assert np.array_equal(G.gate(seed, off, E, c, step), ub == 0)
    assert np.array_equal(G.gate(seed, off, E, c, f32(1.0) - step), ub != f32(1.0) - step)
    half = G.gate(seed, off, E, c, 0.5)
    assert np.array_equal(half, ub < f32(0.5)) and abs(half.mean() - 0.5) < 4 * 0.5 / np.sqrt(E)     # (four standard deviations)
    # the two edges on a draw that hits them: ub = 0 loses against beta = 0 and wins against 2^-24; ub = 1 - 2^-24 loses against
    # itself and wins against 1 (the comparison is strict)
    for u, beta, want in ((0.0, 0.0, False), (0.0, step, True), (1.0 - step, 1.0 - step, False), (1.0 - step, 1.0, True)):
        assert bool(f32(u) < f32(beta)) is want
    per_env = np.where(np.arange(E) % 2 == 0, 1.0, np.nan).astype(f32)
    assert np.array_equal(G.gate(seed, off, E, c, per_env), np.arange(E) % 2 == 0)


def test_applied_control_and_disagreement():
    g = np.array([True, False, True, False])
    qe, qi = np.array([np.nan, np.nan, 0.25, -0.5], f32), np.array([0.1, 0.2, 0.3, 0.4], f32)
    out = G.applied(g, qe, qi)
    assert np.isnan(out[0]) and out[1] == f32(0.2) and out[2] == f32(0.25) and out[3] == f32(0.4)
    s = G.sq_err(np.zeros(2), [[0.5, 1.0], [0.25, -1.0]], [[0.0, 1.0], [0.0, 1.0]])
    assert s.dtype == np.float64 and s.tolist() == [0.3125, 4.0]


# ---------------------------------------------------------------------------------------------- 2. schedule and command line
def test_beta_schedule():
    from cartpolesimulation_amd.train_imitator import beta_schedule
    assert beta_schedule("1,0.5,0.25,0", 4) == [1.0, 0.5, 0.25, 0.0]
    assert beta_schedule("1,0.5", 4) == [1.0, 0.5, 0.5, 0.5]          # the last one is kept
    assert beta_schedule(0.5, 3) == [0.5, 0.5, 0.5] and beta_schedule((1, 0), 2) == [1.0, 0.0]
    for bad, text in (("1,0.5,0", "at most one per iteration"), ("1,x", "numbers separated by commas"), ("1,1.5", r"in \[0, 1\]"),
                      ("-0.1", r"in \[0, 1\]"), ("nan", r"in \[0, 1\]"), ([], "at most one per iteration")):
        with pytest.raises(ValueError, match=text):
            beta_schedule(bad, 2)
    with pytest.raises(ValueError, match="iterations must be at least 1"):
        beta_schedule(1.0, 0)


def test_command_line_refusals():
    from cartpolesimulation_amd.train_imitator import main
    base = ["--out", "unused"]
    for argv, text in ((["--dagger", "2", "--recordings", "x", "--config-root", "y"], "--dagger and --recordings"),
                       (["--dagger", "2", "--validation", "x", "--config-root", "y"], "--dagger and --validation"),
                       (["--dagger", "2"], "--dagger needs --config-root"),
                       (["--dagger", "2", "--config-root", "y", "--beta", "1,0.5,0"], "--beta: .*at most one per iteration"),
                       (["--dagger", "2", "--config-root", "y", "--beta", "2"], r"--beta: .*in \[0, 1\]"),
                       ([], r"--recordings DIR \(or --dagger ITERATIONS\) is required"),
                       (["--recordings", "x", "--experiments", "3"], "--experiments belongs to --dagger"),
                       (["--recordings", "x", "--steps-per-iteration", "3"], "--steps-per-iteration belongs to --dagger"),
                       (["--recordings", "x", "--optimizer", "rpgd"], "--optimizer belongs to --dagger"),
                       (["--recordings", "x", "--graph"], "--graph belongs to --dagger")):
        with pytest.raises(SystemExit, match=text):
            main(base + argv)
    with pytest.raises(SystemExit):                                  # (argparse: the expert is mppi or the fused rpgd)
        main(base + ["--dagger", "2", "--config-root", "y", "--optimizer", "cem"])


# ---------------------------------------------------------------------------------------------- 3. refusals that need no device
class HostEngine:
    """Stands in for MPPIEngine where only buffers are made."""
    device = torch.device("cpu")

    def zeros(self, *shape):
        return torch.zeros(*shape)


def test_dataset_reserve():
    from cartpolesimulation_amd.harness import DaggerDataset
    d = DaggerDataset(HostEngine(), 8, 41)
    assert d.states.shape == (8, 41, 6) and d.gate.dtype == torch.uint8 and d.sq_err.dtype == torch.float64 and d.sq_err.shape == (8,)
    assert all(t.shape == (8, 41) for t in (d.target_position, d.target_equilibrium, d.labels, d.imitator, d.gate))
    assert d.tensors == (d.states, d.target_position, d.target_equilibrium, d.labels) or len(d.tensors) == 4
    assert (d.filled, d.reserve(4), d.filled, d.reserve(4), d.filled) == (0, 0, 4, 4, 8)
    with pytest.raises(ValueError, match="DaggerDataset is full: 8 of its 8 recordings are written, 1 more"):
        d.reserve(1)
    assert d.filled == 8
    with pytest.raises(ValueError, match="DaggerDataset is full: 0 of its 2 recordings are written, 3 more"):
        DaggerDataset(HostEngine(), 2, 5).reserve(3)
    with pytest.raises(ValueError, match="at least one recording and one row"):
        DaggerDataset(HostEngine(), 0, 5)


def test_each_excluded_combination_is_refused_by_name_on_the_host():
    from cartpolesimulation_amd.harness import ENGINE_MODEL, DaggerDataset, check_dagger
    E = 4
    batch = SimpleNamespace(E=E, n_periods=40)
    ds = DaggerDataset(HostEngine(), E, 41)
    ok = dict(dataset=ds, beta=0.5, seed=3)
    model = {"w1": 0}
    got = check_dagger(ok, batch, model)
    assert got[0] is model and got[1] is ds and got[3] == 3 and got[2].dtype == f32 and got[2].tolist() == [0.5] * E
    assert check_dagger(dict(ok, beta=[0, 1, 0.5, np.nan]), batch, "engine-model")[0] is ENGINE_MODEL
    assert check_dagger(dict(dataset=ds, beta=1.0), batch, model)[3] == 0
    fused, paced = SimpleNamespace(fused=True), SimpleNamespace(fused=False)
    assert check_dagger(ok, batch, model, optimizer=fused)[1] is ds
    for text, args, kw in (("dagger= needs imitator=", (ok, batch, None), {}),
                           ("dagger= takes dataset=, beta= and seed=", (dict(ok, gamma=1), batch, model), {}),
                           ("dagger= takes dataset=, beta= and seed=", (dict(beta=1.0), batch, model), {}),
                           ("dagger= takes dataset=, beta= and seed=", (dict(dataset=ds), batch, model), {}),
                           ("dagger= and predictor='GRU'", (ok, batch, model), dict(predictor="GRU")),
                           ("dagger= and h0", (ok, batch, model), dict(h0=np.zeros((E, 2, 32), f32))),
                           ("dagger= and knots_fn", (ok, batch, model), dict(knots_fn=lambda c: None)),
                           ("dagger= and tuning=", (ok, batch, model), dict(tuning=np.zeros((E, 16), f32))),
                           ("dagger= and an optimizer with gru_model=", (ok, batch, model), dict(optimizer=SimpleNamespace(fused=True, gru_model={}))),
                           ("dagger= and an optimizer with gru_model=", (ok, batch, model), dict(optimizer=SimpleNamespace(gru_fused=True, h=object()))),
                           ("dagger= and a host-paced optimizer=", (ok, batch, model), dict(optimizer=paced)),
                           ("dataset must be a harness.DaggerDataset", (dict(ok, dataset=object()), batch, model), {}),
                           ("the dataset has 41 rows per recording, the batch makes 40 controller calls",
                            (ok, SimpleNamespace(E=E, n_periods=39), model), {}),
                           (r"beta must be a scalar or \[4\], got shape \(3,\)", (dict(ok, beta=[1, 1, 1]), batch, model), {})):
        with pytest.raises(ValueError, match=text):
            check_dagger(*args, **kw)
    assert ds.filled == 0                                            # nothing was reserved on the way


def test_run_schedule_without_dagger_keeps_check_imitator():
    """dagger=None: the refusals of imitator= are the ones tests/test_gpu_imitator_loop.py pins, from the same function."""
    import inspect
    from cartpolesimulation_amd import harness as H
    src = inspect.getsource(H.BatchedCartPoleExperiment.run_schedule)
    assert "check_imitator(imitator, optimizer, predictor, h0, knots_fn, tuning)" in src
    assert inspect.signature(H.BatchedCartPoleExperiment.run_schedule).parameters["dagger"].default is None
    assert inspect.signature(H.ScheduleRun.__init__).parameters["dagger"].default is None
    with pytest.raises(ValueError, match="imitator= and optimizer="):
        H.check_imitator({}, optimizer=object())


def test_the_driver_refuses_before_it_touches_the_engine():
    from cartpolesimulation_amd.train_imitator import dagger, identity_normalization, initial_weights
    kw = dict(experiments=2, iterations=2, steps_per_iteration=1, batch_size=8, lr=1e-3, seed=1)
    with pytest.raises(ValueError, match=r"beta\[0\] must be 1, got 0.5"):
        dagger(None, {}, beta="0.5,0", **kw)
    with pytest.raises(ValueError, match="a host-paced optimizer cannot be the expert"):
        dagger(None, {}, beta=1.0, optimizer=SimpleNamespace(fused=False), **kw)
    with pytest.raises(ValueError, match="steps_per_iteration and batch_size must be at least 1"):
        dagger(None, {}, beta=1.0, **dict(kw, batch_size=0))
    with pytest.raises(ValueError, match="weight b1 must have shape"):
        dagger(None, {}, beta=1.0, init={"w1": np.zeros((32, 7), f32)}, **kw)
    # with a normalisation in init, iteration 0 may start below 1: the refusal is not raised (the setter's empty config is, later)
    init = {**initial_weights(3), **identity_normalization()}
    with pytest.raises(Exception) as e:
        dagger(None, {}, beta="0.5,0", init=init, **kw)
    assert "beta[0]" not in str(e.value)


def test_normalization_from_extrema_is_the_recordings_rule():
    from cartpolesimulation_amd.train_imitator import normalization_from_extrema, normalization_from_recordings
    import dense_ref as D
    s, tp, te, lab = D.recordings(5, R=3, T=40)
    want = normalization_from_recordings(s, tp, te, lab)
    cols = np.concatenate([s.reshape(-1, 6)[:, 1:6], te.reshape(-1, 1), tp.reshape(-1, 1), lab.reshape(-1, 1)], axis=1)
    got = normalization_from_extrema(cols.min(axis=0), cols.max(axis=0))
    assert set(got) == set(want) and all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) for k in want)


# ---------------------------------------------------------------------------------------------- 4. the kernel's resources
def test_the_kernel_has_no_scratch_and_no_vgpr_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = [k for k in code_objects.kernels(_lib.LIB_PATH) if re.search(r"dagger_step_kernel", k["name"])]
    assert len(ks) == 1, [k["name"] for k in ks]
    assert ks[0]["private_segment_fixed_size"] == 0 and ks[0]["vgpr_spill_count"] == 0, ks[0]


def test_the_entry_point_is_bound_and_documented():
    from cartpolesimulation_amd import _lib as L
    from cartpolesimulation_amd.engine import MPPIEngine
    assert "cpmppi_dagger_step" in L.EXPORTS and hasattr(MPPIEngine, "dagger_step") and hasattr(MPPIEngine, "prepare_dagger_step")
    names = [n for n, _ in L.cpmppi_dagger_args._fields_]
    with open(os.path.join(ROOT, "include", "cpmppi.h")) as fh:
        header = fh.read()
    block = header[:header.index("} cpmppi_dagger_args;")]
    block = block[block.rindex("typedef struct {"):]
    declared = re.findall(r"(\w+);", block.replace("R, T, r0;", "R; T; r0;"))
    assert declared == names, (declared, names)                      # the same fields in the same order
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            assert "cpmppi_dagger_step" in fh.read(), doc
