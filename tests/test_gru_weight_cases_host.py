"""Host: what the GRU weight-image tests (test_gpu_gru_weights.py) rest on, checked with the oracle alone.

1. The refusal boundary of cpmppi_set_gru, restated: |float32(float64(scale) float64(w))| < 60000 on the value the f16 image stores.
   The largest accepted float32 magnitude and its successor per kind of row, found by nextafter; the three limits as stated.
2. The 13 places are distinct entries, one per matrix and gate, spread over both lane halves and k-blocks.
3. Models A and B: different normalisations, B out of range at exactly one entry.
4. The split cell's cases: per model at most 2 % of the rollouts are rounding-sensitive in the oracle (flag_rounding_sensitive of its
   float32 and float64 evaluations), both evaluations finite - so that a device result outside the rules is the device's.  Each case
   does what its name says (the entries at 0.9 of the limit, the share of tiny entries, the memory's values, the normalised
   inputs inside the +-65504 the split carries)."""
import numpy as np

import gru_weight_cases as W
import parity_util as PU

f32 = np.float32


def test_accept_limits_by_nextafter():
    for kind in ("r", "z", "n", "head"):
        lo, hi = W.accept_limit(kind)
        assert lo.dtype == f32 and hi == np.nextafter(lo, f32(np.inf))
        assert W.accepted(kind, lo) and W.accepted(kind, -lo) and not W.accepted(kind, hi) and not W.accepted(kind, -hi)
        assert lo == W.STATED_LIMITS[kind], (kind, repr(lo))
        # the stored value at the limit is finite in f16 with room to spare; an UNSCALED check, or one at 65504 / scale, differs
        assert abs(float(W.stored(kind, lo))) < 60000.0 <= abs(float(W.stored(kind, hi))) < 65504.0
    assert W.accept_limit("r") == W.accept_limit("z")
    # the limit differs per gate, so a check on the unscaled weight accepts the gate rows' successors
    for kind in ("r", "z", "n"):
        assert abs(float(W.accept_limit(kind)[1])) < 60000.0
    assert not W.accepted("head", np.inf) and not W.accepted("r", np.nan)


def test_places_cover_every_matrix_and_gate():
    assert len(W.PLACES) == 13 and len(set(W.PLACES)) == 13
    assert {(k, g) for k, g, _, _ in W.PLACES[:12]} == {(k, g) for k in W.MATRICES[:4] for g in W.GATES}
    m = W.model_a()
    for key, kind, row, col in W.PLACES:
        assert row < m[key].shape[0] and col < m[key].shape[1]
        if kind != "head":
            assert row // 32 == W.GATES.index(kind)
    rows = [r % 32 for _, _, r, _ in W.PLACES[:12]]
    cols = [c for k, _, _, c in W.PLACES[:12] if k != "w_ih0"]
    assert len(set(rows)) >= 8 and min(cols) < 16 <= max(cols)


def test_models_a_and_b():
    a, b = W.model_a(), W.model_b()
    assert set(a) == set(b) == set(W.GRU_KEYS) | set(W.NORM_KEYS)
    for k in W.NORM_KEYS:
        assert not np.array_equal(a[k], b[k])
    bad = [(k, i) for k in W.MATRICES for i in zip(*np.nonzero(~(np.abs(b[k]) < 1.0)))]
    assert bad == [("w_hh1", (40, 9))] and not W.accepted("z", b["w_hh1"][40, 9])
    for k in W.MATRICES:
        assert np.abs(a[k]).max() <= 0.3


def test_split_cases_are_what_they_say():
    base = {name: W.random_model(2610 + i) for i, name in enumerate(W.SPLIT_CASES)}
    for name in ("a+", "a-"):
        m = W.split_case(name)["model"]
        for j, (key, kind, row, col) in enumerate(W.PLACES[:12]):
            v = float(W.stored(kind, m[key][row, col]))
            assert 0.899 * 60000 < abs(v) < 0.901 * 60000
        changed = sum(int((m[k] != base[name][k]).sum()) for k in W.GRU_KEYS + W.NORM_KEYS)
        assert changed == 12
    signs = [np.sign(W.split_case("a+")["model"][k][r, c]) for k, _, r, c in W.PLACES[:12]]
    assert signs.count(1.0) == 6 and [-s for s in signs] == [np.sign(W.split_case("a-")["model"][k][r, c]) for k, _, r, c in W.PLACES[:12]]
    m = W.split_case("b")["model"]
    for k in W.MATRICES:
        tiny = np.abs(m[k]) < 0.3e-4 * 1.0001
        assert 0.4 < tiny.mean() < 0.6
        # of the tiny ones, most are below f16's smallest normal (6.1e-5) after the gate scale, some below its smallest subnormal
        assert (np.abs(m[k][tiny]) * 2.0 * W.LOG2E < 6.1e-5).mean() > 0.9 and (np.abs(m[k][tiny]) * 2.0 * W.LOG2E < 6e-8).mean() > 0.2
    h0 = W.split_case("c")["h0"]
    assert set(np.unique(h0).tolist()) == set(W.H0_VALUES.tolist())
    for name, sign in (("d+", 1.0), ("d-", -1.0)):
        c = W.split_case(name)
        m = c["model"]
        assert m["in_shift"][0] == f32(sign * 6.0e4) and m["in_shift"][3] == f32(1.0e3)
        # the normalised control stays inside the split's envelope for every control in [-1, 1]
        assert abs(float(m["in_shift"][0])) + float(m["in_scale"][0]) < 65504.0
    assert (W.split_case("e")["model"]["in_scale"] == f32(1e-6)).all()


def test_split_cases_are_well_conditioned_in_the_oracle(capsys):
    for name in W.SPLIT_CASES:
        flagged, worst = 0, 0.0
        for a, b in W.split_reference(name):
            assert np.isfinite(a["S"]).all() and np.isfinite(b["S"]).all() and np.isfinite(a["u_new"]).all() and np.isfinite(b["u_new"]).all()
            assert a["S"].shape == (W.N,)
            flagged += int(PU.flag_rounding_sensitive(a["S"], b["S"]).sum())
            worst = max(worst, float((np.abs(a["S"].astype(np.float64) - b["S"]) / np.abs(b["S"])).max()))
        with capsys.disabled():
            print(f"\n[gru-weights] case {name}: {flagged} of {W.E * W.N} rollouts flagged, worst float32-float64 cost gap {worst:.2e}")
        assert flagged <= 0.02 * W.E * W.N, name


def test_cases_differ_from_one_another():
    """Every case costs its rollouts differently from the unchanged model of the same seed: the change reaches the costs."""
    from oracle import oracle_np as O
    cfg = O.MPPIConfig(N=W.N, H=W.H)
    for i, name in enumerate(W.SPLIT_CASES):
        if name == "c":
            continue                                        # (the model is unchanged there: the memory is the case)
        c = W.split_case(name)
        plain = O.gru_mppi_step(W.random_model(2610 + i), c["s0"][0], c["u0"][0], c["du"][0], c["tp"][0], c["te"][0], cfg, h0=c["h0"][0])
        assert (plain["S"] != W.split_reference(name)[0][0]["S"]).mean() > 0.9, name
