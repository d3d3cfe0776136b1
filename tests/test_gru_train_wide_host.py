"""CPU-only: the shapes of the wide GRU training tests (tests/gru_train_wide_cases.py) judged before the GPU sees them.

1. The slice plan of every case, recomputed from WG_MAX_SLICES and WG_MIN_TILES as csrc/cpmppi_gru_train.hip defines them, is the
   table of gru_train_wide_cases and reaches the edge the case is named for: a change of either constant fails here, by name, and
   does not quietly move the cases off their edges.
2. The reference against itself: at every case, for the four models of gru_train_rollout_ref.MODELS and both modes, the float32
   torch realisation lies within share_min / 16 of float64 autograd (and within a quarter of the project's 5e-4, as
   test_train_gru_rollout_host.py holds it) - the GPU test asserts share_min / 4 with this reference.

Measured here (worst over the four models; float32 against float64, of a tensor's max |g|):
  case   share_min full tiles   ragged tile   float32 teacher-forced   float32 rollout
  A      1.14e-03               -             2.2e-07                  2.9e-07
  B      1.09e-03               5.64e-04      2.1e-07                  2.2e-07
  C      2.73e-03               1.17e-03      4.1e-07                  3.9e-07
  D      3.91e-03               4.27e-03      4.2e-07                  5.8e-07
  E      2.40e-02               2.49e-02      6.0e-07                  5.1e-07
(share_min / 16 is at least 3.5e-5, case B; D and E, where the GPU test asserts a measured bound, pass the same check.)  The
float32 figures are a property of the host's float32 GEMM too: on a second host, with 16 threads, the teacher-forced column reads
7.9e-6, 1.0e-5, 1.7e-5, 4.7e-6, 9.9e-7 for A .. E and the rollout column at most 9.9e-6 - still a factor 3.5 (B) and 4.4 (C) inside
share_min / 16.  The whole module takes about 7 s, most of it the float64 and float32 autograd of case C."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_train_ref as TR  # noqa: E402
import gru_train_rollout_ref as RR  # noqa: E402
import gru_train_wide_cases as WC  # noqa: E402

GRAD_TOL = 5e-4
IDS = [f"{n}-{'norm' if k else 'identity'}" for n, k in RR.MODELS]


def report(capsys, text):
    with capsys.disabled():
        print("\n[gru-train-wide-host] " + text)


# ---------------------------------------------------------------------------------------------- 1. the slice plans
def test_slice_plans_are_the_table_and_sit_on_their_edges(capsys):
    max_slices, min_tiles = WC.source_constants()
    plans = {key: WC.slice_plan(*WC.CASES[key], max_slices, min_tiles) for key in WC.CASES}
    for key, p in plans.items():
        report(capsys, f"case {key}: B {WC.CASES[key][0]} W, P {WC.CASES[key][1:]}: Bp {p['Bp']} tpr {p['tpr']} tiles {p['tiles']}, "
                       f"per_slice {p['per_slice']}, slices {p['slices']} (last {p['last']}), loss partials {p['partials']}")
        got = (p["Bp"], p["tpr"], p["tiles"], p["per_slice"], p["slices"], p["last"])
        assert got == WC.TABLE[key], (f"case {key}: with WG_MAX_SLICES = {max_slices}, WG_MIN_TILES = {min_tiles} the plan is {got}, the "
                                      f"table of gru_train_wide_cases says {WC.TABLE[key]}: choose the shapes again")
        assert p["slices"] <= max_slices and p["per_slice"] >= min_tiles
    a, b, c, d, e = (plans[k] for k in "ABCDE")
    # A: the cap reached exactly at the minimum slice
    assert a["per_slice"] == min_tiles and a["slices"] == max_slices and a["last"] == min_tiles
    # B: the first per_slice beyond the minimum; a short last slice; boundaries inside rows; a ragged window tile
    assert b["per_slice"] == min_tiles + 1 and 0 < b["last"] < b["per_slice"] and b["tpr"] % b["per_slice"] != 0
    assert np.gcd(b["tpr"], b["per_slice"]) == 1 and WC.CASES["B"][0] % 32 != 0
    # C: 40 rows of back-propagation, 6 live lanes in the last tile, a short last slice under the cap
    assert sum(WC.CASES["C"][1:]) == 40 and WC.CASES["C"][0] % 32 == 6
    assert c["per_slice"] > min_tiles and c["slices"] < max_slices and 0 < c["last"] < c["per_slice"] and c["tpr"] % c["per_slice"] != 0
    # D: the finalize kernel loops; the first slices lie wholly in row 0, which the `prev` products skip
    assert d["partials"] == WC.FINALIZE_STRIDE + 1
    assert d["tpr"] > d["per_slice"] and d["tpr"] // d["per_slice"] == 8 and 0 < d["last"] < d["per_slice"]
    # E: slice 0 is exactly row 0
    assert e["per_slice"] == e["tpr"] and e["slices"] == sum(WC.CASES["E"][1:])


def test_the_plan_assertion_names_a_changed_constant():
    """The same arithmetic over an edited copy of the source text: every case leaves the table."""
    text = open(WC.SOURCE).read()
    assert WC.source_constants(text) == (64, 8)
    for old, new in (("WG_MAX_SLICES = 64", "WG_MAX_SLICES = 48"), ("WG_MIN_TILES = 8", "WG_MIN_TILES = 16")):
        assert old in text
        consts = WC.source_constants(text.replace(old, new))
        moved = [k for k in WC.CASES if tuple(WC.slice_plan(*WC.CASES[k], *consts)[f] for f in ("per_slice", "slices", "last")) != WC.TABLE[k][3:]]
        assert len(moved) >= 3, (new, moved)


def test_windows_repeat_overlap_and_end_at_the_last_legal_row():
    for key, (B, W, P) in WC.CASES.items():
        w = WC.case_windows(key)
        legal = WC.legal_windows(W, P)
        assert w.shape == (B, 2) and len(legal) == WC.R * (WC.T - W - P)
        assert tuple(w[0]) == tuple(w[1]) == (0, 4) and tuple(w[2]) == (0, 5) and tuple(w[-1]) == (WC.R - 1, WC.T - 1 - W - P)
        assert w[:, 0].max() == WC.R - 1 and w[:, 1].min() >= 0 and (w[:, 1] + W + P <= WC.T - 1).all()
        assert len(np.unique(w, axis=0)) > min(B, len(legal)) // 2          # drawn over the legal windows, not a few of them


# ---------------------------------------------------------------------------------------------- 2. the reference against itself
@pytest.mark.parametrize("name,norm", RR.MODELS, ids=IDS)
def test_float32_realisation_sits_inside_the_bound_it_is_used_to_assert(name, norm, capsys):
    for key in WC.CASES:
        full, ragged = WC.share_min(key, name, norm)
        bound = WC.share_bound(key, name, norm)
        assert 0 < bound < 1
        line = f"{name} norm={norm} case {key}: share_min full {full:.3e}, ragged " + ("-" if ragged is None else f"{ragged:.3e}")
        for rollout in (False, True):
            l64, g64 = WC.reference(key, name, norm, rollout)
            l32, g32 = WC.reference(key, name, norm, rollout, torch.float32)
            rel = TR.worst_relative(g32, g64)
            line += f"; {'rollout' if rollout else 'teacher-forced'} float32 against float64 {rel:.3e} (loss {abs(l32 - l64) / l64:.1e})"
            assert rel < bound / 16, (key, rollout, rel, bound)
            assert rel < GRAD_TOL / 4, (key, rollout, rel)
            assert abs(l32 - l64) <= GRAD_TOL / 4 * l64, (key, rollout)
        report(capsys, line)
