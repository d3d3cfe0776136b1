"""CPU: the inputs of the wide plant tests (plant_cases.py; the GPU side is test_gpu_plant_wide.py) judged on the oracle alone - that
the seed chosen there delivers the bounces, the wraps and the few flagged envs the GPU test relies on.  These are conditions on the
inputs, not measurements of the kernel."""
import numpy as np
import pytest

import plant_cases as PC


@pytest.fixture(scope="module")
def wide():
    case = PC.wide_case()
    return case, PC.oracle_rows(case)


def test_the_wide_case_has_the_layout_the_issue_names(wide):
    case, _ = wide
    E, s0 = case["E"], case["s0"]
    assert (E, case["T"], case["n_ctrl"], case["n_save"], case["stride"], case["dt"]) == (321, 3, 10, 4, 1, 0.002)
    assert E == PC.BLOCK + PC.WAVE + 1 and case["n_ctrl"] % case["n_save"] != 0
    n_sim = case["T"] * case["n_ctrl"]
    assert case["Qs"].shape == case["qd"].shape == (case["T"] + 1, E) and s0.shape == (E, 6) and s0.dtype == np.float32
    for k in ("tp", "te", "Ltab", "mtab", "Lctab", "off", "told"):
        assert case[k].shape == (n_sim + 1, E), k
    assert (np.diff(case["Ltab"], axis=0) != 0).any(axis=1).sum() == n_sim // 7      # a change every 7 steps, inside control periods
    assert (np.diff(case["mtab"], axis=0) != 0).any(axis=1).sum() == n_sim // 11
    edge, seam = np.arange(0, E, 8), np.arange(4, E, 8)
    gap = float(PC.THL) - np.abs(s0[edge, 4])
    assert np.all((gap > 0.003 - 1e-6) & (gap < 0.013 + 1e-6)) and np.all(s0[edge, 4] * s0[edge, 5] > 0)      # toward the end
    assert np.all((np.abs(s0[edge, 5]) >= 0.4) & (np.abs(s0[edge, 5]) <= 0.8))
    assert np.all(np.sign(s0[edge, 4]) == np.where(np.arange(len(edge)) % 2 == 0, 1, -1))                     # the sign alternates
    assert np.all((np.abs(s0[seam, 0]) >= 3.05) & (np.abs(s0[seam, 0]) <= 3.13)) and np.all(s0[seam, 0] * s0[seam, 1] > 0)
    assert np.all((np.abs(s0[seam, 1]) >= 3.0) & (np.abs(s0[seam, 1]) <= 6.0))
    assert np.all(np.sign(s0[seam, 0]) == np.where(np.arange(len(seam)) % 2 == 0, 1, -1))
    assert np.array_equal(s0[:, 2], np.cos(s0[:, 0])) and np.array_equal(s0[:, 3], np.sin(s0[:, 0]))


def test_the_seed_delivers_bounces_and_wraps_in_every_wave_with_few_envs_flagged(wide):
    case, ref = wide
    E = case["E"]
    ok = PC.unflagged(ref)
    bounced, wrapped = ok & (ref["bounce_step"] > 0), ok & ref["wrapped"]
    wave, block = np.arange(E) // PC.WAVE, np.arange(E) // PC.BLOCK
    per_wave_b = np.bincount(wave[bounced], minlength=6)
    per_wave_w = np.bincount(wave[wrapped], minlength=6)
    per_block_w = np.bincount(block[wrapped], minlength=2)
    print(f"seed {PC.SEED}: flagged {int((~ok).sum())} of {E} envs ({100.0 * (~ok).mean():.2f} %): {np.flatnonzero(~ok).tolist()}")
    print(f"unflagged envs that bounce: {int(bounced.sum())}, per wave {per_wave_b.tolist()}; twice or more: {int((ok & (ref['bounces'] > 1)).sum())}")
    print(f"unflagged envs that wrap:   {int(wrapped.sum())}, per wave {per_wave_w.tolist()}, per workgroup {per_block_w.tolist()}")
    print(f"edge margin: {int((ref['edge_margin'] < 1e-5).sum())} envs within 1e-5, {int((ref['edge_margin'] < 1e-4).sum())} within 1e-4; "
          f"seam margin: {int((ref['seam_margin'] < 1e-4).sum())} within 1e-4, smallest {ref['seam_margin'].min():.2e}")
    print(f"env 320: bounce at step {int(ref['bounce_step'][320])}, flag step {int(ref['flag_step'][320])} (> {ref['n_sim']}: never)")
    assert (~ok).sum() <= 0.05 * E
    assert bounced.sum() >= 24 and len(per_wave_b) == 6 and per_wave_b.min() >= 1
    assert wrapped.sum() >= 24 and len(per_block_w) == 2 and per_block_w.min() >= 1
    # the lone lane of the last wave: unflagged, and with this seed it does bounce (it is what the sixth wave's count above rests on)
    assert ok[320] and ref["bounce_step"][320] > 0
    # the flag rule flags what it says: an env is flagged exactly from the first step inside one of the two margins
    inside = (ref["edge_margin"] < PC.EDGE_FLAG) | (ref["seam_margin"] < PC.SEAM_FLAG)
    assert np.array_equal(inside, ~ok)
    # bounces fall into every control period's steps, so the bounce is met with more than one control and table row
    assert len(np.unique((ref["bounce_step"][bounced] - 1) // case["n_ctrl"])) >= 2


def test_saved_rows_and_the_padding_of_tables(wide):
    case, ref = wide
    R = case["T"] * case["n_ctrl"] // case["n_save"] + 1
    assert ref["states"].shape == (R, case["E"], 6) and ref["step_of_row"].tolist() == [0, 4, 8, 12, 16, 20, 24, 28]
    assert np.array_equal(ref["states"][0], case["s0"]) and PC.compared(ref)[0].all()
    assert np.abs(ref["states"][:, :, 4]).max() <= float(PC.THL) + 0.002      # a bounce leaves the cart at most one step's travel outside
    short = dict(case, **{k: case[k][:17] for k in ("tp", "te", "Ltab", "mtab", "Lctab", "off", "told")})
    padded = PC.pad_tables(short, 31)
    for k in ("tp", "Ltab", "off", "told"):
        assert padded[k].shape == case[k].shape and np.array_equal(padded[k][:17], case[k][:17]) and (padded[k][17:] == case[k][16]).all()
