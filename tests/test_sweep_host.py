"""CPU-only: the controller sweep's host half - grid expansion (order, unknown names), the tiling of the experiments under every
setting, and the table's text."""
import numpy as np
import pytest

from cartpolesimulation_amd import schedule as SC
from cartpolesimulation_amd.sweep import expand_grid, format_table, tile_batch


def test_grid_expansion_is_the_cartesian_product_in_the_mappings_order():
    names, settings = expand_grid(dict(LBD=[50, 100, 200], ep_weight_up=[20, 40]))
    assert names == ["LBD", "ep_weight_up"]
    assert [(s["LBD"], s["ep_weight_up"]) for s in settings] == [(50, 20), (50, 40), (100, 20), (100, 40), (200, 20), (200, 40)]
    assert expand_grid(dict(SQRTRHOINV=0.02))[1] == [dict(SQRTRHOINV=0.02)]
    with pytest.raises(ValueError, match="'NU'"):
        expand_grid(dict(LBD=[1], NU=[2]))
    with pytest.raises(ValueError, match="at least one"):
        expand_grid({})
    with pytest.raises(ValueError, match="at least one"):
        expand_grid(dict(LBD=[]))


def test_every_setting_gets_the_same_experiments():
    b = SC.RandomExperimentSetter(dict(seed=5, length_of_experiment=0.2)).draw(2, 9, L=np.asarray([0.3, 0.4], np.float32))
    t = tile_batch(b, 3)
    assert t.E == 6 and t.target_position.shape == (b.target_position.shape[0], 6)
    for k in range(3):
        assert np.array_equal(t.s0[2 * k:2 * k + 2], b.s0) and np.array_equal(t.L[2 * k:2 * k + 2], b.L)
        assert np.array_equal(t.target_position[:, 2 * k:2 * k + 2], b.target_position)
        assert np.array_equal(t.target_equilibrium[:, 2 * k:2 * k + 2], b.target_equilibrium)
    assert (t.n_sim, t.n_ctrl, t.n_save, t.stride) == (b.n_sim, b.n_ctrl, b.n_save, b.stride)
    import dataclasses
    with pytest.raises(ValueError, match="Q_disturbance"):
        tile_batch(dataclasses.replace(b, Q_disturbance=np.zeros((b.n_periods + 1, 2), np.float32)), 2)


def test_table_text():
    sweep = dict(names=["LBD"], settings=[dict(LBD=50.0), dict(LBD=100.0)], columns=("a", "b"),
                 mean=np.array([[1.0, 2.0], [3.0, 4.5]]), worst=np.array([[1.5, 2.5], [3.5, 5.0]]))
    assert format_table(sweep).splitlines() == ["LBD  a:mean  a:worst  b:mean  b:worst", "50  1  1.5  2  2.5", "100  3  3.5  4.5  5"]
