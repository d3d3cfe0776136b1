"""CPU-only: the device loop's refusals of ``tuning=`` - each ValueError names what was asked for beside the rows; nothing of the
engine is touched before them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cartpolesimulation_amd.harness import BatchedCartPoleExperiment, check_tuning  # noqa: E402


class NoEngine:
    """Any use of the engine before the refusal is an AttributeError, not the ValueError the test expects."""
    H = 8


ROWS = np.zeros((2, 16), np.float32)


@pytest.mark.parametrize("kw,word", [(dict(optimizer=object()), "optimizer="), (dict(predictor="GRU"), "predictor='GRU'"),
                                     (dict(knots_fn=lambda c: None), "knots_fn")])
def test_tuning_conflicts_are_refused_by_name(kw, word):
    with pytest.raises(ValueError, match="tuning= and " + word):
        check_tuning(ROWS, **kw)
    check_tuning(None, **kw)                                         # without rows there is nothing to refuse here
    with pytest.raises(ValueError, match="tuning= and " + word):
        BatchedCartPoleExperiment(NoEngine()).run_schedule(object(), tuning=ROWS, **kw)


def test_run_refuses_tuning_with_the_gru_before_anything_else():
    with pytest.raises(ValueError, match="tuning= and predictor='GRU'"):
        BatchedCartPoleExperiment(NoEngine()).run(np.zeros((2, 6), np.float32), 3, predictor="GRU", tuning=ROWS)
