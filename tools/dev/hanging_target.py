"""The cost bound for default.py's cost with the HANGING target (target_equilibrium < 0): TEST INFRASTRUCTURE shared by
tools/dev/shape_fuzz.py and tests/test_gpu_rollout_matrix.py (through tests/rollout_matrix.py).

default.py's angle term is 20000 * te * 0.25 (1 - cos)^2: NEGATIVE for that target, so a rollout's total is a difference of terms of
~1e4 per stage and a bound relative to |S| is a bound on cancellation, not on the kernel: these costs are compared against the magnitude
of the terms - the 1e-4 band + the envelope of the reference's realisations + 1e-5 of the largest possible stage term (20000 per stage,
x H under the summing horizon reduction)."""
import numpy as np

from oracle import parity


def hanging_default_buckets(S, S_a, S_b, flagged, S_alt=(), H=1, horizon_reduce="sum"):
    """The per-rollout verdict in the form of parity.cost_buckets.  `flagged`: the oracle's H2 flags; nothing joins them here."""
    scale = 20000.0 * (1.0 if horizon_reduce == "mean" else H)
    S_a = np.asarray(S_a, np.float64)
    dev = np.abs(np.asarray(S, np.float64) - S_a)
    allowance = 1e-4 * np.abs(S_a) + parity.envelope(S_a, S_b, *S_alt) + 1e-5 * scale
    flagged = np.asarray(flagged, bool)
    return dict(off=dev > allowance, flagged=flagged, sensitive=np.zeros(flagged.shape, bool), excess=dev / allowance,
                rel=dev / np.maximum(np.abs(S_a), 1e-30))


def assert_hanging_default_costs(S, S_a, S_b, flagged, what="costs (hanging target)", S_alt=(), H=1, horizon_reduce="sum"):
    """No rollout clear of the oracle's flags outside hanging_default_buckets' allowance (flagged ones are not held to it)."""
    b = hanging_default_buckets(S, S_a, S_b, flagged, S_alt, H, horizon_reduce)
    out = int((b["off"] & ~b["flagged"]).sum())
    assert out == 0, f"{what}: {out} outside"
    return b
