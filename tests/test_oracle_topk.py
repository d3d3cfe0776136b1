"""CPU: the contract of the CEM update's top-k and the sorting network that implements it on the device (cpmppi_optim.hip,
cem_update_kernel), restated in numpy (oracle_np.bitonic_topk).  Contract = oracle_np.cem_update: the first best_k of
np.argsort(kind="stable") - NaN after +inf, -0.0 equal to +0.0, ties by index, never a padded index.  The network meets it with the
order-preserving uint32 keys; with float keys and +inf padding (the kernel before the fix) it does not once a cost is NaN."""
import numpy as np
import pytest

from oracle import oracle_np as O

f32 = np.float32


def cost_vectors(N, seed):
    """Cost vectors of length N with every special value the contract names, at random places."""
    rng = np.random.Generator(np.random.SFC64(seed))
    out = []
    base = (1e3 * rng.standard_normal(N)).astype(f32)
    out.append(base.copy())                                                          # plain
    out.append(np.zeros(N, f32))                                                     # all ties
    out.append(rng.integers(0, 4, N).astype(f32))                                    # many ties
    for specials in ([np.nan], [np.nan] * 3, [np.inf, -np.inf], [0.0, -0.0, 0.0, -0.0], [np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan],
                     [-np.nan, np.nan, np.inf, np.inf], [1e-45, -1e-45, 0.0, -0.0]):
        for _ in range(3):
            s = base.copy() if rng.random() < 0.7 else rng.integers(-1, 2, N).astype(f32)
            where = rng.choice(N, min(len(specials), N), replace=False)
            s[where] = np.asarray(specials, f32)[:len(where)]
            out.append(s)
    s = base.copy()                                                                  # a NaN with a payload and a set sign bit
    s.view(np.uint32)[0] = 0xFFC12345
    out.append(s)
    out.append(np.full(N, np.nan, f32))
    return out


@pytest.mark.parametrize("N", [1, 2, 37, 200, 300])
def test_ordered_keys_reproduce_stable_argsort(N):
    for best_k in sorted({1, min(40, N), N}):
        for i, S in enumerate(cost_vectors(N, 100 + N)):
            want = np.argsort(S, kind="stable")[:best_k]
            got = O.bitonic_topk(S, best_k)
            assert np.array_equal(got, want), (N, best_k, i)
            assert got.max() < N
            assert np.array_equal(O.cem_update(S, np.zeros((N, 1), f32), best_k, 0.0)[2], want)


def test_ordered_keys_are_monotone():
    v = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf, np.nan], f32)
    k = O.topk_key_ordered(v, 16)
    assert k.dtype == np.uint32 and np.all(np.diff(k[:9].astype(np.int64))[[0, 1, 2, 4, 5, 6, 7]] > 0) and k[3] == k[4]
    assert np.all(k[9:] == 0xFFFFFFFF) and k[8] < 0xFFFFFFFF
    odd = np.array([np.nan, np.nan], f32)
    odd.view(np.uint32)[:] = [0xFFC12345, 0x7F800001]                                # any NaN, either sign, any payload
    assert np.all(O.topk_key_ordered(odd, 2) == k[8])


def test_float_comparator_with_inf_padding_breaks_on_nan():
    """What the kernel did before: costs as float keys, +inf padding, (ki > kl) || (ki == kl && ii > il).  Correct without NaN; with
    NaNs and best_k = N a padded index (>= N: an out-of-bounds row of Q on the device) enters the elite."""
    old = dict(make_key=O.topk_key_float, gt=O.topk_gt_float)
    rng = np.random.Generator(np.random.SFC64(5))
    for N, best_k in [(37, 37), (200, 40), (300, 300)]:
        S = rng.standard_normal(N).astype(f32)
        S[rng.choice(N, 5, replace=False)] = [np.inf, -np.inf, 0.0, -0.0, np.inf]
        assert np.array_equal(O.bitonic_topk(S, best_k, **old), np.argsort(S, kind="stable")[:best_k])
    N, padded, wrong = 37, 0, 0
    for _ in range(20):
        S = rng.standard_normal(N).astype(f32)
        S[rng.choice(N, 2, replace=False)] = np.nan
        got = O.bitonic_topk(S, N, **old)
        padded += int((got >= N).any())
        wrong += int(not np.array_equal(got, np.argsort(S, kind="stable")))
        assert np.array_equal(O.bitonic_topk(S, N), np.argsort(S, kind="stable"))
    assert padded > 0 and wrong > 0
