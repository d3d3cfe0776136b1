"""Philox4x32-10 and the device sampler's keying, restated in numpy - the pin of the library's own noise stream.

TEST INFRASTRUCTURE (only tests/, bench.py's verify leg and __graft_entry__.smoke may import it).  The reference draws its
perturbations from numpy's SFC64 on the host (Control_Toolkit_ASF/Controllers/controller_mppi_cartpole.py:351, :434-446); parity with
the reference is defined on IDENTICAL perturbations and tested with SFC64 knots fed from the host.  The in-kernel
generator exists for throughput only - but a bench line that says "Philox4x32-10" should be able to prove it: this file restates
  * the Philox4x32-10 bijection of Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC 2011), Random123
    1.x `philox4x32_R(10, ctr, key)`: ten rounds of (hi, lo) = M * c with M0 = 0xD2511F53 on c0 and M1 = 0xCD9E8D57 on c2, output
    (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), key bumped by (0x9E3779B9, 0xBB67AE85) between rounds - checked against the known-answer
    vectors Random123 ships (tests/test_oracle_philox.py);
  * the sampler's counter / key layout and its Box-Muller (cartpolesimulation_amd/csrc/cpmppi_philox.hpp, philox_normal_quad /
    philox_normal_pair): counter = (rollout, GLOBAL env index, knot quad, low word of the step counter), key = (seed_lo ^ 0x51ed270b,
    seed_hi ^ high word of the step counter); words -> uniforms ua, uc in (0, 1] and ub, ud in [0, 1) with 24 bits each; knots
    4q .. 4q+3 = sigma * (ra cos 2 pi ub, ra sin 2 pi ub, rc cos 2 pi ud, rc sin 2 pi ud), r = sqrt(-2 ln u).
The device evaluates ln / sin / cos with the hardware's v_log_f32 / v_sin_f32 / v_cos_f32 (absolute error ~1e-6); here they are
evaluated in float64 and rounded once: the test bound on the normals is that hardware error, the uniforms behind them are exact.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
QUAD_KEY_XOR = 0x51ED270B
f32 = np.float32


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32, broadcastable) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bit products (no overflow in uint64)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _uniforms(words):
    """Four words -> (ua, ub, uc, ud): 24 bits each; a, c in (0, 1], b, d in [0, 1).  Exact in float32."""
    w = words.astype(np.uint64)
    s = 5.9604644775390625e-8                             # 2^-24
    return ((w[..., 0] >> np.uint64(8)) + np.uint64(1)) * s, (w[..., 1] >> np.uint64(8)) * s, \
           ((w[..., 2] >> np.uint64(8)) + np.uint64(1)) * s, (w[..., 3] >> np.uint64(8)) * s


def quad_words(seed, offset, env, rollout, quad):
    """The Philox block behind knots 4 quad .. 4 quad + 3 of (global env, rollout) at step `offset` (philox_normal_quad)."""
    seed, offset = int(seed), int(offset)
    env, rollout, quad = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(rollout, np.uint64), np.asarray(quad, np.uint64))
    ctr = np.stack([rollout, env, quad, np.full(env.shape, offset & 0xFFFFFFFF, np.uint64)], axis=-1)
    key = np.array([(seed & 0xFFFFFFFF) ^ QUAD_KEY_XOR, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)


def quad_uniforms(seed, offset, env, rollout, quad):
    return _uniforms(quad_words(seed, offset, env, rollout, quad))


def standard_normal_quads(seed, offset, env, rollout, quad):
    """-> [..., 4] float64: the four standard normals of a block, before any rounding."""
    ua, ub, uc, ud = quad_uniforms(seed, offset, env, rollout, quad)
    ra, rc = np.sqrt(-2.0 * np.log(ua)), np.sqrt(-2.0 * np.log(uc))
    return np.stack([ra * np.cos(2 * np.pi * ub), ra * np.sin(2 * np.pi * ub), rc * np.cos(2 * np.pi * ud), rc * np.sin(2 * np.pi * ud)], axis=-1)


def knots(seed, offset, env_offset, E, N, P, sigma):
    """What cpmppi_sample(seed, offset, env_offset) writes: knots[E, N, P] float32 = float32(sigma) * float32(z)."""
    nq = (P + 3) // 4
    e = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset))[:, None, None]
    n = np.arange(N, dtype=np.uint64)[None, :, None]
    q = np.arange(nq, dtype=np.uint64)[None, None, :]
    z = standard_normal_quads(seed, offset, e, n, q).reshape(E, N, nq * 4)[:, :, :P]
    return (f32(sigma) * z.astype(f32)).astype(f32)


# --------------------------------------------------------------------------------------------------------------------
# The CEM samplers' stream (cpmppi_philox.hpp, philox_normal_pair; cpmppi_optim.hip, cem_sample_kernel / cem_gmm_sample_kernel):
# counter = (rollout, GLOBAL env index, step pair, low word of the offset), key = (seed_lo, seed_hi ^ high word of the offset) - NO
# XOR constant on the low key word, and only words 0 and 1 of the block are used: time-steps 2 pair and 2 pair + 1 are
# r (cos 2 pi u2, sin 2 pi u2), r = sqrt(-2 ln u1), with the 24-bit uniforms of _uniforms.
GMM_COMPONENT_PAIR = 0x80000000                           # counter word 2 of the block that picks a rollout's mixture component


def pair_words(seed, offset, env, rollout, pair):
    """The Philox block behind time-steps 2 pair, 2 pair + 1 of (global env, rollout) at `offset` (philox_normal_pair)."""
    seed, offset = int(seed), int(offset)
    env, rollout, pair = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(rollout, np.uint64), np.asarray(pair, np.uint64))
    ctr = np.stack([rollout, env, pair, np.full(env.shape, offset & 0xFFFFFFFF, np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)


def standard_normal_pairs(seed, offset, env, rollout, pair):
    """-> [..., 2] float64: the two standard normals of a block (words 0 and 1), before any rounding."""
    u1, u2, _, _ = _uniforms(pair_words(seed, offset, env, rollout, pair))
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], axis=-1)


def _cem_normals(seed, offset, env_offset, E, N, H):
    e = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset))[:, None, None]
    n = np.arange(N, dtype=np.uint64)[None, :, None]
    j = np.arange((H + 1) // 2, dtype=np.uint64)[None, None, :]
    return standard_normal_pairs(seed, offset, e, n, j).reshape(E, N, -1)[:, :, :H].astype(f32)      # (odd H: sin of the last pair unused)


def cem_samples(mean, stdev, seed, offset, env_offset, N, lo=-1.0, hi=1.0):
    """What cpmppi_cem_sample writes, in float64: [E, N, H] = clip(mean[e, k] + stdev[e, k] * float32(z), lo, hi)."""
    mean, stdev = np.asarray(mean, np.float64), np.asarray(stdev, np.float64)
    E, H = mean.shape
    z = _cem_normals(seed, offset, env_offset, E, N, H).astype(np.float64)
    return np.clip(mean[:, None, :] + stdev[:, None, :] * z, float(f32(lo)), float(f32(hi)))


def gmm_components(seed, offset, env_offset, E, N, K):
    """The mixture component of every rollout as cpmppi_cem_gmm_sample picks it: [E, N] = (word 0 * K) >> 32 of the block with counter
    word 2 = GMM_COMPONENT_PAIR (never a real pair index).  Integer-exact."""
    e = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset))[:, None]
    n = np.arange(N, dtype=np.uint64)[None, :]
    w0 = pair_words(seed, offset, e, n, GMM_COMPONENT_PAIR)[..., 0].astype(np.uint64)
    return ((w0 * np.uint64(K)) >> np.uint64(32)).astype(np.int64)


def cem_gmm_samples(centres, stdev, seed, offset, env_offset, N, lo=-1.0, hi=1.0):
    """What cpmppi_cem_gmm_sample writes, in float64: (Q [E, N, H], components [E, N]) - the centre of the rollout's component plus the
    plain CEM sampler's noise for the same (seed, offset)."""
    centres, stdev = np.asarray(centres, np.float64), np.asarray(stdev, np.float64)
    E, K, H = centres.shape
    comp = gmm_components(seed, offset, env_offset, E, N, K)
    z = _cem_normals(seed, offset, env_offset, E, N, H).astype(np.float64)
    Q = centres[np.arange(E)[:, None], comp] + stdev[:, None, :] * z
    return np.clip(Q, float(f32(lo)), float(f32(hi))), comp
