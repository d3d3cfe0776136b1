"""CPU: the numpy restatement of Philox4x32-10 (oracle/philox_np.py) against the known-answer vectors Random123 publishes for
`philox4x32 10` (its kat_vectors file; Salmon et al., SC 2011), and the properties of the sampler's uniforms and normals."""
import numpy as np

from oracle import philox_np as P


def test_random123_known_answer_vectors():
    kat = [  # counter (4 words), key (2 words) -> output (4 words)
        ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        got = P.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert tuple(int(x) for x in got) == want, (ctr, [hex(int(x)) for x in got])
    # vectorised = one at a time
    ctr = np.array([k[0] for k in kat], np.uint32)
    key = np.array([k[1] for k in kat], np.uint32)
    assert np.array_equal(P.philox4x32_10(ctr, key), np.array([k[2] for k in kat], np.uint32))


def test_bijection_and_counter_sensitivity():
    rng = np.random.Generator(np.random.SFC64(1))
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    key = np.array([123, 456], np.uint32)
    out = P.philox4x32_10(ctr, key)
    assert len({tuple(r) for r in out}) == 4096                                     # distinct counters -> distinct blocks
    flip = ctr.copy()
    flip[:, 2] ^= 1                                                                 # one counter bit flips about half of the output bits
    bits = np.unpackbits((out ^ P.philox4x32_10(flip, key)).view(np.uint8)).mean()
    assert 0.49 < bits < 0.51


def test_sampler_uniforms_and_normals():
    ua, ub, uc, ud = P.quad_uniforms(1234, 7, np.arange(8)[:, None, None], np.arange(512)[None, :, None], np.arange(3)[None, None, :])
    for u, lo_open in ((ua, True), (uc, True), (ub, False), (ud, False)):
        assert (u > 0).all() and (u <= 1).all() if lo_open else ((u >= 0).all() and (u < 1).all())
        assert np.array_equal(u, u.astype(np.float32).astype(np.float64))           # 24 bits: exact in float32
        assert abs(u.mean() - 0.5) < 0.01
    z = P.standard_normal_quads(1234, 7, np.arange(8)[:, None, None], np.arange(2048)[None, :, None], np.arange(3)[None, None, :])
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs((z ** 4).mean() - 3.0) < 0.1
    kn = P.knots(1234, 7, 100, 2, 64, 6, 0.2121)
    assert kn.shape == (2, 64, 6) and kn.dtype == np.float32
    # the global env index keys the stream: env_offset 100 + env 1 == env_offset 101 + env 0; steps and seeds give fresh streams
    assert np.array_equal(kn[1], P.knots(1234, 7, 101, 1, 64, 6, 0.2121)[0])
    assert not np.array_equal(kn, P.knots(1234, 8, 100, 2, 64, 6, 0.2121)) and not np.array_equal(kn, P.knots(1235, 7, 100, 2, 64, 6, 0.2121))
    # the high words of seed and step counter enter the key
    assert not np.array_equal(P.knots(1234 + (1 << 32), 7, 0, 1, 8, 6, 1.0), P.knots(1234, 7, 0, 1, 8, 6, 1.0))
    assert not np.array_equal(P.knots(1234, 7 + (1 << 32), 0, 1, 8, 6, 1.0), P.knots(1234, 7, 0, 1, 8, 6, 1.0))


def test_pair_stream_keying():
    """The CEM samplers' blocks: counter (rollout, global env, pair, offset lo), key (seed lo, seed hi ^ offset hi) with no XOR constant -
    stated through philox4x32_10, which the Random123 vectors above pin."""
    seed, offset = (0x1234 << 32) | 0x9ABCDEF0, (0x5 << 32) | 0x77
    env, n, pair = np.arange(3)[:, None, None] + 123456, np.arange(5)[None, :, None], np.arange(4)[None, None, :]
    w = P.pair_words(seed, offset, env, n, pair)
    assert w.shape == (3, 5, 4, 4) and w.dtype == np.uint32
    for e, r, j in [(0, 0, 0), (2, 4, 3), (1, 3, 2)]:
        want = P.philox4x32_10(np.array([r, 123456 + e, j, 0x77], np.uint32), np.array([0x9ABCDEF0, 0x1234 ^ 0x5], np.uint32))
        assert np.array_equal(w[e, r, j], want)
    # not the fused step's stream: same arguments, other key
    assert not np.array_equal(w, P.quad_words(seed, offset, env, n, pair))
    assert np.array_equal(P.quad_words(seed ^ P.QUAD_KEY_XOR, offset, env, n, pair), w)
    # normals from words 0 and 1 only, with the quad stream's 24-bit uniforms
    z = P.standard_normal_pairs(seed, offset, env, n, pair)
    u1, u2 = ((w[..., 0].astype(np.uint64) >> np.uint64(8)) + np.uint64(1)) * 2.0 ** -24, (w[..., 1].astype(np.uint64) >> np.uint64(8)) * 2.0 ** -24
    assert z.shape == (3, 5, 4, 2) and z.dtype == np.float64
    np.testing.assert_array_equal(z[..., 0], np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2))
    np.testing.assert_array_equal(z[..., 1], np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2))
    zz = P.standard_normal_pairs(7, 1, np.arange(4)[:, None, None], np.arange(2048)[None, :, None], np.arange(4)[None, None, :])
    assert abs(zz.mean()) < 0.01 and abs(zz.std() - 1.0) < 0.01 and abs((zz ** 4).mean() - 3.0) < 0.1


def test_cem_samples_and_gmm_components():
    rng = np.random.Generator(np.random.SFC64(2))
    E, N, H = 2, 64, 5                                                              # odd H: the sine of the last pair is unused
    mean, sd = rng.uniform(-0.3, 0.3, (E, H)).astype(np.float32), rng.uniform(0.1, 0.5, (E, H)).astype(np.float32)
    seed, offset = 2 ** 40 + 5, 2 ** 33 + 11
    q = P.cem_samples(mean, sd, seed, offset, 100, N, -0.5, 0.8)
    assert q.shape == (E, N, H) and q.dtype == np.float64 and q.min() >= -0.5 and q.max() <= float(np.float32(0.8))
    assert (q == -0.5).any() and (q == float(np.float32(0.8))).any()
    z = P.standard_normal_pairs(seed, offset, 101, np.arange(N)[:, None], np.arange(3)[None, :]).reshape(N, 6)[:, :H]
    want = np.clip(mean[1].astype(np.float64) + sd[1].astype(np.float64) * z.astype(np.float32), -0.5, float(np.float32(0.8)))
    np.testing.assert_array_equal(q[1], want)
    # the global env index keys the stream: env_offset 100 with env 1 == env_offset 101 with env 0
    assert np.array_equal(q[1], P.cem_samples(mean[1:], sd[1:], seed, offset, 101, N, -0.5, 0.8)[0])
    assert not np.array_equal(q[0], P.cem_samples(mean[:1], sd[:1], seed, offset, 101, N, -0.5, 0.8)[0])
    assert not np.array_equal(q, P.cem_samples(mean, sd, seed, offset + 1, 100, N, -0.5, 0.8))
    assert not np.array_equal(q, P.cem_samples(mean, sd, seed, offset - 2 ** 33, 100, N, -0.5, 0.8))         # offset's high word
    # H = 1: one pair, its cosine only
    q1 = P.cem_samples(mean[:, :1], sd[:, :1], seed, offset, 100, N, -9.0, 9.0)
    z1 = P.standard_normal_pairs(seed, offset, 100, np.arange(N), 0)[:, 0].astype(np.float32)
    np.testing.assert_array_equal(q1[0, :, 0], np.float64(mean[0, 0]) + np.float64(sd[0, 0]) * z1)
    for K in (1, 3, 8):
        c = P.gmm_components(seed, offset, 100, E, 4096, K)
        assert c.shape == (E, 4096) and c.min() == 0 and c.max() == K - 1
        w0 = P.pair_words(seed, offset, 101, np.arange(4096), 0x80000000)[:, 0]
        assert np.array_equal(c[1], [(int(w) * K) >> 32 for w in w0])
        assert np.abs(np.bincount(c.ravel(), minlength=K) - 2 * 4096 / K).max() <= 5 * np.sqrt(2 * 4096 / K)
        assert np.array_equal(c[1], P.gmm_components(seed, offset, 101, 1, 4096, K)[0])
    centres = rng.uniform(-0.4, 0.4, (E, 3, H)).astype(np.float32)
    qg, comp = P.cem_gmm_samples(centres, sd, seed, offset, 100, N, -0.5, 0.8)
    assert np.array_equal(comp, P.gmm_components(seed, offset, 100, E, N, 3))
    for e, n in [(0, 0), (1, 17), (1, 63)]:
        np.testing.assert_array_equal(qg[e, n], P.cem_samples(centres[e, comp[e, n]][None], sd[e][None], seed, offset, 100 + e, N, -0.5, 0.8)[0, n])
