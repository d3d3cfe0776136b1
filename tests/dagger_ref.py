"""TEST INFRASTRUCTURE: what cpmppi_dagger_step computes besides the network, restated on the host (include/cpmppi.h states it).

The gate is one Philox4x32-10 block of the library's own stream (oracle/philox_np.py): the sampler's quad block of rollout index
0xFFFFFFFF, quad 0 - counter (0xFFFFFFFF, env_offset + e, 0, low word of c), key (seed_lo ^ 0x51ed270b, seed_hi ^ high word of c) -,
word 1 as a 24-bit uniform in [0, 1); the expert drives iff that uniform is below beta.  Integer-exact up to the comparison, which is
one of float32 values on both sides."""
import numpy as np

from oracle import philox_np as P

f32 = np.float32
GATE_ROLLOUT = 0xFFFFFFFF


def gate_uniform(seed, env_offset, E, c):
    """-> ub [E] float32 (exact: 24 bits), the uniform of env_offset + e at period c."""
    env = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(0xFFFFFFFF)
    ctr = np.stack([np.full(E, GATE_ROLLOUT, np.uint64), env, np.zeros(E, np.uint64), np.full(E, int(c) & 0xFFFFFFFF, np.uint64)], axis=-1)
    key = np.array([(int(seed) & 0xFFFFFFFF) ^ P.QUAD_KEY_XOR, ((int(seed) >> 32) ^ (int(c) >> 32)) & 0xFFFFFFFF], np.uint64)
    words = P.philox4x32_10(ctr, key)
    return ((words[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(f32)


def gate(seed, env_offset, E, c, beta):
    """-> [E] bool: the expert drives.  ``beta``: a scalar or [E]; a NaN never lets it."""
    beta = np.broadcast_to(np.asarray(beta, f32), (E,))
    with np.errstate(invalid="ignore"):
        return gate_uniform(seed, env_offset, E, c) < beta


def applied(gate_, Q_expert, Q_imitator):
    """-> what the plant is handed: a selection, no arithmetic (a NaN passes where it is chosen)."""
    return np.where(gate_, np.asarray(Q_expert, f32), np.asarray(Q_imitator, f32)).astype(f32)


def sq_err(start, Q_imitator_calls, Q_expert_calls):
    """The recurrence of the disagreement in float64, call by call: s <- s + d * d, d = float64(imitator) - float64(expert)."""
    s = np.array(start, np.float64, copy=True)
    for qi, qe in zip(Q_imitator_calls, Q_expert_calls):
        d = np.asarray(qi, f32).astype(np.float64) - np.asarray(qe, f32).astype(np.float64)
        s = s + d * d
    return s
