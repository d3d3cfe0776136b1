"""Error recovery of the env groups' all-gather (cpmppi_groups_run_gather, include/cpmppi.h): what a call that fails part-way, a
finalize that times out and a lagging group leave behind, checked against the plain EnvGroups loop without a communicator (the
yardstick of test_gpu_pipeline.py) and against the communicator's own flag blocks (cpmppi_debug_comm_flags).

One rank on real RCCL.  Every device-side wait here is bounded by the handle's own timeout."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, H, NSUB, ROWS = 512, 20, 10, 8
STEP, GUARD, PLANT = 1, 2, 3                  # cpmppi_debug_groups_fail: which call of the group fails
ERR_BAD_ARG, ERR_HIP, ERR_COMM = -1, -4, -6
OFFSET = 100                                  # Philox step counter of the first period of every chain here


def _inputs(E, seed):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synthetic_inputs
    return synthetic_inputs(E, H, seed, torch.device("cuda", 0))


def _cfg():
    from cartpolesimulation_amd.configs import MPPIConfig
    return MPPIConfig(num_rollouts=N, mpc_horizon=H, rollouts_per_lane=1)


def _h0(g):
    return C.c_void_p(g.lib.cpmppi_groups_handle(g._g, 0))


def _flags(g):
    """[2, 16] uint32: the communicator's two flag blocks ([0] envs arrived, [1] step published, [2] gathers completed, [3] error)."""
    out = (C.c_uint32 * 32)()
    assert g.lib.cpmppi_debug_comm_flags(_h0(g), out) == 0
    return np.array(out, dtype=np.uint32).reshape(2, 16)


def _assert_idle(g):
    """Device idle and cpmppi_comm_sync returned: no arrival left in either counter, no error word up, no step published that no
    gather was enqueued for (the kernel waiter's published words; signal memory in the stream-operation form is not in the blocks)."""
    torch.cuda.synchronize()
    f = _flags(g)
    assert f[:, 0].tolist() == [0, 0], f"arrival counters left over: {f[:, 0].tolist()}"
    assert f[:, 3].tolist() == [0, 0], f"error words up: {f[:, 3].tolist()}"
    if g.comm_info()["stream_memory_ops"] == 0:
        assert int(f[:, 1].max()) <= g.comm_info()["gathers_enqueued"], f"published {f[:, 1].tolist()} past the gathers enqueued"


def _comm_groups(E, groups, waiter, monkeypatch, timeout_s=None):
    from cartpolesimulation_amd import _lib as L
    from cartpolesimulation_amd.pipeline import EnvGroups
    monkeypatch.setenv("CPMPPI_COMM_WAITER", waiter)
    g = EnvGroups(E, _cfg(), groups, env_offset=40)
    uid = C.create_string_buffer(L.COMM_ID_BYTES)
    assert g.lib.cpmppi_comm_unique_id(uid, None) == 0, g.lib.cpmppi_last_error(None)
    g.comm_init(uid.raw, 1, 0, stamped=True, timeout_s=timeout_s)
    assert g.lib.cpmppi_debug_comm_mode(_h0(g)) == (1 if waiter == "stream-ops" else 0)
    return g


class _Chain:
    """The buffers of one closed loop over all E envs - plant state s, control Q, control log, two stamped nominal-sequence buffers -
    with the argument blocks of `g` over them.  reset() puts the known initial state back."""

    def __init__(self, g, E, seed, plant=True):
        from cartpolesimulation_amd import _lib as L
        self.g, self.E, self.n = g, E, E * H
        self.s0, self.tp, self.te, self.Lt = _inputs(E, seed)
        dev = self.s0.device
        self.s, self.Q = self.s0.clone(), torch.zeros(E, device=dev)
        self.Q_log = torch.zeros(ROWS, E, device=dev)
        self.flat = [torch.zeros(self.n + L.GATHER_STAMP_FLOATS, device=dev) for _ in range(2)]
        self.u = [f[:self.n].view(E, H) for f in self.flat]
        kw = dict(L=self.Lt, seed=91, Q_out=self.Q)
        self.alt = [g.prepare(self.s, self.u[b], self.tp, self.te, u_nom_out=self.u[1 - b], **kw) for b in range(2)]
        self.inplace = [g.prepare(self.s, self.u[b], self.tp, self.te, **kw) for b in range(2)]
        self.plant = g.args_engine.prepare_plant_step(self.s, self.Q, NSUB, Q_log=self.Q_log) if plant else None

    def reset(self, u=None):
        """Known state (u: the nominal sequences to start from, default zeros) in buffer 0; the group streams wait for it."""
        g = self.g
        g.join()
        torch.cuda.synchronize()
        self.s.copy_(self.s0)
        self.Q.zero_()
        self.Q_log.zero_()
        for f in self.flat:
            f.zero_()
        if u is not None:
            self.u[0].copy_(u)
        g.fork()

    def lag(self, group):
        """Hold `group`'s stream back by a few milliseconds: a gather that leaves before that group has written reads its old block."""
        with torch.cuda.stream(self.g.streams[group]):
            torch.cuda._sleep(10_000_000)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.s, self.Q, self.Q_log, self.flat[0], self.flat[1])]

    def equals(self, snap):
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip((self.s, self.Q, self.Q_log, self.flat[0], self.flat[1]), snap))


def _plain(E, groups, seed, periods, plant=True):
    """The yardstick: the same groups WITHOUT a communicator, in place, from the known state -> [u after period j] and the final
    (s, Q).  Period j runs with the Philox counter OFFSET + j and the plant period j."""
    from cartpolesimulation_amd.pipeline import EnvGroups
    s0, tp, te, Lt = _inputs(E, seed)
    p = EnvGroups(E, _cfg(), groups, env_offset=40)
    s, Q, Q_log = s0.clone(), torch.zeros(E, device=s0.device), torch.zeros(ROWS, E, device=s0.device)
    uu = torch.zeros(E, H, device=s0.device)
    sp = p.prepare(s, uu, tp, te, L=Lt, seed=91, Q_out=Q)
    pp = p.args_engine.prepare_plant_step(s, Q, NSUB, Q_log=Q_log) if plant else None
    p.fork()
    want = []
    for j in range(periods):
        p.run(sp, pp, periods=1, offset=OFFSET + j, period=j)
        p.join()
        want.append(uu.clone())
        p.fork()                                               # (the next period waits for the copy)
    torch.cuda.synchronize()
    out = want, s.clone(), Q.clone()
    p.close()
    return out


def _recovery(ch, want, final=None, first=0, alt=4, inplace=3):
    """From the known state: `alt` periods with alternating buffers, then `inplace` periods in place, one call each, the LAST group
    held back before the first call of each form.  Every gathered block must be the plain loop's, with consecutive stamps."""
    from cartpolesimulation_amd.shard import block_stamps
    g, n, last = ch.g, ch.n, len(ch.g) - 1
    base = g.comm_info()["gathers_enqueued"]
    K = alt + inplace
    recv = torch.zeros(K, 1, ch.flat[0].numel(), device=ch.s.device)
    ch.lag(last)
    for j in range(alt):                                       # period j reads u[j & 1], writes u[(j + 1) & 1]
        g.run(ch.alt[j & 1], ch.plant, periods=1, offset=OFFSET + first + j, period=first + j, gather_into=recv[j])
    ch.lag(last)
    for j in range(alt, K):
        g.run(ch.inplace[alt & 1], ch.plant, periods=1, offset=OFFSET + first + j, period=first + j, gather_into=recv[j])
    g.join()
    torch.cuda.synchronize()
    g.comm_sync()
    for j in range(K):
        assert torch.equal(recv[j, 0, :n].view(ch.E, H), want[first + j]), f"recovery: gather {j} is not period {first + j}'s result"
    stamps = torch.stack([block_stamps(recv[j], n) for j in range(K)]).view(-1).tolist()
    assert stamps == list(range(base + 1, base + K + 1)), f"recovery: stamps {stamps}"
    assert torch.equal(ch.u[alt & 1], want[first + K - 1])
    if final is not None:
        assert torch.equal(ch.s, final[0]) and torch.equal(ch.Q, final[1])
    _assert_idle(g)


CASES = [(8, 2), (9, 3)]
WAITERS = ["kernel", "stream-ops"]


@pytest.mark.parametrize("waiter", WAITERS)
@pytest.mark.parametrize("E,groups", CASES)
def test_gather_leaves_only_after_the_last_group_has_written(E, groups, waiter, monkeypatch):
    """No failure: the last group's stream is held back by milliseconds before each form of the chain, so the groups drift far
    apart; every gather still carries every group's new sequences (it never leaves before the last env has published)."""
    want, s, Q = _plain(E, groups, 11, 7)
    g = _comm_groups(E, groups, waiter, monkeypatch)
    ch = _Chain(g, E, 11)
    ch.reset()
    _recovery(ch, want, final=(s, Q))
    ch.reset()
    _recovery(ch, want, final=(s, Q))                          # the second time round both parities hold history
    g.close()


@pytest.mark.parametrize("waiter", WAITERS)
@pytest.mark.parametrize("E,groups", CASES)
def test_plant_period_past_the_control_log_is_refused_before_any_launch(E, groups, waiter, monkeypatch):
    """step + plant over 3 periods whose last plant period lies outside Q_log (plant.period + 2 == ctrl_rows): refused as a bad
    argument with NOTHING enqueued - no gather numbered, no buffer written, cpmppi_comm_sync clean, the flag blocks idle - and the
    next valid call runs normally.  (Before: periods 0 and 1 ran, group 0's step of period 2 was out when its plant call failed,
    and its arrivals stayed in the counter.)"""
    from cartpolesimulation_amd import _lib as L
    want, s, Q = _plain(E, groups, 12, 7)
    g = _comm_groups(E, groups, waiter, monkeypatch)
    ch = _Chain(g, E, 12)
    ch.reset()
    _recovery(ch, want)                                        # some history in both parities and in both buffers
    ch.reset()
    before, snap = g.comm_info()["gathers_enqueued"], ch.snapshot()
    recv = torch.zeros(1, ch.flat[0].numel(), device=ch.s.device)
    with pytest.raises(L.CpmppiError) as ei:
        g.run(ch.alt[0], ch.plant, periods=3, offset=OFFSET, period=ROWS - 2, gather_into=recv)
    assert ei.value.code == ERR_BAD_ARG and "ctrl_rows" in str(ei.value)
    assert g.comm_info()["gathers_enqueued"] == before, "a refused call numbered gathers"
    assert ch.equals(snap) and not recv.any(), "a refused call wrote a buffer"
    g.comm_sync()
    _assert_idle(g)
    ch.reset()
    _recovery(ch, want, final=(s, Q))
    g.close()


def _inject(ch, what, group, k, want):
    """One 3-period call of step + plant from the known state with group `group`'s `what` call of period k failing.  -> whether a
    launch of period k was out (the communicator is then poisoned)."""
    from cartpolesimulation_amd import _lib as L
    from cartpolesimulation_amd.shard import block_stamps
    g, n = ch.g, ch.n
    ch.reset()
    base = g.comm_info()["gathers_enqueued"]
    recv = torch.zeros(1, ch.flat[0].numel(), device=ch.s.device)
    assert g.lib.cpmppi_debug_groups_fail(g._g, what, group, k) == 0
    with pytest.raises(L.CpmppiError) as ei:
        g.run(ch.alt[0], ch.plant, periods=3, offset=OFFSET, period=0, gather_into=recv)
    assert ei.value.code == ERR_HIP and "injected" in str(ei.value)
    out = what == PLANT or group > 0                           # group 0's step of period k (at least) was enqueued
    g.join()
    torch.cuda.synchronize()
    if out:
        with pytest.raises(L.CpmppiError) as ei:               # refused until cpmppi_comm_sync
            g.run(ch.alt[0], ch.plant, periods=1, offset=OFFSET, period=0, gather_into=recv)
        assert ei.value.code == ERR_COMM
        with pytest.raises(L.CpmppiError) as ei:               # reported once ...
            g.comm_sync()
        assert ei.value.code == ERR_COMM
    g.comm_sync()                                              # ... and cleared (no launch out: nothing to report)
    assert g.comm_info()["gathers_enqueued"] == base + k
    if k > 0:                                                  # the complete periods before k ran, stamped and gathered as usual
        assert torch.equal(recv[0, :n].view(ch.E, H), want[k - 1]), "the last complete period's gather"
        assert block_stamps(recv, n).tolist() == [base + k]
        assert torch.equal(ch.u[k & 1], want[k - 1]), "the buffer the last complete period wrote"
    else:
        assert not recv.any()
    _assert_idle(g)
    return out


@pytest.mark.parametrize("what", [STEP, GUARD, PLANT], ids=["step", "guard", "plant"])
@pytest.mark.parametrize("waiter", WAITERS)
@pytest.mark.parametrize("E,groups", CASES)
def test_failed_launch_inside_a_period_poisons_and_recovers_exactly(E, groups, waiter, what, monkeypatch):
    """A step, gather-guard or plant call that fails inside a period (test hook cpmppi_debug_groups_fail, as a HIP launch error
    would), for the first and the last group, in the first and the third period of a 3-period call.  Where a launch of that
    period was already out the communicator is poisoned: the call raises, the gathers of the periods before it are the plain loop's
    with their stamps, the next call is refused with CPMPPI_ERR_COMM, cpmppi_comm_sync reports once and leaves the flag blocks idle;
    where none was out (step or guard of group 0) cpmppi_comm_sync is clean.  After each failure a chain from the known state,
    with the last group held back, is the plain loop bit for bit in both buffer forms."""
    want, s, Q = _plain(E, groups, 13, 7)
    g = _comm_groups(E, groups, waiter, monkeypatch)
    ch = _Chain(g, E, 13)
    for group in (0, len(g) - 1):
        for k in (0, 2):
            _inject(ch, what, group, k, want)
            ch.reset()
            _recovery(ch, want, final=(s, Q))
    g.close()


@pytest.mark.parametrize("waiter", WAITERS)
def test_finalize_timeout_drops_every_later_period_of_both_parities(waiter, monkeypatch):
    """Env groups, alternating buffers, stamped; timeout T = 20 ms.  Gather 0 joins D = 30 ms late (T < D < 2T): period 2's finalize
    waits for it, gives up and drops its store; period 3 waits for gather 1, which completes shortly after gather 0 - it must find
    the error up (raised in BOTH parity blocks) and drop too, as must every later period: no buffer changes after the timeout, the
    next call is refused, cpmppi_comm_sync reports once, the late gathers carry the old stamp, and a clean run from the surviving
    buffers is the plain loop bit for bit."""
    from cartpolesimulation_amd import _lib as L
    from cartpolesimulation_amd.shard import block_stamps
    E, groups = 8, 2
    want, _, _ = _plain(E, groups, 14, 9, plant=False)
    g = _comm_groups(E, groups, waiter, monkeypatch, timeout_s=0.020)
    h0 = _h0(g)
    ch = _Chain(g, E, 14, plant=False)
    n = ch.n
    ch.reset()
    recv = torch.zeros(2, 1, ch.flat[0].numel(), device=ch.s.device)
    assert g.lib.cpmppi_debug_comm_delay(h0, 30000) == 0
    g.run(ch.alt[0], None, periods=1, offset=OFFSET, gather_into=recv[0])          # period 0: u[0] -> u[1]; its gather is late
    assert g.lib.cpmppi_debug_comm_delay(h0, 0) == 0
    g.run(ch.alt[1], None, periods=5, offset=OFFSET + 1, gather_into=recv[1])      # periods 1..5: u[1] -> u[0] -> u[1] ...
    g.join()
    torch.cuda.synchronize()
    # period 1 (no wait: the buffer it writes was never gathered) is the last that stores; 2..5 drop, whichever parity
    assert torch.equal(ch.u[1], want[0]), "a period after the timeout overwrote period 0's buffer"
    assert torch.equal(ch.u[0], want[1]), "a period after the timeout overwrote period 1's buffer"
    with pytest.raises(L.CpmppiError) as ei:
        g.run(ch.alt[0], None, periods=1, offset=OFFSET + 6, gather_into=recv[1])
    assert ei.value.code == ERR_COMM and "timed out" in str(ei.value)
    with pytest.raises(L.CpmppiError) as ei:
        g.comm_sync()
    assert ei.value.code == ERR_COMM
    g.comm_sync()
    assert g.comm_info()["gathers_enqueued"] == 6
    assert torch.equal(recv[0, 0, :n].view(E, H), want[0]) and block_stamps(recv[0], n).tolist() == [1]
    # gather 6 sent u[0] as period 1 left it; its stamp is the buffer's old one (gather 1 ran after the error: none), never 6
    assert torch.equal(recv[1, 0, :n].view(E, H), want[1])
    old = int(ch.flat[0][n:n + 1].view(torch.int32).item())
    assert block_stamps(recv[1], n).tolist() == [old] and old < 2
    _assert_idle(g)
    assert g.lib.cpmppi_comm_set_timeout(h0, 10.0) == 0
    survivor = ch.u[0].clone()                                 # period 1's result: continue from it
    ch.reset(u=survivor)
    _recovery(ch, want, first=2, alt=4, inplace=3)
    g.close()
