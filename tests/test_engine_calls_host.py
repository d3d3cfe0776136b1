"""CPU: engine.PreparedCall, the one type behind prepare_step / prepare_plant_step / prepare_rpgd_step / prepare_cem_step and
behind the direct calls - what `run` writes into the argument block, what it hands to which entry point, and what it keeps
alive.  No device and no library call: a stand-in engine, entry points that record their arguments."""
import ctypes as C
import gc
import inspect
import weakref

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cartpolesimulation_amd import _lib  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine, PreparedCall  # noqa: E402


class Engine:
    """What PreparedCall reads of an MPPIEngine: the handle, the launch stream and the return-code check."""
    _h = C.c_void_p(0x1234)

    def __init__(self):
        self.enqueued, self.checked = [], []

    def _stream(self):
        return "the stream"

    def _check(self, rc):
        self.checked.append(rc)

    def entry(self, name, rc=0):
        def enqueue(*args):
            self.enqueued.append((name,) + args)
            return rc
        return enqueue


def fields_of(block):
    return {name: getattr(block, name) for name, _ in block._fields_}


def step_call(eng, result=None, keep=()):
    a = _lib.cpmppi_step_args()
    a.E, a.seed, a.offset, a.env_offset = 3, 11, 5, 2
    return PreparedCall(eng, eng.entry("step", rc=17), a, keep, result, ("offset",), gather=eng.entry("gather"))


def test_run_enqueues_the_block_as_it_is_and_returns_the_result_given():
    eng, result = Engine(), (object(), None)
    call = step_call(eng, result)
    before = fields_of(call.args)
    assert call.run() is result and call.result is result and call.out is result
    assert call.Q_out is result[0] and call.S_out is None
    assert fields_of(call.args) == before
    (name, handle, ref, stream), = eng.enqueued
    assert (name, handle, stream) == ("step", eng._h, "the stream")
    assert ref is call.ref and ref._obj is call.args                      # the live block, not a copy
    assert eng.checked == [17]                                            # the entry point's return code goes to the engine's check


@pytest.mark.parametrize("value", [7, 7.0, np.int64(7), np.float32(7.0)])
def test_run_sets_exactly_the_field_given_as_an_int(value):
    eng = Engine()
    call = step_call(eng)
    before = fields_of(call.args)
    call.run(offset=value)
    after = fields_of(call.args)
    assert after == dict(before, offset=7) and type(after["offset"]) is int
    assert len(eng.enqueued) == 1
    call.run(offset=None)                                                 # None: the field stays
    assert fields_of(call.args) == after and len(eng.enqueued) == 2
    call.set(offset=9)                                                    # set alone writes and enqueues nothing
    assert call.args.offset == 9 and len(eng.enqueued) == 2


def test_every_field_of_the_tuple_and_no_other():
    eng = Engine()
    a = _lib.cpmppi_rpgd_args()
    call = PreparedCall(eng, eng.entry("rpgd"), a, (), None, ("count", "adam_iteration", "draw_offset", "iterations"))
    before = fields_of(a)
    call.run(count=1, adam_iteration=2, draw_offset=None, iterations=4)
    assert fields_of(a) == dict(before, count=1, adam_iteration=2, iterations=4)
    changed = fields_of(a)
    # a name outside the tuple is refused before anything is written or enqueued: a field of the block that is not a counter
    # (alone, and next to one that is), a name the block does not have, and gather_into where no gathering entry point was given
    for bad in (dict(seed=3), dict(count=9, seed=3), dict(offset=1), dict(gather_into=torch.zeros(4))):
        with pytest.raises(TypeError):
            call.run(**bad)
        with pytest.raises(TypeError):
            call.set(**bad)
    assert fields_of(a) == changed and [e[0] for e in eng.enqueued] == ["rpgd"]


def test_gather_into_goes_to_the_gathering_entry_point_with_the_tensors_address():
    eng, result = Engine(), (object(), object())
    call = step_call(eng, result)
    recv = torch.zeros(2, 12)
    assert call.run(offset=8, gather_into=recv) is result
    (name, handle, ref, address, stream), = eng.enqueued
    assert (name, handle, address, stream) == ("gather", eng._h, recv.data_ptr(), "the stream")
    assert ref._obj is call.args and call.args.offset == 8
    call.run()
    assert [e[0] for e in eng.enqueued] == ["gather", "step"]


def test_the_tensors_of_the_block_live_as_long_as_the_call():
    class Buffer:
        pass

    def build(eng):
        converted = Buffer()                                              # (a builder's local: an uploaded or reshaped tensor)
        return step_call(eng, keep=(converted, None)), weakref.ref(converted)

    call, alive = build(Engine())
    gc.collect()
    assert alive() is not None and alive() is call.keep[0]
    call.run()
    del call
    gc.collect()
    assert alive() is None


def test_the_public_entry_points_have_their_builders_signatures():
    """step / plant_step / rpgd_step / cem_step are "build, then run once": each takes what its builder takes (step also the
    ``gather_into`` of `run`), under its own name."""
    for name in ("plant_step", "rpgd_step", "cem_step", "step"):
        public, builder = getattr(MPPIEngine, name), getattr(MPPIEngine, "_build_" + name)
        assert public.__name__ == name and public.__qualname__ == "MPPIEngine." + name
        mine, its = list(inspect.signature(public).parameters.values()), list(inspect.signature(builder).parameters.values())
        if name == "step":
            assert (mine[-1].name, mine[-1].default) == ("gather_into", None)
            mine = mine[:-1]
        assert mine == its
        assert "_prepare" not in inspect.signature(public).parameters
