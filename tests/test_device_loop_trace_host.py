"""CPU: every form of the device loop hands the library the same calls, with the same arguments, in the same order, as the
commit the trace was recorded on (golden/device_loop_calls.json; device_loop_cases.py says what a trace holds and drives the
cases).  The refusals of what cannot be captured are part of it, each with its sentence."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

import device_loop_cases as DL  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_loop_calls.json")) as f:
    RECORDED = json.load(f)["cases"]


def test_the_trace_covers_every_case_and_every_case_says_something():
    assert sorted(RECORDED) == sorted(DL.CASES)
    calls = {ev["call"] for events in RECORDED.values() for ev in events}
    assert calls == {"step", "plant_step", "plant_advance", "gru_advance", "set_pole_mass", "set_pole_mass_rows", "apply_pole_mass_of",
                     "optimizer.step", "optimizer.step_device", "optimizer.reserve_fused", "groups_run", "replay", "ValueError"}
    # a run that ends inside a control period, and one that does not: the last plant step is shorter, or records only
    last = {name: RECORDED[name][-1]["args"]["n_substeps"] for name in ("schedule/plain", "schedule/whole_periods")}
    assert last == {"schedule/plain": 5, "schedule/whole_periods": 0}
    for name, events in RECORDED.items():
        captured = [ev for ev in events if ev.get("captured")]
        assert bool(captured) == (name.startswith("captured/") or name.endswith("_captured")), name
        assert any(ev["call"] == "replay" for ev in events) == bool(captured), name


def test_a_run_and_its_graph_are_freed_when_dropped_not_by_the_cycle_collector(monkeypatch):
    """A captured run holds a HIP graph.  Were the run part of a reference cycle, the graph would be destroyed whenever the cycle
    collector next runs - possibly inside a later run's capture, where the runtime refuses that."""
    import gc
    import weakref
    from cartpolesimulation_amd.harness import ScheduleRun
    trace = DL.Trace()
    DL.install_cuda_stand_ins(monkeypatch, trace)
    run = ScheduleRun(DL.RecordingEngine(trace, DL.E, DL._mppi()), DL.batch(), DL.SEED)
    run.capture(4)
    while run.periods_left:
        run.enqueue_next()
    run.finish()
    gc.collect()
    gc.disable()
    try:
        gone = [weakref.ref(run), weakref.ref(run.loop.graph), weakref.ref(run.controller)]
        del run
        assert [ref() for ref in gone] == [None, None, None]
    finally:
        gc.enable()


@pytest.mark.parametrize("name", sorted(DL.CASES))
def test_the_library_is_handed_the_recorded_calls(name, monkeypatch):
    events = DL.record(name, monkeypatch)
    want = RECORDED[name]
    for i, (got, rec) in enumerate(zip(events, want)):
        assert got == rec, f"{name}: call {i}"
    assert len(events) == len(want), name
    if name in DL.REFUSALS:
        assert events[-1] == {"call": "ValueError", "text": DL.REFUSALS[name]}
