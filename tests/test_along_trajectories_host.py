"""CPU: control along recorded trajectories without a GPU - the new entry point's declaration, export and ctypes mirror; the files
(a column appended byte for byte, refusals, the -i file name); the column mapping; and what the loop hands the library, call by
call, recorded with the stand-in engine of device_loop_cases.py: prime, then per period step + replay, the captured body naming its
period by the device counter only."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import device_loop_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAME = "Q_calculated_offline"


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
def header_fields(struct):
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    end = text.index("} %s;" % struct)
    body = re.sub(r"/\*.*?\*/", "", text[text.rindex("typedef struct {", 0, end):end], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if decl:
            names = re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1)
            fields += [(x.strip().lstrip("*").strip(), "*" in decl) for x in names.split(",")]
    return fields


def test_export_declaration_and_ctypes_struct_agree():
    from cartpolesimulation_amd import _lib
    lib = _lib.load()
    assert "cpmppi_replay_step" in _lib.EXPORTS and hasattr(lib, "cpmppi_replay_step")
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert "int cpmppi_replay_step(cpmppi_handle* h, const cpmppi_replay_args* args, void* stream);" in text
    assert lib.cpmppi_abi_version() == 5 == _lib.ABI_VERSION
    fields = header_fields("cpmppi_replay_args")
    mirror = _lib.cpmppi_replay_args._fields_
    assert [n for n, _ in fields] == [n for n, _ in mirror]
    for (name, pointer), (_, ctype) in zip(fields, mirror):
        assert (ctype is C.c_void_p) == pointer, name
    assert dict(mirror)["period"] is C.c_uint64 and dict(mirror)["R"] is C.c_uint32
    assert lib.cpmppi_replay_step.argtypes[1]._type_ is _lib.cpmppi_replay_args


def test_the_unit_is_built_with_the_library():
    import __graft_entry__ as G
    assert "cpmppi_replay.hip" in G.HIP_UNITS and os.path.exists(os.path.join(G.CSRC, "cpmppi_replay.hip"))


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def write_input(path, rows=6, seed=1, extra=None):
    from cartpolesimulation_amd.recording import write_recording
    rng = np.random.Generator(np.random.SFC64(seed))
    py = lambda a: [float(x) for x in np.asarray(a, f32)]           # noqa: E731
    angle = rng.uniform(-1, 1, rows)
    cols = {"time": [0.02 * i for i in range(rows)], "angle": py(angle), "angleD": py(rng.uniform(-1, 1, rows)),
            "angle_cos": py(np.cos(angle)), "angle_sin": py(np.sin(angle)), "position": py(rng.uniform(-0.1, 0.1, rows)),
            "positionD": py(rng.uniform(-0.1, 0.1, rows)), "Q_calculated": py(rng.uniform(-1, 1, rows)),
            "target_position": py(rng.uniform(-0.1, 0.1, rows)), "target_equilibrium": [1] * rows, "L": py(np.full(rows, 0.395))}
    cols.update(extra or {})
    return write_recording(str(path), cols, title="test", header=["Length of experiment: 1 s", "", "Data:"])


@pytest.fixture
def fake_control(monkeypatch):
    """control_along_trajectories without a device: float32 values that need all their digits, one more per recording and row."""
    from cartpolesimulation_amd import along_trajectories as A
    calls = []

    def control(recordings, **kw):
        states, rows, attrs = A.stack_recordings(recordings, kw.get("columns"))
        calls.append(dict(kw, files=list(recordings), attrs=attrs))
        R, T = states.shape[:2]
        Q = (np.arange(R * T, dtype=np.float64).reshape(R, T) / 7.0 - 0.3).astype(f32)
        Q[np.arange(T)[None, :] >= rows[:, None]] = np.nan
        return dict(Q=Q, Q_std=np.zeros_like(Q), rows=rows)

    monkeypatch.setattr(A, "control_along_trajectories", control)
    return calls


def test_csv_round_trip(tmp_path, fake_control):
    from cartpolesimulation_amd import along_trajectories as A
    src = tmp_path / "in"
    src.mkdir()
    a, b = write_input(src / "b.csv", rows=6), write_input(src / "a.csv", rows=4, seed=2)
    out = A.transform_recordings(str(src), str(tmp_path / "out"))
    assert [os.path.basename(p) for p in out] == ["a.csv", "b.csv"]                      # sorted
    assert fake_control[0]["files"] == [b, a]
    for r, (inp, res) in enumerate(zip((b, a), out)):
        raw_in, raw_out = open(inp, "rb").read(), open(res, "rb").read()
        lines_in, lines_out = raw_in.splitlines(keepends=True), raw_out.splitlines(keepends=True)
        assert len(lines_in) == len(lines_out)
        preamble = [l for l in lines_in if l.startswith(b"#")]
        assert [l for l in lines_out if l.startswith(b"#")] == preamble and lines_out[:len(preamble)] == preamble
        stripped = b"".join(l if l.startswith(b"#") else l[:l.rstrip(b"\r\n").rindex(b",")] + l[len(l.rstrip(b"\r\n")):] for l in lines_out)
        assert stripped == raw_in
        cols = A.load_columns(res, [NAME, "target_position"])
        assert cols["names"][-1] == NAME and cols["names"][:-1] == A.load_columns(inp)["names"]
        T = len(cols[NAME])
        want = (np.arange(r * 6, r * 6 + T, dtype=np.float64) / 7.0 - 0.3).astype(f32)
        assert cols[NAME].tobytes() == want.tobytes()                                    # repr(float(x)) reads back exactly
        text = raw_out.decode().splitlines()
        assert text[len(preamble) + 1].endswith("," + repr(float(want[0])))


def test_save_output_only_and_the_index_file_name(tmp_path, fake_control):
    from cartpolesimulation_amd import along_trajectories as A
    src = tmp_path / "in"
    src.mkdir()
    for i in (3, 7):
        write_input(src / f"Experiment-{i:03d}.csv", rows=5, seed=i)
    out = A.main(["--get-files-from", str(src), "--save-files-to", str(tmp_path / "out"), "-i", "7", "--save-output-only",
                  "--output-name", "Q_mine", "--num-evals", "5", "--no-warm-start", "--column", "L=L", "--graph"])
    assert [os.path.basename(p) for p in out] == ["Experiment-007.csv"]
    kw = fake_control[0]
    assert kw["files"] == [str(src / "Experiment-007.csv")] and kw["num_evals"] == 5 and kw["warm_start"] is False
    assert kw["columns"] == {"L": "L"} and kw["graph"] is True and kw["optimizer"] == "mppi"
    lines_in = open(src / "Experiment-007.csv", "rb").read().splitlines(keepends=True)
    lines_out = open(out[0], "rb").read().splitlines(keepends=True)
    n = sum(l.startswith(b"#") for l in lines_in)
    assert lines_out[:n] == lines_in[:n] and lines_out[n] == b"time,Q_mine\r\n"
    for li, lo in zip(lines_in[n + 1:], lines_out[n + 1:]):
        assert lo.split(b",")[0] == li.split(b",")[0] and len(lo.split(b",")) == 2
    assert len(lines_out) == len(lines_in)


def test_file_refusals(tmp_path, fake_control):
    from cartpolesimulation_amd import along_trajectories as A
    src = tmp_path / "in"
    src.mkdir()
    write_input(src / "a.csv")
    out = tmp_path / "out"
    A.transform_recordings(str(src), str(out))
    with pytest.raises(FileExistsError, match="never overwrites a recording"):
        A.transform_recordings(str(src), str(out))
    with pytest.raises(ValueError, match=f"already has a column '{NAME}'"):
        A.transform_recordings(str(out), str(tmp_path / "again"))
    assert len(fake_control) == 1 and not (tmp_path / "again").exists()                  # refused before anything was computed
    with pytest.raises(FileExistsError):
        A.append_column(str(src / "a.csv"), str(out / "a.csv"), "x", np.zeros(6, f32))


def test_refusals_before_any_device_work(tmp_path):
    from cartpolesimulation_amd.along_trajectories import control_along_trajectories
    from cartpolesimulation_amd.harness import REPLAY_REFUSALS
    path = write_input(tmp_path / "a.csv")
    with pytest.raises(ValueError, match=r"column 'nope' \(mapped to L\) is missing"):
        control_along_trajectories([path], columns={"L": "nope"})
    with pytest.raises(ValueError, match="unknown controller attribute"):
        control_along_trajectories([path], columns={"m_pole": "L"})
    with pytest.raises(ValueError, match="does not serve the GRU predictor") as err:
        control_along_trajectories([path], predictor_specification="GRU-6IN-32H1-32H2-5OUT-0")
    assert REPLAY_REFUSALS["gru"] in str(err.value)
    with pytest.raises(ValueError, match="does not serve the GRU predictor"):
        control_along_trajectories([path], config={"predictor_specification": "GRU-6IN-32H1-32H2-5OUT-0"})
    with pytest.raises(ValueError, match="an optimizer object is paced by the host"):
        control_along_trajectories([path], optimizer=SimpleNamespace(fused=False, num_envs=1))
    with pytest.raises(ValueError, match="optimizer 'cem'"):
        control_along_trajectories([path], optimizer="cem")
    with pytest.raises(ValueError, match="num_evals 9 exceeds max_envs 8"):
        control_along_trajectories([path], num_evals=9, max_envs=8)
    with pytest.raises(ValueError, match="warm_start=False is served by the fused MPPI step alone"):
        control_along_trajectories([path], optimizer="rpgd", warm_start=False)


def test_column_mapping_and_the_previous_input_fallback(tmp_path):
    from cartpolesimulation_amd import along_trajectories as A
    rows = 5
    prev = [float(f32(0.1 * i)) for i in range(rows)]
    plain = write_input(tmp_path / "plain.csv", rows=rows)
    ccrc = write_input(tmp_path / "ccrc.csv", rows=rows, extra={"Q_ccrc": prev, "Q_applied_-1": [0.0] * rows})
    applied = write_input(tmp_path / "applied.csv", rows=rows, extra={"Q_applied_-1": prev, "L_other": [0.3] * rows})
    names = A.load_columns(plain)["names"]
    assert A.resolve_columns(None, names) == dict(target_position="target_position", target_equilibrium="target_equilibrium", L="L", Q_ccrc=None)
    assert A.resolve_columns(None, names + ["Q_applied_-1"])["Q_ccrc"] == "Q_applied_-1"
    assert A.resolve_columns(None, names + ["Q_applied_-1", "Q_ccrc"])["Q_ccrc"] == "Q_ccrc"
    assert A.resolve_columns(None, [n for n in names if n != "L"])["L"] is None         # -> the config's pole length
    with pytest.raises(ValueError, match="column 'target_position' is missing"):
        A.resolve_columns(None, [n for n in names if n != "target_position"])
    for path in (ccrc, applied):
        states, lengths, attrs = A.stack_recordings([path])
        assert states.shape == (1, rows, 6) and list(lengths) == [rows]
        assert attrs["Q_ccrc"].tobytes() == np.asarray([prev], f32).tobytes()
    assert A.stack_recordings([plain])[2]["Q_ccrc"] is None
    _, _, attrs = A.stack_recordings([applied], columns={"L": "L_other", "Q_ccrc": "Q_calculated"})
    assert (attrs["L"] == f32(0.3)).all() and attrs["Q_ccrc"].tobytes() == A.load_columns(applied)["Q_calculated"][None].tobytes()
    with pytest.raises(ValueError, match="some recordings carry a column for Q_ccrc and some do not"):
        A.stack_recordings([plain, ccrc])
    # ragged lengths are padded, the true lengths kept
    short = write_input(tmp_path / "short.csv", rows=3, seed=4)
    states, lengths, attrs = A.stack_recordings([plain, short])
    assert states.shape == (2, rows, 6) and list(lengths) == [rows, 3] and not states[1, 3:].any()
    # the loader keeps what brunton.load_recording drops, and load_recording is as it was
    from cartpolesimulation_amd.brunton import load_recording
    assert "target_position" in A.load_columns(plain) and "target_position" not in load_recording(plain)


# ---- the loop's call sequence ---------------------------------------------------------------------------------------------------------
class ReplayRecordingEngine(D.RecordingEngine):
    def __init__(self, *args, **kw):
        from cartpolesimulation_amd.engine import MPPIEngine
        super().__init__(*args, **kw)
        self._sig["_build_replay_step"] = inspect.signature(MPPIEngine._build_replay_step)

    def prepare_replay_step(self, *args, **kwargs):
        return D.Prepared(self, "replay_step", D._resolved(self._sig["_build_replay_step"], args, kwargs), ("period", "prime"))

    def replay_step(self, *args, **kwargs):
        self.prepare_replay_step(*args, **kwargs).run()


def loop_events(monkeypatch, graph, warm_start=True, optimizer=None, K=2):
    from cartpolesimulation_amd.harness import ReplayBuffers, ReplayRun
    trace = D.Trace()
    eng = ReplayRecordingEngine(trace, 3 * K, D._mppi())
    if graph:
        D.install_cuda_stand_ins(monkeypatch, trace)
    rng = np.random.Generator(np.random.SFC64(2))
    R, T = 3, 9
    col = lambda: rng.standard_normal((R, T)).astype(f32)            # noqa: E731
    buf = ReplayBuffers(eng, rng.standard_normal((R, T, 6)).astype(f32), [5, 9, 7], K, col(), col(), L=col(), previous=col())
    opt = optimizer(eng) if optimizer else None
    ReplayRun(eng, buf, D.SEED, optimizer=opt, warm_start=warm_start).run(graph=graph, steps_per_graph=4)
    return trace.events, buf


def label(v):
    return v.split()[0]


def test_the_launched_loop_is_prime_then_step_and_replay_per_period(monkeypatch):
    events, buf = loop_events(monkeypatch, graph=False)
    assert [e["call"] for e in events] == ["replay_step"] + ["step", "replay_step"] * 9
    prime = events[0]["args"]
    assert prime["prime"] == 1 and prime["period"] == 0 and prime["K"] == 2 and "period_dev" not in prime and "u_nom_reset" not in prime
    for c in range(9):
        step, replay = events[1 + 2 * c]["args"], events[2 + 2 * c]["args"]
        assert step["offset"] == c and step["seed"] == D.SEED and step["env_offset"] == 0 and "offset_dev" not in step
        assert replay["period"] == c and replay["prime"] == 0 and "period_dev" not in replay
        # the step reads what the replay publishes, and the replay collects what the step writes
        assert label(step["s0"]) == label(replay["s_out"]) and label(step["target_position"]) == label(replay["target_position_out"])
        assert label(step["target_equilibrium"]) == label(replay["target_equilibrium_out"]) and label(step["L"]) == label(replay["L_out"])
        assert label(step["Q_out"]) == label(replay["Q"])
        assert "previous_input" not in step                            # (this cost reads none)
    cold, _ = loop_events(monkeypatch, graph=False, warm_start=False)
    assert all(label(e["args"]["u_nom_reset"]) == label(cold[1]["args"]["u_nom"]) for e in cold if e["call"] == "replay_step")


def test_the_captured_body_names_its_period_by_the_device_counter_only(monkeypatch):
    events, _ = loop_events(monkeypatch, graph=True)
    calls = [(e["call"], bool(e.get("captured"))) for e in events]
    assert calls == [("replay_step", False)] + [("step", True), ("replay_step", True)] * 4 + [("replay", False)] * 2 + \
        [("step", False), ("replay_step", False)]
    assert events[0]["args"]["prime"] == 1
    for e in events[1:]:
        if e["call"] == "replay":
            continue
        a = e["args"]
        if e["call"] == "step":
            assert a["offset"] == 0 and a["offset_dev"].startswith("t") and "int64 1" in a["offset_dev"]
            counter = label(a["offset_dev"])
        else:
            assert a["period"] == 0 and a["prime"] == 0 and label(a["period_dev"]) == counter


def test_a_fused_optimizer_is_handed_the_recorded_previous_control(monkeypatch):
    events, buf = loop_events(monkeypatch, graph=True, optimizer=lambda eng: D.FusedOptimizer(eng, warmup=False))
    steps = [e for e in events if e["call"] == "optimizer.step_device"]
    replays = [e for e in events if e["call"] == "replay_step"]
    assert len(steps) == 5 and len(replays) == 6
    for s in steps:
        assert label(s["args"]["previous_input"]) == label(replays[0]["args"]["previous_input_out"])
        assert label(s["args"]["previous_input"]) != label(replays[0]["args"]["Q"])
        assert label(s["args"]["count_dev"]) == label(replays[1]["args"]["period_dev"])
        assert label(s["args"]["s"]) == label(replays[0]["args"]["s_out"])


def test_loop_refusals(monkeypatch):
    from cartpolesimulation_amd.harness import REPLAY_REFUSALS
    with pytest.raises(ValueError, match="an optimizer object is paced by the host"):
        loop_events(monkeypatch, graph=False, optimizer=D.HostPacedOptimizer)
    with pytest.raises(ValueError, match="warmup=True needs the host to tell the first step from the others"):
        loop_events(monkeypatch, graph=True, optimizer=lambda eng: D.FusedOptimizer(eng, warmup=True))
    with pytest.raises(ValueError, match="warm_start=False is served by the fused MPPI step alone"):
        loop_events(monkeypatch, graph=False, warm_start=False, optimizer=lambda eng: D.FusedOptimizer(eng, warmup=False))
    from cartpolesimulation_amd.harness import ReplayBuffers, ReplayRun
    eng = ReplayRecordingEngine(D.Trace(), 3, D._mppi(), has_gru=True)
    buf = ReplayBuffers(eng, np.zeros((3, 4, 6), f32), [4, 4, 4], 1, np.zeros((3, 4), f32), np.ones((3, 4), f32))
    with pytest.raises(ValueError) as err:
        ReplayRun(eng, buf, 0, predictor="GRU")
    assert str(err.value) == REPLAY_REFUSALS["gru"]
    # a cost that reads the previous control needs the recorded column
    eng = ReplayRecordingEngine(D.Trace(), 3, D._mppi(cost_function_specification="quadratic_boundary_grad"))
    with pytest.raises(ValueError, match="reads the control applied before each row"):
        ReplayBuffers(eng, np.zeros((3, 4, 6), f32), [4, 4, 4], 1, np.zeros((3, 4), f32), np.ones((3, 4), f32))
