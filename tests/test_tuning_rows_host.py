"""CPU-only: what the per-env controller tuning (cpmppi_set_tuning_rows) has that needs no GPU - the export, the row packing of
configs.tuning_rows (order, defaults, unknown names), the launch plan's new input, the instance lists of the tuned kernel and the
resource figures of its builds beside their untuned siblings (the BUILT library, read with tools/code_objects.py)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import launch_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_export_and_row_layout():
    from cartpolesimulation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cpmppi.h")).read(), flags=re.S)
    lib = _lib.load()
    assert "cpmppi_set_tuning_rows" in set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text))
    assert "cpmppi_set_tuning_rows" in _lib.EXPORTS and hasattr(lib, "cpmppi_set_tuning_rows")
    assert f"#define CPMPPI_TUNING_ROW_FLOATS {_lib.TUNING_ROW_FLOATS}u" in text
    assert f"CPMPPI_TUNING_LBD = {_lib.TUNING_LBD}, CPMPPI_TUNING_SIGMA = {_lib.TUNING_SIGMA}" in text
    params = open(os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_params.hpp")).read()
    assert f"TUNING_ROW_FLOATS = {_lib.TUNING_ROW_FLOATS}, TUNING_LBD = {_lib.TUNING_LBD}, TUNING_SIGMA = {_lib.TUNING_SIGMA};" in params
    assert _lib.ABI_VERSION == 5 and "#define CPMPPI_ABI_VERSION 5u" in text       # a new entry point: no layout changes
    assert (_lib.TUNING_ROW_FLOATS * 4) % 64 == 0                                    # a row never straddles a 64-byte line


def test_row_packing_order_defaults_and_unknown_names():
    from cartpolesimulation_amd import _lib
    from cartpolesimulation_amd.configs import COST_WEIGHTS, TUNING_COLUMNS, MPPIConfig, build_c_config, tuning_rows
    assert TUNING_COLUMNS == tuple(COST_WEIGHTS["quadratic_boundary_grad_minimal"][1]) + ("LBD", "SQRTRHOINV")
    m = MPPIConfig(cost_weights=dict(ep_weight_up=55.0), LBD=70.0)
    c = build_c_config(4, m)
    rows = tuning_rows(m, 4)
    assert rows.shape == (4, _lib.TUNING_ROW_FLOATS) and rows.dtype == f32
    # defaults: exactly the floats the handle is created with, in cpmppi_set_cost_weights order
    for e in range(4):
        assert list(rows[e, :7]) == [f32(x) for x in list(c.cost_w)[:7]] and rows[e, 2] == f32(55.0)
        assert rows[e, _lib.TUNING_LBD] == f32(c.LBD) == f32(70.0) and rows[e, _lib.TUNING_SIGMA] == f32(c.sigma)
        assert not rows[e, 9:].any()
    # columns per env and scalars for all
    rows = tuning_rows(m, 3, LBD=[50, 100, 200], permissible_track_fraction=0.5, SQRTRHOINV=[0.01, 0.02, 0.03], R=[1, 2, 3])
    assert list(rows[:, 7]) == [50, 100, 200] and list(rows[:, 6]) == [0.5] * 3 and list(rows[:, 5]) == [1, 2, 3]
    assert list(rows[:, 2]) == [55.0] * 3
    for e, s in enumerate((0.01, 0.02, 0.03)):
        assert rows[e, 8] == f32(MPPIConfig(SQRTRHOINV=s).sigma)
    with pytest.raises(ValueError, match="'ep_weight'"):
        tuning_rows(m, 3, ep_weight=[1, 2, 3])
    with pytest.raises(ValueError, match="'NU'"):
        tuning_rows(m, 3, NU=5.0)
    with pytest.raises(ValueError, match="one value per env"):
        tuning_rows(m, 3, LBD=[1, 2])
    with pytest.raises(ValueError, match="LBD must be positive"):
        tuning_rows(m, 3, LBD=[1, 0, 2])
    with pytest.raises(ValueError, match="quadratic_boundary_grad_minimal"):
        tuning_rows(MPPIConfig(cost_function_specification="default"), 3)


def test_launch_plan_with_tuning_rows_registered(tmp_path):
    """The plan's one new input changes WHICH table the kernel is looked up in (and which fold kernel runs in front), nothing else:
    build, lane mapping, grid, LDS and fold_first of every boundary shape of launch_table.py are what they are without rows."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tuned_probe")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "cartpolesimulation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_plan", "tuned_probe.cpp"), "-o", exe])
    rows = [r for r in T.BOUNDARY_ROWS if not r.mass_rows]
    P = (T.H + T.PERIOD - 1) // T.PERIOD + 1
    text = "".join(f"{int(r.predictor == 'ODE')} {int(r.options.get('math_mode', 'fast') == 'fast')} "
                   f"{r.options.get('rollouts_per_lane', 0)} {r.N} {T.H} {P} {r.E} {T.NOISES.index('philox')} {tuned}\n"
                   for r in rows for tuned in (0, 1))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(rows)
    seen = set()
    for r, plain, tuned in zip(rows, out[0::2], out[1::2]):
        plain, tuned = plain.split(), tuned.split()
        assert plain[-1] == "0" and tuned[-1] == "1" and plain[:-1] == tuned[:-1], T.row_id(r)
        fast, rpl, variant, integ = (int(x) for x in tuned[:4])
        assert (fast, rpl, variant, int(tuned[6]), bool(int(tuned[10]))) == (r.fast, r.rpl, r.variant, r.blocks, r.fold), T.row_id(r)
        assert integ == (T.INTEG_ODE if r.predictor == "ODE" else T.INTEG_V0)
        seen.add((fast, rpl, variant, integ))
    # every (FAST, R, VARIANT, INTEG) the plan selects with rows registered is an instance of the tuned kernel's lists
    hdr = open(os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_rollout.hpp")).read()
    lists = hdr[hdr.index("#define CPMPPI_TUNED_LATENCY_INSTANCES"):hdr.index("#define CPMPPI_DEFINE_ROLLOUT_TUNED")]
    inst = {(int(f == "true"), int(r), int(v), int(i == "PREDICTOR_ODE"))
            for f, r, v, i in re.findall(r"X\(COST_QBGM, (true|false), NOISE_PHILOX, (\d), (\d), (PREDICTOR_ODE_V0|PREDICTOR_ODE)\)", lists)}
    assert len(inst) == 11 and seen <= inst, seen - inst


def test_tuned_kernels_have_no_scratch_and_their_siblings_occupancy():
    """Every build of rollout_cost_tuned_kernel in the built library: scratch 0, no VGPR spill, and the waves-per-SIMD bucket (512
    registers / VGPRs in granules of 8) of the untuned kernel with the same template arguments."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = {k["name"]: k for k in code_objects.kernels(_lib.LIB_PATH)}
    tuned = [n for n in ks if "25rollout_cost_tuned_kernel" in n]
    assert len(tuned) == 11
    waves = lambda k: min(8, 512 // (-(-(k["vgpr_count"] + k["agpr_count"]) // 8) * 8))       # noqa: E731
    for n in tuned + [x for x in ks if "fold_env_tuned_kernel" in x or "score_runs_kernel" in x]:
        assert ks[n]["private_segment_fixed_size"] == 0 and ks[n]["vgpr_spill_count"] == 0, n
    for n in tuned:
        sibling = ks[n.replace("25rollout_cost_tuned_kernel", "19rollout_cost_kernel")]
        assert waves(ks[n]) == waves(sibling), (n, ks[n]["vgpr_count"], sibling["vgpr_count"])
