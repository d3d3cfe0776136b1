"""CPU-only: the C-ABI library loads and exports every symbol include/cpmppi.h declares; host-side config logic."""
import ctypes as C
import sys
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference checkout's YAML files, stored in its own layout (settings only)
CHECKOUT = os.path.join(ROOT, "tests", "golden", "reference_checkout")


def declared_functions():
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpmppi_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from cartpolesimulation_amd import _lib
    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cpmppi.h but not exported by libcpmppi.so"
    assert set(names) == set(_lib.EXPORTS)
    assert lib.cpmppi_version().startswith(b"cpmppi 1 gfx950")


def test_struct_layout_matches_header():
    """ctypes mirrors of cpmppi_config / cpmppi_step_args: field order and count as in the header."""
    from cartpolesimulation_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    body = text[text.index("typedef struct {\n  uint32_t abi_version"):text.index("} cpmppi_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1]
        fields += [re.sub(r"\[.*\]", "", x).strip() for x in names.split(",")]
    assert fields == [f[0] for f in _lib.cpmppi_config._fields_]
    assert C.sizeof(_lib.cpmppi_config) == 4 * (len(fields) - 1) + 96


def test_header_is_plain_c_and_struct_sizes_match(tmp_path):
    """include/cpmppi.h compiles on its own as C99 and as C++ (what a cgo / ctypes / JNI binding generator would feed it to),
    and sizeof / offsetof of the argument structs as a C compiler lays them out equal the ctypes mirrors'."""
    import shutil
    import subprocess
    from cartpolesimulation_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(ROOT, "include", "cpmppi.h")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    gxx = shutil.which("g++")
    if gxx:
        subprocess.run([gxx, "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", hdr], check=True)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cpmppi.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cpmppi_config), sizeof(cpmppi_step_args), '
                   'sizeof(cpmppi_gru_model), offsetof(cpmppi_step_args, noise), offsetof(cpmppi_step_args, Q_out), '
                   'offsetof(cpmppi_step_args, offset_dev), offsetof(cpmppi_step_args, u_nom_out), '
                   'sizeof(cpmppi_plant_args), offsetof(cpmppi_plant_args, period), offsetof(cpmppi_plant_args, save_every), '
                   'offsetof(cpmppi_plant_args, sched_stride), offsetof(cpmppi_plant_args, row_envs), sizeof(cpmppi_recording), '
                   'offsetof(cpmppi_recording, q_update_time), sizeof(cpmppi_comm_info) + sizeof(cpmppi_launch_info), '
                   'offsetof(cpmppi_plant_args, informed_table), offsetof(cpmppi_recording, angle_offset)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A, P, R = _lib.cpmppi_step_args, _lib.cpmppi_plant_args, _lib.cpmppi_recording
    assert got == [C.sizeof(_lib.cpmppi_config), C.sizeof(A), C.sizeof(_lib.cpmppi_gru_model), A.noise.offset, A.Q_out.offset,
                   A.offset_dev.offset, A.u_nom_out.offset, C.sizeof(P), P.period.offset, P.save_every.offset, P.sched_stride.offset,
                   P.row_envs.offset, C.sizeof(R), R.q_update_time.offset, C.sizeof(_lib.cpmppi_comm_info) + C.sizeof(_lib.cpmppi_launch_info),
                   P.informed_table.offset, R.angle_offset.offset]


def test_integration_doc_binding_matches_the_library():
    """The ctypes stub INTEGRATION.md shows a maintainer (section 2) lists the same fields, in the same order and with the
    same ctypes types, as the package's own binding."""
    from cartpolesimulation_amd import _lib
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for cls in (_lib.cpmppi_config, _lib.cpmppi_step_args):
        block = text[text.index(f"class {cls.__name__}(C.Structure):"):]
        block = block[block.index("_fields_ = ["):]
        block = block[:block.index("]\n")]                      # (no field spec ends a line with ']': arrays are C.c_float * 24)
        doc = re.findall(r'\("(\w+)",\s*C\.(\w+)(?:\s*\*\s*(\d+))?\)', block)
        doc = [(n, getattr(C, t), k) for n, t, k in doc]         # (C.c_uint32 is an alias of c_uint: compare the types)
        own = []
        for name, typ in cls._fields_:
            if hasattr(typ, "_length_"):
                own.append((name, typ._type_, str(typ._length_)))
            else:
                own.append((name, typ, ""))
        assert doc == own, cls.__name__


def test_no_cpu_fallback():
    """Without a GPU the library refuses to create a handle and the engine refuses to construct."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cartpolesimulation_amd import _lib
    from cartpolesimulation_amd.configs import MPPIConfig, build_c_config
    lib = _lib.load()
    h = C.c_void_p()
    cfg = build_c_config(1, MPPIConfig(num_rollouts=8, mpc_horizon=4))
    assert lib.cpmppi_create(C.byref(cfg), 0, C.byref(h)) == -3 and not h.value
    assert b"no CPU fallback" in lib.cpmppi_last_error(None)
    from cartpolesimulation_amd.engine import MPPIEngine
    with pytest.raises(RuntimeError):
        MPPIEngine(1, MPPIConfig(num_rollouts=8, mpc_horizon=4))
    cfg.abi_version = 99
    assert lib.cpmppi_create(C.byref(cfg), 0, C.byref(h)) == -2
    assert lib.cpmppi_create(None, 0, C.byref(h)) == -1


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cartpolesimulation_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, f


def test_config_defaults_match_reference_yaml_values():
    from cartpolesimulation_amd.configs import MPPIConfig, PhysicalParameters, build_c_config, cost_vector, legacy_mppi_config
    m = MPPIConfig()
    assert (m.mpc_horizon, m.num_rollouts, m.LBD, m.NU, m.SQRTRHOINV, m.period_interpolation_inducing_points) == \
        (35, 3500, 100.0, 1000.0, 0.03, 10)
    assert abs(m.sigma - 0.03 / np.sqrt(0.02)) < 1e-12 and m.num_knots == 5
    assert MPPIConfig(mpc_horizon=50).num_knots == 6 and MPPIConfig(mpc_horizon=100).num_knots == 11
    p = PhysicalParameters()
    assert np.float32(p.TrackHalfLength) == np.float32(0.198) and np.float32(p.k) == np.float32(1.0 / 3.0)
    c = build_c_config(7, m)
    assert (c.E, c.N, c.H, c.S, c.period) == (7, 3500, 35, 10, 10) and c.cost_id == 0
    assert list(c.cost_w)[:7] == pytest.approx([10.0, 10000.0, 40.0, 1.0, 5.0, 1.0, 0.85])
    assert cost_vector("default")[1] == [600.0, 20000.0, 1.0, 1.0]
    lg = legacy_mppi_config()
    assert (lg.control_mode, lg.shift_mode, lg.correction_u, lg.SQRTRHOINV) == ("penalise", "append_zero", "u_nom", 0.02)
    with pytest.raises(ValueError):
        build_c_config(1, MPPIConfig(shift_mode="rotate"))
    assert cost_vector("quadratic_boundary") == (4, [600.0, 20000.0, 1.0, 1.0, 1.0])          # config_cost_function.yml:53-58
    assert cost_vector("quadratic_boundary_nonconvex", dict(ccrc_weight=2.0)) == (5, [600.0, 20000.0, 1.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        cost_vector("no_such_cost")


def test_reading_a_reference_checkout_reproduces_the_defaults():
    from cartpolesimulation_amd.configs import MPPIConfig, PhysicalParameters, load_reference_yaml, mppi_config_from_yaml
    phys, cfgs = load_reference_yaml(CHECKOUT)
    assert phys == PhysicalParameters()
    m = mppi_config_from_yaml(cfgs, seed=None)
    d = MPPIConfig()
    for k in ("mpc_horizon", "num_rollouts", "cc_weight", "R", "LBD", "NU", "SQRTRHOINV", "mpc_timestep",
              "period_interpolation_inducing_points", "intermediate_steps", "cost_function_specification"):
        assert getattr(m, k) == getattr(d, k), k
    assert m.predictor_type == "ODE"        # config_controllers.yml:3 ships predictor_specification: "ODE" (Euler-Cromer, no bounce)


def test_state_utilities_mirror():
    from cartpolesimulation_amd import state_utilities as su
    assert list(su.STATE_VARIABLES) == ["angle", "angleD", "angle_cos", "angle_sin", "position", "positionD"]
    assert (su.ANGLE_IDX, su.ANGLED_IDX, su.ANGLE_COS_IDX, su.ANGLE_SIN_IDX, su.POSITION_IDX, su.POSITIOND_IDX) == \
        (0, 1, 2, 3, 4, 5)
    s = su.create_cartpole_state({"angle": 0.5, "positionD": -0.2})
    assert s.dtype == np.float32 and s[2] == np.float32(np.cos(0.5)) and s[3] == np.float32(np.sin(0.5)) and s[5] == np.float32(-0.2)
    assert su.create_cartpole_state()[2] == 1.0


def test_sfc64_knots_match_the_reference_sampler(golden_dir):
    """Host sampler used for identical-noise-seed runs == the reference's initialize_perturbations knots."""
    from cartpolesimulation_amd.configs import MPPIConfig
    from cartpolesimulation_amd.sampling import sample_knots_sfc64
    h = np.load(os.path.join(golden_dir, "sampler_rwa.npz"))
    rng = np.random.Generator(np.random.SFC64(int(h["seed"])))
    for _ in range(5):
        rng.uniform(-1.0, 1.0)
    cfg = MPPIConfig(num_rollouts=int(h["N"]), mpc_horizon=int(h["H"]), SQRTRHOINV=0.02)
    kn = sample_knots_sfc64(rng, 1, cfg.num_rollouts, cfg)[0]
    assert np.array_equal(kn[0][:4], h["du_row0"][::10]) and np.array_equal(kn[-1][:4], h["du_row3499"][::10])


def test_controller_reads_a_checkout():
    from cartpolesimulation_amd.controller_mpc import controller_mpc
    c = controller_mpc("CartPole", {"target_position": 0.0}, config_root=CHECKOUT, config=dict(num_rollouts=512))
    assert c.config_optimizer["mpc_horizon"] == 35 and c.config_optimizer["num_rollouts"] == 512
    assert c.config_optimizer["cost_function_specification"] == "quadratic_boundary_grad_minimal"
    assert c.config_optimizer["cost_weights"]["db_weight_up"] == 10000 and c.has_optimizer
    assert c.config_optimizer["predictor_type"] == "ODE"
    with pytest.raises(ValueError):
        controller_mpc("Pendulum")


def test_rollout_kernels_have_no_scratch_and_no_vgpr_spills():
    """Round 1 lost 4 % (Philox) / 15 % (buffer mode) of the hot kernel to a 28-byte private slot per lane that a compiler
    pass had introduced silently.  The bench line cannot see that (its traffic figure comes from a committed profile), so
    the BUILT library is inspected: every instantiation of rollout_cost_kernel — and the GRU rollout kernels — must have
    .private_segment_fixed_size == 0 and no VGPR spills in the code object's metadata."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = [k for k in code_objects.kernels(_lib.LIB_PATH) if "rollout_cost_kernel" in k["name"] or "gru_predict_kernel" in k["name"]]
    hot = [k for k in ks if "19rollout_cost_kernel" in k["name"]]
    # 4 costs x 4 noise sources x (latency R1, throughput R1 fast + precise, throughput R2, mid R2, mid R2 for launches of one
    # wave per SIMD) for predictor_ODE_v0 + (latency R1, throughput R1 fast + precise, throughput R2, its form for launches of
    # one wave per SIMD) for predictor_ODE
    assert len(hot) == 4 * 4 * (6 + 5), len(hot)
    # the mid-size build must keep three waves per SIMD (512 registers / 168); its variant for launches of at most one wave
    # per SIMD (straight-line control steps) two, so that a guest kernel - the overlapped all-gather - still fits beside it
    for k in hot:
        tail = k["name"].split("EEEv")[0]
        assert tail.endswith(("ELi0", "ELi1")), tail            # the last template argument: the ODE predictor
        if tail.endswith("ELi1"):
            assert tail[:-4].endswith(("ELi0", "ELi1", "ELi2ELi3")), tail   # predictor_ODE: latency / throughput builds (+ lone-wave R2)
        tail = tail[:-4]
        if tail.endswith("ELi2ELi2"):
            assert k["vgpr_count"] + k["agpr_count"] <= 168, (k["name"], k["vgpr_count"])
        if tail.endswith("ELi2ELi3"):
            assert k["vgpr_count"] + k["agpr_count"] <= 256, (k["name"], k["vgpr_count"])
    bad = [(k["name"], k["private_segment_fixed_size"], k["vgpr_spill_count"]) for k in ks
           if k["private_segment_fixed_size"] != 0 or k["vgpr_spill_count"] != 0]
    assert not bad, bad
    # the headline kernel (quadratic_boundary_grad_minimal, FAST, Philox, two rollouts per lane, throughput build) must
    # keep four waves per SIMD (512 registers / 128)
    for k in hot:
        if "kernelILi0ELb1ELi2ELi2ELi1ELi" in k["name"]:      # (both ODE predictors)
            assert k["vgpr_count"] + k["agpr_count"] <= 128, (k["name"], k["vgpr_count"])


def test_the_built_library_compared_with_itself_by_name_has_no_difference(capsys):
    """tools/code_objects.py --diff --by-name, how a change that moves kernels between translation units is checked: every kernel
    of kernels() is found by name with a code range of its own, and a library does not differ from itself."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    listed = code_objects.kernels(_lib.LIB_PATH)
    code = code_objects.kernel_code(_lib.LIB_PATH)
    assert len(code) == len(listed) == len(code_objects.kernels_by_name(_lib.LIB_PATH)) > 0
    assert all(len(c) > 0 for c in code.values())
    assert code_objects.diff_by_name(_lib.LIB_PATH, _lib.LIB_PATH) == 0
    n = len(listed)
    assert f"kernels by name: {n} / {n}, {n} identical; no difference" in capsys.readouterr().out


def test_the_stand_in_collective_library_exports_what_the_communicator_binds():
    """tests/fake_rccl/libfake_rccl.so (test infrastructure for the two-process GPU tests) exports exactly the symbols
    csrc/cpmppi_comm.hip looks up with dlsym, and draws ids only it accepts - no GPU call here."""
    import ctypes as C
    import re
    path = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build_fake_rccl()
    src = open(os.path.join(ROOT, "cartpolesimulation_amd", "csrc", "cpmppi_comm.hip")).read()
    bound = set(re.findall(r'dlsym\(r\.dl, "(nccl\w+)"\)', src))
    assert len(bound) == 8
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name in bound:
        getattr(lib, name)
    ident = C.create_string_buffer(128)
    assert lib.ncclGetUniqueId(ident) == 0 and ident.raw[:4] == b"EKAF" and any(ident.raw[4:20])
    v = C.c_int()
    assert lib.ncclGetVersion(C.byref(v)) == 0 and v.value == 99
