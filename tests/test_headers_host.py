"""CPU: the include structure of csrc/.  The definition of the rollout kernel (cpmppi_rollout_kernel.inc, through cpmppi_rollout.hpp)
reaches the cpmppi_rollout_*.hip units alone - a unit that saw it could compile the kernel a second time with its own flags - the
host-only units parse none of the integrators, costs or the noise generator, and every header compiles on its own.  Preprocessor and
front-end runs of hipcc: no code is generated, no GPU is needed."""
import glob
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as G

CSRC = G.CSRC
INCLUDES = ["-I", os.path.join(G.ROOT, "include"), "-I", CSRC]
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))
HOST_ONLY = ["cpmppi_comm.hip", "cpmppi_groups.hip", "cpmppi_io.hip"]


def hipcc():
    path = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    path = path if os.path.exists(path) else shutil.which("hipcc")
    if path is None:
        pytest.skip("no hipcc")
    return path


@pytest.fixture(scope="module")
def deps():
    """unit -> the base names of the files of csrc/ and include/ that its host pass reads (hipcc -MM)"""
    cc = hipcc()
    jobs = {unit: subprocess.Popen([cc, "-MM", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", *INCLUDES,
                                    os.path.join(CSRC, unit)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for unit in G.HIP_UNITS}
    out = {}
    for unit, job in jobs.items():
        text, err = job.communicate()
        assert job.returncode == 0, err
        out[unit] = {os.path.basename(word) for word in text.replace("\\\n", " ").split()[1:]}
    return out


def test_every_unit_reads_the_shared_headers(deps):
    # (the dependency lists are what they claim to be: every unit reads the public header and the parameter block)
    for unit, files in deps.items():
        assert unit in files and "cpmppi.h" in files, unit
        assert "cpmppi_params.hpp" in files, unit


def test_only_the_rollout_units_see_the_rollout_kernels_definition(deps):
    for unit, files in deps.items():
        if unit.startswith("cpmppi_rollout_"):
            assert {"cpmppi_rollout.hpp", "cpmppi_rollout_kernel.inc"} <= files, unit
        elif unit == "cpmppi.hip":
            # the launcher: the declarations and the instance lists (CPMPPI_ROLLOUT_DECLARATIONS_ONLY), never the definition
            assert "cpmppi_rollout.hpp" in files and "cpmppi_rollout_kernel.inc" not in files
        else:
            assert not files & {"cpmppi_rollout.hpp", "cpmppi_rollout_kernel.inc"}, unit


@pytest.mark.parametrize("unit", HOST_ONLY)
def test_host_only_units_parse_no_integrator_cost_or_generator(deps, unit):
    assert not deps[unit] & {"cpmppi_ode.hpp", "cpmppi_cost.hpp", "cpmppi_philox.hpp"}


def test_the_brunton_header_is_the_two_seam_units_own(deps):
    assert {u for u, files in deps.items() if "cpmppi_brunton.hpp" in files} == {"cpmppi_seams.hip", "cpmppi_gru_seam.hip"}


@pytest.mark.parametrize("header", HEADERS)
def test_header_is_self_contained(header, tmp_path):
    src = tmp_path / "only.hip"
    src.write_text('#include "%s"\n' % header)
    run = subprocess.run([hipcc(), "-fsyntax-only", "--offload-arch=gfx950", "-std=c++17", *INCLUDES, str(src)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_the_header_list_is_not_empty():
    assert "cpmppi_step.hpp" in HEADERS and "cpmppi_rollout.hpp" in HEADERS and len(HEADERS) >= 16
