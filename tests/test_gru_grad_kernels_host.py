"""CPU: the BUILT library's kernels of cpmppi_rollout_cost_grad_gru - gru_grad_forward_kernel<COST, F16> and
gru_grad_reverse_kernel<COST> - have no private segment and spill no VGPR (read from the code object's metadata, the way
test_rollout_kernels_have_no_scratch_and_no_vgpr_spills does it), the reverse sweep stays inside one wave's 512 registers, and the
header, the binding and the library agree on the entry point."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gradient_kernels_have_no_scratch_and_no_vgpr_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = [k for k in code_objects.kernels(_lib.LIB_PATH) if "gru_grad_" in k["name"]]
    forward = [k for k in ks if "gru_grad_forward_kernel" in k["name"]]
    reverse = [k for k in ks if "gru_grad_reverse_kernel" in k["name"]]
    assert len(forward) == 4 and len(reverse) == 2, [k["name"] for k in ks]          # 2 costs x 2 math modes; 2 costs
    bad = [(k["name"], k["private_segment_fixed_size"], k["vgpr_spill_count"]) for k in ks
           if k["private_segment_fixed_size"] != 0 or k["vgpr_spill_count"] != 0]
    assert not bad, bad
    for k in forward:                                        # two waves per SIMD, as the cost-only kernel
        assert k["vgpr_count"] + k["agpr_count"] <= 256, (k["name"], k["vgpr_count"], k["agpr_count"])
    for k in reverse:
        assert k["vgpr_count"] + k["agpr_count"] <= 512, (k["name"], k["vgpr_count"], k["agpr_count"])


def test_entry_point_is_declared_bound_and_exported():
    from cartpolesimulation_amd import _lib
    text = open(os.path.join(ROOT, "include", "cpmppi.h")).read()
    assert re.search(r"int cpmppi_rollout_cost_grad_gru\(cpmppi_handle\* h, uint32_t E, const float\* s0, const float\* inputs,\s+"
                     r"const float\* target_position, const float\* target_equilibrium, const float\* h0,\s+"
                     r"float\* S_out, float\* grad_out, void\* stream\);", text)
    assert "cpmppi_rollout_cost_grad_gru" in _lib.EXPORTS and _lib.ABI_VERSION == 5
    assert re.search(r"#define CPMPPI_ABI_VERSION 5u", text)
    lib = _lib.load()
    assert len(lib.cpmppi_rollout_cost_grad_gru.argtypes) == 10
