"""CPU: the table behind the oracle comparison of every rollout-kernel instantiation (rollout_matrix.py) is complete - it visits
exactly the rollout_cost_kernel / rollout_cost_rows_kernel symbols of the built library -, plan_rollout gives every row the build
the table names, and the inputs of the GPU test (test_gpu_rollout_matrix.py) exercise what they are meant to, judged by the oracle
alone: most rollouts of the mild envs are compared at full strength, the edge envs run the eventful path."""
import os
import sys

import numpy as np
import pytest

import launch_table as T
import rollout_matrix as M
from test_launch_plan import MATH, probe  # noqa: F401  (the fixture: plan_rollout built with the host compiler, plain and sanitized)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matrix_visits_every_rollout_kernel_of_the_library():
    """256 in both directions: a kernel added later without a matrix cell fails here, and so does a cell no kernel serves."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    built = {k["name"] for k in code_objects.kernels(_lib.LIB_PATH)
             if "19rollout_cost_kernelI" in k["name"] or "24rollout_cost_rows_kernelI" in k["name"]}
    visited = {M.instantiation(row, c, n) for row in M.ROWS for c, n in M.cells(row)}
    assert len(built) == 256 and len(visited) == 256, (len(built), len(visited))
    assert {M.instantiation(row, c, n) for row in M.MAIN_ROWS for c, n in M.cells(row)} == visited     # (the secondary shapes add none)
    served = {inst: [name for name in built if M.mangled_fragment(inst) in name] for inst in visited}
    assert all(len(names) == 1 for names in served.values()), {i: n for i, n in served.items() if len(n) != 1}
    assert {names[0] for names in served.values()} == built, sorted(built - {names[0] for names in served.values()})


def test_plan_gives_every_row_its_build(probe):  # noqa: F811
    launches = [(r.predictor == "ODE", MATH[r.options.get("math_mode", "fast")], r.options.get("rollouts_per_lane", 0), r.N, M.H,
                 M.knot_count(r), r.E, M.NOISES.index(n), r.mass_rows) for r in M.ROWS for n in r.noises]
    plans = iter(probe(launches))
    for r in M.ROWS:
        for n in r.noises:
            p = next(plans)
            got = (p["fast"], p["rpl"], p["variant"], p["blocks"], p["integ"], p["noise"], p["stash"])
            want = (r.fast, r.rpl, r.variant, r.blocks, T.integ(r), M.NOISES.index(n), r.stash if n == "philox" else 0)
            assert got == want, (r.name, n)
            assert bool(p["fold"]) == bool(r.fast and r.predictor == "ODE_v0" and r.variant == 1), (r.name, n)
    assert all(M.knot_count(r) == 34 for r in M.REGEN_ROWS) and all(M.knot_count(r) == 8 for r in M.MAIN_ROWS + M.N700_ROWS)
    assert sorted(r.E for r in M.N700_ROWS) == [129, 1537] and all(r.N == 300 for r in M.MAIN_ROWS + M.REGEN_ROWS)


def test_inputs_of_an_env_do_not_depend_on_the_launch_size():
    small, big = M.inputs(6), M.inputs(257)
    for k in small:
        assert np.array_equal(small[k], big[k][:6]), k
    assert set(M.COMMON_ENVS) <= set(M.checked_envs(6)) and {M.regime(e) for e in M.COMMON_ENVS} == {0, 1, 2, 3}
    for r in M.ROWS:
        assert {0, r.E - 1} <= set(M.checked_envs(r.E)) <= set(range(r.E)) and len(M.checked_envs(r.E)) <= 8


def _shapes():
    """One row per distinct (predictor, mass per env, E, N): what the oracle's verdict on the inputs depends on."""
    seen = {}
    for r in M.MAIN_ROWS + M.N700_ROWS:
        seen.setdefault((r.predictor, r.mass_rows, r.E, r.N), r)
    return list(seen.values())


@pytest.mark.parametrize("row", _shapes(), ids=M.row_id)
def test_inputs_exercise_what_they_are_meant_to(row):
    """From the oracle alone (perturbations from the oracle's own sampler), for the costs with a C oracle: every checked env of the two
    mild regimes has at least a third of its rollouts clear of every flag and together they have 70 %; in every checked env of the edge
    regime at least 90 % of the oracle's rollouts reach |x| > 0.95 THL.
    Measured: mild envs 260 to 294 clear of 300 (628 to 683 of 700), edge envs 300 of 300; an oracle call with probes <= 0.2 s."""
    from oracle import oracle_np as O
    envs = M.checked_envs(row.E)
    inp = M.inputs(row.E)
    rng = np.random.Generator(np.random.SFC64(5))
    du = np.stack([O.sample_delta_u(rng, row.N, M.H, np.float64(0.03 / np.sqrt(0.02)), row.period) for _ in envs]).astype(np.float32)
    for cost in M.COSTS[:3]:
        ref = M.reference(row, cost, inp, du, envs, trajectories=True)
        clear = {e: int((~M.buckets(row, cost, inp["te"][e], ref["S_a"][i], ref, i)["flagged"]).sum()) for i, e in enumerate(envs)}
        mild = [e for e in envs if M.regime(e) in (M.MILD_UP, M.MILD_DOWN)]
        edge = [i for i, e in enumerate(envs) if M.regime(e) == M.EDGE]
        assert mild and edge
        assert all(3 * clear[e] >= row.N for e in mild), (cost, clear)
        assert sum(clear[e] for e in mild) >= 0.70 * row.N * len(mild), (cost, clear)
        for i in edge:
            assert (ref["x_max"][i] > 0.95 * M.THL).sum() >= 0.90 * row.N, (cost, envs[i])
