"""CPU: the launch policy of the rollout kernel (csrc/cpmppi_launch_plan.hpp, plan_rollout) is plain host C++: compiled here into
a small program of its own and held to the table of boundary shapes (launch_table.py) that the GPU suite holds the library to."""
import os
import shutil
import subprocess

import pytest

import launch_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan", "plan_probe.cpp")
FIELDS = "fast rpl variant integ noise nb blocks W lds_bytes stash fold".split()
MATH = {"fast": 1, "precise": 0}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """-> plans(launches): the probe built with g++ alone (no HIP), once plainly and once with the address and undefined-behaviour
    sanitizers (a program with its own main: nothing of it is loaded into this process)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("launch_plan") / ("probe_" + request.param))
    # (the sanitizers' runtimes linked statically: the program then runs whatever else the environment preloads into it)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] \
        if request.param == "sanitized" else []
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "cartpolesimulation_amd", "csrc"), SRC, "-o", exe])

    def plans(launches):
        text = "".join(" ".join(str(int(x)) for x in launch) + "\n" for launch in launches)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(launches)
        return [dict(zip(FIELDS, map(int, line.split()))) for line in lines]
    return plans


def knot_count(H, period):
    return (H + period - 1) // period + 1


def test_plan_matches_the_table_of_boundary_shapes(probe):
    launches = [(r.predictor == "ODE", MATH[r.options.get("math_mode", "fast")], r.options.get("rollouts_per_lane", 0), r.N, T.H,
                 knot_count(T.H, T.PERIOD), r.E, T.NOISES.index(r.noise), r.mass_rows) for r in T.ROWS]
    for r, p in zip(T.ROWS, probe(launches)):
        got = (p["fast"], p["rpl"], p["variant"], p["blocks"], bool(p["fold"]), p["integ"], p["noise"])
        assert got == (r.fast, r.rpl, r.variant, r.blocks, r.fold, T.integ(r), T.NOISES.index(r.noise)), T.row_id(r)
        assert p["nb"] * r.E == p["blocks"] and p["nb"] == -(-r.N // (256 * r.rpl)), T.row_id(r)
        assert p["W"] == (T.H if r.noise.startswith("delta_u") else knot_count(T.H, T.PERIOD)), T.row_id(r)


def test_philox_knots_are_parked_in_lds_only_while_they_fit(probe):
    """Dynamic LDS: 4 waves x W floats of weighted sums; Philox alone adds its W x R x 256 generated knots while both stay within
    32 KB.  H = 50, period 10: W = 6 knots; two rollouts per lane: 96 + 12 288 bytes.  W = 16 (H = 150): 256 + 32 768 does not fit."""
    E, N = 1, 512
    philox, knots, delta_u, tiled = (T.NOISES.index(n) for n in ("philox", "knots", "delta_u", "delta_u_tiled"))
    P6, P16 = knot_count(50, 10), knot_count(150, 10)
    assert (P6, P16) == (6, 16)
    launch = lambda rpl, H, P, noise: (0, 1, rpl, N, H, P, E, noise, 0)
    fit2, fit1, over2, under1, kn, du, dt, cost_only = probe([
        launch(2, 50, P6, philox), launch(1, 50, P6, philox), launch(2, 150, P16, philox), launch(1, 150, P16, philox),
        launch(2, 50, P6, knots), launch(2, 50, P6, delta_u), launch(2, 50, P6, tiled), launch(0, 50, P6, delta_u)])
    assert (fit2["W"], fit2["stash"], fit2["lds_bytes"]) == (6, 1, 96 + 12288)
    assert (fit1["W"], fit1["stash"], fit1["lds_bytes"]) == (6, 1, 96 + 6144)
    assert (over2["W"], over2["stash"], over2["lds_bytes"]) == (16, 0, 256)
    assert (under1["W"], under1["stash"], under1["lds_bytes"]) == (16, 1, 256 + 16384)      # (one rollout per lane: half the knots)
    assert (kn["W"], kn["stash"], kn["lds_bytes"]) == (6, 0, 96)
    for p in (du, dt, cost_only):          # delta_u space: W = H; a cost-only launch (cpmppi_rollout_cost) is a delta_u launch
        assert (p["W"], p["stash"], p["lds_bytes"]) == (50, 0, 4 * 50 * 4)
