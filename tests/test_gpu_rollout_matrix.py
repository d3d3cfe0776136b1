"""GPU: every instantiation of the rollout kernel against the oracle at the smallest launch that selects it (rollout_matrix.py; the
host test test_rollout_matrix_host.py holds the table to the library's kernels and to plan_rollout).  One test per table row: one
sample of knots + perturbations, then for each of the row's costs the row's noise sources - in-kernel Philox of the sample's seed,
the knots, the perturbation buffer in the reference layout and re-tiled -, 16 launches for a main row.  Per launch:

  * cpmppi_last_launch equals the table's cell, kernel string included (a moved limit must not make the comparison vacuous);
  * the per-rollout costs of the checked envs (first and last block of the grid, one in the middle; one env of each input regime
    among them) against the reference, computed once per cost and shared by the noise sources, under the project's rules unchanged:
    parity's assert_costs with the quarter-band sensitivity flag under rule ODE_V0 (predictor_ODE_v0) / PREDICTOR_ODE
    (predictor_ODE), the hanging-target bound for default.py's cost with target_equilibrium < 0;
  * the updated sequence and Q against the reference (assert_controls with softmin_allowance and the probes' scatter), and against
    a float64 soft-min of the kernel's OWN costs over the read-back perturbations, shifted and clipped, to 2e-5: that pins each noise
    source's reduction whatever the conditioning.

Then, across the builds of one lane mapping (throughput vs mid-size vs lone-wave, throughput vs latency; both predictors, with and
without a pole mass per env): the costs of the envs every row checks are bit-equal for every cost and every noise source, and so
are the updated sequence and Q - every pair sums in the same order; none needed the 5e-6 granted to another summation order."""
import json

import numpy as np
import pytest

import rollout_matrix as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import parity_util as PU  # noqa: E402

f32 = np.float32
_launched = {}


def launches(row):
    """All of a row's launches, once per session: -> dict(envs, inp, du [n,N,H] of the checked envs, out {(cost, noise): dict(info,
    S [n,N], u [n,H], Q [n])}).  Only the checked envs' slices are read back."""
    if row.name in _launched:
        return _launched[row.name]
    from cartpolesimulation_amd.engine import MPPIEngine
    from cartpolesimulation_amd.configs import MPPIConfig
    E, N = row.E, row.N
    envs, inp = M.checked_envs(E), M.inputs(E)
    out, du_h, shared = {}, None, None
    for cost in row.costs:
        eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=M.H, intermediate_steps=M.SUBSTEPS, predictor_type=row.predictor,
                                       period_interpolation_inducing_points=row.period, cost_function_specification=cost,
                                       cost_weights=M.COST_WEIGHTS.get(cost, {}), **row.options))
        assert eng.P == M.knot_count(row)
        if row.mass_rows:
            eng.set_pole_mass_rows(inp["m"])
        if shared is None:
            kn, du = eng.sample(seed=M.NOISE_SEED, offset=M.NOISE_OFFSET, knots=True, delta_u=True)
            idx = torch.as_tensor(envs, device=du.device)
            du_h = du[idx].cpu().numpy()
            shared = dict(philox=dict(seed=M.NOISE_SEED, offset=M.NOISE_OFFSET), knots=dict(knots=kn), delta_u=dict(delta_u=du))
            if "delta_u_tiled" in row.noises:
                shared["delta_u_tiled"] = dict(delta_u_tiled=eng.tile_delta_u(du))
        s0, tp, te, Lv = (eng.tensor(inp[k]) for k in ("s0", "tp", "te", "L"))
        for noise in row.noises:
            un, S = eng.tensor(inp["u0"].copy()), eng.empty(E, N)
            Q, _ = eng.step(s0, un, tp, te, L=Lv, S_out=S, **shared[noise])
            info = eng.last_launch()
            out[cost, noise] = dict(info=info, S=S[idx].cpu().numpy(), u=un[idx].cpu().numpy(), Q=Q[idx].cpu().numpy())
        eng.close()
    del shared
    _launched[row.name] = dict(envs=envs, inp=inp, du=du_h, out=out)
    return _launched[row.name]


def softmin_of_own_costs(S, du, u0, LBD=100.0):
    """The update GIVEN the kernel's own costs: float64 soft-min of S over the perturbations, on the shifted sequence, clipped."""
    S = S.astype(np.float64)
    w = np.exp(-(S - S.min()) / LBD)
    ush = np.concatenate([u0[1:], u0[-1:]]).astype(np.float64)
    return np.clip(ush + (w @ du.astype(np.float64)) / w.sum(), -1.0, 1.0)


@pytest.mark.parametrize("row", M.ROWS, ids=M.row_id)
def test_every_cell_of_the_row_against_the_oracle(row):
    """Measured on MI355X (profiles/HISTORY.md holds the record per row): in all 256 cells and the secondary shapes no rollout is
    outside its allowance, flagged ones included; the worst clear rollout uses 0.31 of its allowance (mid-size build, N = 700); the
    worst |u - u_A| is 3.0e-4 in the legacy cells (costs of 1e6 at LBD = 100: inside the soft-min allowance) and 6.8e-5 elsewhere;
    the update sits within 1.9e-7 of the soft-min of the kernel's own costs everywhere.  A row takes 0.2 s."""
    L = launches(row)
    envs, inp, du = L["envs"], L["inp"], L["du"]
    te, u0 = inp["te"][envs], inp["u0"][envs]
    fails = []
    rec = dict(row=row.name, cells=0, clear=0, flagged=0, flagged_off=0, worst_clear_excess=0.0, worst_u_abs=0.0, worst_own_softmin=0.0)

    def attempt(what, check, *args, **kw):
        try:
            return check(*args, **kw)
        except AssertionError as ex:
            fails.append(f"{what}: {str(ex)[:300]}")

    for cost in row.costs:
        c_oracle = cost != "quadratic_boundary_grad"
        ref = M.reference(row, cost, inp, du, envs, trajectories=c_oracle)
        if c_oracle:
            # the comparison is not vacuous (the host test's conditions, here on the launch's own perturbations; oracle alone)
            clear = {e: int((~M.buckets(row, cost, te[i], ref["S_a"][i], ref, i)["flagged"]).sum()) for i, e in enumerate(envs)}
            mild = [e for e in envs if M.regime(e) in (M.MILD_UP, M.MILD_DOWN)]
            assert all(3 * clear[e] >= row.N for e in mild) and sum(clear[e] for e in mild) >= 0.70 * row.N * len(mild), (cost, clear)
            for i, e in enumerate(envs):
                if M.regime(e) == M.EDGE:
                    assert (ref["x_max"][i] > 0.95 * M.THL).sum() >= 0.90 * row.N, (cost, e)
        for noise in row.noises:
            o = L["out"][cost, noise]
            cell = f"{row.name} {cost} {noise}"
            rec["cells"] += 1
            want = M.expected_launch(row, cost, noise)
            if {k: o["info"][k] for k in want} != want:
                fails.append(f"{cell}: launched {o['info']}, the table says {want}")
            if not (np.isfinite(o["S"]).all() and np.isfinite(o["u"]).all() and np.array_equal(o["Q"], o["u"][:, 0])):
                fails.append(f"{cell}: a non-finite output, or Q is not the sequence's first element")
                continue
            for i, e in enumerate(envs):
                what = f"{cell} env {e} (regime {M.regime(e)})"
                b = M.buckets(row, cost, te[i], o["S"][i], ref, i)
                clear = ~b["flagged"]
                rec["clear"] += int(clear.sum()); rec["flagged"] += int(b["flagged"].sum())
                rec["flagged_off"] += int((b["off"] & b["flagged"]).sum())
                if clear.any():
                    rec["worst_clear_excess"] = max(rec["worst_clear_excess"], float(b["excess"][clear].max()))
                if cost == "default" and te[i] < 0:
                    attempt(what + " costs", M.hanging_target().assert_hanging_default_costs, o["S"][i], ref["S_a"][i], ref["S_b"][i], ref["flags"][i],
                            "hanging target", S_alt=[a[i] for a in ref["S_alt"]], H=M.H)
                else:
                    attempt(what + " costs", PU.assert_costs, o["S"][i], ref["S_a"][i], ref["S_b"][i], ref["flags"][i], "costs",
                            flag_sensitive=True, S_alt=[a[i] for a in ref["S_alt"]], rule=M.rule(row))
                rec["worst_u_abs"] = max(rec["worst_u_abs"], float(np.abs(o["u"][i] - ref["u_a"][i]).max()))
                attempt(what + " u_nom", PU.assert_controls, o["u"][i], ref["u_a"][i], ref["u_b"][i], "u_nom",
                        u_alt=[a[i] for a in ref["u_alt"]], allowance=PU.softmin_allowance(ref["S_a"][i], ref["S_b"][i], du[i]))
                own = float(np.abs(o["u"][i] - softmin_of_own_costs(o["S"][i], du[i], u0[i])).max())
                rec["worst_own_softmin"] = max(rec["worst_own_softmin"], own)
                if not own <= 2e-5:
                    fails.append(f"{what}: update differs from the soft-min of the kernel's own costs by {own:.2e}")
    print("[rollout-matrix] " + json.dumps(rec))
    assert rec["cells"] == len(M.cells(row))
    bad_cells = sorted({" ".join(f.split(" ")[1:3]) for f in fails})
    assert not fails, f"{len(fails)} failures in {len(bad_cells)} cells {bad_cells}:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("reference_row,others", M.BUILD_GROUPS, ids=[g[0] for g in M.BUILD_GROUPS])
def test_builds_of_one_lane_mapping_agree_bit_for_bit(reference_row, others):
    """An env's result must not depend on which build integrated it (test_gpu_boundary.py states this for
    quadratic_boundary_grad_minimal with Philox and knots): for every cost and every noise source the costs, the updated sequence
    and Q of envs 0 .. 3 (one of each regime) in the throughput build's launch equal, bit for bit, those of the same envs in the
    launches small enough for the mid-size, lone-wave or latency build.  The two buffer noise sources included: there the
    perturbation is read, not computed.  Which builds ran is asserted by the per-row test."""
    big = launches(M.BY_NAME[reference_row])
    assert big["envs"][:4] == M.COMMON_ENVS
    fails = []
    for name in others:
        small = launches(M.BY_NAME[name])
        assert small["envs"][:4] == M.COMMON_ENVS and np.array_equal(small["du"][:4], big["du"][:4])
        assert small["out"].keys() == big["out"].keys() and len(small["out"]) == 16
        for cell, o in small["out"].items():
            assert o["info"]["build_variant"] != big["out"][cell]["info"]["build_variant"]
            for k in ("S", "u", "Q"):
                a, b = o[k][:4], big["out"][cell][k][:4]
                if not np.array_equal(a, b):
                    d = np.abs(a.astype(np.float64) - b)
                    fails.append(f"{name} vs {reference_row} {cell} {k}: {int((a != b).sum())} of {a.size} differ, max {d.max():.3e} "
                                 f"(relative {(d / np.maximum(np.abs(b), 1e-30)).max():.3e})")
    print(f"[rollout-matrix builds] {reference_row} vs {others}: {len(fails)} differences")
    assert not fails, f"{len(fails)} differences:\n" + "\n".join(fails[:60])
