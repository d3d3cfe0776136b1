// cpmppi_launch_plan.hpp — which build of rollout_cost_kernel a launch gets, and with what grid and LDS: the ONE statement of
// the library's launch policy.  plan_rollout() is a pure host function of the handle's configuration and the launch's size;
// cpmppi.hip looks the planned instantiation up and launches it, cpmppi_step and cpmppi_rollout_cost take their block split and
// LDS size from the same plan.  Plain C++ without HIP, so that a host compiler builds it into a test on its own
// (tests/test_launch_plan.py).
#pragma once
#include <stdint.h>
#include "cpmppi.h"

namespace cpmppi_plan {

// (the rollout kernels' workgroup, restated: cpmppi.hip asserts that these equal cpmppi_k::BLOCK / WAVES and that INTEG_* equal
// cpmppi::PREDICTOR_*)
constexpr uint32_t BLOCK = 256, WAVES = BLOCK / 64;
enum : uint32_t { INTEG_ODE_V0 = 0, INTEG_ODE = 1, INTEG_ODE_ROWS = 2 };
// the build VARIANT of an instantiation: the translation unit, hence the scheduling strategy, it is compiled in
enum : uint32_t { BUILD_LATENCY = 0, BUILD_THROUGHPUT = 1, BUILD_MID = 2, BUILD_LONE = 3 };

// Every size threshold of the policy (measured on MI355X with tools/kbench.py; profiles/HISTORY.md).  The *_rollouts limits of
// the build choice are compared with the launch's LANES x R (blocks x BLOCK x R), the *_waves limits with blocks x WAVES - not
// with E x N: a block that N does not fill counts whole.
struct RolloutLimits {
  // Lane mapping: two rollouts per lane (packed float2) once the launch fills every SIMD with at least one such wave
  // (1024 SIMDs x 128 rollouts); one rollout per lane (shortest critical path) below.  Measured at 128 envs x 1024 x 50:
  // 76 us packed vs 90 us one per lane; at 64 envs the packed mapping would leave half the SIMDs empty.  (E x N, the one limit
  // that is: the mapping decides the block split.)
  uint64_t packed_min_rollouts = 131072ull;
  // One rollout per lane, predictor_ODE_v0: latency build up to here, throughput build above.  (Round 5,
  // tools/variant_sweep.py: between 65536 and 131072 rollouts - where the size rule still picks one rollout per lane - the
  // straight-line latency build beats the throughput build's loop: 48 x 2048 x 50 71.3 vs 79.8 us, 96 x 1024 x 50 74.9 vs 83.3.)
  // A -DCPMPPI_DEV_KNOBS build may override it (CPMPPI_LATENCY_MAX_ROLLOUTS).
  uint64_t latency_max_rollouts = 131071ull;
  // ... predictor_ODE: latency build up to one wave per SIMD (1024 SIMDs x 64 lanes)
  uint64_t ode_latency_max_rollouts = 65536ull;
  // Two rollouts per lane, predictor_ODE_v0: at most one wave per SIMD (256 CUs x 4) gets the phased build with the quiet control
  // step unrolled (variant 3).  A -DCPMPPI_DEV_KNOBS build may override it (CPMPPI_LONE_FORM_MAX_WAVES).
  uint64_t lone_form_max_waves = 1024ull;
  // ... predictor_ODE: the substeps as straight-line code, raised wave priority (no development override)
  uint64_t ode_lone_form_max_waves = 1024ull;
  // Two rollouts per lane, predictor_ODE_v0: mid-size build (phased horizon loop: quiet control steps and eventful ones in
  // separate loops) up to here, the throughput build beyond (the 1.5 M crossover).  Phased mid-size vs throughput build,
  // envs x 1024 x 50: 256 envs 126 vs 133 us, 1024 envs 350 vs 355, 1536 envs 482 vs 495, 2048 envs 630 vs 636, 3072 envs 904
  // vs 890, 8192 envs 2.34 vs 2.29 ms
  uint64_t mid_size_max_rollouts = 1572864ull;
  // Philox: the generated knots are parked in LDS for the reduction while weighted sums + knots fit in this many bytes
  uint32_t stash_max_lds_bytes = 32u * 1024u;
};

struct RolloutPlan {
  uint32_t fast, rpl, variant, integ;   // template arguments FAST, R, VARIANT (BUILD_*), INTEG (INTEG_*)
  uint32_t noise;                       // ... and NOISE (CPMPPI_NOISE_*)
  uint32_t nb, blocks;                  // blocks per env, grid.x
  uint32_t W, lds_bytes, stash;         // width of the weighted-sum vector, dynamic LDS, Philox knots parked in LDS
  bool fold_first;                      // fold_env_kernel runs in front (throughput build, FAST, predictor_ODE_v0)
  bool tuned;                           // rollout_cost_tuned_kernel: the cost weights, LBD and sigma per env (cpmppi_set_tuning_rows)
};

// The plan of a launch of E envs of a handle configured as `cfg` (P = its knot count), perturbations of `noise_kind`; mass_rows:
// a per-env pole mass is registered (predictor_ODE only: cpmppi_set_pole_mass_rows refuses predictor_ODE_v0 handles).
// A cost-only launch (cpmppi_rollout_cost) is noise_kind = CPMPPI_NOISE_DELTA_U: W = H, nothing parked.
// tuning_rows: per-env tuning rows are registered (cpmppi_set_tuning_rows) - the same build, block split and LDS, from the tuned
// kernel's table (and, in front of the throughput build, the fold kernel that folds from the rows).
//   one rollout per lane : latency build while small, throughput build above
//   two rollouts per lane: predictor_ODE_v0: mid-size build - variant 3 while the launch has at most one wave per SIMD, variant 2
//                          above - and the throughput build beyond; predictor_ODE has no events, hence no mid-size (phased)
//                          build: its lone-wave form up to one wave per SIMD, the throughput build otherwise
//   PRECISE              : one rollout per lane, throughput build, whatever cfg.rollouts_per_lane says
inline RolloutPlan plan_rollout(const cpmppi_config& cfg, uint32_t P, uint32_t E, uint32_t noise_kind, bool mass_rows,
                                const RolloutLimits& lim = RolloutLimits{}, bool tuning_rows = false) {
  RolloutPlan r{};
  r.tuned = tuning_rows;
  r.fast = (cfg.math_mode == CPMPPI_MATH_FAST) ? 1u : 0u;
  r.noise = noise_kind;
  r.rpl = 1;
  if (r.fast) {
    if (cfg.rollouts_per_lane != 0) r.rpl = cfg.rollouts_per_lane;           // (the caller's choice wins over the size rule)
    else r.rpl = ((uint64_t)E * cfg.N >= lim.packed_min_rollouts) ? 2u : 1u;
  }
  r.nb = (cfg.N + BLOCK * r.rpl - 1) / (BLOCK * r.rpl);
  r.blocks = E * r.nb;
  const uint64_t lanes = (uint64_t)r.blocks * BLOCK, waves = (uint64_t)r.blocks * WAVES;
  const bool ode = cfg.ode_predictor == CPMPPI_ODE_CROMER;
  r.integ = ode ? (mass_rows ? INTEG_ODE_ROWS : INTEG_ODE) : INTEG_ODE_V0;
  if (!r.fast) r.variant = BUILD_THROUGHPUT;
  else if (ode && r.rpl == 2) r.variant = (waves <= lim.ode_lone_form_max_waves) ? BUILD_LONE : BUILD_THROUGHPUT;
  else if (ode) r.variant = (lanes <= lim.ode_latency_max_rollouts) ? BUILD_LATENCY : BUILD_THROUGHPUT;
  else if (r.rpl == 2)
    r.variant = (waves <= lim.lone_form_max_waves) ? BUILD_LONE : (lanes * 2 <= lim.mid_size_max_rollouts) ? BUILD_MID : BUILD_THROUGHPUT;
  else r.variant = (lanes <= lim.latency_max_rollouts) ? BUILD_LATENCY : BUILD_THROUGHPUT;
  // the throughput build reads its per-env constants (EnvFold) from memory: written on the same stream, first
  r.fold_first = r.fast && !ode && r.variant == BUILD_THROUGHPUT;
  const bool du_space = (noise_kind == CPMPPI_NOISE_DELTA_U || noise_kind == CPMPPI_NOISE_DELTA_U_TILED);
  r.W = du_space ? cfg.H : P;
  r.lds_bytes = WAVES * r.W * (uint32_t)sizeof(float);
  if (noise_kind == CPMPPI_NOISE_PHILOX) {                                   // park the generated knots in LDS when they fit
    const uint64_t park = (uint64_t)r.W * r.rpl * BLOCK * sizeof(float);
    if (r.lds_bytes + park <= lim.stash_max_lds_bytes) { r.stash = 1; r.lds_bytes += (uint32_t)park; }
  }
  return r;
}

}  // namespace cpmppi_plan
