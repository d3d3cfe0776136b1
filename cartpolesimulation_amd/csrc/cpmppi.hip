// cpmppi.hip — the hot path of libcpmppi.so: the handle, the MPPI step entry points and the launch of the rollout kernel: the
// build a launch gets is decided by plan_rollout (cpmppi_launch_plan.hpp, the one statement of that policy) and looked up here in
// a table generated from the instance lists.   See include/cpmppi.h for the contract and cpmppi_internal.hpp for the other units.
//
// Kernel inventory
//   rollout_cost_kernel<COST,FAST,NOISE,R,VARIANT,INTEG> / rollout_cost_rows_kernel<...>  (cpmppi_rollout.hpp, instantiated in cpmppi_rollout_*.hip; launched
//                                         here by launch_rollout) one lane = R rollouts, 6-float state + held control + running
//                                         cost in VGPRs; per-env data wave-uniform (SGPR); block-level soft-min partials
//                                         {min S, sum e, sum e*du[.]}; the env's last block finalizes in-kernel.
//   fold_env_kernel / fold_env_tuned_kernel  per-env constants of the throughput build, in front of each of its launches.
//   finalize_kernel<KNOT_SPACE>           merges the per-block partials of one env (rescaled to the env-wide minimum),
//                                         applies shift / update / clip, writes u_nom and Q (launches without the fused finalize).
//   finalize_tuned_kernel                 ... of a launch with per-env tuning rows: the soft-min's LBD from the env's row.
//   bump_counter_kernel                   advances a device-resident Philox step counter.
// Entry points: cpmppi_create / _destroy / _get_config / _set_cost_weights / _set_pole_mass / _set_pole_mass_rows / _set_tuning_rows / _last_error / _last_launch /
// _version / _abi_version; cpmppi_step / _step_gather / _step_host; cpmppi_set_profiling / _get_profile,
// cpmppi_debug_host_times; cpmppi_stream_create / _destroy.
#include <hip/hip_runtime.h>
#include <chrono>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <exception>
#include <vector>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_launch_plan.hpp"
#include "cpmppi_cost.hpp"          // (EnvFold and its makers: fold_env_kernel)
// the rollout kernels are launched here and defined elsewhere: this unit sees their declarations and the instance lists, not
// the definition (cpmppi_rollout.hpp)
#define CPMPPI_ROLLOUT_DECLARATIONS_ONLY
#include "cpmppi_rollout.hpp"

using namespace cpmppi_k;

// rollout_cost_kernel is instantiated in the cpmppi_rollout_*.hip units, each with its own compiler flags; nothing of it can
// be instantiated here (no definition in sight), and every instantiation the lookup below names is declared extern
namespace cpmppi_k {
CPMPPI_LATENCY_INSTANCES(CPMPPI_DECLARE_ROLLOUT)
CPMPPI_LATENCY_BUFFER_INSTANCES(CPMPPI_DECLARE_ROLLOUT)
CPMPPI_MID_INSTANCES(CPMPPI_DECLARE_ROLLOUT)
CPMPPI_MID_BUFFER_INSTANCES(CPMPPI_DECLARE_ROLLOUT)
CPMPPI_THROUGHPUT_INSTANCES(CPMPPI_DECLARE_ROLLOUT)
CPMPPI_ODE_LATENCY_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE)
CPMPPI_ODE_THROUGHPUT_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE)
CPMPPI_ODE_LONE_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE)
CPMPPI_ODE_LATENCY_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE_ROWS)
CPMPPI_ODE_THROUGHPUT_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE_ROWS)
CPMPPI_ODE_LONE_INSTANCES(CPMPPI_DECLARE_ROLLOUT_ODE_ROWS)
CPMPPI_TUNED_LATENCY_INSTANCES(CPMPPI_DECLARE_ROLLOUT_TUNED)
CPMPPI_TUNED_MID_INSTANCES(CPMPPI_DECLARE_ROLLOUT_TUNED)
CPMPPI_TUNED_THROUGHPUT_INSTANCES(CPMPPI_DECLARE_ROLLOUT_TUNED)
}  // namespace cpmppi_k
// ... and the same lists generate the launcher's lookup (find_rollout_kernel): one case per declared instantiation
#define CPMPPI_MATCH_ROLLOUT(COST, FAST, NOISE, R, V) \
  case rollout_key(COST, FAST, NOISE, R, V, PREDICTOR_ODE_V0): return &rollout_cost_kernel<COST, FAST, NOISE, R, V>;
#define CPMPPI_MATCH_ROLLOUT_ODE(COST, FAST, NOISE, R, V) \
  case rollout_key(COST, FAST, NOISE, R, V, PREDICTOR_ODE): return &rollout_cost_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>;
#define CPMPPI_MATCH_ROLLOUT_ODE_ROWS(COST, FAST, NOISE, R, V) \
  case rollout_key(COST, FAST, NOISE, R, V, PREDICTOR_ODE_ROWS): return &rollout_cost_rows_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>;
#define CPMPPI_MATCH_ROLLOUT_TUNED(COST, FAST, NOISE, R, V, INTEG) \
  case rollout_key(COST, FAST, NOISE, R, V, INTEG, 1u): return &rollout_cost_tuned_kernel<COST, FAST, NOISE, R, V, INTEG>;

// the launch plan's own constants (cpmppi_launch_plan.hpp includes nothing of the kernels) are the kernels'
static_assert(cpmppi_plan::BLOCK == BLOCK && cpmppi_plan::WAVES == WAVES, "launch plan: workgroup size");
static_assert(cpmppi_plan::INTEG_ODE_V0 == PREDICTOR_ODE_V0 && cpmppi_plan::INTEG_ODE == PREDICTOR_ODE &&
              cpmppi_plan::INTEG_ODE_ROWS == PREDICTOR_ODE_ROWS, "launch plan: INTEG");
static_assert(CPMPPI_COST_QBGM == COST_QBGM && CPMPPI_COST_DEFAULT == COST_DEFAULT && CPMPPI_COST_LEGACY == COST_LEGACY &&
              CPMPPI_COST_QBG == COST_QBG && CPMPPI_NOISE_DELTA_U == NOISE_DELTA_U && CPMPPI_NOISE_KNOTS == NOISE_KNOTS &&
              CPMPPI_NOISE_PHILOX == NOISE_PHILOX && CPMPPI_NOISE_DELTA_U_TILED == NOISE_TILED,
              "rollout lookup: the public cost / noise ids are the kernels' template arguments");

namespace {

thread_local std::string g_create_error;

template <bool KNOT_SPACE>
__global__ __launch_bounds__(BLOCK) void finalize_kernel(const Params p, const float* __restrict__ partial,
                                                         uint32_t nb, uint32_t W, const float* u_nom, float* u_nom_out,
                                                         float* __restrict__ Q_out, const GatherSync gs) {
  finalize_env<KNOT_SPACE, false>(p, partial, nb, W, u_nom, u_nom_out, Q_out, blockIdx.x, nullptr, gs);
}
// ... after a launch with per-env tuning rows (cpmppi_set_tuning_rows; Philox noise, hence knot space): the block partials were
// scaled with the ROW's LBD, so the merge takes it from the row as well (with_tuning, as the fused finalize of the tuned rollout
// kernel does).  A sibling, not an argument: finalize_kernel stays the code it was.
__global__ __launch_bounds__(BLOCK) void finalize_tuned_kernel(const Params p, const float* __restrict__ partial,
                                                               uint32_t nb, uint32_t W, const float* u_nom, float* u_nom_out,
                                                               float* __restrict__ Q_out, const GatherSync gs,
                                                               const float* tuning) {
  const Params pe = with_tuning(p, tuning + (size_t)blockIdx.x * TUNING_ROW_FLOATS);
  finalize_env<true, false>(pe, partial, nb, W, u_nom, u_nom_out, Q_out, blockIdx.x, nullptr, gs);
}

// advances a device-resident Philox step counter after a step that used it (stream-ordered; graph-replayable)
__global__ void bump_counter_kernel(unsigned long long* c) { *c += 1ull; }

uint32_t knot_count(uint32_t H, uint32_t period) { return (H + period - 1) / period + 1; }

// A public cost id as the kernels take it: their COST template argument, and for quadratic_boundary / _nonconvex - which run on
// default.py's kernels - the sub-mode.  (The way back, cpmppi_launch_info.cost_plugin, is the handle's cfg.cost_id itself.)
void set_kernel_cost(Params& p, uint32_t cost_id) {
  const bool qb = cost_id == CPMPPI_COST_QB || cost_id == CPMPPI_COST_QB_NONCONVEX;
  p.cost_id = qb ? (uint32_t)CPMPPI_COST_DEFAULT : cost_id;
  p.qb_mode = qb ? (cost_id == CPMPPI_COST_QB ? 1u : 2u) : 0u;
}

void fill_params(const cpmppi_config& c, Params& p) {
  memset(&p, 0, sizeof(p));
  p.E = c.E; p.N = c.N; p.H = c.H; p.S = c.S; p.period = c.period;
  p.P = knot_count(c.H, c.period);
  p.t_step = (float)((double)c.dt / (double)c.S);      // predictors_customization_v0.py:39
  p.k = c.k; p.m_cart = c.m_cart; p.m_pole = c.m_pole; p.g = c.g; p.J_fric = c.J_fric; p.M_fric = c.M_fric;
  p.u_max = c.u_max; p.THL = c.track_half_length; p.L_default = c.L_default;
  set_kernel_cost(p, c.cost_id);
  memcpy(p.w, c.cost_w, sizeof(p.w));
  p.R = c.R; p.LBD = c.LBD; p.NU = c.NU; p.cc_weight = c.cc_weight; p.sigma = c.sigma;
  p.lo = c.action_low; p.hi = c.action_high;
  const bool clip_run = c.control_mode == CPMPPI_CONTROL_CLIP;
  p.run_lo = clip_run ? c.action_low : -INFINITY; p.run_hi = clip_run ? c.action_high : INFINITY;
  p.horizon_reduce = c.horizon_reduce; p.control_mode = c.control_mode; p.shift_mode = c.shift_mode;
  p.correction_u = c.correction_u;
  p.interp_f32 = (c.math_mode == CPMPPI_MATH_FAST) ? 1u : 0u;
}

// Per-env constants of the throughput build (EnvFold, cpmppi_cost.hpp): one lane per env, the very device functions the
// other builds call in their prologues.  Runs in front of every throughput-build launch on the same stream (L, the targets and
// s0 are the caller's device arrays and may change between any two steps): ~2 us against launches of a millisecond and more.
__global__ __launch_bounds__(BLOCK) void fold_env_kernel(const Params p, const float* __restrict__ L, const float* __restrict__ te,
                                                         const float* __restrict__ s0, EnvFold* __restrict__ out, uint32_t envs) {
  const uint32_t env = blockIdx.x * BLOCK + threadIdx.x;
  if (env >= envs) return;
  EnvFold f;
  f.ec = make_env_const(p, L ? L[env] : p.L_default);
  f.qf = make_qbgm_folded_lane(p, te[env]);
  f.cos0 = cosf(s0[(size_t)env * 6]);
  f.inv_period = 1.0f / (float)p.period;
  f.nearlim = __builtin_fminf(p.w[6], 1.0f) * p.THL;
  out[env] = f;
}
// ... and of a launch with per-env tuning rows (cpmppi_set_tuning_rows): the same folds from the launch's block with the env's
// row in place (with_tuning_lane), so that the block holds what a handle with that row's scalars would fold.  A sibling, not a
// flag: fold_env_kernel stays the code it was.
__global__ __launch_bounds__(BLOCK) void fold_env_tuned_kernel(const Params p, const float* __restrict__ L, const float* __restrict__ te,
                                                               const float* __restrict__ s0, const float* __restrict__ tuning,
                                                               EnvFold* __restrict__ out, uint32_t envs) {
  const uint32_t env = blockIdx.x * BLOCK + threadIdx.x;
  if (env >= envs) return;
  const Params q = with_tuning_lane(p, tuning + (size_t)env * TUNING_ROW_FLOATS);
  EnvFold f;
  f.ec = make_env_const(p, L ? L[env] : p.L_default);
  f.qf = make_qbgm_folded_lane(q, te[env]);
  f.cos0 = cosf(s0[(size_t)env * 6]);
  f.inv_period = 1.0f / (float)p.period;
  f.nearlim = __builtin_fminf(q.w[6], 1.0f) * p.THL;
  out[env] = f;
}

// development aid (tools/variant_sweep.py, tools/dev/placement.py): the two size limits below which the straight-line builds are
// launched and an LDS pad, overridable from the environment - in a -DCPMPPI_DEV_KNOBS build ONLY (build_variant "devknobs"), and
// read when a handle is created, not per launch.  The shipped library has the constants of cpmppi_launch_plan.hpp: no getenv on
// the launch path, and no stray environment variable can change which kernel production launches (advisor, round 5).
struct DevKnobs { cpmppi_plan::RolloutLimits limits; uint64_t lds_pad = 0; };
static DevKnobs g_knobs;
static void refresh_dev_knobs() {
#ifdef CPMPPI_DEV_KNOBS
  auto env_u64 = [](const char* name, uint64_t dflt) {
    const char* v = getenv(name);
    return (v && *v) ? (uint64_t)strtoull(v, nullptr, 10) : dflt;
  };
  const cpmppi_plan::RolloutLimits d;
  g_knobs.limits.lone_form_max_waves = env_u64("CPMPPI_LONE_FORM_MAX_WAVES", d.lone_form_max_waves);
  g_knobs.limits.latency_max_rollouts = env_u64("CPMPPI_LATENCY_MAX_ROLLOUTS", d.latency_max_rollouts);
  g_knobs.lds_pad = env_u64("CPMPPI_LDS_PAD", 0);
#endif
}

// The instantiation a plan names, looked up in the very lists that declare the instantiations above: the launcher cannot name a
// kernel the rollout units do not define, and one listed in two units is a duplicate case.  NULL: no such build.
using RolloutKernel = void (*)(const Params, const StepPtrs);
constexpr uint32_t rollout_key(uint32_t cost, uint32_t fast, uint32_t noise, uint32_t r, uint32_t variant, uint32_t integ,
                               uint32_t tuned = 0u) {
  return cost | fast << 2 | noise << 3 | (r - 1u) << 5 | variant << 6 | integ << 8 | tuned << 10;
}
RolloutKernel find_rollout_kernel(uint32_t cost, const cpmppi_plan::RolloutPlan& plan) {
  switch (rollout_key(cost, plan.fast, plan.noise, plan.rpl, plan.variant, plan.integ, plan.tuned ? 1u : 0u)) {
    CPMPPI_LATENCY_INSTANCES(CPMPPI_MATCH_ROLLOUT)
    CPMPPI_LATENCY_BUFFER_INSTANCES(CPMPPI_MATCH_ROLLOUT)
    CPMPPI_MID_INSTANCES(CPMPPI_MATCH_ROLLOUT)
    CPMPPI_MID_BUFFER_INSTANCES(CPMPPI_MATCH_ROLLOUT)
    CPMPPI_THROUGHPUT_INSTANCES(CPMPPI_MATCH_ROLLOUT)
    CPMPPI_ODE_LATENCY_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE)
    CPMPPI_ODE_THROUGHPUT_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE)
    CPMPPI_ODE_LONE_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE)
    CPMPPI_ODE_LATENCY_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE_ROWS)
    CPMPPI_ODE_THROUGHPUT_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE_ROWS)
    CPMPPI_ODE_LONE_INSTANCES(CPMPPI_MATCH_ROLLOUT_ODE_ROWS)
    CPMPPI_TUNED_LATENCY_INSTANCES(CPMPPI_MATCH_ROLLOUT_TUNED)
    CPMPPI_TUNED_MID_INSTANCES(CPMPPI_MATCH_ROLLOUT_TUNED)
    CPMPPI_TUNED_THROUGHPUT_INSTANCES(CPMPPI_MATCH_ROLLOUT_TUNED)
    default: return nullptr;
  }
}

}  // namespace

int fail(cpmppi_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}

cpmppi_plan::RolloutPlan plan_launch(const cpmppi_handle* h, uint32_t E, uint32_t noise_kind) {
  return cpmppi_plan::plan_rollout(h->cfg, h->prm.P, E, noise_kind, h->m_pole_rows != nullptr, g_knobs.limits, h->tuning_rows != nullptr);
}

int launch_rollout(cpmppi_handle* h, const Params& prm, const cpmppi_plan::RolloutPlan& plan, hipStream_t s, const StepPtrs& a_in) {
  const RolloutKernel kernel = find_rollout_kernel(prm.cost_id, plan);
  if (!kernel)
    return fail(h, CPMPPI_ERR_BAD_ARG, "launch_rollout: no build of the rollout kernel for cost " + std::to_string(prm.cost_id) +
                ", FAST " + std::to_string(plan.fast) + ", noise " + std::to_string(plan.noise) + ", R " + std::to_string(plan.rpl) +
                ", variant " + std::to_string(plan.variant) + ", predictor " + std::to_string(plan.integ) +
                (plan.tuned ? ", tuning rows" : ""));
  StepPtrs a = a_in;
  a.env_fold = h->env_fold;
  a.m_pole = h->m_pole_rows;                       // (NULL on every predictor_ODE_v0 handle: cpmppi_set_pole_mass_rows refuses those)
  if (plan.tuned) a.tuning = h->tuning_rows;       // (the slot of m_pole: cpmppi_set_tuning_rows and _set_pole_mass_rows exclude each other)
  if (plan.fold_first && plan.tuned) {
    const uint32_t envs = plan.blocks / plan.nb;
    hipLaunchKernelGGL(fold_env_tuned_kernel, dim3((envs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, prm, a.L, a.te, a.s0, a.tuning,
                       h->env_fold, envs);
    CPMPPI_HIP(h, hipGetLastError());
  } else if (plan.fold_first) {
    const uint32_t envs = plan.blocks / plan.nb;
    hipLaunchKernelGGL(fold_env_kernel, dim3((envs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, prm, a.L, a.te, a.s0, h->env_fold, envs);
    CPMPPI_HIP(h, hipGetLastError());
  }
  size_t lds = plan.lds_bytes;
  if (g_knobs.lds_pad && plan.noise == CPMPPI_NOISE_PHILOX) {
    // development aid (tools/dev/placement.py): CPMPPI_LDS_PAD=<bytes> of extra dynamic LDS per workgroup caps how many
    // workgroups the dispatcher can put on one CU (160 KB each)
    lds += (size_t)g_knobs.lds_pad;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  hipLaunchKernelGGL(kernel, dim3(plan.blocks), dim3(BLOCK), lds, s, prm, a);
  h->last_launch = cpmppi_launch_info{prm.cost_id, h->cfg.math_mode, plan.noise, plan.rpl, plan.variant, h->cfg.ode_predictor,
                                      plan.blocks, h->cfg.cost_id};
  CPMPPI_HIP(h, hipGetLastError());
  return CPMPPI_OK;
}

int check_step(cpmppi_handle* h, const cpmppi_step_args* a) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: null args");
  if (a->E == 0 || a->E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: E out of range");
  if (!a->s0 || !a->u_nom || !a->target_position || !a->target_equilibrium)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: s0, u_nom, target_position, target_equilibrium are required");
  if (a->noise_kind > CPMPPI_NOISE_DELTA_U_TILED) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: unknown noise_kind");
  if (a->noise_kind == CPMPPI_NOISE_DELTA_U_TILED && (reinterpret_cast<uintptr_t>(a->noise) & 15u) != 0)
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_step: the tiled perturbation buffer must be 16-byte aligned");
  if (a->noise_kind == CPMPPI_NOISE_DELTA_U_TILED && a->predictor == CPMPPI_PREDICTOR_GRU)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: the GRU predictor takes delta_u, knots or Philox noise");
  if (a->noise_kind != CPMPPI_NOISE_PHILOX && !a->noise)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: noise buffer required for this noise_kind");
  if (misaligned(a->s0) || misaligned(a->u_nom) || misaligned(a->noise) || misaligned(a->S_out) ||
      misaligned(a->Q_out) || misaligned(a->u_nom_out))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_step: misaligned pointer");
  // (every check that can fail comes BEFORE the event recorder is touched: a failed step must not leave a half-recorded
  // bracket behind for cpmppi_get_profile)
  if (a->predictor > CPMPPI_PREDICTOR_GRU) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: unknown predictor");
  if (h->tuning_rows) {                            // cpmppi_set_tuning_rows: the fused ODE step with in-kernel Philox noise reads them
    if (a->predictor == CPMPPI_PREDICTOR_GRU)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: per-env tuning rows are registered (cpmppi_set_tuning_rows): not with the GRU predictor");
    if (a->noise_kind != CPMPPI_NOISE_PHILOX)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: per-env tuning rows are registered (cpmppi_set_tuning_rows): the noise must be "
                                         "CPMPPI_NOISE_PHILOX (a row holds the sampler's sigma)");
    if (a->E > h->tuning_rows_n)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: " + std::to_string(a->E) + " envs, but cpmppi_set_tuning_rows registered " +
                                         std::to_string(h->tuning_rows_n) + " rows");
  }
  if (a->predictor == CPMPPI_PREDICTOR_GRU) {
    if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: predictor GRU requested but no model set (cpmppi_set_gru)");
    if ((h->prm.cost_id != CPMPPI_COST_QBGM && h->prm.cost_id != CPMPPI_COST_DEFAULT) || h->prm.qb_mode != 0u)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step: the GRU predictor supports quadratic_boundary_grad_minimal and default");
  } else if (!pole_mass_rows_cover(h, a->E)) {     // (a GRU step does not read the pole mass)
    return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short("cpmppi_step", h, a->E));
  }
  return CPMPPI_OK;
}

// ---- the event recorder of cpmppi_set_profiling: a step's launch sequence calls begin, after_rollout and end in that order ----
// handle state: ev (triples: before the rollout kernel, after it, after the trailing kernels), ev_tail, ev_used, group_open,
// profile_count; cpmppi_get_profile reads and resets it
namespace {

struct StepBracket {
  hipEvent_t* ev = nullptr;      // this step's triple: profile_every == 1 only (no events inside a group)
  uint32_t group_pos = 0;
};

int profile_begin(cpmppi_handle* h, hipStream_t s, StepBracket* b) {
  if (!h->profile_every) return CPMPPI_OK;
  b->group_pos = h->profile_count++ % h->profile_every;
  if (b->group_pos != 0) return CPMPPI_OK;
  if (h->ev_used + 3 > h->ev.size()) {
    for (int i = 0; i < 3; ++i) {
      hipEvent_t e;
      CPMPPI_HIP(h, hipEventCreate(&e));
      h->ev.push_back(e);
    }
  }
  hipEvent_t* ev = &h->ev[h->ev_used];
  if (h->ev_tail.size() < h->ev.size() / 3) h->ev_tail.resize(h->ev.size() / 3, 0);
  h->ev_used += 3;
  h->group_open = h->profile_every > 1;
  CPMPPI_HIP(h, hipEventRecord(ev[0], s));
  if (!h->group_open) b->ev = ev;
  return CPMPPI_OK;
}

int profile_after_rollout(cpmppi_handle* h, hipStream_t s, const StepBracket& b) {
  if (b.ev) CPMPPI_HIP(h, hipEventRecord(b.ev[1], s));
  return CPMPPI_OK;
}

// tail: something ran after the rollout kernel (a separate finalize, the counter bump)
int profile_end(cpmppi_handle* h, hipStream_t s, const StepBracket& b, bool tail) {
  if (b.ev) {
    // an event costs ~5 us on the stream: the third one only if something ran after the rollout kernel
    h->ev_tail[(size_t)(b.ev - h->ev.data()) / 3] = tail ? 1 : 0;
    if (tail) CPMPPI_HIP(h, hipEventRecord(b.ev[2], s));
  }
  if (h->profile_every > 1 && h->group_open && b.group_pos == h->profile_every - 1) {     // the group's last step: close the bracket
    hipEvent_t* g = &h->ev[h->ev_used - 3];
    h->ev_tail[(h->ev_used - 3) / 3] = 0;
    CPMPPI_HIP(h, hipEventRecord(g[1], s));
    h->group_open = false;
  }
  return CPMPPI_OK;
}

}  // namespace

// check -> plan -> bracket -> launch -> finalize -> bump the counter
int step_impl(cpmppi_handle* h, const cpmppi_step_args* a, void* stream, uint32_t* host_ticket,
              const cpmppi_comm::GatherTicket* gather) {
  if (const int rc = check_step(h, a); rc != CPMPPI_OK) return rc;
  CPMPPI_ON_DEVICE(h);
  const cpmppi_plan::RolloutPlan plan = plan_launch(h, a->E, a->noise_kind);
  const bool gru = a->predictor == CPMPPI_PREDICTOR_GRU;
  const hipStream_t s = (hipStream_t)stream;
  StepPtrs p{};
  p.s0 = a->s0; p.u_nom = a->u_nom; p.u_prev = a->u_prev; p.x_t = a->target_position; p.te = a->target_equilibrium;
  p.L = a->L; p.noise = a->noise; p.prev_in = a->previous_input; p.seed = a->seed; p.offset = a->offset; p.env_offset = a->env_offset;
  p.offset_dev = (a->noise_kind == CPMPPI_NOISE_PHILOX) ? (const unsigned long long*)a->offset_dev : nullptr;
  // (the GRU rollout kernel has its own block split and never parks knots; it is no part of the plan)
  p.nb = gru ? (h->cfg.N + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK : plan.nb;
  p.W = plan.W;
  p.stash = gru ? 0u : plan.stash;
  p.S_out = a->S_out; p.partial = h->workspace;
  p.counter = (!gru && h->fuse_finalize) ? h->counters : nullptr;
  p.u_nom_out = a->u_nom_out ? a->u_nom_out : a->u_nom; p.Q_out = a->Q_out;
  p.host_ticket = host_ticket;
  p.gs = gather ? GatherSync{gather->flags, gather->publish, gather->need, gather->envs ? gather->envs : a->E} : GatherSync{nullptr, 0u, 0u, 0u};
  StepBracket bracket;
  if (const int rc = profile_begin(h, s, &bracket); rc != CPMPPI_OK) return rc;
  if (gru) {
    launch_gru_rollout(h, a, p, s);
    CPMPPI_HIP(h, hipGetLastError());
  } else if (const int rc = launch_rollout(h, h->prm, plan, s, p); rc != CPMPPI_OK) {
    return rc;
  }
  if (const int rc = profile_after_rollout(h, s, bracket); rc != CPMPPI_OK) return rc;
  const bool separate_finalize = (p.counter == nullptr);
  if (separate_finalize) {
    const bool du_space = (a->noise_kind == CPMPPI_NOISE_DELTA_U || a->noise_kind == CPMPPI_NOISE_DELTA_U_TILED);
    const auto finalize = du_space ? finalize_kernel<false> : finalize_kernel<true>;
    if (!gru && plan.tuned)                        // (check_step: Philox noise, and rows for every env of the launch)
      hipLaunchKernelGGL(finalize_tuned_kernel, dim3(a->E), dim3(BLOCK), 0, s, h->prm, (const float*)h->workspace, p.nb, p.W,
                         (const float*)a->u_nom, p.u_nom_out, a->Q_out, p.gs, h->tuning_rows);
    else
      hipLaunchKernelGGL(finalize, dim3(a->E), dim3(BLOCK), 0, s, h->prm, (const float*)h->workspace, p.nb, p.W,
                         (const float*)a->u_nom, p.u_nom_out, a->Q_out, p.gs);
  }
  CPMPPI_HIP(h, hipGetLastError());
  if (p.offset_dev) {
    hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, s, (unsigned long long*)a->offset_dev);
    CPMPPI_HIP(h, hipGetLastError());
  }
  return profile_end(h, s, bracket, separate_finalize || p.offset_dev);
}

extern "C" {

const char* cpmppi_version(void) { return "cpmppi 1 gfx950 hip"; }

const char* cpmppi_last_error(const cpmppi_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int cpmppi_last_launch(const cpmppi_handle* h, cpmppi_launch_info* out) {
  if (!h || !out) return CPMPPI_ERR_BAD_ARG;
  *out = h->last_launch;
  return CPMPPI_OK;
}

int cpmppi_create(const cpmppi_config* cfg, int device, cpmppi_handle** out) try {
  if (!cfg || !out) return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != CPMPPI_ABI_VERSION)
    return fail(nullptr, CPMPPI_ERR_ABI, "cpmppi_create: abi_version mismatch");
  if (cfg->E == 0 || cfg->N == 0 || cfg->H == 0 || cfg->S == 0 || cfg->period == 0 || cfg->H > CPMPPI_MAX_HORIZON)
    return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_create: E, N, H, S, period must be > 0 and H <= 1024");
  if (!(cfg->dt > 0.0f) || !(cfg->LBD > 0.0f) || !(cfg->NU > 0.0f) || !(cfg->L_default > 0.0f))
    return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_create: dt, LBD, NU, L_default must be > 0");
  if (cfg->cost_id > CPMPPI_COST_QB_NONCONVEX || cfg->horizon_reduce > 1 || cfg->control_mode > 1 || cfg->shift_mode > 2 ||
      cfg->correction_u > 1 || cfg->math_mode > 1 || cfg->rollouts_per_lane > 2 || cfg->ode_predictor > CPMPPI_ODE_CROMER)
    return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_create: unknown enum value");
  if ((cfg->cost_id == CPMPPI_COST_QB || cfg->cost_id == CPMPPI_COST_QB_NONCONVEX) && cfg->ode_predictor != CPMPPI_ODE_V0)
    return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_create: quadratic_boundary / _nonconvex are built for predictor_ODE_v0");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return fail(nullptr, CPMPPI_ERR_NO_DEVICE, "cpmppi_create: no HIP device (this library has no CPU fallback)");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail(nullptr, CPMPPI_ERR_NO_DEVICE, "cpmppi_create: hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, CPMPPI_ERR_NO_DEVICE,
                std::string("cpmppi_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  cpmppi_handle* h = new cpmppi_handle();
  h->cfg = *cfg;
  h->device = device;
  fill_params(*cfg, h->prm);
  h->plant_m_pole = cfg->m_pole;
  h->nb = (cfg->N + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK;     // the finest block split in use
  refresh_dev_knobs();
  if (const char* ev = getenv("CPMPPI_FUSE_FINALIZE")) h->fuse_finalize = ev[0] != '0';
  if (const char* ev = getenv("CPMPPI_HOST_ZERO_COPY_MAX")) h->host_zero_copy_max = (uint32_t)strtoul(ev, nullptr, 10);
  DeviceGuard guard(device);                     // the caller's current device is restored on every exit path
  if (guard.err != hipSuccess) {
    delete h;
    return fail(nullptr, CPMPPI_ERR_HIP, std::string("cpmppi_create: hipSetDevice: ") + hipGetErrorString(guard.err));
  }
  allow_large_lds_seams();
  allow_large_lds_optim();
  const uint32_t Wmax = cfg->H > h->prm.P ? cfg->H : h->prm.P;
  h->workspace_floats = (size_t)cfg->E * h->nb * (2 + Wmax);
  h->workspace = nullptr;
  hipError_t e = hipMalloc(&h->workspace, h->workspace_floats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&h->counters, (size_t)cfg->E * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(h->counters, 0, (size_t)cfg->E * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&h->env_fold, (size_t)cfg->E * sizeof(EnvFold));
  if (e == hipSuccess) e = hipMalloc(&h->zeros_H, (size_t)cfg->E * cfg->H * sizeof(float));
  if (e == hipSuccess) e = hipMemset(h->zeros_H, 0, (size_t)cfg->E * cfg->H * sizeof(float));
  if (e != hipSuccess) {
    std::string msg = std::string("cpmppi_create: hipMalloc workspace: ") + hipGetErrorString(e);
    delete h;
    return fail(nullptr, CPMPPI_ERR_HIP, msg);
  }
  *out = h;
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

void cpmppi_destroy(cpmppi_handle* h) {
  if (!h) return;
  DeviceGuard guard(h->device);                    // (frees, the side stream and the communicator belong to the handle's device)
  if (h->comm) { cpmppi_comm::destroy(h->comm); h->comm = nullptr; }
  if (h->workspace) (void)hipFree(h->workspace);
  if (h->gru_image) (void)hipFree(h->gru_image);
  if (h->gru16_image) (void)hipFree(h->gru16_image);
  if (h->gru_t_image) (void)hipFree(h->gru_t_image);
  if (h->gru_grad_ws) (void)hipFree(h->gru_grad_ws);
  gru_train_destroy(h);
  ode_fit_destroy(h);
  dense_destroy(h);
  if (h->brunton_ws) (void)hipFree(h->brunton_ws);
  if (h->grad_ckpt) (void)hipFree(h->grad_ckpt);
  if (h->rpgd_ws) (void)hipFree(h->rpgd_ws);
  if (h->cem_ws) (void)hipFree(h->cem_ws);
  if (h->counters) (void)hipFree(h->counters);
  if (h->env_fold) (void)hipFree(h->env_fold);
  if (h->zeros_H) (void)hipFree(h->zeros_H);
  if (h->host_stage) (void)hipHostFree(h->host_stage);
  if (h->dev_stage) (void)hipFree(h->dev_stage);
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  delete h;
}

int cpmppi_get_config(const cpmppi_handle* h, cpmppi_config* out) {
  if (!h || !out) return CPMPPI_ERR_BAD_ARG;
  *out = h->cfg;
  return CPMPPI_OK;
}

int cpmppi_set_cost_weights(cpmppi_handle* h, uint32_t cost_id, const float* cost_w, uint32_t n) {
  if (!h || !cost_w || n > 24 || cost_id > CPMPPI_COST_QB_NONCONVEX)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_cost_weights: bad argument");
  const bool qb = cost_id == CPMPPI_COST_QB || cost_id == CPMPPI_COST_QB_NONCONVEX;
  if (qb && h->cfg.ode_predictor != CPMPPI_ODE_V0)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_cost_weights: quadratic_boundary / _nonconvex are built for predictor_ODE_v0");
  if (h->tuning_rows && cost_id != CPMPPI_COST_QBGM)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_cost_weights: per-env tuning rows are registered (cpmppi_set_tuning_rows), which "
                                       "hold the cost vector of quadratic_boundary_grad_minimal");
  h->cfg.cost_id = cost_id;
  set_kernel_cost(h->prm, cost_id);
  for (uint32_t i = 0; i < n; ++i) h->cfg.cost_w[i] = h->prm.w[i] = cost_w[i];
  return CPMPPI_OK;
}

int cpmppi_set_pole_mass(cpmppi_handle* h, float m_pole) {
  if (!h || !(m_pole > 0.0f) || !(m_pole < INFINITY)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_pole_mass: m_pole must be a positive number");
  // the CONTROLLER's belief (CartPole/__init__.py:516 sends m_pole_for_controller): the predictor / cost kernels compute with it.
  // The PLANT of cpmppi_plant_advance* is the simulated system itself and keeps the mass the handle was created with
  // (plant_m_pole): a handle that serves as both must not change the plant by updating the controller's attribute.
  h->cfg.m_pole = m_pole;
  h->prm.m_pole = m_pole;
  return CPMPPI_OK;
}

int cpmppi_set_pole_mass_rows(cpmppi_handle* h, const float* m_pole, uint32_t n) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!m_pole) {                                   // back to the handle's scalar
    h->m_pole_rows = nullptr;
    h->m_pole_rows_n = 0;
    return CPMPPI_OK;
  }
  if (h->tuning_rows)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_pole_mass_rows: per-env tuning rows are registered (cpmppi_set_tuning_rows); "
                                       "the two are not built to be combined");
  if (h->cfg.ode_predictor != CPMPPI_ODE_CROMER)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_pole_mass_rows: predictor_ODE_v0 does not read the pole mass attribute "
                                       "(a per-row mass needs ode_predictor = CPMPPI_ODE_CROMER)");
  if (n == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_pole_mass_rows: n must be > 0 with a non-null array");
  if (misaligned(m_pole)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_pole_mass_rows: misaligned pointer");
  // only the POINTER is taken: the kernels of every later launch read the values when they run, so a caller (or a captured graph
  // with a copy node in front) may rewrite the array between launches without calling this again
  h->m_pole_rows = m_pole;
  h->m_pole_rows_n = n;
  return CPMPPI_OK;
}

int cpmppi_set_tuning_rows(cpmppi_handle* h, const float* rows, uint32_t n) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!rows) {                                     // back to the handle's scalars
    h->tuning_rows = nullptr;
    h->tuning_rows_n = 0;
    return CPMPPI_OK;
  }
  const auto refuse = [&](const char* why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string("cpmppi_set_tuning_rows: ") + why); };
  if (h->cfg.cost_id != CPMPPI_COST_QBGM) return refuse("a row holds the cost vector of quadratic_boundary_grad_minimal: the handle has another cost plugin");
  if (h->m_pole_rows) return refuse("per-row pole masses are registered (cpmppi_set_pole_mass_rows); the two are not built to be combined");
  if (n == 0) return refuse("n must be > 0 with a non-null array");
  if ((reinterpret_cast<uintptr_t>(rows) & (CPMPPI_TUNING_ROW_FLOATS * sizeof(float) - 1u)) != 0)
    return refuse("misaligned pointer (rows are 64 bytes and 64-byte aligned)");
  // only the POINTER is taken (as cpmppi_set_pole_mass_rows): the kernels of every later launch read the values when they run
  h->tuning_rows = rows;
  h->tuning_rows_n = n;
  return CPMPPI_OK;
}

int cpmppi_step(cpmppi_handle* h, const cpmppi_step_args* a, void* stream) { return step_impl(h, a, stream, nullptr); }

// The step and the all-gather of its result in ONE call (contract in cpmppi.h; mechanism in cpmppi_comm.hip): the launch
// stream gets the rollout kernel and nothing else; the side stream gets waiter -> ncclAllGather -> post.
int cpmppi_step_gather(cpmppi_handle* h, const cpmppi_step_args* a, float* recv_all, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a || !recv_all) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step_gather: null argument");
  if (!h->comm) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step_gather: no communicator (cpmppi_comm_init)");
  if (a->E == 0 || a->E > h->cfg.E || !a->u_nom) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step_gather: bad step arguments");
  // a wait on the device gave up (a peer rank stalled beyond cpmppi_comm_set_timeout): the steps since then have dropped their
  // results and the gathered blocks are not to be used - say so NOW, not at a cpmppi_comm_sync the caller may never make
  if (cpmppi_comm::comm_error_pending(h))
    return fail(h, CPMPPI_ERR_COMM, "cpmppi_step_gather: an earlier step's device-side wait for an all-gather timed out; "
                                    "cpmppi_comm_sync reports and clears the condition");
  // a stream being captured would bake THIS step's number into the graph: every replay would re-publish it and the side
  // stream's wait for the next step could never be satisfied (advisor, round 4)
  {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step_gather: the launch stream is being captured; a step with its all-gather "
                                         "carries a step number and cannot be part of a graph");
    (void)hipGetLastError();
  }
  const bool in_place = !a->u_nom_out || a->u_nom_out == a->u_nom;
  cpmppi_comm::GatherTicket t;
  cpmppi_comm::begin_step_gather(h->comm, in_place ? a->u_nom : a->u_nom_out, &t);
  int rc = cpmppi_comm::enqueue_guard(h, t, a->E, stream);
  if (rc == CPMPPI_OK) rc = step_impl(h, a, stream, nullptr, &t);
  if (rc != CPMPPI_OK) {
    cpmppi_comm::abort_step_gather(h->comm);
    return rc;
  }
  return cpmppi_comm::enqueue_gather(h, in_place ? a->u_nom : a->u_nom_out, recv_all, (size_t)a->E * h->cfg.H);
}

int cpmppi_step_host(cpmppi_handle* h, uint32_t E, const float* s0, const float* target_position,
                     const float* target_equilibrium, const float* L, float* u_nom, uint64_t seed, uint64_t offset,
                     uint32_t env_offset, float* Q, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !s0 || !target_position || !target_equilibrium || !u_nom || !Q)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_step_host: bad argument");
  const auto tp0 = std::chrono::steady_clock::now();
  CPMPPI_ON_DEVICE(h);
  // pinned, fine-grained, device-mapped block: [cfg.E * 10 floats: state 6, target, equilibrium, L | Q][ticket]
  const size_t cap = (size_t)h->cfg.E * 10;
  if (!h->host_stage) {
    CPMPPI_HIP(h, hipHostMalloc((void**)&h->host_stage, (cap + 16) * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h->host_stage, 0, (cap + 16) * sizeof(float));
  }
  const hipStream_t st = (hipStream_t)stream;
  float* hs = h->host_stage;
  memcpy(hs, s0, (size_t)E * 6 * sizeof(float));
  memcpy(hs + 6 * E, target_position, (size_t)E * sizeof(float));
  memcpy(hs + 7 * E, target_equilibrium, (size_t)E * sizeof(float));
  for (uint32_t e = 0; e < E; ++e) hs[8 * E + e] = L ? L[e] : h->cfg.L_default;
  cpmppi_step_args a{};
  a.E = E; a.u_nom = u_nom;
  a.noise_kind = CPMPPI_NOISE_PHILOX; a.seed = seed; a.offset = offset; a.env_offset = env_offset;
  if (h->fuse_finalize && E <= h->host_zero_copy_max) {
    // Few envs (the simulator's own call: one): no copy packets and no stream wait at all.  The kernel reads the 9 floats
    // per env straight from the pinned block over the host link, the env's finalizing block stores Q into the same
    // block and bumps a system-scope ticket; this thread spins on the ticket (a stream wait is an interrupt + a thread
    // wake-up: ~15 us of an 80 us control step).  The stream is polled now and then so that a failed launch cannot hang the caller.
    uint32_t* ticket = reinterpret_cast<uint32_t*>(hs + cap);
    const auto tp1 = std::chrono::steady_clock::now();
    a.s0 = hs; a.target_position = hs + 6 * E; a.target_equilibrium = hs + 7 * E; a.L = hs + 8 * E; a.Q_out = hs + 9 * E;
    const uint32_t target = (h->host_ticket_value += E);
    const int rc = step_impl(h, &a, stream, ticket);
    if (rc != CPMPPI_OK) { h->host_ticket_value -= E; return rc; }
    const auto tp2 = std::chrono::steady_clock::now();
    for (uint32_t spins = 1;; ++spins) {
      if (__atomic_load_n(ticket, __ATOMIC_ACQUIRE) == target) break;
      __builtin_ia32_pause();
      if ((spins & 0xFFFu) == 0u) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return fail(h, CPMPPI_ERR_HIP, std::string("cpmppi_step_host: ") + hipGetErrorString(q));
        if (__atomic_load_n(ticket, __ATOMIC_ACQUIRE) == target) break;
        // the stream drained without the ticket: resynchronise the counter and report
        h->host_ticket_value = __atomic_load_n(ticket, __ATOMIC_ACQUIRE);
        return fail(h, CPMPPI_ERR_HIP, "cpmppi_step_host: the launch completed without delivering its controls");
      }
    }
    memcpy(Q, hs + 9 * E, (size_t)E * sizeof(float));
    const auto tp3 = std::chrono::steady_clock::now();
    h->host_t[0] += std::chrono::duration<double>(tp1 - tp0).count();
    h->host_t[1] += std::chrono::duration<double>(tp2 - tp1).count();
    h->host_t[2] += std::chrono::duration<double>(tp3 - tp2).count();
    h->host_t[3] += 1.0;
    return CPMPPI_OK;
  }
  if (!h->dev_stage) CPMPPI_HIP(h, hipMalloc((void**)&h->dev_stage, cap * sizeof(float)));
  float* d = h->dev_stage;
  CPMPPI_HIP(h, hipMemcpyAsync(d, hs, (size_t)E * 9 * sizeof(float), hipMemcpyHostToDevice, st));
  a.s0 = d; a.target_position = d + 6 * E; a.target_equilibrium = d + 7 * E; a.L = d + 8 * E; a.Q_out = d + 9 * E;
  const int rc = cpmppi_step(h, &a, stream);
  if (rc != CPMPPI_OK) return rc;
  CPMPPI_HIP(h, hipMemcpyAsync(hs + 9 * E, d + 9 * E, (size_t)E * sizeof(float), hipMemcpyDeviceToHost, st));
  CPMPPI_HIP(h, hipStreamSynchronize(st));
  memcpy(Q, hs + 9 * E, (size_t)E * sizeof(float));
  return CPMPPI_OK;
}

// development aid (tools/dev/seam_latency.py; not part of the contract): mean seconds per zero-copy cpmppi_step_host call
// spent staging the inputs, inside the launch call, and spinning on the ticket; the number of calls; resets the sums
int cpmppi_debug_host_times(cpmppi_handle* h, double out[4]) {
  if (!h || !out) return CPMPPI_ERR_BAD_ARG;
  const double n = h->host_t[3] > 0 ? h->host_t[3] : 1.0;
  for (int i = 0; i < 3; ++i) out[i] = h->host_t[i] / n;
  out[3] = h->host_t[3];
  for (double& v : h->host_t) v = 0.0;
  return CPMPPI_OK;
}

int cpmppi_set_profiling(cpmppi_handle* h, int enable) {
  if (!h || enable < 0) return CPMPPI_ERR_BAD_ARG;
  h->profile_every = (uint32_t)enable;
  h->profile_count = 0;
  h->ev_used = 0;
  h->group_open = false;
  return CPMPPI_OK;
}

int cpmppi_get_profile(cpmppi_handle* h, float* rollout_ms, float* finalize_ms, uint32_t max_steps, uint32_t* n_steps) {
  if (!h || !n_steps) return CPMPPI_ERR_BAD_ARG;
  if (h->group_open) { h->ev_used -= 3; h->group_open = false; }       // an unfinished group has no closing event
  const uint32_t n = (uint32_t)(h->ev_used / 3);
  const float per = h->profile_every > 1 ? 1.0f / (float)h->profile_every : 1.0f;
  *n_steps = n;
  for (uint32_t i = 0; i < n && i < max_steps; ++i) {
    hipEvent_t* ev = &h->ev[(size_t)i * 3];
    const bool tail = h->ev_tail[i] != 0;
    CPMPPI_HIP(h, hipEventSynchronize(ev[tail ? 2 : 1]));
    float a = 0.f, b = 0.f;
    CPMPPI_HIP(h, hipEventElapsedTime(&a, ev[0], ev[1]));
    if (tail) CPMPPI_HIP(h, hipEventElapsedTime(&b, ev[1], ev[2]));
    if (rollout_ms) rollout_ms[i] = a * per;
    if (finalize_ms) finalize_ms[i] = b;
  }
  h->ev_used = 0;
  h->profile_count = 0;
  return CPMPPI_OK;
}

uint32_t cpmppi_abi_version(void) { return CPMPPI_ABI_VERSION; }

int cpmppi_stream_create(int device, void** stream_out) try {
  if (!stream_out) return fail(nullptr, CPMPPI_ERR_BAD_ARG, "cpmppi_stream_create: null argument");
  *stream_out = nullptr;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return fail(nullptr, CPMPPI_ERR_HIP, std::string("cpmppi_stream_create: hipSetDevice: ") + hipGetErrorString(guard.err));
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail(nullptr, CPMPPI_ERR_HIP, std::string("cpmppi_stream_create: ") + hipGetErrorString(e));
  // one bit per CU, all set: the mask only serves to make the runtime give this stream a queue of its own
  const uint32_t words = ((uint32_t)prop.multiProcessorCount + 31u) / 32u;
  std::vector<uint32_t> mask(words, 0xFFFFFFFFu);
  if (prop.multiProcessorCount % 32) mask[words - 1] = (1u << (prop.multiProcessorCount % 32)) - 1u;
  hipStream_t st = nullptr;
  e = hipExtStreamCreateWithCUMask(&st, words, mask.data());
  if (e != hipSuccess) {
    (void)hipGetLastError();
    e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);          // (a runtime without CU masks: an ordinary stream)
  }
  if (e != hipSuccess) return fail(nullptr, CPMPPI_ERR_HIP, std::string("cpmppi_stream_create: ") + hipGetErrorString(e));
  *stream_out = st;
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

int cpmppi_stream_destroy(void* stream) {
  if (!stream) return CPMPPI_OK;
  const hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? CPMPPI_OK : fail(nullptr, CPMPPI_ERR_HIP, std::string("cpmppi_stream_destroy: ") + hipGetErrorString(e));
}

}  // extern "C"
