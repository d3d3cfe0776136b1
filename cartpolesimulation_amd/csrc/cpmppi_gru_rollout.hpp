// cpmppi_gru_rollout.hpp — the one rollout of the GRU kernels that cost plans: GruRollout with its set-up, control step and cost
// epilogue, and the dispatch on the handle's cost plugin and math mode.  Included by the units whose kernels roll plans out:
// cpmppi_gru.hip (the fused MPPI step, the cost-only rollout, the gradient's forward sweep, the fused CEM step) and
// cpmppi_gru_rpgd.hip (the fused rpgd / gradient step).  The cell itself: cpmppi_gru.hpp (exact f32) and cpmppi_gru16.hpp (f16 split).
#pragma once
#include <type_traits>
#include "cpmppi_cost.hpp"
#include "cpmppi_gru16.hpp"      // (and cpmppi_gru.hpp, cpmppi_internal.hpp)

namespace {
using namespace cpmppi_k;

// The weights image of the rollout kernels: the f16 split (FAST) or the exact f32 fragments.
template <bool F16>
constexpr int GRU_ROLLOUT_IMAGE_FLOATS = F16 ? G16_IMAGE_BYTES / 4 : GRU_IMAGE_FLOATS;

// One rollout on its pair of lanes (c and c + 32 of a wave) through the horizon, as gru_rollout_cost_kernel and
// gru_cost_only_kernel carry it: set-up, one control step, cost epilogue.  How a step's input is obtained is the kernel's.
// GruRollout holds what a step changes.  What stays - the image `lds`, the env's state `s0`, the targets, `lane`, `c` = lane & 31,
// `half1` = lane >= 32 - is handed to the three functions as plain arguments without __restrict__: as members of the state, or as
// noalias arguments, the PRECISE horizon loop compiled to another schedule (0.3 % slower at 1 x 200 x 35); like this it is the
// loop the kernels had with these statements written out in each of them.
struct GruRollout {
  float st[6];
  float cost, cosang;
  f16v x, h1, h2;
  GruCarry carry;          // PRECISE
  Gru16Carry carry16;      // FAST, with gs
  Gru16State gs;
};

// development aid (-DCPMPPI_GRU_STAMPS): the stamp sums a step adds to.  The fused MPPI kernel publishes them (cpmppi_gru.hip); the
// other kernels have no stamps of their own and hand the cell an object they drop (the stamped cell takes no other form).  Empty
// in product builds.
struct GruStamps {
#ifdef CPMPPI_GRU_STAMPS
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long prev = 0;
#endif
};

// h1src, h2src: the env's two hidden states [32] or NULL = 0
template <bool F16>
__device__ __forceinline__ void gru_rollout_init(GruRollout& r, const float* lds, const float* s0, uint32_t lane,
                                                 const float* h1src, const float* h2src) {
  r.h1 = gru_load_hidden(h1src, lane);
  r.h2 = gru_load_hidden(h2src, lane);
  for (int i = 0; i < 6; ++i) r.st[i] = s0[i];
  r.cost = 0.0f;
  r.cosang = cosf(s0[0]);                 // the plugins take cos(angle) of the given state at stage 0
  if constexpr (F16) {
    r.gs.h1 = r.h1; r.gs.h2 = r.h2;
    gru16_carry_init(reinterpret_cast<const char*>(lds), r.gs, lane, r.carry16);
  } else {
    gru_carry_init(lds, r.h1, lane, r.carry);
  }
}

// Control step k with the input `ur`: clamp, stage cost, `after_stage(ur)` (what else the kernel accumulates from the clamped
// input), then the cell, the output state and the feedback.
template <int COST, bool F16, class AfterStage>
__device__ __forceinline__ void gru_rollout_step(GruRollout& r, const float* lds, const float* s0, float x_t, float te,
                                                 uint32_t lane, uint32_t c, bool half1, const Params& p, const GruNorm& nm,
                                                 uint32_t k, float ur, GruStamps& stamps, AfterStage&& after_stage) {
  if (p.control_mode == CPMPPI_CONTROL_CLIP) ur = clamp_(ur, p.lo, p.hi);
  if constexpr (COST == COST_QBGM) r.cost += stage_qbgm<float, F16>(p, r.st[4], r.cosang, r.st[1], ur, x_t, te);
  else r.cost += stage_default<float, F16>(p, r.st[4], r.cosang, ur, x_t, te);
  after_stage(ur);
  if (k == 0) r.x = gru_input_tile(nm, s0, ur, lane);
  else if (half1) r.x[1] = __builtin_fmaf(ur, nm.in_scale[0], nm.in_shift[0]);
  float out[5];
  if constexpr (F16) {
    const char* ldsb = reinterpret_cast<const char*>(lds);
#ifdef CPMPPI_GRU_STAMPS
    const f16v o = gru16_step(ldsb, r.x, r.gs, r.carry16, lane, stamps.acc, stamps.prev);
#else
    const f16v o = gru16_step(ldsb, r.x, r.gs, r.carry16, lane);
#endif
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3];
    out[4] = __shfl(o[0], (int)(c + 32u), 64);           // positionD (row 4) lives on the partner lane-half
    if (half1) out[4] = o[0];
  } else {
#ifdef CPMPPI_GRU_STAMPS
    gru_step_pipelined(lds, r.x, r.h1, r.h2, r.carry, lane, out, stamps.acc, stamps.prev);
#else
    gru_step_pipelined(lds, r.x, r.h1, r.h2, r.carry, lane, out);
#endif
  }
  gru_output_state_fast(nm, out, r.st, r.cosang);
  // normalised outputs are fed back unchanged: rows 0..3 on lane-half 0, row 4 (and Q, row 5) on lane-half 1
  r.x[0] = half1 ? out[4] : out[0];
  r.x[1] = half1 ? 0.0f : out[1];
  r.x[2] = half1 ? 0.0f : out[2];
  r.x[3] = half1 ? 0.0f : out[3];
}

// The rollout's cost after the last step: stage costs + terminal cost, reduced over the horizon.
template <int COST>
__device__ __forceinline__ float gru_rollout_total(GruRollout& r, float x_t, const Params& p) {
  r.st[0] = atan2f(r.st[3], r.st[2]);       // predictors_customization.py:121-127, needed for the terminal cost only
  const float term = (COST == COST_DEFAULT) ? terminal_indicator<float>(p, r.st[0], r.st[4], x_t) : 0.0f;
  return (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? (r.cost + term) : (r.cost + term) / (float)(p.H + 1);
}

// What gru_grad_forward_kernel parks behind control step k (k + 1 < H) for the reverse sweep, at the rollout's check-point `ck` of
// that step: both hidden tiles, each lane-half its 16 slots, and the five fed-back outputs (lane-half 0: rows 0..3, lane-half 1: row 4).
template <bool F16>
__device__ __forceinline__ void gru_rollout_park(const GruRollout& r, float* ck, bool half1) {
  gru_park_tile(ck + (half1 ? 16 : 0), F16 ? r.gs.h1 : r.h1);
  gru_park_tile(ck + 32 + (half1 ? 16 : 0), F16 ? r.gs.h2 : r.h2);
  if (!half1) *reinterpret_cast<f4v*>(ck + 64) = f4v{r.x[0], r.x[1], r.x[2], r.x[3]};
  else ck[68] = r.x[0];
}

// f(cost, f16) with the handle's cost plugin and math mode as compile-time constants (std::integral_constant).  FAST:
// float32-equivalent split products on the f16 matrix cores (cpmppi_gru16.hpp); PRECISE: exact f32 MFMA chains.
template <class F>
void gru_dispatch(const cpmppi_handle* h, F&& f) {
  const bool q = h->prm.cost_id == CPMPPI_COST_QBGM;
  const std::integral_constant<int, COST_QBGM> Q;
  const std::integral_constant<int, COST_DEFAULT> D;
  if (h->cfg.math_mode == CPMPPI_MATH_FAST && h->gru16_image) q ? f(Q, std::true_type{}) : f(D, std::true_type{});
  else q ? f(Q, std::false_type{}) : f(D, std::false_type{});
}

}  // namespace
