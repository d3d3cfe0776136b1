// cpmppi_gru.hip — the GRU predictor (BASELINE configs[4]): model upload, its predictor seam, and the fused MPPI step with it.
// The cell and its mapping onto the matrix cores: cpmppi_gru.hpp (exact f32 MFMA chains) and cpmppi_gru16.hpp (f16 split).
//
// Kernel inventory
//   gru_predict_kernel                      predictor seam with the neural predictor: trajectories [B,H+1,6], hidden states.
//   gru_advance_kernel                      one exact cell step on (state seen, control chosen), in place on h[E,2,32]: the memory
//                                           hand-over between two control periods of the device loop.
//   gru_washout_kernel                      that step along whole recordings, every row's memory kept: h_rows[R,T,2,32] (cpmppi_gru_washout).
//   gru_brunton_kernel                      Brunton test with the neural predictor (cpmppi_brunton, cpmppi_seams.hip): gru_predict_kernel's
//                                           rollout from every start row of the recordings, per-wave error statistics per horizon step.
//   gru_rollout_cost_kernel<COST,NOISE,F16> the fused MPPI step with the GRU predictor: same contract as rollout_cost_kernel
//                                           (plugin costs); launched by step_impl through launch_gru_rollout.
//   gru_cost_only_kernel<COST,F16>          costs of GIVEN input plans under the GRU predictor, nothing of the MPPI update: the
//                                           building block of the sampling optimizers (cem, cem-gmm, random-action).
//   gru_grad_forward_kernel<COST,F16>       the cost-only rollout that also parks, per control step, what the reverse sweep needs;
//   gru_grad_reverse_kernel<COST>           the reverse sweep through head, layer 2 and layer 1 (exact f32 MFMA on a transposed weights
//                                           image): d cost / d inputs of GIVEN plans - the building block of gradient, rpgd and the
//                                           CEM + gradient hybrids over the GRU (gru_adjoint=True).
// The rollout kernels share one rollout (GruRollout: gru_rollout_init, gru_rollout_step, gru_rollout_total) and differ in where
// a step's input comes from and in what becomes of the costs; gru_predict_kernel runs the exact cell (gru_step) on its own.
// Entry points: cpmppi_set_gru, cpmppi_gru_predict, cpmppi_gru_advance, cpmppi_gru_washout, cpmppi_rollout_cost_gru, cpmppi_rollout_cost_grad_gru; -DCPMPPI_GRU_STAMPS: cpmppi_debug_gru_stamps (the kernels that write
// g_gru_stamp_sum are this unit's).
#include <hip/hip_runtime.h>
#include <math.h>
#include <exception>
#include <string>
#include <vector>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_gru.hpp"
#include "cpmppi_gru16.hpp"
#include "cpmppi_grad.hpp"       // (stage_qbgm_grad, stage_default_grad)

using namespace cpmppi_k;

namespace {

__device__ __forceinline__ void gru_load_image(float* __restrict__ lds, const float* __restrict__ image, int floats) {
  for (int i = threadIdx.x; i < floats; i += BLOCK) lds[i] = image[i];
  __syncthreads();
}

// The weights image of the two rollout kernels: the f16 split (FAST) or the exact f32 fragments.
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

// development aid (-DCPMPPI_GRU_STAMPS): the stamp sums a step adds to.  The fused kernel publishes them; the cost-only kernel has no
// stamps of its own and hands the cell an object it drops (the stamped cell takes no other form).  Empty in product builds.
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

// predictor seam with the neural predictor: s0[B,6], Q[B,H], h0[2,B,32] or NULL -> traj[B,H+1,6], h_out[2,B,32] or NULL
// (one wave per SIMD: the exact-f32 MFMA chain of gru_step with all its fragment loads in flight wants more than 256 registers -
// compiled for two waves per SIMD it spilled 38 of them to a 156-byte scratch slot; the seam is bound by the matrix pipe either way)
__global__ __launch_bounds__(BLOCK, 1) void gru_predict_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t B,
                                                            uint32_t H, const float* __restrict__ s0,
                                                            const float* __restrict__ Q, const float* __restrict__ h0,
                                                            float* __restrict__ traj, float* __restrict__ h_out) {
  extern __shared__ float lds[];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u;
  const size_t b = (size_t)blockIdx.x * GRU_ROLLOUTS_PER_BLOCK + wave * 32 + c;
  const bool valid = b < B;
  const size_t bb = valid ? b : 0;
  const float* s = s0 + bb * 6;
  f16v h1 = gru_load_hidden(h0 ? h0 + bb * 32 : nullptr, lane);
  f16v h2 = gru_load_hidden(h0 ? h0 + ((size_t)B + bb) * 32 : nullptr, lane);
  f16v x = gru_input_tile(nm, s, Q[bb * H], lane);
  float* o = traj + bb * (size_t)(H + 1) * 6;
  if (valid && lane < 32) for (int i = 0; i < 6; ++i) o[i] = s[i];
  for (uint32_t k = 0; k < H; ++k) {
    const f16v out = gru_step(lds, x, h1, h2, lane);
    float st[6];
    gru_output_state(nm, out, lane, st);
    if (valid && lane < 32) {
      o += 6;
      for (int i = 0; i < 6; ++i) o[i] = st[i];
    }
    x = out;                                               // normalised outputs are fed back unchanged
    if (lane >= 32 && k + 1 < H) x[1] = __builtin_fmaf(Q[bb * H + k + 1], nm.in_scale[0], nm.in_shift[0]);
  }
  if (h_out && valid) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      h_out[bb * 32 + gru_tile_row(v, lane >> 5)] = h1[v];
      h_out[((size_t)B + bb) * 32 + gru_tile_row(v, lane >> 5)] = h2[v];
    }
  }
}

// The memory hand-over of the device loop: h_io[E,2,32] (the rollout kernels' layout) <- hidden states after ONE exact cell step
// on (s[E,6], Q[E]), in place.  gru_predict_kernel's mapping (env e on lanes c and c + 32 of a wave, one wave per SIMD for the
// same reason) and its cell, so what it stores is what that kernel writes to h_out for B = E, H = 1; the head's result is
// dropped, nothing is de-normalised.  In place is safe: all of a live env's loads precede its stores in its own wave, and no
// other wave stores to its rows.  A lane beyond E repeats row 0, which block 0 may be rewriting at that moment: what it then
// computes is undefined but never stored (an MFMA column depends on its own column only, so it reaches no live env either).
__global__ __launch_bounds__(BLOCK, 1) void gru_advance_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t E,
                                                            const float* __restrict__ s, const float* __restrict__ Q,
                                                            float* h_io) {
  extern __shared__ float lds[];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u;
  const size_t e = (size_t)blockIdx.x * GRU_ROLLOUTS_PER_BLOCK + wave * 32 + c;
  const bool valid = e < E;
  const size_t ee = valid ? e : 0;
  float* hrow = h_io + ee * 64;
  f16v h1 = gru_load_hidden(hrow, lane);
  f16v h2 = gru_load_hidden(hrow + 32, lane);
  const f16v x = gru_input_tile(nm, s + ee * 6, Q[ee], lane);
  (void)gru_step(lds, x, h1, h2, lane);
  if (valid) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      hrow[gru_tile_row(v, lane >> 5)] = h1[v];
      hrow[32 + gru_tile_row(v, lane >> 5)] = h2[v];
    }
  }
}

// A lane's registers of both hidden tiles -> one memory row [2,32] (the layout of cpmppi_step_args.h0).
__device__ __forceinline__ void gru_store_memory(float* hrow, const f16v& h1, const f16v& h2, uint32_t lane) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    hrow[gru_tile_row(v, lane >> 5)] = h1[v];
    hrow[32 + gru_tile_row(v, lane >> 5)] = h2[v];
  }
}

// The memory along recordings (update_before_predicting of the reference's Brunton test): h_rows[r,0] = h0[r] (NULL: zeros),
// h_rows[r,t+1] = the memory after ONE exact cell step on (states[r,t], Q[r,t]) from h_rows[r,t] - what T-1 successive
// cpmppi_gru_advance calls leave, bit for bit: gru_advance_kernel's mapping (recording r on lanes c and c + 32 of a wave, one wave
// per SIMD) and its cell, with the memory kept in registers between the rows instead of going through h_io.  The next row's state
// and control do not depend on the cell: they are loaded one row ahead.  A wave without a recording leaves behind the image
// load's barrier, the kernel's only one; a lane beyond R in a live wave repeats recording 0 and stores nothing.
__global__ __launch_bounds__(BLOCK, 1) void gru_washout_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t R,
                                                            uint32_t T, const float* __restrict__ states,
                                                            const float* __restrict__ Q, const float* __restrict__ h0,
                                                            float* __restrict__ h_rows) {
  extern __shared__ float lds[];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u;
  const size_t r0 = (size_t)blockIdx.x * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (r0 >= R) return;                                     // (wave-uniform) a tile without a recording
  const bool valid = r0 + c < R;
  const size_t rr = valid ? r0 + c : 0;
  f16v h1 = gru_load_hidden(h0 ? h0 + rr * 64 : nullptr, lane);
  f16v h2 = gru_load_hidden(h0 ? h0 + rr * 64 + 32 : nullptr, lane);
  const float* __restrict__ s = states + rr * T * 6;
  const float* __restrict__ q = Q + rr * T;
  float* hrow = h_rows + rr * T * 64;
  if (valid) gru_store_memory(hrow, h1, h2, lane);
  float sn[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
  float qn = q[0];
  for (uint32_t t = 0; t + 1 < T; ++t) {
    const f16v x = gru_input_tile(nm, sn, qn, lane);
    if (t + 2 < T) {                                       // in flight during this row's cell
#pragma unroll
      for (int i = 0; i < 6; ++i) sn[i] = s[(size_t)(t + 1) * 6 + i];
      qn = q[t + 1];
    }
    (void)gru_step(lds, x, h1, h2, lane);
    hrow += 64;
    if (valid) gru_store_memory(hrow, h1, h2, lane);
  }
}

// Brunton test with the neural predictor: gru_predict_kernel's mapping (32 starts per wave on lanes c and c + 32, one wave per
// SIMD) and its exact-f32 cell, begun at states[r,t] with the memory h_rows[r,t] (NULL: zeros) and fed the RECORDED controls
// Q[r,t+k]; after step k the de-normalised state (gru_output_state: angle = atan2(sin, cos), as in the seam) is compared with
// states[r,t+k+1] (brunton_errors).  The states live on lanes 0..31; the other half and the lanes beyond the last start enter the
// statistics as zeros.  One partial row per WAVE, written by its lane 0 with plain stores: after the image load no wave depends
// on another, so a wave whose 32 starts all lie beyond the last one leaves at once - there is no second barrier it could be
// missed at, and no row of the partials for it (brunton_gru_rows counts the live waves, which are the first ones).
__global__ __launch_bounds__(BLOCK, 1) void gru_brunton_kernel(const GruNorm nm, const float* __restrict__ image,
                                                            const BruntonArgs a) {
  extern __shared__ float lds[];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);            // the kernel's only barrier
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u;
  const size_t starts = (size_t)a.R * a.count;
  const size_t wave_row = (size_t)blockIdx.x * WAVES + wave;
  const size_t b0 = wave_row * 32;
  if (b0 >= starts) return;                                // (wave-uniform) a tile without a start
  const bool valid = b0 + c < starts;
  const size_t b = valid ? b0 + c : 0;
  const size_t row = (b / a.count) * a.T + a.start + b % a.count;          // (r, t) in the series
  const float* s = a.states + row * 6;
  f16v h1 = gru_load_hidden(a.h_rows ? a.h_rows + row * 64 : nullptr, lane);
  f16v h2 = gru_load_hidden(a.h_rows ? a.h_rows + row * 64 + 32 : nullptr, lane);
  f16v x = gru_input_tile(nm, s, a.Q[row], lane);
  const bool owner = valid && lane < 32;                   // the lane that accounts for start b
  float* o = a.pred ? a.pred + b * (size_t)(a.horizon + 1) * 6 : nullptr;
  if (o && owner) for (int i = 0; i < 6; ++i) o[i] = s[i];
  float* __restrict__ out = a.partials + wave_row * a.horizon * BRUNTON_STATS;
  for (uint32_t k = 0; k < a.horizon; ++k) {
    const f16v y = gru_step(lds, x, h1, h2, lane);
    float st[6];
    gru_output_state(nm, y, lane, st);
    if (o && owner) {
      o += 6;
      for (int i = 0; i < 6; ++i) o[i] = st[i];
    }
    float e[6];
    brunton_errors(st, a.states + (row + k + 1) * 6, e);
    brunton_wave_stats(e, owner, lane == 0, out + (size_t)k * BRUNTON_STATS);
    x = y;                                                 // normalised outputs are fed back unchanged
    if (lane >= 32 && k + 1 < a.horizon) x[1] = __builtin_fmaf(a.Q[row + k + 1], nm.in_scale[0], nm.in_shift[0]);
  }
}

// Fused MPPI step with the GRU predictor: same contract as rollout_cost_kernel (plugin costs), h0[E,2,32] or NULL.
template <int COST, int NOISE, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_rollout_cost_kernel(const Params p, const StepPtrs a, const GruNorm nm,
                                                                 const float* __restrict__ image,
                                                                 const float* __restrict__ h0) {
  extern __shared__ float lds[];                           // GRU image, then [WAVES][W] weighted sums
  __shared__ float red[2 * WAVES];
  constexpr int IMAGE_FLOATS = GRU_ROLLOUT_IMAGE_FLOATS<F16>;
  gru_load_image(lds, image, IMAGE_FLOATS);
  float* bsum = lds + IMAGE_FLOATS;
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  const uint32_t n = row0 + c;
  const bool owner = lane < 32 && n < p.N;                 // the lane that accounts for rollout n
  const uint32_t nn = n < p.N ? n : 0;
  const uint32_t H = p.H;
  const uint64_t step_offset = a.offset_dev ? (uint64_t)*a.offset_dev : a.offset;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ un = a.u_nom + (size_t)env * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, h0 ? h0 + (size_t)env * 64 : nullptr, h0 ? h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;

  auto knot = [&](uint32_t j) __attribute__((always_inline)) -> float {
    if constexpr (NOISE == NOISE_KNOTS) return a.noise[((size_t)env * p.N + nn) * p.P + j];
    else return philox_knot(a.seed, step_offset, a.env_offset + env, nn, j, p.sigma);
  };
  float z_lo = 0.0f, z_hi = 0.0f;
  if constexpr (NOISE != NOISE_DELTA_U) { z_lo = knot(0); z_hi = knot(1); }
  uint32_t ii = 0, j = 0;
  float corr = 0.0f;
  GruStamps stamps;
#ifdef CPMPPI_GRU_STAMPS
  stamps.prev = __builtin_amdgcn_s_memtime();
#endif
  for (uint32_t k = 0; k < H; ++k) {
    float du;
    if constexpr (NOISE == NOISE_DELTA_U) du = a.noise[((size_t)env * p.N + nn) * H + k];
    else if constexpr (F16 && NOISE == NOISE_PHILOX)      // FAST + own noise: one float32 FMA, as the ODE kernel and the sampler
      du = interp_from_slope32(knot_slope32(z_lo, z_hi, 1.0f / (float)p.period), z_lo, ii);
    else du = interp_knots(z_lo, z_hi, ii, p.period);
    const float uk = shifted_nominal(p, un, k);
    float ur = uk + du;
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, stamps, [&](float u) __attribute__((always_inline)) {
      corr += mppi_correction<float>(p, p.correction_u == CPMPPI_CORRECTION_U_RUN ? u : uk, du);
    });
    if constexpr (NOISE != NOISE_DELTA_U) {
      if (++ii == p.period) {
        ii = 0; ++j;
        z_lo = z_hi;
        if (j + 1 < p.P) z_hi = knot(j + 1);
      }
    }
  }
#ifdef CPMPPI_GRU_STAMPS
  if (lane == 0)
    for (int i = 0; i < 6; ++i) atomicAdd(&g_gru_stamp_sum[i], stamps.acc[i]);
  if (lane == 0) atomicAdd(&g_gru_stamp_sum[6], 1ull);
#endif
  const float S_total = gru_rollout_total<COST>(ro, x_t, p) + corr;
  if (a.S_out && owner) a.S_out[(size_t)env * p.N + n] = S_total;

  const float m_w = wave_min(owner ? S_total : INFINITY);
  if (lane == 0) red[wave] = m_w;
  __syncthreads();
  float m_b = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) m_b = fminf(m_b, red[w]);
  const float e = owner ? expf((-1.0f / p.LBD) * (S_total - m_b)) : 0.0f;
  const float a_w = wave_sum(e);
  if (lane == 0) red[WAVES + wave] = a_w;
  const uint32_t W = a.W;
  float* __restrict__ my_bsum = bsum + wave * W;
  if constexpr (NOISE == NOISE_PHILOX) {
    for (uint32_t jj = 0; jj < W; ++jj) {
      const float v = wave_sum(e * philox_knot(a.seed, step_offset, a.env_offset + env, nn, jj, p.sigma));
      if (lane == 0) my_bsum[jj] = v;
    }
  } else {
    const float* __restrict__ src = a.noise + ((size_t)env * p.N + row0) * W;
    const uint32_t rows = (row0 < p.N) ? ((p.N - row0 < 32u) ? p.N - row0 : 32u) : 0u;
    for (uint32_t c0 = 0; c0 < W; c0 += 64) {
      const uint32_t col = c0 + lane;
      float acc = 0.0f;
      const float* __restrict__ colp = src + (col < W ? col : 0u);
      uint32_t r = 0;
      for (; r + 8 <= rows; r += 8) {                      // eight independent row loads in flight (latency-bound pass)
        float xr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xr[u] = colp[(size_t)(r + u) * W];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), r + u)), xr[u], acc);
      }
      for (; r < rows; ++r)
        acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), r)), colp[(size_t)r * W], acc);
      if (col < W) my_bsum[col] = acc;
    }
  }
  __syncthreads();
  float* __restrict__ outp = a.partial + ((size_t)env * a.nb + blk) * (2 + W);
  if (tid == 0) {
    float a_b = red[WAVES];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) a_b += red[WAVES + w];
    outp[0] = m_b;
    outp[1] = a_b;
  }
  for (uint32_t cc = tid; cc < W; cc += BLOCK) {
    float v = bsum[cc];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += bsum[w * W + cc];
    outp[2 + cc] = v;
  }
}

// Cost-only rollout with the GRU predictor: S[env][n] = get_trajectory_cost(predict_core_GRU(s0[env], inputs[env][n]), inputs[env][n]).
// What gru_rollout_cost_kernel<COST, NOISE_DELTA_U, F16> computes for a zero nominal sequence, no shift and cc_weight = 0 - same
// tile mapping (32 rollouts per wave, GRU_ROLLOUTS_PER_BLOCK per workgroup, grid E x nb) and the same GruRollout set-up, step and
// epilogue - without anything that serves the MPPI update: no block minimum, no weights, no weighted sums of the noise, no
// partials.  Dynamic LDS holds the weights image only, and after its load no wave depends on another: a wave whose 32 rollouts
// all lie beyond N leaves at once, and there is no barrier behind the one of the image load.
// The lane's next input does not depend on the state: it is loaded one control step ahead, off the recurrent chain.
struct GruCostPtrs {
  const float* s0;       // [E,6]
  const float* inputs;   // [E,N,H]
  const float* x_t;      // [E] target position
  const float* te;       // [E] target equilibrium
  const float* h0;       // [E,2,32] or NULL = 0
  float* S_out;          // [E,N]
  uint32_t nb;           // blocks per env
};

template <int COST, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_cost_only_kernel(const Params p, const GruCostPtrs a, const GruNorm nm,
                                                                              const float* __restrict__ image) {
  extern __shared__ float lds[];                           // GRU image only
  gru_load_image(lds, image, GRU_ROLLOUT_IMAGE_FLOATS<F16>);   // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool owner = lane < 32 && n < p.N;                 // the lane that accounts for rollout n
  const uint32_t nn = n < p.N ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, a.h0 ? a.h0 + (size_t)env * 64 : nullptr, a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;
  GruStamps none;
  float u_next = in[0];
  for (uint32_t k = 0; k < H; ++k) {
    const float ur = u_next;
    if (k + 1 < H) u_next = in[k + 1];                     // in flight during this step's cell
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
  }
  const float S_total = gru_rollout_total<COST>(ro, x_t, p);
  if (owner) a.S_out[(size_t)env * p.N + n] = S_total;
}

// FAST: float32-equivalent split products on the f16 matrix cores (cpmppi_gru16.hpp); PRECISE: exact f32 MFMA chains
inline bool gru_runs_f16(const cpmppi_handle* h) { return h->cfg.math_mode == CPMPPI_MATH_FAST && h->gru16_image != nullptr; }

template <int COST>
void launch_gru_cost_only(cpmppi_handle* h, const GruCostPtrs& a, uint32_t E, hipStream_t s) {
  const bool f16 = gru_runs_f16(h);
  const dim3 grid(E * a.nb);
  if (f16) hipLaunchKernelGGL((gru_cost_only_kernel<COST, true>), grid, dim3(BLOCK), (size_t)G16_IMAGE_BYTES, s, h->prm, a,
                              h->gru_norm, (const float*)h->gru16_image);
  else hipLaunchKernelGGL((gru_cost_only_kernel<COST, false>), grid, dim3(BLOCK), (size_t)GRU_IMAGE_FLOATS * sizeof(float), s,
                          h->prm, a, h->gru_norm, (const float*)h->gru_image);
}

// ---- cost and gradient: cpmppi_rollout_cost_grad_gru = gru_grad_forward_kernel, then gru_grad_reverse_kernel, on one stream.
// Two launches rather than one kernel that swaps its LDS image between the sweeps: each keeps the cost-only kernel's shape (one
// barrier, behind the image load; a wave without a rollout leaves at once) and the forward half IS the cost-only kernel plus
// its check-point stores.  The sweeps meet in global memory either way.
struct GruGradPtrs {
  const float* s0;       // [E,6]
  const float* inputs;   // [E,N,H]
  const float* x_t;      // [E] target position
  const float* te;       // [E] target equilibrium
  const float* h0;       // [E,2,32] or NULL = 0
  float* S_out;          // [E,N] or NULL
  float* grad;           // [E,N,H]
  float* ckpt;           // [H][rows][GRU_CKPT_FLOATS]: after control step k, hidden tiles and fed-back outputs of every rollout
  size_t rows;           // E N of this launch
  uint32_t nb;           // blocks per env
};
constexpr size_t GRU_GRAD_REVERSE_LDS = ((size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS) * sizeof(float);   // 98 208 B: opt-in

typedef float f4v __attribute__((ext_vector_type(4)));

// A lane's 16 registers of a hidden tile <-> 16 consecutive floats of a check-point (4 x 16 bytes).
__device__ __forceinline__ void gru_park_tile(float* dst, const f16v& h) {
#pragma unroll
  for (int q = 0; q < 4; ++q) reinterpret_cast<f4v*>(dst)[q] = f4v{h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]};
}
__device__ __forceinline__ f16v gru_fetch_tile(const float* src) {
  f16v h;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f4v t = reinterpret_cast<const f4v*>(src)[q];
    h[4 * q] = t.x; h[4 * q + 1] = t.y; h[4 * q + 2] = t.z; h[4 * q + 3] = t.w;
  }
  return h;
}

// Forward sweep: gru_cost_only_kernel (same set-up, step and epilogue, in the handle's math mode) that parks, after every control
// step but the last, what the reverse sweep starts from - the last step's cell produces a state that no stage costs.
template <int COST, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_grad_forward_kernel(const Params p, const GruGradPtrs a, const GruNorm nm,
                                                                                 const float* __restrict__ image) {
  extern __shared__ float lds[];                           // GRU image only
  gru_load_image(lds, image, GRU_ROLLOUT_IMAGE_FLOATS<F16>);   // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool live = n < p.N, owner = lane < 32 && live;
  const uint32_t nn = live ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, a.h0 ? a.h0 + (size_t)env * 64 : nullptr, a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;
  float* ck = a.ckpt + ((size_t)env * p.N + nn) * GRU_CKPT_FLOATS;        // the rollout's check-point of step 0
  const size_t ck_step = a.rows * GRU_CKPT_FLOATS;
  GruStamps none;
  float u_next = in[0];
  for (uint32_t k = 0; k < H; ++k) {
    const float ur = u_next;
    if (k + 1 < H) u_next = in[k + 1];                     // in flight during this step's cell
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
    if (k + 1 < H && live) {                               // rows >= N are never written
      gru_park_tile(ck + (half1 ? 16 : 0), F16 ? ro.gs.h1 : ro.h1);
      gru_park_tile(ck + 32 + (half1 ? 16 : 0), F16 ? ro.gs.h2 : ro.h2);
      if (!half1) *reinterpret_cast<f4v*>(ck + 64) = f4v{ro.x[0], ro.x[1], ro.x[2], ro.x[3]};
      else ck[68] = ro.x[0];
    }
    ck += ck_step;
  }
  const float S_total = gru_rollout_total<COST>(ro, x_t, p);
  if (a.S_out && owner) a.S_out[(size_t)env * p.N + n] = S_total;
}

// One GRU layer of the reverse sweep for the wave's 32 rollouts.  Recomputes the layer's gates (exact f32, the order of gru_layer)
// from its input tile x (KX k-steps) and the hidden tile hp the step began with, then turns dh - in: the adjoint of the step's
// new hidden state, out: the direct part z * dh of the adjoint of hp - into the adjoints of the four pre-activation tiles: r, z,
// n's input part and n's hidden part.
template <int KX>
__device__ __forceinline__ void gru_layer_reverse(const float* lds, int fx, int fh, int b0, const f16v& x, const f16v& hp,
                                                  uint32_t lane, f16v& dh, f16v& dar, f16v& daz, f16v& danx, f16v& danh) {
  f16v ar = gru_mm<KX>(gru_bias_v(lds, b0 + 0, lane), lds + (fx + 0 * KX) * 64, x, lane);
  f16v az = gru_mm<KX>(gru_bias_v(lds, b0 + 1, lane), lds + (fx + 1 * KX) * 64, x, lane);
  const f16v anx = gru_mm<KX>(gru_bias_v(lds, b0 + 2, lane), lds + (fx + 2 * KX) * 64, x, lane);
  ar = gru_mm<16>(ar, lds + (fh + 0) * 64, hp, lane);
  az = gru_mm<16>(az, lds + (fh + 16) * 64, hp, lane);
  const f16v anh = gru_mm<16>(gru_bias_v(lds, b0 + 3, lane), lds + (fh + 32) * 64, hp, lane);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float r = gru_sigmoid(ar[v]);
    const float z = gru_sigmoid(az[v]);
    const float n = gru_tanh(__builtin_fmaf(r, anh[v], anx[v]));
    const float d = dh[v];
    const float dn = d * (1.0f - z);                          // h = (1 - z) n + z hp
    const float dz = d * (hp[v] - n);
    const float dan = dn * __builtin_fmaf(-n, n, 1.0f);       // n = tanh(anx + r anh)
    danx[v] = dan;
    danh[v] = dan * r;
    dar[v] = (dan * anh[v]) * (r * (1.0f - r));
    daz[v] = dz * (z * (1.0f - z));
    dh[v] = d * z;
  }
}

// Reverse sweep, exact-f32 MFMA in both math modes.  Per control step k = H-2 .. 0 (the cell of step H-1 feeds no cost), from the
// check-points of steps k (outputs, layer-1 hidden tile) and k-1 (both hidden tiles, outputs = the input features; k = 0: the
// env's memory and state): head adjoint, layer-2 cell, layer-1 cell, each layer's gates recomputed right before its adjoint.
// Row 5 of the input adjoint is d/dQ[k]; rows 0..4 are the feedback into the outputs of step k-1, which also collect the
// partials of stage k through the de-normalisation.  LDS: the forward f32 image (gates) and the transposed one.  A column
// beyond N repeats the env's rollout 0 and is never written.
template <int COST>
__global__ __launch_bounds__(BLOCK, 1) void gru_grad_reverse_kernel(const Params p, const GruGradPtrs a, const GruNorm nm,
                                                                    const float* __restrict__ image,
                                                                    const float* __restrict__ image_t) {
  extern __shared__ float lds[];                           // forward f32 image, then the transposed image
  float* ldst = lds + GRU_IMAGE_FLOATS;
  for (int i = threadIdx.x; i < GRU_T_IMAGE_FLOATS; i += BLOCK) ldst[i] = image_t[i];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);            // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool live = n < p.N, half1 = lane >= 32, owner = !half1 && live;
  const uint32_t nn = live ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  float* __restrict__ g = a.grad + ((size_t)env * p.N + nn) * H;
  const size_t ck_step = a.rows * GRU_CKPT_FLOATS;
  const uint32_t hoff = half1 ? 16u : 0u;                  // the lane's 16 slots inside a hidden tile
  const float scale = (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? 1.0f : 1.0f / (float)(p.H + 1);
  const bool clip = p.control_mode == CPMPPI_CONTROL_CLIP;
  auto stage_u = [&](float u) __attribute__((always_inline)) -> float {      // d stage / d u: the direct control term
    if constexpr (COST == COST_QBGM) return stage_qbgm_grad(p, 0.0f, 1.0f, 0.0f, u, x_t, te).u;
    else return stage_default_grad(p, 0.0f, 1.0f, u, x_t, te).u;
  };
  {                                                        // the last input: its cell is never costed
    const float q = in[H - 1];
    const bool clipped = clip && (q < p.lo || q > p.hi);
    if (owner) g[H - 1] = clipped ? 0.0f : scale * stage_u(q);
  }
  if (H < 2) return;

  f16v dh1, dh2;                                           // adjoints of the hidden tiles behind step k
#pragma unroll
  for (int v = 0; v < 16; ++v) { dh1[v] = 0.0f; dh2[v] = 0.0f; }
  float dfb[4] = {0.0f, 0.0f, 0.0f, 0.0f};                 // feedback: adjoint of step k's outputs through the input tile of step k + 1
  const float* ck = a.ckpt + ((size_t)env * p.N + nn) * GRU_CKPT_FLOATS + (size_t)(H - 2) * ck_step;   // check-point of step k
  for (uint32_t k = H - 1; k-- > 0; ck -= ck_step) {
    const float* ckp = ck - ck_step;                       // check-point of step k - 1 (k = 0: not read)
    const float q = in[k];
    const bool clipped = clip && (q < p.lo || q > p.hi);
    const float ur = clip ? clamp_(q, p.lo, p.hi) : q;
    // ---- outputs of step k = state of stage k + 1: its partials through the de-normalisation, plus the feedback
    f16v gout;
#pragma unroll
    for (int v = 0; v < 16; ++v) gout[v] = 0.0f;
    {
      const f4v o = *reinterpret_cast<const f4v*>(ck + 64);
      const float w_ang = __builtin_fmaf(o.x, nm.out_scale[0], nm.out_shift[0]);
      const float ca = __builtin_fmaf(o.y, nm.out_scale[1], nm.out_shift[1]);
      const float sa = __builtin_fmaf(o.z, nm.out_scale[2], nm.out_shift[2]);
      const float x = __builtin_fmaf(o.w, nm.out_scale[3], nm.out_shift[3]);
      const float rr = __builtin_fmaf(ca, ca, sa * sa);
      const float ir = rr > 0.0f ? __builtin_amdgcn_rsqf(rr) : 0.0f;
      const float cosang = rr > 0.0f ? ca * ir : 1.0f;     // cos(atan2(s, c)) = c / |(c, s)|, differentiated through both
      const float ir3 = ir * ir * ir;
      StageGrad sg;
      if constexpr (COST == COST_QBGM) sg = stage_qbgm_grad(p, x, cosang, w_ang, 0.0f, x_t, te);
      else sg = stage_default_grad(p, x, cosang, 0.0f, x_t, te);
      const float gc = scale * sg.cosang;
      if (!half1) {
        gout[0] = __builtin_fmaf(scale * sg.w, nm.out_scale[0], dfb[0]);
        gout[1] = __builtin_fmaf(gc * (sa * sa * ir3), nm.out_scale[1], dfb[1]);
        gout[2] = __builtin_fmaf(gc * (-(ca * sa) * ir3), nm.out_scale[2], dfb[2]);
        gout[3] = __builtin_fmaf(scale * sg.x, nm.out_scale[3], dfb[3]);
      } else {
        gout[0] = dfb[0];                                  // positionD (row 4): no stage costs it
      }
    }
    f16v dar, daz, danx, danh;
    // ---- head adjoint, then the layer-2 cell: input = the layer-1 hidden tile of step k, hidden = layer 2's of step k - 1
    {
      const f16v h1 = gru_fetch_tile(ck + hoff);
      const f16v h2p = k ? gru_fetch_tile(ckp + 32 + hoff) : gru_load_hidden(a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr, lane);
      dh2 = gru_mm<4>(dh2, ldst + GT_HEAD * 64, gout, lane);
      gru_layer_reverse<16>(lds, GF_L2X, GF_L2H, 4, h1, h2p, lane, dh2, dar, daz, danx, danh);
    }
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 0) * 64, dar, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 16) * 64, daz, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 32) * 64, danx, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 0) * 64, dar, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 16) * 64, daz, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 32) * 64, danh, lane);
    __builtin_amdgcn_sched_barrier(0);
    // ---- the layer-1 cell: input = the step's feature tile, hidden = layer 1's of step k - 1
    {
      f16v xt;
      if (k == 0) {
        xt = gru_input_tile(nm, s0, ur, lane);
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) xt[v] = 0.0f;
        if (!half1) {
          const f4v o = *reinterpret_cast<const f4v*>(ckp + 64);
          xt[0] = o.x; xt[1] = o.y; xt[2] = o.z; xt[3] = o.w;
        } else {
          xt[0] = ckp[68];
          xt[1] = __builtin_fmaf(ur, nm.in_scale[0], nm.in_shift[0]);
        }
      }
      const f16v h1p = k ? gru_fetch_tile(ckp + hoff) : gru_load_hidden(a.h0 ? a.h0 + (size_t)env * 64 : nullptr, lane);
      gru_layer_reverse<4>(lds, GF_L1X, GF_L1H, 0, xt, h1p, lane, dh1, dar, daz, danx, danh);
    }
    // ---- the input adjoint (rows 0..4: feedback, row 5: d/dQ) and the hidden adjoint
    f16v dx;
#pragma unroll
    for (int v = 0; v < 16; ++v) dx[v] = 0.0f;
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 0) * 64, dar, lane);
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 16) * 64, daz, lane);
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 32) * 64, danx, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 0) * 64, dar, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 16) * 64, daz, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 32) * 64, danh, lane);
    dfb[0] = dx[0]; dfb[1] = dx[1]; dfb[2] = dx[2]; dfb[3] = dx[3];          // (lane-half 1: [0] = row 4; [1..3] are not read)
    const float dq = __shfl(dx[1], (int)(c + 32u), 64);                       // row 5 lives on the partner lane-half
    if (owner) g[k] = clipped ? 0.0f : __builtin_fmaf(dq, nm.in_scale[0], scale * stage_u(ur));
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int COST>
void launch_gru_grad(cpmppi_handle* h, const GruGradPtrs& a, uint32_t E, hipStream_t s) {
  const bool f16 = gru_runs_f16(h);
  const dim3 grid(E * a.nb);
  if (f16) hipLaunchKernelGGL((gru_grad_forward_kernel<COST, true>), grid, dim3(BLOCK), (size_t)G16_IMAGE_BYTES, s, h->prm, a,
                              h->gru_norm, (const float*)h->gru16_image);
  else hipLaunchKernelGGL((gru_grad_forward_kernel<COST, false>), grid, dim3(BLOCK), (size_t)GRU_IMAGE_FLOATS * sizeof(float), s,
                          h->prm, a, h->gru_norm, (const float*)h->gru_image);
  hipLaunchKernelGGL((gru_grad_reverse_kernel<COST>), grid, dim3(BLOCK), GRU_GRAD_REVERSE_LDS, s, h->prm, a, h->gru_norm,
                     (const float*)h->gru_image, (const float*)h->gru_t_image);
}

template <int COST, int NOISE>
void launch_gru(cpmppi_handle* h, const cpmppi_step_args* a, const StepPtrs& p, hipStream_t s) {
  const bool f16 = gru_runs_f16(h);
  const size_t lds = ((f16 ? (size_t)G16_IMAGE_BYTES / 4 : (size_t)GRU_IMAGE_FLOATS) + (size_t)WAVES * p.W) * sizeof(float);
  // (host code that no allowed H reaches: at H = CPMPPI_MAX_HORIZON = 1024 the images need 64 640 B (FAST) and 64 416 B (PRECISE))
  if (lds > 64 * 1024) {   // long horizons with a perturbation buffer: weights image + [WAVES][H] sums
    allow_large_lds(&gru_rollout_cost_kernel<COST, NOISE, true>);
    allow_large_lds(&gru_rollout_cost_kernel<COST, NOISE, false>);
  }
  const dim3 grid(a->E * p.nb);
  if (f16) hipLaunchKernelGGL((gru_rollout_cost_kernel<COST, NOISE, true>), grid, dim3(BLOCK), lds, s, h->prm, p,
                              h->gru_norm, (const float*)h->gru16_image, a->h0);
  else hipLaunchKernelGGL((gru_rollout_cost_kernel<COST, NOISE, false>), grid, dim3(BLOCK), lds, s, h->prm, p,
                          h->gru_norm, (const float*)h->gru_image, a->h0);
}

}  // namespace

void launch_gru_brunton(cpmppi_handle* h, const BruntonArgs& a, hipStream_t s) {
  const size_t waves = brunton_gru_rows((size_t)a.R * a.count);
  hipLaunchKernelGGL(gru_brunton_kernel, dim3((unsigned)((waves + WAVES - 1) / WAVES)), dim3(BLOCK),
                     (size_t)GRU_IMAGE_FLOATS * sizeof(float), s, h->gru_norm, (const float*)h->gru_image, a);
}

void launch_gru_rollout(cpmppi_handle* h, const cpmppi_step_args* a, const StepPtrs& p, hipStream_t s) {
  const bool q = h->prm.cost_id == CPMPPI_COST_QBGM;
  if (a->noise_kind == CPMPPI_NOISE_DELTA_U) { if (q) launch_gru<COST_QBGM, NOISE_DELTA_U>(h, a, p, s); else launch_gru<COST_DEFAULT, NOISE_DELTA_U>(h, a, p, s); }
  else if (a->noise_kind == CPMPPI_NOISE_KNOTS) { if (q) launch_gru<COST_QBGM, NOISE_KNOTS>(h, a, p, s); else launch_gru<COST_DEFAULT, NOISE_KNOTS>(h, a, p, s); }
  else { if (q) launch_gru<COST_QBGM, NOISE_PHILOX>(h, a, p, s); else launch_gru<COST_DEFAULT, NOISE_PHILOX>(h, a, p, s); }
}

extern "C" {

int cpmppi_set_gru(cpmppi_handle* h, const cpmppi_gru_model* m) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!m || m->hidden != 32 || m->layers != 2 || m->inputs != 6 || m->outputs != 5)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: only GRU-6IN-32H1-32H2-5OUT is built");
  for (int l = 0; l < 2; ++l)
    if (!m->w_ih[l] || !m->w_hh[l] || !m->b_ih[l] || !m->b_hh[l]) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: null weights");
  if (!m->w_out || !m->b_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: null head weights");
  std::vector<float> img((size_t)GRU_IMAGE_FLOATS, 0.0f);
  auto frag = [&](int f) { return img.data() + (size_t)f * 64; };
  // x-tile row r -> network input column: rows 0..4 = the 5 state features (inputs 1..5), row 5 = Q (input 0)
  auto xcol = [](int r) { return r < 5 ? r + 1 : (r == 5 ? 0 : -1); };
  for (int g = 0; g < 3; ++g) {
    for (int s = 0; s < 4; ++s)
      for (int l = 0; l < 64; ++l) {
        const int col = xcol(gru_tile_row(s, l >> 5));
        frag(GF_L1X + g * 4 + s)[l] = col < 0 ? 0.0f : m->w_ih[0][(size_t)(g * 32 + (l & 31)) * 6 + col];
      }
    for (int s = 0; s < 16; ++s)
      for (int l = 0; l < 64; ++l) {
        const int k = gru_tile_row(s, l >> 5);
        const size_t row = (size_t)(g * 32 + (l & 31));
        frag(GF_L1H + g * 16 + s)[l] = m->w_hh[0][row * 32 + k];
        frag(GF_L2X + g * 16 + s)[l] = m->w_ih[1][row * 32 + k];
        frag(GF_L2H + g * 16 + s)[l] = m->w_hh[1][row * 32 + k];
      }
  }
  for (int layer = 0; layer < 2; ++layer) {
    const int fb = layer == 0 ? GF_L1B : GF_L2B;
    for (int l = 0; l < 32; ++l) {                           // lane-half 0 carries the bias (k = 0), half 1 zeros
      frag(fb + 0)[l] = m->b_ih[layer][l] + m->b_hh[layer][l];
      frag(fb + 1)[l] = m->b_ih[layer][32 + l] + m->b_hh[layer][32 + l];
      frag(fb + 2)[l] = m->b_ih[layer][64 + l];
      frag(fb + 3)[l] = m->b_hh[layer][64 + l];
    }
  }
  for (int s = 0; s < 16; ++s)
    for (int l = 0; l < 64; ++l)
      frag(GF_DW + s)[l] = (l & 31) < 5 ? m->w_out[(size_t)(l & 31) * 32 + gru_tile_row(s, l >> 5)] : 0.0f;
  for (int l = 0; l < 5; ++l) frag(GF_DB)[l] = m->b_out[l];
  // plain vectors of the fused rollout kernel (biases as accumulator tiles, dense head on the VALU)
  for (int layer = 0; layer < 2; ++layer)
    for (int hf = 0; hf < 2; ++hf)
      for (int v = 0; v < 16; ++v) {
        const int r = gru_tile_row(v, hf);
        float* b = img.data() + GV_BIAS + (size_t)layer * 4 * 32 + hf * 16 + v;
        b[0 * 32] = m->b_ih[layer][r] + m->b_hh[layer][r];
        b[1 * 32] = m->b_ih[layer][32 + r] + m->b_hh[layer][32 + r];
        b[2 * 32] = m->b_ih[layer][64 + r];
        b[3 * 32] = m->b_hh[layer][64 + r];
      }
  for (int hf = 0; hf < 2; ++hf)
    for (int o = 0; o < 5; ++o)
      for (int v = 0; v < 16; ++v)
        img[GV_HEAD + (size_t)hf * 80 + o * 16 + v] = m->w_out[(size_t)o * 32 + gru_tile_row(v, hf)];
  for (int o = 0; o < 5; ++o) img[GV_HEADB + o] = m->b_out[o];
  for (int i = 0; i < 6; ++i) {
    h->gru_norm.in_scale[i] = m->in_scale ? m->in_scale[i] : 1.0f;
    h->gru_norm.in_shift[i] = m->in_shift ? m->in_shift[i] : 0.0f;
  }
  for (int i = 0; i < 5; ++i) {
    h->gru_norm.out_scale[i] = m->out_scale ? m->out_scale[i] : 1.0f;
    h->gru_norm.out_shift[i] = m->out_shift ? m->out_shift[i] : 0.0f;
  }
  // ---- f16 split image (cpmppi_gru16.hpp): fragment f holds, for lane l and t = 0..7, the weight of output row l%32
  // against k-slot (block b, lane half l/32, t) = tile register v = 8b + t of that half
  std::vector<unsigned char> img16((size_t)G16_IMAGE_BYTES, 0);
  bool in_range = true;
  auto put16 = [&](int f, int lane, int t, float w) {
    const _Float16 hi = (_Float16)w;
    const _Float16 lo = (_Float16)(w - (float)hi);
    if (!(fabsf(w) < 60000.0f)) in_range = false;
    reinterpret_cast<_Float16*>(img16.data() + (size_t)f * G16_FRAG_BYTES + lane * 16)[t] = hi;
    reinterpret_cast<_Float16*>(img16.data() + (size_t)(f + 1) * G16_FRAG_BYTES + lane * 16)[t] = lo;
  };
  // gate rows pre-scaled so that the gates need no multiply before v_exp_f32 (gru16_gates_overlapped): r, z by -log2(e), n by 2 log2(e)
  const double LOG2E = 1.4426950408889634;
  const double gate_scale[3] = {-LOG2E, -LOG2E, 2.0 * LOG2E};
  auto sc = [&](int g, float w) { return (float)(gate_scale[g] * (double)w); };
  for (int g = 0; g < 3; ++g)
    for (int l = 0; l < 64; ++l)
      for (int tt = 0; tt < 8; ++tt) {
        const size_t row = (size_t)(g * 32 + (l & 31));
        const int col = xcol(gru_tile_row(tt, l >> 5));                       // x tile registers 0..7
        put16(HF_L1X + g * 2, l, tt, (col < 0 || tt >= 4) ? 0.0f : sc(g, m->w_ih[0][row * 6 + col]));
        for (int b = 0; b < 2; ++b) {
          const int k = gru_tile_row(8 * b + tt, l >> 5);
          put16(HF_L1H + (g * 2 + b) * 2, l, tt, sc(g, m->w_hh[0][row * 32 + k]));
          put16(HF_L2X + (g * 2 + b) * 2, l, tt, sc(g, m->w_ih[1][row * 32 + k]));
          put16(HF_L2H + (g * 2 + b) * 2, l, tt, sc(g, m->w_hh[1][row * 32 + k]));
        }
      }
  for (int b = 0; b < 2; ++b)
    for (int l = 0; l < 64; ++l)
      for (int tt = 0; tt < 8; ++tt)
        put16(HF_HEAD + b * 2, l, tt, (l & 31) < 5 ? m->w_out[(size_t)(l & 31) * 32 + gru_tile_row(8 * b + tt, l >> 5)] : 0.0f);
  if (!in_range) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: weights beyond the f16 range");
  {
    float* bv = reinterpret_cast<float*>(img16.data() + G16_BIAS_OFF);
    for (int i = 0; i < 8 * 32; ++i) {                                        // the same 8 gate-bias tiles, scaled alike
      const int kind = (i / 32) % 4;                                          // r, z, n_x, n_h
      bv[i] = (float)(gate_scale[kind < 2 ? kind : 2] * (double)img[GV_BIAS + i]);
    }
    for (int hf = 0; hf < 2; ++hf)
      for (int v = 0; v < 16; ++v) {
        const int r = gru_tile_row(v, hf);
        bv[8 * 32 + hf * 16 + v] = r < 5 ? m->b_out[r] : 0.0f;
      }
  }
  // ---- transposed image of the reverse sweep (cpmppi_gru.hpp, GT_*): fragment s of W^T holds W[unit(s, lane half)][lane % 32]
  std::vector<float> imgt((size_t)GRU_T_IMAGE_FLOATS, 0.0f);
  auto fragt = [&](int f) { return imgt.data() + (size_t)f * 64; };
  for (int g = 0; g < 3; ++g)
    for (int s = 0; s < 16; ++s)
      for (int l = 0; l < 64; ++l) {
        const size_t unit = (size_t)(g * 32 + gru_tile_row(s, l >> 5));
        const int mrow = l & 31;
        const int col = mrow < 8 ? xcol(mrow) : -1;
        fragt(GT_L1X + g * 16 + s)[l] = col < 0 ? 0.0f : m->w_ih[0][unit * 6 + col];
        fragt(GT_L1H + g * 16 + s)[l] = m->w_hh[0][unit * 32 + mrow];
        fragt(GT_L2X + g * 16 + s)[l] = m->w_ih[1][unit * 32 + mrow];
        fragt(GT_L2H + g * 16 + s)[l] = m->w_hh[1][unit * 32 + mrow];
      }
  for (int s = 0; s < 4; ++s)
    for (int l = 0; l < 64; ++l) {
      const int o = gru_tile_row(s, l >> 5);
      fragt(GT_HEAD + s)[l] = o < 5 ? m->w_out[(size_t)o * 32 + (l & 31)] : 0.0f;
    }
  CPMPPI_ON_DEVICE(h);
  if (!h->gru_image) CPMPPI_HIP(h, hipMalloc(&h->gru_image, img.size() * sizeof(float)));
  CPMPPI_HIP(h, hipMemcpy(h->gru_image, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!h->gru_t_image) CPMPPI_HIP(h, hipMalloc(&h->gru_t_image, imgt.size() * sizeof(float)));
  CPMPPI_HIP(h, hipMemcpy(h->gru_t_image, imgt.data(), imgt.size() * sizeof(float), hipMemcpyHostToDevice));
  allow_large_lds(&gru_grad_reverse_kernel<COST_QBGM>);      // both images in LDS: beyond the default 64 KB
  allow_large_lds(&gru_grad_reverse_kernel<COST_DEFAULT>);
  if (!h->gru16_image) CPMPPI_HIP(h, hipMalloc(&h->gru16_image, img16.size()));
  CPMPPI_HIP(h, hipMemcpy(h->gru16_image, img16.data(), img16.size(), hipMemcpyHostToDevice));
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

int cpmppi_gru_predict(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* s0, const float* Q, const float* h0,
                       float* traj_out, float* h_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_predict: no model set (cpmppi_set_gru)");
  if (horizon == 0) horizon = h->cfg.H;
  if (B == 0 || !s0 || !Q || !traj_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_predict: bad argument");
  CPMPPI_ON_DEVICE(h);
  hipLaunchKernelGGL(gru_predict_kernel, dim3((B + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK), dim3(BLOCK),
                     (size_t)GRU_IMAGE_FLOATS * sizeof(float), (hipStream_t)stream, h->gru_norm,
                     (const float*)h->gru_image, B, horizon, s0, Q, h0, traj_out, h_out);
  return launched(h);
}

int cpmppi_gru_advance(cpmppi_handle* h, uint32_t E, const float* s, const float* Q, float* h_io, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_advance: no model set (cpmppi_set_gru)");
  if (E == 0 || E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_advance: E out of range");
  if (!s || !Q || !h_io) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_advance: s, Q, h_io are required");
  CPMPPI_ON_DEVICE(h);
  // (one launch, nothing allocated, nothing awaited: the call can be captured)
  hipLaunchKernelGGL(gru_advance_kernel, dim3((E + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK), dim3(BLOCK),
                     (size_t)GRU_IMAGE_FLOATS * sizeof(float), (hipStream_t)stream, h->gru_norm, (const float*)h->gru_image, E, s,
                     Q, h_io);
  return launched(h);
}

int cpmppi_gru_washout(cpmppi_handle* h, uint32_t R, uint32_t T, const float* states, const float* Q, const float* h0,
                       float* h_rows_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_washout: no model set (cpmppi_set_gru)");
  if (R == 0 || T == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_washout: R and T must be at least 1");
  if (!states || !Q || !h_rows_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_washout: states, Q, h_rows_out are required");
  if (misaligned(states) || misaligned(Q) || misaligned(h0) || misaligned(h_rows_out))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_gru_washout: misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  // (one launch, nothing allocated, nothing awaited: the call can be captured)
  hipLaunchKernelGGL(gru_washout_kernel, dim3((R + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK), dim3(BLOCK),
                     (size_t)GRU_IMAGE_FLOATS * sizeof(float), (hipStream_t)stream, h->gru_norm, (const float*)h->gru_image, R, T,
                     states, Q, h0, h_rows_out);
  return launched(h);
}

int cpmppi_rollout_cost_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                            const float* target_equilibrium, const float* h0, float* S_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rollout_cost_gru: no model set (cpmppi_set_gru)");
  if (E == 0 || E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rollout_cost_gru: E out of range");
  if (!s0 || !inputs || !target_position || !target_equilibrium || !S_out)
    return fail(h, CPMPPI_ERR_BAD_ARG,
                "cpmppi_rollout_cost_gru: s0, inputs, target_position, target_equilibrium, S_out are required");
  if ((h->prm.cost_id != CPMPPI_COST_QBGM && h->prm.cost_id != CPMPPI_COST_DEFAULT) || h->prm.qb_mode != 0u)
    return fail(h, CPMPPI_ERR_BAD_ARG,
                "cpmppi_rollout_cost_gru: the GRU predictor supports quadratic_boundary_grad_minimal and default");
  CPMPPI_ON_DEVICE(h);
  // (one launch, nothing allocated, nothing awaited: the call can be captured; no pole mass and no L - the network is the plant model)
  const GruCostPtrs a{s0, inputs, target_position, target_equilibrium, h0, S_out,
                      (h->cfg.N + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK};
  if (h->prm.cost_id == CPMPPI_COST_QBGM) launch_gru_cost_only<COST_QBGM>(h, a, E, (hipStream_t)stream);
  else launch_gru_cost_only<COST_DEFAULT>(h, a, E, (hipStream_t)stream);
  return launched(h);
}

int cpmppi_rollout_cost_grad_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                                 const float* target_equilibrium, const float* h0, float* S_out, float* grad_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_rollout_cost_grad_gru";
  if (!h->gru_image) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": no model set (cpmppi_set_gru)");
  if (E == 0 || E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": E out of range");
  if (!s0 || !inputs || !target_position || !target_equilibrium || !grad_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": s0, inputs, target_position, target_equilibrium, grad_out are required");
  if ((h->prm.cost_id != CPMPPI_COST_QBGM && h->prm.cost_id != CPMPPI_COST_DEFAULT) || h->prm.qb_mode != 0u)
    return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": the GRU predictor supports quadratic_boundary_grad_minimal and default");
  CPMPPI_ON_DEVICE(h);
  // check-points of the handle's largest launch; allocated on first use, never inside a capture
  const size_t need = (size_t)h->cfg.H * GRU_CKPT_FLOATS * (size_t)h->cfg.E * h->cfg.N;
  if (h->gru_grad_ws_floats < need) {
    if (const int rc = refuse_unreserved_capture(h, (hipStream_t)stream, who, "cpmppi_rollout_cost_grad_gru once")) return rc;
    if (const int rc = grow_workspace(h, h->gru_grad_ws, h->gru_grad_ws_floats, need)) return rc;
  }
  const GruGradPtrs a{s0, inputs, target_position, target_equilibrium, h0, S_out, grad_out, h->gru_grad_ws, (size_t)E * h->cfg.N,
                      (h->cfg.N + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK};
  if (h->prm.cost_id == CPMPPI_COST_QBGM) launch_gru_grad<COST_QBGM>(h, a, E, (hipStream_t)stream);
  else launch_gru_grad<COST_DEFAULT>(h, a, E, (hipStream_t)stream);
  return launched(h);
}

#ifdef CPMPPI_GRU_STAMPS
int cpmppi_debug_gru_stamps(unsigned long long out[8], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gru_stamp_sum), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gru_stamp_sum), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

}  // extern "C"
