// cpmppi_dense.hip — the neural imitator of the MPC, Dense-7IN-32H1-32H2-1OUT (tanh, tanh, linear): the controller's forward pass,
// the loss and its gradient over recordings, and Adam on the device.   Contract: include/cpmppi.h.
//
// Kernel inventory
//   dense_control_kernel        one lane = one env: normalise, three layers, de-normalise, clip; *count_dev += 1 by one lane.
//   dense_grad_kernel<GRAD>     one workgroup = ONE wave = WG_TILES tiles of 64 samples, a lane per sample.  Forward and backward run
//                               lane-per-sample on the vector ALUs; with GRAD the tile's h1, h2, dz1, dz2, inputs and head adjoint
//                               are parked in LDS and contracted over the samples on v_mfma_f32_32x32x2_f32 (the SAMPLE is the
//                               contraction index, two per MFMA, as in gru_wgrad_kernel) into three accumulator tiles that live
//                               across the workgroup's tiles.  The workgroup writes its own row of the partials with plain stores.
//   dense_finalize_kernel       ONE workgroup walks the partial rows first to last in float64: loss, gradient; with `update` Adam on
//                               the parameter vector in place.  `guard`: the cost steps - norm clip, and no update from a non-finite
//                               loss or norm.
//   dense_policy_kernel<COST, INTEG, GRAD>   fine-tuning on the task cost (cpmppi_dense_policy_*): the closed loop net -> ODE plant
//                               per lane, its cost, and with GRAD the reverse sweep of cpmppi_grad.hpp per control step feeding the
//                               same backward body and tile contraction as dense_grad_kernel.
//   dagger_step_kernel          one lane = one env (cpmppi_dagger_step): the control kernel's forward body on the live parameter
//                               vector, one Philox block for the gate, the applied control, the sample into the trainer's tensors.
// The parameter vector is the only image of the weights.  Every kernel reads it through the constant address space: the index is
// wave-uniform, so a weight arrives as a scalar-load operand of the lane's FMA - no LDS staging, no barrier in front of the first
// layer, and the 5.4 KB vector stays in the scalar cache for every wave of the launch (DESIGN.md N7 records the choice).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <vector>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_gru.hpp"          // (gru_tanh, f16v, gru_tile_row: the exact-f32 cell's tanh and the MFMA accumulator layout)
#include "cpmppi_wave.hpp"
#include "cpmppi_train.hpp"
#include "cpmppi_philox.hpp"       // (philox4x32_10: the gate of dagger_step_kernel)
#include "cpmppi_grad.hpp"         // (substep_reverse, stage_*_grad, the plain substeps: dense_policy_kernel)

using namespace cpmppi_k;
using cpmppi::f16v;

namespace {

constexpr int NIN = 7, NH = 32;
constexpr int NPAR = (int)CPMPPI_DENSE_PARAMS;
enum : int { OFF_W1 = 0, OFF_B1 = NH * NIN, OFF_W2 = OFF_B1 + NH, OFF_B2 = OFF_W2 + NH * NH, OFF_W3 = OFF_B2 + NH, OFF_B3 = OFF_W3 + NH };
static_assert(OFF_B3 + 1 == NPAR, "the flat order of cpmppi.h");
constexpr int LOSS_COL = NPAR, ROW = NPAR + 1;       // a partial row: the gradient sums in the flat order, then the loss sum
constexpr int TILE = 64;                             // samples per tile: a lane each
constexpr int WG_TILES = 2;                          // tiles per workgroup
constexpr int WG_SAMPLES = TILE * WG_TILES;
constexpr int LDS_STRIDE = NH + 1;                   // (a lane writes its sample's row: odd stride, no bank conflict)
constexpr int FIN_BLOCK = 1024;                      // lanes of the finalize kernel, a column of the partial rows each (two passes)
constexpr int FIN_CHUNK = 8;                         // ... which loads this many rows at a time, and adds them in row order

struct DenseNorm {
  float in_scale[NIN], in_shift[NIN], out_scale, out_shift;
};

typedef const __attribute__((address_space(4))) float* wptr;
__device__ __forceinline__ wptr constant_(const float* p) { return (wptr)(uintptr_t)p; }

// y (normalised) of the normalised inputs x; h1, h2: the hidden activations.  Every sum in index order, every step an explicit FMA.
__device__ __forceinline__ float dense_forward(wptr w, const float (&x)[NIN], float (&h1)[NH], float (&h2)[NH]) {
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    float z = w[OFF_B1 + i];
#pragma unroll
    for (int k = 0; k < NIN; ++k) z = __builtin_fmaf(w[OFF_W1 + i * NIN + k], x[k], z);
    h1[i] = cpmppi::gru_tanh(z);
  }
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    float z = w[OFF_B2 + i];
#pragma unroll
    for (int k = 0; k < NH; ++k) z = __builtin_fmaf(w[OFF_W2 + i * NH + k], h1[k], z);
    h2[i] = cpmppi::gru_tanh(z);
  }
  float y = w[OFF_B3];
#pragma unroll
  for (int k = 0; k < NH; ++k) y = __builtin_fmaf(w[OFF_W3 + k], h2[k], y);
  return y;
}

// The seven inputs of one row, normalised: angleD, angle_cos, angle_sin, position, positionD (s[1..5]), target_equilibrium,
// target_position.
__device__ __forceinline__ void dense_inputs(const DenseNorm& nm, const float* s, float te, float tp, float (&x)[NIN]) {
  const float raw[NIN] = {s[1], s[2], s[3], s[4], s[5], te, tp};
#pragma unroll
  for (int k = 0; k < NIN; ++k) x[k] = __builtin_fmaf(nm.in_scale[k], raw[k], nm.in_shift[k]);
}

__global__ __launch_bounds__(BLOCK) void dense_control_kernel(const DenseNorm nm, const float* params,
                                                              const cpmppi_dense_control_args a) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e == 0 && a.count_dev) *a.count_dev += 1;      // (nothing in this launch reads it)
  if (e >= a.E) return;
  float x[NIN], h1[NH], h2[NH];
  dense_inputs(nm, a.s + (size_t)e * 6, a.target_equilibrium[e], a.target_position[e], x);
  const float y = dense_forward(constant_(params), x, h1, h2);
  const float q = __builtin_fmaf(nm.out_scale, y, nm.out_shift);
  a.Q_out[e] = q > 1.0f ? 1.0f : (q < -1.0f ? -1.0f : q);   // (both comparisons are false for a NaN: it passes)
  if (a.y_out) a.y_out[e] = y;
}

// sum + d * d in two roundings, as a host evaluation of the recurrence forms it (no FMA: cpmppi.h promises these bits)
__device__ __forceinline__ double add_square(double sum, double d) {
#pragma clang fp contract(off)
  const double sq = d * d;
  return sum + sq;
}

// One DAgger control period, a lane per env: the imitator's control (the body of dense_control_kernel), the gate's Philox block,
// the applied control, the sample into row (r0 + e, c) of the trainer's tensors, the disagreement.  Nothing is shared between lanes.
__global__ __launch_bounds__(BLOCK) void dagger_step_kernel(const DenseNorm nm, const float* params, const cpmppi_dagger_args a) {
  const uint32_t e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= a.E) return;
  // the period: the host's, or the device counter's (already advanced by the expert's step); a counter still 0 counts as period 0
  uint64_t c = a.period;
  if (a.period_dev) {
    const uint64_t cnt = (uint64_t)*a.period_dev;
    c = cnt ? cnt - 1u : 0u;
  }
  const float* se = a.s + (size_t)e * 6;
  const float te = a.target_equilibrium[e], tp = a.target_position[e], q_exp = a.Q_expert[e];
  float x[NIN], h1[NH], h2[NH];
  dense_inputs(nm, se, te, tp, x);
  const float y = dense_forward(constant_(params), x, h1, h2);
  const float q = __builtin_fmaf(nm.out_scale, y, nm.out_shift);
  const float q_imi = q > 1.0f ? 1.0f : (q < -1.0f ? -1.0f : q);
  // the gate: rollout index 0xFFFFFFFF is no rollout's, so the block is none of the sampler's; the sampler's key
  uint32_t c0 = 0xFFFFFFFFu, c1 = a.env_offset + e, c2 = 0u, c3 = (uint32_t)c;
  cpmppi::philox4x32_10(c0, c1, c2, c3, (uint32_t)a.seed ^ 0x51ed270bu, (uint32_t)(a.seed >> 32) ^ (uint32_t)(c >> 32));
  const float ub = (float)(c1 >> 8) * 5.9604644775390625e-8f;          // [0, 1), 24 bits
  const bool expert = ub < a.beta[e];                                  // (false for a NaN beta)
  a.Q_out[e] = expert ? q_exp : q_imi;
  if (c < (uint64_t)a.T) {
    const size_t row = (size_t)(a.r0 + e) * a.T + (size_t)c;
    float* so = a.states + row * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) so[k] = se[k];
    a.rec_target_position[row] = tp;
    a.rec_target_equilibrium[row] = te;
    a.labels[row] = q_exp;
    if (a.imitator_out) a.imitator_out[row] = q_imi;
    if (a.gate_out) a.gate_out[row] = expert ? 1u : 0u;
    if (a.sq_err) a.sq_err[e] = add_square(a.sq_err[e], (double)q_imi - (double)q_exp);   // (of the samples recorded: past the end, none)
  }
}

struct DenseLossArgs {
  const float* states;     // [R,T,6]
  const float* tp;         // [R,T]
  const float* te;         // [R,T]
  const float* labels;     // [R,T]
  const uint32_t* windows; // [B][2]
  const float* params;     // [NPAR]
  float* partials;         // [gridDim.x][ROW]
  uint32_t N, R, T, P, shift;
};

__device__ __forceinline__ f16v mfma_(float a, float b, f16v acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }

// Where a tile of 64 samples is parked for the contraction over them (LDS of the one wave).
struct DenseTile {
  float* dz1; float* dz2; float* h1; float* h2;   // [TILE][LDS_STRIDE]
  float* x;                                       // [TILE][8]: the seven inputs and the bias column
  float* e;                                       // [TILE] the head adjoint
};

// The backward pass of the lane's sample from `e` = d (the sum) / d y, as dense_grad_kernel forms it, parked into the lane's row
// of the tile; dx = W1^T dz1: the adjoint of the seven normalised inputs (dense_policy_kernel).
__device__ __forceinline__ void dense_backward_park(wptr w, const DenseTile& t, uint32_t lane, float e, const float (&x)[NIN],
                                                    const float (&h1)[NH], const float (&h2)[NH], float (&dx)[NIN]) {
  float dz2[NH], dz1[NH];
#pragma unroll
  for (int i = 0; i < NH; ++i) dz2[i] = (e * w[OFF_W3 + i]) * __builtin_fmaf(-h2[i], h2[i], 1.0f);
#pragma unroll
  for (int k = 0; k < NH; ++k) dz1[k] = 0.0f;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
#pragma unroll
    for (int k = 0; k < NH; ++k) dz1[k] = __builtin_fmaf(w[OFF_W2 + i * NH + k], dz2[i], dz1[k]);
  }
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    dz1[k] = dz1[k] * __builtin_fmaf(-h1[k], h1[k], 1.0f);
    t.dz1[lane * LDS_STRIDE + k] = dz1[k];
    t.dz2[lane * LDS_STRIDE + k] = dz2[k];
    t.h1[lane * LDS_STRIDE + k] = h1[k];
    t.h2[lane * LDS_STRIDE + k] = h2[k];
  }
#pragma unroll
  for (int k = 0; k < NIN; ++k) t.x[lane * 8 + k] = x[k];
  t.x[lane * 8 + NIN] = 1.0f;                                        // the bias column of layer 1
  t.e[lane] = e;
#pragma unroll
  for (int k = 0; k < NIN; ++k) dx[k] = 0.0f;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
#pragma unroll
    for (int k = 0; k < NIN; ++k) dx[k] = __builtin_fmaf(w[OFF_W1 + i * NIN + k], dz1[i], dx[k]);
  }
}

// The parked tile contracted over its 64 samples into the three accumulator tiles (between two barriers of the caller's).
// D[i][n] += sum over the tile's samples of A[sample][i] B[sample][n]; k-step ks contracts samples 2 ks and 2 ks + 1, the
// lane half supplies one each; lane % 32 is A's row i and B's column n.
//   acc1: dz1 x (x0..x6, 1)   -> d w1 [i][0..6], d b1 [i] in column 7
//   acc2: dz2 x h1            -> d w2 [i][n]
//   acc3: dz2 x e_0 + h2 x (e of the sample) e_1 + (e of the sample) x e_2
//                             -> d b2 [i] in column 0, d w3 [i] in column 1, d b3 in column 2 (every row alike)
__device__ __forceinline__ void dense_contract_tile(const DenseTile& t, uint32_t m, uint32_t hf, f16v& acc1, f16v& acc2, f16v& acc3) {
  const float one0 = m == 0 ? 1.0f : 0.0f, one2 = m == 2 ? 1.0f : 0.0f;
#pragma unroll 4
  for (int ks = 0; ks < TILE / 2; ++ks) {
    const int smp = 2 * ks + (int)hf;
    const float a1 = t.dz1[smp * LDS_STRIDE + m], a2 = t.dz2[smp * LDS_STRIDE + m];
    const float bh1 = t.h1[smp * LDS_STRIDE + m], ah2 = t.h2[smp * LDS_STRIDE + m];
    const float bx = m < 8u ? t.x[smp * 8 + m] : 0.0f;
    const float es = t.e[smp];
    acc1 = mfma_(a1, bx, acc1);
    acc2 = mfma_(a2, bh1, acc2);
    acc3 = mfma_(a2, one0, acc3);
    acc3 = mfma_(ah2, m == 1u ? es : 0.0f, acc3);
    acc3 = mfma_(es, one2, acc3);
  }
}

// The three accumulator tiles -> the workgroup's partial row, in the flat order.
__device__ __forceinline__ void dense_store_row(float* out, uint32_t m, uint32_t hf, const f16v& acc1, const f16v& acc2, const f16v& acc3) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = cpmppi::gru_tile_row(v, (int)hf);
    out[OFF_W2 + i * NH + m] = acc2[v];
    if (m < (uint32_t)NIN) out[OFF_W1 + i * NIN + m] = acc1[v];
    if (m == (uint32_t)NIN) out[OFF_B1 + i] = acc1[v];
    if (m == 0) out[OFF_B2 + i] = acc3[v];
    if (m == 1) out[OFF_W3 + i] = acc3[v];
    if (m == 2 && i == 0) out[OFF_B3] = acc3[v];
  }
}

template <bool GRAD>
__global__ __launch_bounds__(TILE) void dense_grad_kernel(const DenseNorm nm, const DenseLossArgs a) {
  __shared__ float sh_dz1[GRAD ? TILE * LDS_STRIDE : 1], sh_dz2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_h1[GRAD ? TILE * LDS_STRIDE : 1], sh_h2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_x[GRAD ? TILE * 8 : 1], sh_e[GRAD ? TILE : 1];
  const DenseTile park{sh_dz1, sh_dz2, sh_h1, sh_h2, sh_x, sh_e};
  const uint32_t lane = threadIdx.x, m = lane & 31u, hf = lane >> 5;
  const wptr w = constant_(a.params);
  f16v acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
  float loss = 0.0f;
  for (int tile = 0; tile < WG_TILES; ++tile) {
    const uint32_t base = (blockIdx.x * WG_TILES + tile) * TILE;
    if (base >= a.N) break;                                          // (wave-uniform; the workgroup is one wave)
    const uint32_t n = base + lane;
    const bool live = n < a.N;
    float x[NIN] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, h1[NH], h2[NH], target = 0.0f;
    if (live) {
      // (the host copy of the windows is what every call checks; the device copy is clamped into the recordings, so that one that
      // differs from it costs a wrong number, never a read outside the recordings)
      const uint32_t b = n / a.P, j = n - b * a.P;
      const uint32_t wr = min(a.windows[2 * b], a.R - 1u), wt = min(a.windows[2 * b + 1], a.T - a.P - a.shift);
      const size_t row = (size_t)wr * a.T + wt + j;
      dense_inputs(nm, a.states + row * 6, a.te[row], a.tp[row], x);
      target = (a.labels[row + a.shift] - nm.out_shift) / nm.out_scale;
    }
    const float y = dense_forward(w, x, h1, h2);
    const float e = live ? y - target : 0.0f;                        // d loss / d y = 2 e / N: the finalize kernel scales
    loss = __builtin_fmaf(e, e, loss);
    if constexpr (GRAD) {
      // (dense_backward_park's arithmetic, kept in line: behind a call the compiler merges this kernel's weight loads into
      // 8-dword scalar loads and spills 639 SGPRs where this form spills 47 - DESIGN.md N9)
      float dz2[NH], dh1[NH];
#pragma unroll
      for (int i = 0; i < NH; ++i) dz2[i] = (e * w[OFF_W3 + i]) * __builtin_fmaf(-h2[i], h2[i], 1.0f);
#pragma unroll
      for (int k = 0; k < NH; ++k) dh1[k] = 0.0f;
#pragma unroll
      for (int i = 0; i < NH; ++i) {
#pragma unroll
        for (int k = 0; k < NH; ++k) dh1[k] = __builtin_fmaf(w[OFF_W2 + i * NH + k], dz2[i], dh1[k]);
      }
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        sh_dz1[lane * LDS_STRIDE + k] = dh1[k] * __builtin_fmaf(-h1[k], h1[k], 1.0f);
        sh_dz2[lane * LDS_STRIDE + k] = dz2[k];
        sh_h1[lane * LDS_STRIDE + k] = h1[k];
        sh_h2[lane * LDS_STRIDE + k] = h2[k];
      }
#pragma unroll
      for (int k = 0; k < NIN; ++k) sh_x[lane * 8 + k] = x[k];
      sh_x[lane * 8 + NIN] = 1.0f;                                   // the bias column of layer 1
      sh_e[lane] = e;
      __syncthreads();
      dense_contract_tile(park, m, hf, acc1, acc2, acc3);
      __syncthreads();                                               // the tile is read: the next one may be parked
    }
  }
  float* out = a.partials + (size_t)blockIdx.x * ROW;
  const float wl = wave_sum(loss);
  if (lane == 0) out[LOSS_COL] = wl;
  if constexpr (GRAD) dense_store_row(out, m, hf, acc1, acc2, acc3);
}

// ------------------------------------------------------------------------------------------------------------------
// Fine-tuning on the task cost through the ODE plant (cpmppi_dense_policy_*): the closed loop net -> clip -> S substeps of the
// handle's predictor over `p.H` control steps from a recorded row, its plugin cost, and the derivative of the batch's mean cost
// with respect to the parameter vector.  One lane = one start state, one workgroup = ONE wave = one partial row.
//   forward   the body of dense_control_kernel per control step, the stage cost and the plain substeps of adjoint_sweep
//             (cpmppi_grad.hpp); GRAD: s_k check-pointed per control step, lane-contiguous as SweepLane::ckpt is.
//   backward  k = H-1 .. 0: the check-point, the net's forward pass again, the S sub-states into LDS and substep_reverse over
//             them, the stage gradient; e_k = d J / d y_k (0 where the control was clipped) takes the MSE residual's place in
//             dense_backward_park / dense_contract_tile, the accumulators living across all H steps; W1^T dz1 goes back into the
//             state's adjoint through in_scale (angle_cos / angle_sin: through -sin / +cos into the angle's).
struct PolicyArgs {
  const float* states;     // [R,T,6]
  const float* tp;         // [R,T]
  const float* te;         // [R,T]
  const float* L;          // [R] or NULL
  const uint32_t* windows; // [B][2]
  const float* params;     // [NPAR]
  float* partials;         // [gridDim.x][ROW]
  float* ckpt;             // [H][6][gridDim.x * TILE]
  float* cost_out;         // [B] or NULL
  float* Q_out;            // [B][H] or NULL
  uint32_t B, R, T;
};

template <int COST, int INTEG, bool GRAD>
__global__ __launch_bounds__(TILE) void dense_policy_kernel(const DenseNorm nm, const cpmppi::Params p, const PolicyArgs a) {
  using namespace cpmppi;
  __shared__ float sh_dz1[GRAD ? TILE * LDS_STRIDE : 1], sh_dz2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_h1[GRAD ? TILE * LDS_STRIDE : 1], sh_h2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_x[GRAD ? TILE * 8 : 1], sh_e[GRAD ? TILE : 1];
  extern __shared__ float sub_states[];                              // GRAD: [S][6][TILE]
  const DenseTile park{sh_dz1, sh_dz2, sh_h1, sh_h2, sh_x, sh_e};
  const uint32_t lane = threadIdx.x, m = lane & 31u, hf = lane >> 5;
  const wptr w = constant_(a.params);
  const uint32_t H = p.H, S = p.S;
  const size_t lanes = (size_t)gridDim.x * TILE;
  const size_t b = (size_t)blockIdx.x * TILE + lane;
  const bool live = b < a.B;
  // a lane beyond the batch runs the loop from the upright rest state; it writes nothing and its head adjoint is 0
  float s0[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f}, te = 0.0f, x_t = 0.0f, L = p.L_default;
  if (live) {
    // (the device copy of the windows is clamped into the recordings, as in dense_grad_kernel)
    const uint32_t wr = min(a.windows[2 * b], a.R - 1u), wt = min(a.windows[2 * b + 1], a.T - 1u);
    const size_t row = (size_t)wr * a.T + wt;
#pragma unroll
    for (int i = 0; i < 6; ++i) s0[i] = a.states[row * 6 + i];
    te = a.te[row]; x_t = a.tp[row];
    if (a.L) L = a.L[wr];
  }
  const EnvConst ec = make_env_const(p, L);
  const float t = p.t_step;
  const float scale = (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? 1.0f : 1.0f / (float)(p.H + 1);
  const float cos0 = cosf(s0[0]);                                    // the plugins take cos(angle) of the given state at stage 0
  auto forward_substep = [&](State<float>& s, float uK) __attribute__((always_inline)) {
    if constexpr (INTEG == PREDICTOR_ODE) substep_cromer_plain(s, uK, t, p, ec);
    else substep_fast<float>(s, uK, t, p, ec, p.THL);
  };
  // q_k and the net's activations at the state `s`
  auto policy = [&](const State<float>& s, float (&x)[NIN], float (&h1)[NH], float (&h2)[NH]) __attribute__((always_inline)) {
    const float sv[6] = {s.th, s.w, s.c, s.s, s.x, s.v};
    dense_inputs(nm, sv, te, x_t, x);
    const float y = dense_forward(w, x, h1, h2);
    return __builtin_fmaf(nm.out_scale, y, nm.out_shift);
  };

  // ---- forward, check-pointing every control step
  State<float> st{s0[0], s0[1], s0[2], s0[3], s0[4], s0[5]};
  float cost = 0.0f, cosang = cos0;
  for (uint32_t k = 0; k < H; ++k) {
    if constexpr (GRAD) {
      float* ck = a.ckpt + ((size_t)k * 6) * lanes + b;
      ck[0] = st.th; ck[lanes] = st.w; ck[2 * lanes] = st.c; ck[3 * lanes] = st.s; ck[4 * lanes] = st.x; ck[5 * lanes] = st.v;
    }
    float x[NIN], h1[NH], h2[NH];
    const float q = policy(st, x, h1, h2);
    const float ur = q > 1.0f ? 1.0f : (q < -1.0f ? -1.0f : q);      // (the bits of dense_control_kernel; a NaN passes)
    if (live && a.Q_out) a.Q_out[b * H + k] = ur;
    if constexpr (COST == COST_QBGM) cost += stage_qbgm<float, true>(p, st.x, cosang, st.w, ur, x_t, te);
    else cost += stage_default<float, true>(p, st.x, cosang, ur, x_t, te);
    const float uK = ur * ec.uK_scale;
    for (uint32_t s = 0; s < S; ++s) forward_substep(st, uK);
    cosang = st.c;
  }
  const float term = (COST == COST_DEFAULT) ? terminal_indicator<float>(p, st.th, st.x, x_t) : 0.0f;
  const float total = (cost + term) * scale;
  if (live && a.cost_out) a.cost_out[b] = total;
  float* out = a.partials + (size_t)blockIdx.x * ROW;
  const float wl = wave_sum(live ? total : 0.0f);
  if (lane == 0) out[LOSS_COL] = wl;

  // ---- backward
  if constexpr (GRAD) {
    f16v acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
    float* sub = sub_states + lane;
    Adjoint lam{0.0f, 0.0f, 0.0f, 0.0f};                             // the terminal indicator has zero derivative
    for (uint32_t k = H; k-- > 0;) {
      const float* ck = a.ckpt + ((size_t)k * 6) * lanes + b;
      const State<float> st0{ck[0], ck[lanes], ck[2 * lanes], ck[3 * lanes], ck[4 * lanes], ck[5 * lanes]};
      float x[NIN], h1[NH], h2[NH];
      const float q = policy(st0, x, h1, h2);
      const bool clipped = q < -1.0f || q > 1.0f;
      const float ur = q > 1.0f ? 1.0f : (q < -1.0f ? -1.0f : q);
      const float uK = ur * ec.uK_scale;
      State<float> s = st0;
      for (uint32_t i = 0; i < S; ++i) {
        float* d = sub + (size_t)i * 6 * TILE;
        d[0] = s.th; d[TILE] = s.w; d[2 * TILE] = s.c; d[3 * TILE] = s.s; d[4 * TILE] = s.x; d[5 * TILE] = s.v;
        forward_substep(s, uK);
      }
      float guK = 0.0f;
      for (uint32_t i = S; i-- > 0;) {
        const float* d = sub + (size_t)i * 6 * TILE;
        const State<float> si{d[0], d[TILE], d[2 * TILE], d[3 * TILE], d[4 * TILE], d[5 * TILE]};
        substep_reverse<(INTEG == PREDICTOR_ODE)>(si, uK, t, p, ec, lam, guK);
      }
      // stage k: its own state and control, as adjoint_sweep adds them
      const float ca = (k == 0) ? cos0 : st0.c;
      StageGrad sg;
      if constexpr (COST == COST_QBGM) sg = stage_qbgm_grad(p, st0.x, ca, st0.w, ur, x_t, te);
      else sg = stage_default_grad(p, st0.x, ca, ur, x_t, te);
      lam.x = __builtin_fmaf(scale, sg.x, lam.x);
      lam.w = __builtin_fmaf(scale, sg.w, lam.w);
      lam.th = __builtin_fmaf(scale * sg.cosang, -st0.s, lam.th);
      const float gk = __builtin_fmaf(guK, ec.uK_scale, scale * sg.u);
      const float e = (live && !clipped) ? gk * nm.out_scale : 0.0f;  // d J / d y_k
      float dx[NIN];
      dense_backward_park(w, park, lane, e, x, h1, h2, dx);
      __syncthreads();
      dense_contract_tile(park, m, hf, acc1, acc2, acc3);
      __syncthreads();                                               // the tile is read: the next step may be parked
      // u_k is a function of s_k: the inputs' adjoint joins the state's (the stage-0 state's adjoint has no reader)
      lam.w = __builtin_fmaf(nm.in_scale[0], dx[0], lam.w);
      lam.th = __builtin_fmaf(nm.in_scale[1] * dx[1], -st0.s, lam.th);
      lam.th = __builtin_fmaf(nm.in_scale[2] * dx[2], st0.c, lam.th);
      lam.x = __builtin_fmaf(nm.in_scale[3], dx[3], lam.x);
      lam.v = __builtin_fmaf(nm.in_scale[4], dx[4], lam.v);
    }
    dense_store_row(out, m, hf, acc1, acc2, acc3);
  }
}

// ONE workgroup; lane p owns column p of the partial rows (and column p + FIN_BLOCK), which it walks first to last in float64.
// Column LOSS_COL: loss = sum / count.  A parameter's column (with_grad): g = 2 sum / count -> grad_out; update != 0: Adam on the
// parameter in place with t = *step + 1 (cpmppi.h states the update; float64 arithmetic, moments and parameter stored as float32),
// then *step = t.  state: params[NPAR] | m[NPAR] | v[NPAR].  `gscale`: what a column's sum is scaled by - 2 / count for the mean
// squared error, 1 / count for the mean cost.
// `guard` != 0 (the cost steps, cpmppi_dense_policy_*; a launch argument, so the unit keeps one finalize kernel): the scaled
// gradient waits in LDS for its global 2-norm - the squares added
// per lane (column p, then p + FIN_BLOCK), then over the lanes in a halving tree: a fixed order -, is scaled by
// min(1, clip_norm / norm) (clip_norm <= 0: off), and parameters, moments and counter move only if the loss and the norm are finite.
__global__ __launch_bounds__(FIN_BLOCK) void dense_finalize_kernel(const float* __restrict__ partials, uint32_t rows, double count,
                                                                   double gscale, float* state, double* __restrict__ loss_out,
                                                                   float* __restrict__ grad_out, unsigned long long* step, float lr,
                                                                   float beta1, float beta2, float eps, float clip_norm, int update,
                                                                   int with_grad, int guard) {
  __shared__ double sh_g[2 * FIN_BLOCK], sh_sq[FIN_BLOCK], sh_loss[1];                             // (guard alone)
  const bool guarded = guard != 0;
  const unsigned long long t = update ? *step + 1 : 0;
  __syncthreads();                                                   // every lane has read *step
  if (guarded) sh_g[threadIdx.x] = sh_g[threadIdx.x + FIN_BLOCK] = 0.0;
  for (uint32_t p = threadIdx.x; p < (uint32_t)ROW; p += FIN_BLOCK) {
    if (p != (uint32_t)LOSS_COL && !with_grad) continue;
    const float* col = partials + p;
    double acc = 0.0;
    uint32_t r = 0;
    for (; r + FIN_CHUNK <= rows; r += FIN_CHUNK) {
      float v[FIN_CHUNK];
#pragma unroll
      for (int q = 0; q < FIN_CHUNK; ++q) v[q] = col[(size_t)(r + q) * ROW];
#pragma unroll
      for (int q = 0; q < FIN_CHUNK; ++q) acc += (double)v[q];
    }
    for (; r < rows; ++r) acc += (double)col[(size_t)r * ROW];
    if (p == (uint32_t)LOSS_COL) {
      *loss_out = acc / count;
      if (guarded) sh_loss[0] = acc / count;
      else if (update) *step = t;
      continue;
    }
    const double g = acc * gscale;
    if (guarded) {
      sh_g[p] = g;
    } else {
      if (grad_out) grad_out[p] = (float)g;
      if (update) {
        const AdamStep adam(beta1, beta2, lr, eps, t);
        state[p] = (float)adam(state[NPAR + p], state[2 * NPAR + p], g, state[p]);
      }
    }
  }
  if (guarded) {
    {
#pragma clang fp contract(off)
      const double g0 = sh_g[threadIdx.x], g1 = sh_g[threadIdx.x + FIN_BLOCK];   // (own stores; zero beyond the gradient)
      const double q0 = g0 * g0, q1 = g1 * g1;
      sh_sq[threadIdx.x] = q0 + q1;
    }
    __syncthreads();
    for (uint32_t half = FIN_BLOCK / 2; half > 0; half >>= 1) {
      if (threadIdx.x < half) sh_sq[threadIdx.x] += sh_sq[threadIdx.x + half];
      __syncthreads();
    }
    const double norm = sqrt(sh_sq[0]), loss = sh_loss[0];
    const bool finite = fabs(loss) < (double)INFINITY && fabs(norm) < (double)INFINITY;
    const double sc = (clip_norm > 0.0f && norm > (double)clip_norm) ? (double)clip_norm / norm : 1.0;
    for (uint32_t p = threadIdx.x; p < (uint32_t)NPAR && with_grad; p += FIN_BLOCK) {
      const double g = sh_g[p] * sc;
      if (grad_out) grad_out[p] = (float)g;
      if (update && finite) {
        const AdamStep adam(beta1, beta2, lr, eps, t);
        state[p] = (float)adam(state[NPAR + p], state[2 * NPAR + p], g, state[p]);
      }
    }
    if (threadIdx.x == 0 && update && finite) *step = t;
  }
}

}  // namespace

// The handle's imitator.  state: params[NPAR] | m[NPAR] | v[NPAR] floats on the device; params is what every kernel reads.
struct DenseNet {
  float* state = nullptr;
  float* ws = nullptr;                 // [rows][ROW] partial sums, one row per workgroup
  size_t ws_floats = 0;
  float* ckpt = nullptr;               // [horizon][6][rows * TILE] check-points of cpmppi_dense_policy_* (cpmppi_dense_policy_reserve)
  size_t ckpt_floats = 0;
  unsigned long long* step = nullptr;
  DenseNorm norm = {};
  bool set = false, begun = false;
};

namespace {

size_t grad_rows(uint64_t samples) { return (size_t)((samples + WG_SAMPLES - 1) / WG_SAMPLES); }
size_t policy_rows(uint64_t B) { return (size_t)((B + TILE - 1) / TILE); }      // a start state per lane, a row per wave

DenseNet* net(cpmppi_handle* h) {
  if (!h->dense) h->dense = new DenseNet();
  return h->dense;
}

// `rows` partial rows, `ckpt_floats` check-point floats and the step counter: allocated on first use, never inside a capture
// (`reserve`: the call that does it beforehand).
int ensure_rows(cpmppi_handle* h, size_t rows, size_t ckpt_floats, hipStream_t s, const char* who, const char* reserve) {
  const size_t need = rows * ROW;
  DenseNet* st = h->dense;
  if (st && st->step && st->ws_floats >= need && st->ckpt_floats >= ckpt_floats) return CPMPPI_OK;
  if (const int rc = refuse_unreserved_capture(h, s, who, reserve)) return rc;
  st = net(h);
  if (!st->step) {
    CPMPPI_HIP(h, hipMalloc(&st->step, sizeof(unsigned long long)));
    CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  }
  if (const int rc = grow_workspace(h, st->ws, st->ws_floats, need)) return rc;
  return grow_workspace(h, st->ckpt, st->ckpt_floats, ckpt_floats);
}

// Partial rows for `samples` samples of the recordings loss.
int ensure(cpmppi_handle* h, uint64_t samples, hipStream_t s, const char* who) {
  return ensure_rows(h, grad_rows(samples), 0, s, who, "cpmppi_dense_train_reserve");
}

bool has_model(const cpmppi_handle* h) { return h->dense && h->dense->set; }

int no_model(cpmppi_handle* h, const char* who) {
  return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": no model set (cpmppi_set_dense)");
}

// What cpmppi_dense_loss_grad refuses before it launches (cpmppi.h lists it), in `who`'s name.
int check_loss_args(cpmppi_handle* h, const cpmppi_dense_loss_args* a, const char* who) {
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": " + why); };
  if (!has_model(h)) return no_model(h, who);
  if (!a->states || !a->target_position || !a->target_equilibrium || !a->labels || !a->windows || !a->windows_host || !a->loss_out)
    return refuse("states, target_position, target_equilibrium, labels, windows, windows_host and loss_out are required");
  if (a->B == 0 || a->R == 0 || a->T == 0 || a->post_wash_out == 0) return refuse("B, R, T and post_wash_out must be at least 1");
  if ((uint64_t)a->B * a->post_wash_out > (1ull << 31))
    return refuse(std::to_string((uint64_t)a->B * a->post_wash_out) + " samples: at most 2^31 per call");
  if (misaligned(a->states) || misaligned(a->target_position) || misaligned(a->target_equilibrium) || misaligned(a->labels) ||
      misaligned(a->windows) || misaligned(a->windows_host) || misaligned(a->grad_out) || misaligned8(a->loss_out))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  return check_windows(h, who, a->windows_host, a->B, a->R, a->T, (uint64_t)a->post_wash_out + a->shift_labels,
                       "r < R, t0 + post_wash_out - 1 + shift_labels <= T - 1");
}

// The loss (and the gradient into `grad`, or NULL) on `s`; `update`: and Adam.  Checks, workspace, the two launches.
int loss_grad_impl(cpmppi_handle* h, const cpmppi_dense_loss_args* a, float* grad, int update, float lr, float beta1, float beta2,
                   float eps, hipStream_t s, const char* who) {
  if (const int rc = check_loss_args(h, a, who)) return rc;
  const uint64_t N = (uint64_t)a->B * a->post_wash_out;
  if (const int rc = ensure(h, N, s, who)) return rc;
  DenseNet* st = h->dense;
  const bool with_grad = grad || update;
  const uint32_t rows = (uint32_t)grad_rows(N);
  const DenseLossArgs k{a->states, a->target_position, a->target_equilibrium, a->labels, a->windows, st->state, st->ws,
                        (uint32_t)N, a->R, a->T, a->post_wash_out, a->shift_labels};
  hipLaunchKernelGGL(with_grad ? &dense_grad_kernel<true> : &dense_grad_kernel<false>, dim3(rows), dim3(TILE), 0, s, st->norm, k);
  CPMPPI_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(1), dim3(FIN_BLOCK), 0, s, (const float*)st->ws, rows, (double)N,
                     2.0 / (double)N, st->state, a->loss_out, grad, st->step, lr, beta1, beta2, eps, 0.0f, update, with_grad ? 1 : 0, 0);
  return launched(h);
}

int not_begun(cpmppi_handle* h, const char* who) {
  return begun_or_refuse(h, who, has_model(h) && h->dense->begun, "cpmppi_dense_train_begin");
}

// dense_policy_kernel's LDS: the parked tile (static) and the S x 6 sub-states per lane (dynamic) share the default 64 KB.
constexpr size_t POLICY_TILE_LDS = (size_t)(4 * TILE * LDS_STRIDE + TILE * 8 + TILE) * sizeof(float);
constexpr uint32_t POLICY_S_MAX = (uint32_t)((64 * 1024 - POLICY_TILE_LDS) / (6 * TILE * sizeof(float)));

// What the cost steps refuse about the HANDLE (cpmppi.h lists it), in `who`'s name.
int check_policy_handle(cpmppi_handle* h, const char* who) {
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": " + why); };
  if (!has_model(h)) return no_model(h, who);
  if (h->gru_image)
    return refuse("the handle's predictor is the GRU (cpmppi_set_gru): the differentiated plant is ODE_v0 or ODE");
  if ((h->prm.cost_id != CPMPPI_COST_QBGM && h->prm.cost_id != CPMPPI_COST_DEFAULT) || h->prm.qb_mode != 0u)
    return refuse("the cost is differentiated for quadratic_boundary_grad_minimal and default alone");
  if (h->cfg.math_mode != CPMPPI_MATH_FAST) return refuse("the adjoint is written for the FAST arithmetic");
  if (const int rc = refuse_tuning_rows(h, who)) return rc;
  if (h->m_pole_rows) return refuse("per-row pole masses are registered (cpmppi_set_pole_mass_rows): the plant has the handle's pole mass");
  if (h->cfg.S > POLICY_S_MAX)
    return refuse("S too large for the LDS sub-state buffer (<= " + std::to_string(POLICY_S_MAX) + ")");
  return CPMPPI_OK;
}

int check_policy_args(cpmppi_handle* h, const cpmppi_dense_policy_args* a, const char* who) {
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": " + why); };
  if (const int rc = check_policy_handle(h, who)) return rc;
  if (!a->states || !a->target_position || !a->target_equilibrium || !a->windows || !a->windows_host || !a->loss_out)
    return refuse("states, target_position, target_equilibrium, windows, windows_host and loss_out are required");
  if (a->B == 0 || a->R == 0 || a->T == 0 || a->horizon == 0) return refuse("B, R, T and horizon must be at least 1");
  if (a->horizon > CPMPPI_MAX_HORIZON)
    return refuse("horizon " + std::to_string(a->horizon) + ": at most " + std::to_string(CPMPPI_MAX_HORIZON));
  if (misaligned(a->states) || misaligned(a->target_position) || misaligned(a->target_equilibrium) || misaligned(a->L) ||
      misaligned(a->windows) || misaligned(a->windows_host) || misaligned(a->grad_out) || misaligned(a->cost_out) ||
      misaligned(a->Q_out) || misaligned8(a->loss_out))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  return check_windows(h, who, a->windows_host, a->B, a->R, a->T, 1, "r < R, t0 <= T - 1");
}

size_t policy_ckpt_floats(uint64_t B, uint32_t horizon) { return (size_t)horizon * 6 * policy_rows(B) * TILE; }

template <int COST, int INTEG>
void launch_policy(bool grad, dim3 grid, size_t lds, hipStream_t s, const DenseNorm& nm, const cpmppi::Params& p, const PolicyArgs& k) {
  if (grad) hipLaunchKernelGGL((dense_policy_kernel<COST, INTEG, true>), grid, dim3(TILE), lds, s, nm, p, k);
  else hipLaunchKernelGGL((dense_policy_kernel<COST, INTEG, false>), grid, dim3(TILE), 0, s, nm, p, k);
}

// The mean cost (and its gradient into `grad`, or NULL) on `s`; `update`: and the clipped, guarded Adam.  Checks, workspace, the
// two launches.
int policy_impl(cpmppi_handle* h, const cpmppi_dense_policy_args* a, float* grad, int update, float lr, float beta1, float beta2,
                float eps, float clip_norm, hipStream_t s, const char* who) {
  if (const int rc = check_policy_args(h, a, who)) return rc;
  const bool with_grad = grad || update;
  const size_t rows = policy_rows(a->B);
  if (const int rc = ensure_rows(h, rows, with_grad ? policy_ckpt_floats(a->B, a->horizon) : 0, s, who, "cpmppi_dense_policy_reserve"))
    return rc;
  DenseNet* st = h->dense;
  cpmppi::Params p = h->prm;
  p.H = a->horizon;                                                  // (the mean's 1 / (H + 1) is this call's horizon's)
  const PolicyArgs k{a->states, a->target_position, a->target_equilibrium, a->L, a->windows, st->state, st->ws, st->ckpt,
                     a->cost_out, a->Q_out, a->B, a->R, a->T};
  const size_t lds = (size_t)h->cfg.S * 6 * TILE * sizeof(float);
  const bool cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
  const auto launch = h->prm.cost_id == CPMPPI_COST_QBGM
                          ? (cromer ? launch_policy<cpmppi::COST_QBGM, cpmppi::PREDICTOR_ODE> : launch_policy<cpmppi::COST_QBGM, cpmppi::PREDICTOR_ODE_V0>)
                          : (cromer ? launch_policy<cpmppi::COST_DEFAULT, cpmppi::PREDICTOR_ODE> : launch_policy<cpmppi::COST_DEFAULT, cpmppi::PREDICTOR_ODE_V0>);
  launch(with_grad, dim3((unsigned)rows), lds, s, st->norm, p, k);
  CPMPPI_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(1), dim3(FIN_BLOCK), 0, s, (const float*)st->ws, (uint32_t)rows, (double)a->B,
                     1.0 / (double)a->B, st->state, a->loss_out, grad, st->step, lr, beta1, beta2, eps, clip_norm, update,
                     with_grad ? 1 : 0, 1);
  return launched(h);
}

}  // namespace

void dense_destroy(cpmppi_handle* h) {
  DenseNet* st = h->dense;
  if (!st) return;
  if (st->state) (void)hipFree(st->state);
  if (st->ws) (void)hipFree(st->ws);
  if (st->ckpt) (void)hipFree(st->ckpt);
  if (st->step) (void)hipFree(st->step);
  delete st;
  h->dense = nullptr;
}

extern "C" {

int cpmppi_set_dense(cpmppi_handle* h, const cpmppi_dense_model* mdl) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!mdl) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_dense: null model");
  // everything that can refuse, on host copies, before the handle changes
  const struct { const char* name; const float* p; int n; } parts[6] = {{"w1", mdl->w1, NH * NIN}, {"b1", mdl->b1, NH},
                                                                         {"w2", mdl->w2, NH * NH},  {"b2", mdl->b2, NH},
                                                                         {"w3", mdl->w3, NH},       {"b3", mdl->b3, 1}};
  std::vector<float> flat;
  flat.reserve(NPAR);
  for (const auto& part : parts) {
    if (!part.p) return fail(h, CPMPPI_ERR_BAD_ARG, std::string("cpmppi_set_dense: ") + part.name + " is NULL");
    for (int i = 0; i < part.n; ++i) {
      if (!(fabsf(part.p[i]) < INFINITY))
        return fail(h, CPMPPI_ERR_BAD_ARG, std::string("cpmppi_set_dense: ") + part.name + "[" + std::to_string(i) + "] is not finite");
      flat.push_back(part.p[i]);
    }
  }
  DenseNorm nm;
  for (int k = 0; k < NIN; ++k) {
    nm.in_scale[k] = mdl->in_scale ? mdl->in_scale[k] : 1.0f;
    nm.in_shift[k] = mdl->in_shift ? mdl->in_shift[k] : 0.0f;
    if (!(fabsf(nm.in_scale[k]) < INFINITY) || !(fabsf(nm.in_shift[k]) < INFINITY))
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_dense: in_scale / in_shift[" + std::to_string(k) + "] is not finite");
  }
  nm.out_scale = mdl->out_scale ? mdl->out_scale[0] : 1.0f;
  nm.out_shift = mdl->out_shift ? mdl->out_shift[0] : 0.0f;
  if (!(fabsf(nm.out_scale) < INFINITY) || !(fabsf(nm.out_shift) < INFINITY))
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_dense: out_scale / out_shift is not finite");
  if (nm.out_scale == 0.0f) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_dense: out_scale is 0 (the label is divided by it)");
  CPMPPI_ON_DEVICE(h);
  DenseNet* st = net(h);
  if (!st->state) CPMPPI_HIP(h, hipMalloc(&st->state, 3 * (size_t)NPAR * sizeof(float)));
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemcpy(st->state, flat.data(), (size_t)NPAR * sizeof(float), hipMemcpyHostToDevice));
  st->norm = nm;
  st->set = true;
  st->begun = false;                   // (the moments and the counter belong to the model before this one: cpmppi_dense_train_begin again)
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

int cpmppi_dense_control(cpmppi_handle* h, const cpmppi_dense_control_args* a, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_dense_control";
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": no argument block");
  if (!has_model(h)) return no_model(h, who);
  if (a->E == 0) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": E must be at least 1");
  if (!a->s || !a->target_position || !a->target_equilibrium || !a->Q_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": s, target_position, target_equilibrium and Q_out are required");
  if (misaligned(a->s) || misaligned(a->target_position) || misaligned(a->target_equilibrium) || misaligned(a->Q_out) ||
      misaligned(a->y_out) || misaligned8(a->count_dev))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  const DenseNet* st = h->dense;
  hipLaunchKernelGGL(dense_control_kernel, dim3((a->E + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, st->norm,
                     (const float*)st->state, *a);
  return launched(h);
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dagger_step(cpmppi_handle* h, const cpmppi_dagger_args* a, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_dagger_step";
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": " + why); };
  if (!a) return refuse("no argument block");
  if (!has_model(h)) return no_model(h, who);
  if (a->E == 0) return refuse("E must be at least 1");
  if (a->E > h->cfg.E) return refuse(std::to_string(a->E) + " envs, the handle has " + std::to_string(h->cfg.E));
  if (!a->s || !a->target_position || !a->target_equilibrium || !a->Q_expert || !a->beta || !a->Q_out)
    return refuse("s, target_position, target_equilibrium, Q_expert, beta and Q_out are required");
  if (!a->states || !a->rec_target_position || !a->rec_target_equilibrium || !a->labels)
    return refuse("the dataset's states, rec_target_position, rec_target_equilibrium and labels are required");
  if (a->R == 0 || a->T == 0) return refuse("R and T must be at least 1");
  if ((uint64_t)a->r0 + a->E > a->R)
    return refuse("recordings r0 .. r0 + E - 1 = " + std::to_string(a->r0) + " .. " + std::to_string((uint64_t)a->r0 + a->E - 1) +
                  " do not lie in the dataset's " + std::to_string(a->R));
  if (a->Q_out < a->Q_expert + a->E && a->Q_expert < a->Q_out + a->E)
    return refuse("Q_out overlaps Q_expert (the label is the expert's control, whichever of the two drives)");
  if (misaligned(a->s) || misaligned(a->target_position) || misaligned(a->target_equilibrium) || misaligned(a->Q_expert) ||
      misaligned(a->beta) || misaligned(a->Q_out) || misaligned(a->states) || misaligned(a->rec_target_position) ||
      misaligned(a->rec_target_equilibrium) || misaligned(a->labels) || misaligned(a->imitator_out) || misaligned8(a->sq_err) ||
      misaligned8(a->period_dev))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  const DenseNet* st = h->dense;
  hipLaunchKernelGGL(dagger_step_kernel, dim3((a->E + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, st->norm,
                     (const float*)st->state, *a);
  return launched(h);
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_train_reserve(cpmppi_handle* h, uint32_t samples) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (samples == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_train_reserve: samples must be at least 1");
  CPMPPI_ON_DEVICE(h);
  return ensure(h, samples, nullptr, "cpmppi_dense_train_reserve");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_loss_grad(cpmppi_handle* h, const cpmppi_dense_loss_args* a, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_loss_grad: no argument block");
  CPMPPI_ON_DEVICE(h);
  return loss_grad_impl(h, a, a->grad_out, 0, 0.0f, 0.0f, 0.0f, 0.0f, (hipStream_t)stream, "cpmppi_dense_loss_grad");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_train_begin(cpmppi_handle* h) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!has_model(h)) return no_model(h, "cpmppi_dense_train_begin");
  CPMPPI_ON_DEVICE(h);
  if (const int rc = ensure(h, 1, nullptr, "cpmppi_dense_train_begin")) return rc;
  DenseNet* st = h->dense;
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemset(st->state + NPAR, 0, 2 * (size_t)NPAR * sizeof(float)));
  CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  CPMPPI_HIP(h, hipDeviceSynchronize());
  st->begun = true;
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_train_step(cpmppi_handle* h, const cpmppi_dense_loss_args* a, float lr, float beta1, float beta2, float eps,
                            void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_train_step: no argument block");
  if (const int rc = not_begun(h, "cpmppi_dense_train_step")) return rc;
  CPMPPI_ON_DEVICE(h);
  return loss_grad_impl(h, a, nullptr, 1, lr, beta1, beta2, eps, (hipStream_t)stream, "cpmppi_dense_train_step");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_policy_reserve(cpmppi_handle* h, uint32_t B, uint32_t horizon) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (B == 0 || horizon == 0 || horizon > CPMPPI_MAX_HORIZON)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_policy_reserve: B and horizon must be at least 1, horizon at most " +
                                           std::to_string(CPMPPI_MAX_HORIZON));
  CPMPPI_ON_DEVICE(h);
  return ensure_rows(h, policy_rows(B), policy_ckpt_floats(B, horizon), nullptr, "cpmppi_dense_policy_reserve",
                     "cpmppi_dense_policy_reserve");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_policy_loss_grad(cpmppi_handle* h, const cpmppi_dense_policy_args* a, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_policy_loss_grad: no argument block");
  CPMPPI_ON_DEVICE(h);
  return policy_impl(h, a, a->grad_out, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, (hipStream_t)stream, "cpmppi_dense_policy_loss_grad");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_dense_policy_train_step(cpmppi_handle* h, const cpmppi_dense_policy_args* a, float lr, float beta1, float beta2, float eps,
                                   float clip_norm, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_policy_train_step: no argument block");
  if (!has_model(h)) return no_model(h, "cpmppi_dense_policy_train_step");
  if (const int rc = not_begun(h, "cpmppi_dense_policy_train_step")) return rc;
  CPMPPI_ON_DEVICE(h);
  return policy_impl(h, a, nullptr, 1, lr, beta1, beta2, eps, clip_norm, (hipStream_t)stream, "cpmppi_dense_policy_train_step");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

uint64_t cpmppi_dense_policy_ckpt_floats(cpmppi_handle* h) { return h && h->dense ? (uint64_t)h->dense->ckpt_floats : 0; }

int cpmppi_dense_policy_ckpt_copy(cpmppi_handle* h, float* host, uint64_t floats, int to_device) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!host) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_policy_ckpt_copy: host is required");
  if (floats > cpmppi_dense_policy_ckpt_floats(h))
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_policy_ckpt_copy: " + std::to_string(floats) + " floats, " +
                                           std::to_string(cpmppi_dense_policy_ckpt_floats(h)) + " are reserved");
  if (floats == 0) return CPMPPI_OK;
  CPMPPI_ON_DEVICE(h);
  CPMPPI_HIP(h, hipDeviceSynchronize());
  if (to_device) CPMPPI_HIP(h, hipMemcpy(h->dense->ckpt, host, (size_t)floats * sizeof(float), hipMemcpyHostToDevice));
  else CPMPPI_HIP(h, hipMemcpy(host, h->dense->ckpt, (size_t)floats * sizeof(float), hipMemcpyDeviceToHost));
  CPMPPI_HIP(h, hipDeviceSynchronize());
  return CPMPPI_OK;
}

int cpmppi_dense_train_get(cpmppi_handle* h, float* params_host) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!params_host) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_dense_train_get: params_host is required");
  if (const int rc = not_begun(h, "cpmppi_dense_train_get")) return rc;
  CPMPPI_ON_DEVICE(h);
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemcpy(params_host, h->dense->state, (size_t)NPAR * sizeof(float), hipMemcpyDeviceToHost));
  return CPMPPI_OK;
}

}  // extern "C"
