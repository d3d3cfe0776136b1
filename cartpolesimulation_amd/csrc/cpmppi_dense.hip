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
//                               the parameter vector in place.
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

template <bool GRAD>
__global__ __launch_bounds__(TILE) void dense_grad_kernel(const DenseNorm nm, const DenseLossArgs a) {
  __shared__ float sh_dz1[GRAD ? TILE * LDS_STRIDE : 1], sh_dz2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_h1[GRAD ? TILE * LDS_STRIDE : 1], sh_h2[GRAD ? TILE * LDS_STRIDE : 1];
  __shared__ float sh_x[GRAD ? TILE * 8 : 1], sh_e[GRAD ? TILE : 1];
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
      // D[i][n] += sum over the tile's samples of A[sample][i] B[sample][n]; k-step ks contracts samples 2 ks and 2 ks + 1, the
      // lane half supplies one each; lane % 32 is A's row i and B's column n.
      //   acc1: dz1 x (x0..x6, 1)   -> d w1 [i][0..6], d b1 [i] in column 7
      //   acc2: dz2 x h1            -> d w2 [i][n]
      //   acc3: dz2 x e_0 + h2 x (e of the sample) e_1 + (e of the sample) x e_2
      //                             -> d b2 [i] in column 0, d w3 [i] in column 1, d b3 in column 2 (every row alike)
      const float one0 = m == 0 ? 1.0f : 0.0f, one2 = m == 2 ? 1.0f : 0.0f;
#pragma unroll 4
      for (int ks = 0; ks < TILE / 2; ++ks) {
        const int smp = 2 * ks + (int)hf;
        const float a1 = sh_dz1[smp * LDS_STRIDE + m], a2 = sh_dz2[smp * LDS_STRIDE + m];
        const float bh1 = sh_h1[smp * LDS_STRIDE + m], ah2 = sh_h2[smp * LDS_STRIDE + m];
        const float bx = m < 8u ? sh_x[smp * 8 + m] : 0.0f;
        const float es = sh_e[smp];
        acc1 = mfma_(a1, bx, acc1);
        acc2 = mfma_(a2, bh1, acc2);
        acc3 = mfma_(a2, one0, acc3);
        acc3 = mfma_(ah2, m == 1u ? es : 0.0f, acc3);
        acc3 = mfma_(es, one2, acc3);
      }
      __syncthreads();                                               // the tile is read: the next one may be parked
    }
  }
  float* out = a.partials + (size_t)blockIdx.x * ROW;
  const float wl = wave_sum(loss);
  if (lane == 0) out[LOSS_COL] = wl;
  if constexpr (GRAD) {
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
}

// ONE workgroup; lane p owns column p of the partial rows (and column p + FIN_BLOCK), which it walks first to last in float64.
// Column LOSS_COL: loss = sum / count.  A parameter's column (with_grad): g = 2 sum / count -> grad_out; update != 0: Adam on the
// parameter in place with t = *step + 1 (cpmppi.h states the update; float64 arithmetic, moments and parameter stored as float32),
// then *step = t.  state: params[NPAR] | m[NPAR] | v[NPAR].
__global__ __launch_bounds__(FIN_BLOCK) void dense_finalize_kernel(const float* __restrict__ partials, uint32_t rows, double count,
                                                                   float* state, double* __restrict__ loss_out,
                                                                   float* __restrict__ grad_out, unsigned long long* step, float lr,
                                                                   float beta1, float beta2, float eps, int update, int with_grad) {
  const unsigned long long t = update ? *step + 1 : 0;
  __syncthreads();                                                   // every lane has read *step
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
      if (update) *step = t;
      continue;
    }
    const double g = acc * (2.0 / count);
    if (grad_out) grad_out[p] = (float)g;
    if (update) {
      const AdamStep adam(beta1, beta2, lr, eps, t);
      state[p] = (float)adam(state[NPAR + p], state[2 * NPAR + p], g, state[p]);
    }
  }
}

}  // namespace

// The handle's imitator.  state: params[NPAR] | m[NPAR] | v[NPAR] floats on the device; params is what every kernel reads.
struct DenseNet {
  float* state = nullptr;
  float* ws = nullptr;                 // [rows][ROW] partial sums, one row per workgroup
  size_t ws_floats = 0;
  unsigned long long* step = nullptr;
  DenseNorm norm = {};
  bool set = false, begun = false;
};

namespace {

size_t grad_rows(uint64_t samples) { return (size_t)((samples + WG_SAMPLES - 1) / WG_SAMPLES); }

DenseNet* net(cpmppi_handle* h) {
  if (!h->dense) h->dense = new DenseNet();
  return h->dense;
}

// Partial rows for `samples` samples and the step counter: allocated on first use, never inside a capture.
int ensure(cpmppi_handle* h, uint64_t samples, hipStream_t s, const char* who) {
  const size_t need = grad_rows(samples) * ROW;
  DenseNet* st = h->dense;
  if (st && st->step && st->ws_floats >= need) return CPMPPI_OK;
  if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_dense_train_reserve")) return rc;
  st = net(h);
  if (!st->step) {
    CPMPPI_HIP(h, hipMalloc(&st->step, sizeof(unsigned long long)));
    CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  }
  return grow_workspace(h, st->ws, st->ws_floats, need);
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
  hipLaunchKernelGGL(dense_finalize_kernel, dim3(1), dim3(FIN_BLOCK), 0, s, (const float*)st->ws, rows, (double)N, st->state,
                     a->loss_out, grad, st->step, lr, beta1, beta2, eps, update, with_grad ? 1 : 0);
  return launched(h);
}

int not_begun(cpmppi_handle* h, const char* who) {
  return begun_or_refuse(h, who, has_model(h) && h->dense->begun, "cpmppi_dense_train_begin");
}

}  // namespace

void dense_destroy(cpmppi_handle* h) {
  DenseNet* st = h->dense;
  if (!st) return;
  if (st->state) (void)hipFree(st->state);
  if (st->ws) (void)hipFree(st->ws);
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
