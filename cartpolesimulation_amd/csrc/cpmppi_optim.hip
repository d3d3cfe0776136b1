// cpmppi_optim.hip — what the other optimizers of the reference need on the device: cost-only rollouts, the adjoint of
// rollout + cost, Adam / SGD steps on input sequences, and CEM's sampler and elite update.   Contract: include/cpmppi.h.
//
// Kernel inventory
//   rollout_grad_kernel<COST, INTEG>      rollout + plugin cost + its gradient w.r.t. the inputs, one lane per (env, rollout).
//   adam_step_kernel, sgd_step_kernel     gradient steps with per-rollout norm clipping and the action limits.
//   cem_sample_kernel, cem_gmm_sample_kernel   CEM's sampler: one Gaussian per env, or a mixture of K elite-centred ones.
//   cem_update_kernel                     top-k (bitonic sort in LDS) -> mean and stdev of the elite.
//   rpgd_step_kernel<COST, INTEG, ROWS>   the whole rpgd / gradient-tf control step, one workgroup per env (cpmppi_rpgd.hpp); ROWS: the
//                                         cost weights, learning rate and gradient clip per env (cpmppi_rpgd_step_rows).
//   cem_step_kernel<COST, INTEG, REFINE>  the whole cem / cem-naive-grad / cem-grad-bharadhwaj control step, likewise (cpmppi_cem.hpp).
// The three templated kernels run the one adjoint sweep of cpmppi_grad.hpp (adjoint_sweep over a SweepLane); the two fused steps
// rank their costs with rank_costs.  cpmppi_rollout_cost launches rollout_cost_kernel through launch_rollout (cpmppi.hip).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <type_traits>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_philox.hpp"
#include "cpmppi_grad.hpp"
#include "cpmppi_rpgd.hpp"
#include "cpmppi_cem.hpp"

using namespace cpmppi_k;

namespace {

// The kernels below are built for the three costs with an adjoint; `f` gets the handle's as a compile-time constant:
//   with_cost(id, [&](auto cost) { constexpr int COST = decltype(cost)::value; ... });
template <class F>
void with_cost(uint32_t cost_id, F&& f) {
  switch (cost_id) {
    case CPMPPI_COST_QBGM: f(std::integral_constant<int, COST_QBGM>{}); break;
    case CPMPPI_COST_DEFAULT: f(std::integral_constant<int, COST_DEFAULT>{}); break;
    default: f(std::integral_constant<int, COST_QBG>{}); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Rollout + plugin cost + its gradient w.r.t. the inputs (adjoint_sweep, cpmppi_grad.hpp).  One lane = one (env, rollout) of the
// flattened [E*N] axis (the gradient optimizers run 16-40 rollouts per env, config_optimizers.yml:60,75: a block per
// env would idle), so per-env quantities are per-lane here.  Check-points ckpt[H][6][E*N] (lane-contiguous) hold the
// state at every control step; sub[S][6][BLOCK] in LDS holds the sub-states of the control step being reversed.
struct GradPtrs {
  const float* s0; const float* Q; const float* x_t; const float* te; const float* L; const float* prev_in;
  float* ckpt; float* S_out; float* grad; uint32_t E;
  const float* m_pole;      // [E] predictor_ODE: the pole mass per env (cpmppi_set_pole_mass_rows), or NULL = the handle's
};

template <int COST, int INTEG = PREDICTOR_ODE_V0>
__global__ __launch_bounds__(BLOCK) void rollout_grad_kernel(const Params p, const GradPtrs a) {
  extern __shared__ float sub_states[];            // [S][6][BLOCK]
  const uint32_t tid = threadIdx.x;
  const size_t B = (size_t)a.E * p.N;
  const size_t g = (size_t)blockIdx.x * BLOCK + tid;
  if (g >= B) return;                               // (no block-level barrier below)
  const uint32_t env = (uint32_t)(g / p.N);
  // `pi`: the block the integration and its adjoint compute with - predictor_ODE: the env's own pole mass in place (the costs
  // never read the mass)
  Params pm_;
  if constexpr (INTEG == PREDICTOR_ODE) pm_ = with_pole_mass(p, a.m_pole ? a.m_pole[env] : p.m_pole);
  const Params& pi = (INTEG == PREDICTOR_ODE) ? pm_ : p;
  const EnvConst ec = make_env_const(pi, a.L ? a.L[env] : p.L_default);
  SweepLane w;
  sweep_lane_env(w, p, a, env);
  w.Q = a.Q + g * p.H;
  w.ckpt_stride = B; w.sub_stride = BLOCK; w.grad_stride = 1;
  w.ckpt = a.ckpt + g;
  w.grad = a.grad + g * p.H;
  w.sub = sub_states + tid;
  const float S = adjoint_sweep<COST, INTEG>(p, pi, ec, w, true);
  if (a.S_out) a.S_out[g] = S;
}

// Adam on input sequences with per-rollout gradient-norm clipping (tf.clip_by_norm over the horizon) and the final
// clip to the action limits; hyper-parameters config_optimizers.yml:52-58,69-73.  One lane = one (env, rollout) row.
__global__ __launch_bounds__(BLOCK) void adam_step_kernel(size_t rows, uint32_t H, float* __restrict__ Q,
                                                          const float* __restrict__ grad, float* __restrict__ m,
                                                          float* __restrict__ v, float lr_t, float beta1, float beta2,
                                                          float eps, float gradmax_clip, float lo, float hi) {
  const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= rows) return;
  const float* __restrict__ gr = grad + r * H;
  float ss = 0.0f;
  for (uint32_t k = 0; k < H; ++k) ss = __builtin_fmaf(gr[k], gr[k], ss);
  const float nrm = sqrtf(ss);
  const float sc = (gradmax_clip > 0.0f && nrm > gradmax_clip) ? gradmax_clip / nrm : 1.0f;
  for (uint32_t k = 0; k < H; ++k) {
    const size_t i = r * H + k;
    const float gk = gr[k] * sc;
    const float mk = beta1 * m[i] + (1.0f - beta1) * gk;
    const float vk = beta2 * v[i] + (1.0f - beta2) * gk * gk;
    m[i] = mk; v[i] = vk;
    Q[i] = clamp_(Q[i] - lr_t * mk / (sqrtf(vk) + eps), lo, hi);
  }
}

// Plain gradient step with the same per-rollout norm clipping and limit clip (cem-naive-grad-tf, config_optimizers.yml:21-31).
__global__ __launch_bounds__(BLOCK) void sgd_step_kernel(size_t rows, uint32_t H, float* __restrict__ Q,
                                                         const float* __restrict__ grad, float lr, float gradmax_clip,
                                                         float lo, float hi) {
  const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= rows) return;
  const float* __restrict__ gr = grad + r * H;
  float ss = 0.0f;
  for (uint32_t k = 0; k < H; ++k) ss = __builtin_fmaf(gr[k], gr[k], ss);
  const float nrm = sqrtf(ss);
  const float sc = (gradmax_clip > 0.0f && nrm > gradmax_clip) ? gradmax_clip / nrm : 1.0f;
  for (uint32_t k = 0; k < H; ++k) Q[r * H + k] = clamp_(Q[r * H + k] - lr * (gr[k] * sc), lo, hi);
}

// ------------------------------------------------------------------------------------------------------------------
// CEM (hyper-parameters Control_Toolkit_ASF/config_optimizers.yml:1-11 "cem-tf"): the same rollout +
// cost kernel, a different sampler and a top-k reduction instead of the soft-min.
// Q[e,n,k] = clip(mean[e,k] + stdev[e,k] * z), z ~ N(0,1) from Philox (rollout, env, step pair, offset).
__global__ __launch_bounds__(BLOCK) void cem_sample_kernel(const Params p, uint32_t E, const float* __restrict__ mean,
                                                           const float* __restrict__ stdev, uint64_t seed, uint64_t offset,
                                                           uint32_t env_offset, float* __restrict__ Q) {
  const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= (size_t)E * p.N) return;
  const uint32_t env = (uint32_t)(r / p.N), n = (uint32_t)(r % p.N);
  const float* m = mean + (size_t)env * p.H;
  const float* sd = stdev + (size_t)env * p.H;
  float* q = Q + r * p.H;
  for (uint32_t k = 0; k < p.H; k += 2) {
    float z0, z1;
    philox_normal_pair(seed, offset, env_offset + env, n, k >> 1, z0, z1);
    q[k] = fminf(fmaxf(__builtin_fmaf(sd[k], z0, m[k]), p.lo), p.hi);
    if (k + 1 < p.H) q[k + 1] = fminf(fmaxf(__builtin_fmaf(sd[k + 1], z1, m[k + 1]), p.lo), p.hi);
  }
}

// cem-gmm: samples from a mixture of K Gaussians with equal weights — component c of env e is centred on the elite
// sequence centres[e, c, :] and shares the per-time-step stdev[e, :] — clipped to the control limits.  The component of
// a rollout comes from the same Philox stream as its normals (counter word `pair` = 0x80000000: never a real pair index).
__global__ __launch_bounds__(BLOCK) void cem_gmm_sample_kernel(const Params p, uint32_t E, const float* __restrict__ centres,
                                                               uint32_t K, const float* __restrict__ stdev, uint64_t seed,
                                                               uint64_t offset, uint32_t env_offset, float* __restrict__ Q,
                                                               uint32_t* __restrict__ comp_out) {
  const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= (size_t)E * p.N) return;
  const uint32_t env = (uint32_t)(r / p.N), n = (uint32_t)(r % p.N);
  uint32_t c0 = n, c1 = env_offset + env, c2 = 0x80000000u, c3 = (uint32_t)offset;
  philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32));
  const uint32_t comp = (uint32_t)(((uint64_t)c0 * K) >> 32);              // uniform over 0 .. K-1
  if (comp_out) comp_out[r] = comp;
  const float* m = centres + ((size_t)env * K + comp) * p.H;
  const float* sd = stdev + (size_t)env * p.H;
  float* q = Q + r * p.H;
  for (uint32_t k = 0; k < p.H; k += 2) {
    float z0, z1;
    philox_normal_pair(seed, offset, env_offset + env, n, k >> 1, z0, z1);
    q[k] = fminf(fmaxf(__builtin_fmaf(sd[k], z0, m[k]), p.lo), p.hi);
    if (k + 1 < p.H) q[k + 1] = fminf(fmaxf(__builtin_fmaf(sd[k + 1], z1, m[k + 1]), p.lo), p.hi);
  }
}

// One block per env: sort (S, index) ascending with a bitonic network in LDS (ties by index = stable argsort), then
// mean and population standard deviation of the best_k input sequences per time-step, stdev floored at stdev_min.
// The order and its keys: cem_sort_key (cpmppi_cem.hpp), which the fused steps rank with as well (rank_costs).
__global__ __launch_bounds__(BLOCK) void cem_update_kernel(const Params p, const float* __restrict__ S,
                                                           const float* __restrict__ Q, uint32_t best_k, float stdev_min,
                                                           uint32_t Np, float* __restrict__ mean_out,
                                                           float* __restrict__ stdev_out, uint32_t* __restrict__ elite_out) {
  extern __shared__ uint32_t cem_lds[];                  // keys[Np], idx[Np]
  uint32_t* key = cem_lds;
  uint32_t* idx = cem_lds + Np;
  const uint32_t env = blockIdx.x, tid = threadIdx.x;
  for (uint32_t i = tid; i < Np; i += BLOCK) {
    key[i] = i < p.N ? cem_sort_key(S[(size_t)env * p.N + i]) : 0xFFFFFFFFu;
    idx[i] = i;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= Np; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < Np; i += BLOCK) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          const uint32_t ki = key[i], kl = key[l];
          const uint32_t ii = idx[i], il = idx[l];
          // (key, index) lexicographically: one 64-bit comparison
          const bool gt = (((uint64_t)ki << 32) | ii) > (((uint64_t)kl << 32) | il);
          if (gt == up) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
        }
      }
      __syncthreads();
    }
  }
  if (elite_out) for (uint32_t i = tid; i < best_k; i += BLOCK) elite_out[(size_t)env * best_k + i] = idx[i];
  const float* Qe = Q + (size_t)env * p.N * p.H;
  for (uint32_t k = tid; k < p.H; k += BLOCK) {
    float m = 0.0f;
    for (uint32_t i = 0; i < best_k; ++i) m += Qe[(size_t)idx[i] * p.H + k];
    m /= (float)best_k;
    float v = 0.0f;
    for (uint32_t i = 0; i < best_k; ++i) { const float d = Qe[(size_t)idx[i] * p.H + k] - m; v = __builtin_fmaf(d, d, v); }
    mean_out[(size_t)env * p.H + k] = m;
    stdev_out[(size_t)env * p.H + k] = fmaxf(sqrtf(v / (float)best_k), stdev_min);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The fused rpgd / gradient-tf control step (cpmppi_rpgd_step; device pieces in cpmppi_rpgd.hpp).  One workgroup = one env,
// one lane = one plan; the block is N rounded up to whole waves, the surplus lanes only keep the barriers company.  A lane
// carries its own row of Q, m, v through `iterations` x (adjoint sweep + Adam) and the final forward sweep: nothing crosses
// lanes until the ranking (rank_costs: the stable order of cem_update_kernel).  Permutation + shift: rpgd_permute_shift.
struct RpgdPtrs {
  const float* s0; const float* x_t; const float* te; const float* L; const float* prev_in; const float* m_pole;
  float* Q; float* m; float* v;
  float* ckpt;            // [E][H][6][block]
  float* grad;            // [E][H][block]
  const unsigned long long* count_dev;
  unsigned long long count, seed, draw_offset;
  uint32_t iterations, adam_iteration, keep_k, resamp_per, shift, uniform, env_offset;
  float lr, beta1, beta2, eps, gradmax_clip, sample_mean, uniform_lo, uniform_hi;
  float* Q_out; float* S_out; float* plan_out; uint32_t* order_out;
};

// ROWS (cpmppi_rpgd_step_rows): the cost weights, Adam's learning rate and the gradient clip read PER ENV - the pointer block grows
// by the rows' address, which the plain kernels' block, and with it their code, never sees.
struct RpgdRowPtrs : RpgdPtrs {
  const float* rows;      // [E][TUNING_ROW_FLOATS]
};

template <int COST, int INTEG, bool ROWS = false>
__global__ __launch_bounds__(BLOCK) void rpgd_step_kernel(const Params p, const std::conditional_t<ROWS, RpgdRowPtrs, RpgdPtrs> a) {
  extern __shared__ float rpgd_lds[];               // sub[S][6][block] | key[block] | order[block]
  const uint32_t tid = threadIdx.x, Nb = blockDim.x, env = blockIdx.x, N = p.N, H = p.H;
  uint32_t* key = reinterpret_cast<uint32_t*>(rpgd_lds + (size_t)p.S * 6 * Nb);
  uint32_t* order = key + Nb;
  const bool active = tid < N;
  const uint64_t c = a.count_dev ? (uint64_t)*a.count_dev : (uint64_t)a.count;
  const uint64_t it0 = a.count_dev ? c * a.iterations : (uint64_t)a.adam_iteration;
  const size_t row = ((size_t)env * N + tid) * H;
  float S = 0.0f;
  // `pc`: the block the COSTS compute with - ROWS: the env's row in place (block-uniform: one workgroup = one env), read once, here;
  // the pole mass then goes into THAT block, so pole-mass rows and these rows combine.  The ranking and the redraw keep `p`.
  Params pq_;
  float lr0 = a.lr, clip = a.gradmax_clip;
  if constexpr (ROWS) {
    const float* r = a.rows + (size_t)env * TUNING_ROW_FLOATS;
    pq_ = with_rpgd_row(p, r);
    lr0 = rpgd_row_value(r, RPGD_ROW_LR);
    clip = rpgd_row_value(r, RPGD_ROW_GRADMAX_CLIP);
  }
  const Params& pc = ROWS ? pq_ : p;
  if (active) {
    Params pm_;
    if constexpr (INTEG == PREDICTOR_ODE) pm_ = with_pole_mass(pc, a.m_pole ? a.m_pole[env] : p.m_pole);
    const Params& pi = (INTEG == PREDICTOR_ODE) ? pm_ : pc;
    const EnvConst ec = make_env_const(pi, a.L ? a.L[env] : p.L_default);
    SweepLane w;
    sweep_lane_env(w, p, a, env);
    w.Q = a.Q + row;
    w.ckpt_stride = w.sub_stride = w.grad_stride = Nb;
    w.ckpt = a.ckpt + (size_t)env * H * 6 * Nb + tid;
    w.grad = a.grad + (size_t)env * H * Nb + tid;
    w.sub = rpgd_lds + tid;
    RpgdLr lr(a.beta1, a.beta2, it0);
    for (uint32_t i = 1; i <= a.iterations + 1; ++i) {
      const bool descend = i <= a.iterations;      // the last pass is the final cost: forward only
      S = adjoint_sweep<COST, INTEG>(pc, pi, ec, w, descend);
      if (!descend) break;
      const float lr_t = lr.next(lr0, a.beta1, a.beta2);
      rpgd_adam_row(H, a.Q + row, a.m + row, a.v + row, w.grad, Nb, lr_t, a.beta1, a.beta2, a.eps, clip, p.lo, p.hi);
    }
    if (a.S_out) a.S_out[(size_t)env * N + tid] = S;
  }
  rank_costs(key, order, S, active, N, env, a.order_out, true);
  const float* best = a.Q + ((size_t)env * N + order[0]) * H;
  if (tid == 0) a.Q_out[env] = best[0];
  if (a.plan_out) for (uint32_t k = tid; k < H; k += Nb) a.plan_out[(size_t)env * H + k] = best[k];

  rpgd_permute_shift(p, a, env, tid, active, c, order);
}

__global__ void rpgd_count_kernel(unsigned long long* c) { *c += 1ull; }

template <int INTEG>
void launch_rpgd(uint32_t cost_id, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Params& p, const RpgdPtrs& a) {
  with_cost(cost_id, [&](auto cost) {
    hipLaunchKernelGGL((rpgd_step_kernel<decltype(cost)::value, INTEG>), grid, block, lds, st, p, a);
  });
}
// ... and with per-env rows: quadratic_boundary_grad_minimal, whose cost vector a row holds (the entry point has checked)
template <int INTEG>
void launch_rpgd_rows(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Params& p, const RpgdRowPtrs& a) {
  hipLaunchKernelGGL((rpgd_step_kernel<COST_QBGM, INTEG, true>), grid, block, lds, st, p, a);
}

inline size_t rpgd_floats(const cpmppi_handle* h, uint32_t E) { return (size_t)h->cfg.H * 7 * E * rpgd_block(h); }
inline size_t rpgd_lds_bytes(const cpmppi_handle* h) { return ((size_t)h->cfg.S * 6 + 2) * rpgd_block(h) * sizeof(float); }

// ------------------------------------------------------------------------------------------------------------------
// The fused CEM control step (cpmppi_cem_step; device pieces in cpmppi_cem.hpp): cem-tf and, with REFINE, its two gradient
// hybrids.  One workgroup = one env, one lane = one sample, the block and its surplus lanes as in rpgd_step_kernel.  The env's mean
// and stdev live in LDS for the whole step; a lane's sample is a workspace column.  Per outer iteration: every lane draws its row
// (cem_sample_kernel's statement), refines it (one adjoint sweep + sgd / Adam row update), costs it (forward sweep); the block
// ranks the costs (rank_costs = cem_update_kernel's stable order); lanes k < H refit time-step k to the elite in rank order
// (cem_update_kernel's statements).  The barrier that opens an iteration closes the refit of the one before: no sample is
// overwritten while a refit still reads it.
struct CemPtrs {
  const float* s0; const float* x_t; const float* te; const float* L; const float* prev_in; const float* m_pole;
  float* mean; float* stdev;       // [E][H], in place
  float* samples;                  // [E][H][block]
  float* ckpt;                     // [E][H][6][block]   (REFINE)
  float* grad;                     // [E][H][block]      (REFINE)
  float* m; float* v;              // [E][H][block]      (REFINE, Adam)
  const unsigned long long* count_dev;
  unsigned long long seed, offset;
  uint32_t iterations, best_k, adam, shift, env_offset;
  float stdev_min, lr, beta1, beta2, eps, gradmax_clip, mean_fill, stdev_fill;
  float* Q_out; float* S_out; float* plan_out; float* samples_out; uint32_t* order_out;
};

template <int COST, int INTEG, bool REFINE>
__global__ __launch_bounds__(BLOCK) void cem_step_kernel(const Params p, const CemPtrs a) {
  extern __shared__ float cem_step_lds[];            // REFINE: sub[S][6][block] | key[block] | order[block] | mean[H] | stdev[H]
  const uint32_t tid = threadIdx.x, Nb = blockDim.x, env = blockIdx.x, N = p.N, H = p.H;
  uint32_t* key = reinterpret_cast<uint32_t*>(cem_step_lds + (REFINE ? (size_t)p.S * 6 * Nb : 0));
  uint32_t* order = key + Nb;
  float* mu = reinterpret_cast<float*>(order + Nb);
  float* sd = mu + H;
  const bool active = tid < N;
  const uint64_t base = a.offset + (a.count_dev ? (uint64_t)*a.count_dev * a.iterations : 0ull);
  for (uint32_t k = tid; k < H; k += Nb) { mu[k] = a.mean[(size_t)env * H + k]; sd[k] = a.stdev[(size_t)env * H + k]; }

  Params pm_;
  if constexpr (INTEG == PREDICTOR_ODE) pm_ = with_pole_mass(p, a.m_pole ? a.m_pole[env] : p.m_pole);
  const Params& pi = (INTEG == PREDICTOR_ODE) ? pm_ : p;
  const EnvConst ec = make_env_const(pi, a.L ? a.L[env] : p.L_default);
  const size_t col = (size_t)env * H * Nb + tid;
  float* q = a.samples + col;
  SweepLane w;
  sweep_lane_env(w, p, a, env);
  w.Q = q;
  w.ckpt_stride = w.sub_stride = w.grad_stride = Nb;
  w.ckpt = REFINE ? a.ckpt + (size_t)env * H * 6 * Nb + tid : nullptr;
  w.grad = REFINE ? a.grad + col : nullptr;
  w.sub = REFINE ? cem_step_lds + tid : nullptr;
  RpgdLr lr(a.beta1, a.beta2, 0);                    // Adam counts the outer iterations of THIS control step from 1
  if (REFINE && a.adam && active)                    // ... with fresh moments
    for (uint32_t k = 0; k < H; ++k) { a.m[col + (size_t)k * Nb] = 0.0f; a.v[col + (size_t)k * Nb] = 0.0f; }

  for (uint32_t it = 0; it < a.iterations; ++it) {
    const bool last = it + 1 == a.iterations;
    __syncthreads();                                 // mean / stdev of this iteration stand; the refit before is through
    float S = 0.0f;
    if (active) {
      cem_sample_row(p, mu, sd, a.seed, base + it, a.env_offset + env, tid, q, Nb);
      if constexpr (REFINE) {
        (void)adjoint_sweep<COST, INTEG, true>(p, pi, ec, w, true);
        if (a.adam) {
          const float lr_t = lr.next(a.lr, a.beta1, a.beta2);
          rpgd_adam_row<true>(H, q, a.m + col, a.v + col, w.grad, Nb, lr_t, a.beta1, a.beta2, a.eps, a.gradmax_clip, p.lo, p.hi);
        } else {
          cem_sgd_row(H, q, w.grad, Nb, a.lr, a.gradmax_clip, p.lo, p.hi);
        }
      }
      S = adjoint_sweep<COST, INTEG, true>(p, pi, ec, w, false);
      if (last) {
        if (a.S_out) a.S_out[(size_t)env * N + tid] = S;
        if (a.samples_out) {
          float* out = a.samples_out + ((size_t)env * N + tid) * H;
          for (uint32_t k = 0; k < H; ++k) out[k] = q[(size_t)k * Nb];
        }
      }
    }
    // (its closing barrier: the order, and every lane's row - global memory, block scope)
    rank_costs(key, order, S, active, N, env, a.order_out, last);
    for (uint32_t k = tid; k < H; k += Nb)
      cem_refit_column(a.samples + ((size_t)env * H + k) * Nb, order, a.best_k, a.stdev_min, mu[k], sd[k]);
  }
  __syncthreads();
  if (tid == 0) a.Q_out[env] = mu[0];
  for (uint32_t k = tid; k < H; k += Nb) {
    if (a.plan_out) a.plan_out[(size_t)env * H + k] = mu[k];
    const uint32_t kk = k + a.shift;
    a.mean[(size_t)env * H + k] = kk < H ? mu[kk] : a.mean_fill;
    a.stdev[(size_t)env * H + k] = kk < H ? sd[kk] : a.stdev_fill;
  }
}

template <int INTEG, bool REFINE>
void launch_cem(uint32_t cost_id, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Params& p, const CemPtrs& a) {
  with_cost(cost_id, [&](auto cost) {
    hipLaunchKernelGGL((cem_step_kernel<decltype(cost)::value, INTEG, REFINE>), grid, block, lds, st, p, a);
  });
}

inline size_t cem_lds_bytes(const cpmppi_handle* h, bool refine) {
  return (((size_t)(refine ? h->cfg.S * 6 : 0) + 2) * rpgd_block(h) + 2 * (size_t)h->cfg.H) * sizeof(float);
}

// rollout_grad_kernel for the handle's cost (the three costs it is built for: sweep_check_handle)
template <int INTEG>
void launch_grad(uint32_t cost_id, dim3 grid, size_t lds, hipStream_t st, const Params& p, const GradPtrs& a) {
  with_cost(cost_id, [&](auto cost) {
    hipLaunchKernelGGL((rollout_grad_kernel<decltype(cost)::value, INTEG>), grid, dim3(BLOCK), lds, st, p, a);
  });
}

}  // namespace

void launch_step_count(unsigned long long* count_dev, hipStream_t s) {
  hipLaunchKernelGGL(rpgd_count_kernel, dim3(1), dim3(1), 0, s, count_dev);
}

void allow_large_lds_optim() {
  // every kernel that runs the adjoint parks S x 6 sub-states per lane in LDS (61 KB at S = 10 and 256 lanes; more substeps
  // need the opt-in as well)
  for (const uint32_t cost_id : {CPMPPI_COST_QBGM, CPMPPI_COST_DEFAULT, CPMPPI_COST_QBG})
    with_cost(cost_id, [](auto cost) {
      constexpr int COST = decltype(cost)::value;
      allow_large_lds(&rollout_grad_kernel<COST, PREDICTOR_ODE_V0>);
      allow_large_lds(&rollout_grad_kernel<COST, PREDICTOR_ODE>);
      allow_large_lds(&rpgd_step_kernel<COST, PREDICTOR_ODE_V0>);
      allow_large_lds(&rpgd_step_kernel<COST, PREDICTOR_ODE>);
      allow_large_lds(&cem_step_kernel<COST, PREDICTOR_ODE_V0, true>);
      allow_large_lds(&cem_step_kernel<COST, PREDICTOR_ODE, true>);
    });
  allow_large_lds(&rpgd_step_kernel<COST_QBGM, PREDICTOR_ODE_V0, true>);
  allow_large_lds(&rpgd_step_kernel<COST_QBGM, PREDICTOR_ODE, true>);
  // the CEM top-k sorts N (padded to a power of two) 8-byte records in LDS: 128 KB at N = 16384
  allow_large_lds(&cem_update_kernel);
}

extern "C" {

int cpmppi_rollout_cost(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                        const float* target_equilibrium, const float* L, float* S_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !s0 || !inputs || !target_position || !target_equilibrium || !S_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rollout_cost: bad argument");
  if (h->prm.cost_id == CPMPPI_COST_LEGACY)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rollout_cost: plugin costs only");
  if (!pole_mass_rows_cover(h, E)) return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short("cpmppi_rollout_cost", h, E));
  if (const int rc = refuse_tuning_rows(h, "cpmppi_rollout_cost")) return rc;
  CPMPPI_ON_DEVICE(h);
  Params prm = h->prm;
  prm.shift_mode = CPMPPI_SHIFT_NONE;
  prm.cc_weight = 0.0f;
  // (a cost-only launch: the inputs are the perturbations of a zero nominal sequence; no finalize)
  const cpmppi_plan::RolloutPlan plan = plan_launch(h, E, CPMPPI_NOISE_DELTA_U);
  StepPtrs p{};
  p.s0 = s0; p.u_nom = h->zeros_H; p.x_t = target_position; p.te = target_equilibrium; p.L = L; p.noise = inputs;
  p.nb = plan.nb; p.W = plan.W; p.stash = plan.stash;
  p.S_out = S_out; p.partial = h->workspace;
  return launch_rollout(h, prm, plan, (hipStream_t)stream, p);
}

// What the entry points that run the adjoint sweep refuse about the HANDLE, in two parts (cpmppi_rollout_cost_grad asks for the
// pole-mass rows between them): the cost and the arithmetic, then the launch's shape - N <= BLOCK for the one-workgroup-per-env
// steps, and `lds`, the launch's dynamic LDS bytes.  The three families word the refusals their own way.
struct SweepWords {
  const char* unbuilt;     // "<who>: <unbuilt> quadratic_boundary / ..."
  const char* subject;     // "<who>: <subject> is written for the FAST arithmetic"
  const char* rows;        // what a lane of a one-workgroup-per-env step holds; NULL: the flat launch, any N
  const char* lds_hint;    // behind "S too large for the LDS sub-state buffer"
};
constexpr SweepWords GRAD_WORDS{"no adjoint for", "the adjoint", nullptr, " (<= 25)"};
constexpr SweepWords RPGD_WORDS{"no adjoint for", "the adjoint", "plans", ""};
constexpr SweepWords CEM_WORDS{"not built for", "the sweep", "samples", ""};       // (cem also runs without the adjoint)

static int sweep_check_handle(cpmppi_handle* h, const char* who, const SweepWords& words) {
  const std::string w(who);
  if (h->prm.cost_id == CPMPPI_COST_LEGACY) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": plugin costs only");
  if (h->prm.qb_mode != 0u)
    return fail(h, CPMPPI_ERR_BAD_ARG, w + ": " + words.unbuilt + " quadratic_boundary / quadratic_boundary_nonconvex "
                                           "(built: quadratic_boundary_grad_minimal, default, quadratic_boundary_grad)");
  if (h->cfg.math_mode != CPMPPI_MATH_FAST)
    return fail(h, CPMPPI_ERR_BAD_ARG, w + ": " + words.subject + " is written for the FAST arithmetic");
  return CPMPPI_OK;
}

static int sweep_check_shape(cpmppi_handle* h, const char* who, const SweepWords& words, size_t lds) {
  const std::string w(who);
  if (words.rows && h->cfg.N > (uint32_t)BLOCK)
    return fail(h, CPMPPI_ERR_BAD_ARG, w + ": one workgroup per env holds at most " + std::to_string(BLOCK) + " " + words.rows +
                                           " (N = " + std::to_string(h->cfg.N) + ")");
  if (lds > 150 * 1024) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": S too large for the LDS sub-state buffer" + words.lds_hint);
  return CPMPPI_OK;
}

// (grow_workspace and refuse_unreserved_capture, which the entry points below share with cpmppi_rollout_cost_grad_gru, are in
// cpmppi_internal.hpp)

int cpmppi_rollout_cost_grad(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs,
                             const float* target_position, const float* target_equilibrium, const float* L,
                             const float* previous_input, float* S_out, float* grad_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !s0 || !inputs || !target_position || !target_equilibrium || !grad_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rollout_cost_grad: bad argument");
  const size_t lds = (size_t)h->cfg.S * 6 * BLOCK * sizeof(float);
  if (const int rc = sweep_check_handle(h, "cpmppi_rollout_cost_grad", GRAD_WORDS)) return rc;
  if (!pole_mass_rows_cover(h, E)) return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short("cpmppi_rollout_cost_grad", h, E));
  if (const int rc = refuse_tuning_rows(h, "cpmppi_rollout_cost_grad")) return rc;
  if (const int rc = sweep_check_shape(h, "cpmppi_rollout_cost_grad", GRAD_WORDS, lds)) return rc;
  CPMPPI_ON_DEVICE(h);
  const size_t B = (size_t)E * h->cfg.N;
  if (const int rc = grow_workspace(h, h->grad_ckpt, h->grad_ckpt_floats, (size_t)h->cfg.H * 6 * (size_t)h->cfg.E * h->cfg.N)) return rc;
  GradPtrs a{s0, inputs, target_position, target_equilibrium, L, previous_input, h->grad_ckpt, S_out, grad_out, E, h->m_pole_rows};
  const auto launch = h->cfg.ode_predictor == CPMPPI_ODE_CROMER ? launch_grad<PREDICTOR_ODE> : launch_grad<PREDICTOR_ODE_V0>;
  launch(h->prm.cost_id, dim3((unsigned)((B + BLOCK - 1) / BLOCK)), lds, (hipStream_t)stream, h->prm, a);
  return launched(h);
}

int cpmppi_adam_step(cpmppi_handle* h, uint32_t E, float* Q, const float* grad, float* m, float* v, uint32_t iteration,
                     float learning_rate, float beta1, float beta2, float epsilon, float gradmax_clip, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !Q || !grad || !m || !v || iteration == 0)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_adam_step: bad argument (iteration counts from 1)");
  CPMPPI_ON_DEVICE(h);
  const size_t rows = (size_t)E * h->cfg.N;
  // Keras Adam: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), epsilon outside the square root
  const double lr_t = (double)learning_rate * sqrt(1.0 - pow((double)beta2, (double)iteration)) /
                      (1.0 - pow((double)beta1, (double)iteration));
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)((rows + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                     rows, h->cfg.H, Q, grad, m, v, (float)lr_t, beta1, beta2, epsilon, gradmax_clip, h->prm.lo, h->prm.hi);
  return launched(h);
}

int cpmppi_rpgd_reserve(cpmppi_handle* h, uint32_t E) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_rpgd_reserve: bad argument (0 < E <= config.E)");
  if (const int rc = sweep_check_handle(h, "cpmppi_rpgd_reserve", RPGD_WORDS)) return rc;
  if (const int rc = sweep_check_shape(h, "cpmppi_rpgd_reserve", RPGD_WORDS, rpgd_lds_bytes(h))) return rc;
  CPMPPI_ON_DEVICE(h);
  return grow_workspace(h, h->rpgd_ws, h->rpgd_ws_floats, rpgd_floats(h, E));
}

// cpmppi_rpgd_step and cpmppi_rpgd_step_rows: one body that checks and launches.  `who`: the caller's name, which every refusal
// begins with; `with_rows`: the second one, whose `rows` [n_rows][CPMPPI_TUNING_ROW_FLOATS] the kernel reads per env.
static int rpgd_step_impl(cpmppi_handle* h, const cpmppi_rpgd_args* a, void* stream, const char* who, bool with_rows,
                          const float* rows, uint32_t n_rows) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const std::string w(who);
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": null argument block");
  if (a->E == 0 || a->E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": bad argument (0 < E <= config.E)");
  if (!a->s0 || !a->target_position || !a->target_equilibrium || !a->Q || !a->m || !a->v || !a->Q_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, w + ": null pointer (s0, target_position, target_equilibrium, Q, m, v and Q_out are required)");
  for (const void* ptr : {(const void*)a->s0, (const void*)a->target_position, (const void*)a->target_equilibrium, (const void*)a->L,
                          (const void*)a->previous_input, (const void*)a->Q, (const void*)a->m, (const void*)a->v, (const void*)a->Q_out,
                          (const void*)a->S_out, (const void*)a->plan_out, (const void*)a->order_out})
    if (misaligned(ptr)) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": misaligned pointer");
  if (reinterpret_cast<uintptr_t>(a->count_dev) & 7u) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": misaligned pointer (count_dev: 8 bytes)");
  if (a->iterations == 0) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": iterations must be > 0");
  if (a->keep_k == 0 || a->keep_k > h->cfg.N) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": bad argument (0 < keep_k <= N)");
  if (a->shift > h->cfg.H) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": shift exceeds the horizon");
  if (a->distribution > CPMPPI_RPGD_UNIFORM) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": unknown distribution");
  if (const int rc = sweep_check_handle(h, who, RPGD_WORDS)) return rc;
  if (const int rc = sweep_check_shape(h, who, RPGD_WORDS, rpgd_lds_bytes(h))) return rc;
  if (!pole_mass_rows_cover(h, a->E)) return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short(who, h, a->E));
  if (with_rows) {
    if (!rows) return fail(h, CPMPPI_ERR_BAD_ARG, w + ": null pointer (rows)");
    if ((reinterpret_cast<uintptr_t>(rows) & (CPMPPI_TUNING_ROW_FLOATS * sizeof(float) - 1u)) != 0)
      return fail(h, CPMPPI_ERR_BAD_ARG, w + ": misaligned pointer (rows are 64 bytes and 64-byte aligned)");
    if (n_rows < a->E)
      return fail(h, CPMPPI_ERR_BAD_ARG, w + ": " + std::to_string(a->E) + " envs, but rows holds " + std::to_string(n_rows) + " rows");
    if (h->cfg.cost_id != CPMPPI_COST_QBGM)
      return fail(h, CPMPPI_ERR_BAD_ARG, w + ": a row holds the cost vector of quadratic_boundary_grad_minimal: the handle has another cost plugin");
  }
  if (const int rc = refuse_tuning_rows(h, who)) return rc;
  CPMPPI_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  if (h->rpgd_ws_floats < rpgd_floats(h, a->E)) {
    if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_rpgd_reserve")) return rc;
    if (const int rc = cpmppi_rpgd_reserve(h, a->E)) return rc;
  }
  const uint32_t Nb = rpgd_block(h);
  RpgdPtrs p{};
  p.s0 = a->s0; p.x_t = a->target_position; p.te = a->target_equilibrium; p.L = a->L; p.prev_in = a->previous_input;
  p.m_pole = h->m_pole_rows;
  p.Q = a->Q; p.m = a->m; p.v = a->v;
  p.ckpt = h->rpgd_ws; p.grad = h->rpgd_ws + (size_t)h->cfg.H * 6 * a->E * Nb;
  p.count_dev = (const unsigned long long*)a->count_dev;
  p.count = a->count; p.seed = a->seed; p.draw_offset = a->draw_offset;
  p.iterations = a->iterations; p.adam_iteration = a->adam_iteration; p.keep_k = a->keep_k; p.resamp_per = a->resamp_per;
  p.shift = a->shift; p.uniform = a->distribution == CPMPPI_RPGD_UNIFORM; p.env_offset = a->env_offset;
  p.lr = a->learning_rate; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->epsilon; p.gradmax_clip = a->gradmax_clip;
  p.sample_mean = a->sample_mean; p.uniform_lo = a->uniform_lo; p.uniform_hi = a->uniform_hi;
  p.Q_out = a->Q_out; p.S_out = a->S_out; p.plan_out = a->plan_out; p.order_out = a->order_out;
  const bool cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
  if (with_rows) {
    RpgdRowPtrs pr{};
    static_cast<RpgdPtrs&>(pr) = p;
    pr.rows = rows;
    const auto launch = cromer ? launch_rpgd_rows<PREDICTOR_ODE> : launch_rpgd_rows<PREDICTOR_ODE_V0>;
    launch(dim3(a->E), dim3(Nb), rpgd_lds_bytes(h), s, h->prm, pr);
  } else {
    const auto launch = cromer ? launch_rpgd<PREDICTOR_ODE> : launch_rpgd<PREDICTOR_ODE_V0>;
    launch(h->prm.cost_id, dim3(a->E), dim3(Nb), rpgd_lds_bytes(h), s, h->prm, p);
  }
  CPMPPI_HIP(h, hipGetLastError());
  if (a->count_dev) launch_step_count((unsigned long long*)a->count_dev, s);
  return launched(h);
}

int cpmppi_rpgd_step(cpmppi_handle* h, const cpmppi_rpgd_args* a, void* stream) {
  return rpgd_step_impl(h, a, stream, "cpmppi_rpgd_step", false, nullptr, 0);
}

int cpmppi_rpgd_step_rows(cpmppi_handle* h, const cpmppi_rpgd_args* a, const float* rows, uint32_t n_rows, void* stream) {
  return rpgd_step_impl(h, a, stream, "cpmppi_rpgd_step_rows", true, rows, n_rows);
}

int cpmppi_cem_reserve(cpmppi_handle* h, uint32_t E, uint32_t refine) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_reserve: bad argument (0 < E <= config.E)");
  if (refine > CPMPPI_CEM_REFINE_ADAM) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_reserve: unknown refine kind");
  const bool refining = refine != CPMPPI_CEM_REFINE_NONE;
  // (a handle with a network reserves the samples for cpmppi_cem_step_gru, which has both math modes and checks its costs itself)
  if (refining || !h->gru_image)
    if (const int rc = sweep_check_handle(h, "cpmppi_cem_reserve", CEM_WORDS)) return rc;
  if (const int rc = sweep_check_shape(h, "cpmppi_cem_reserve", CEM_WORDS, cem_lds_bytes(h, refining))) return rc;
  CPMPPI_ON_DEVICE(h);
  return grow_workspace(h, h->cem_ws, h->cem_ws_floats, cem_floats(h, E, refining));
}

int cpmppi_cem_step(cpmppi_handle* h, const cpmppi_cem_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: null argument block");
  if (a->E == 0 || a->E > h->cfg.E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: bad argument (0 < E <= config.E)");
  if (!a->s0 || !a->target_position || !a->target_equilibrium || !a->mean || !a->stdev || !a->Q_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: null pointer (s0, target_position, target_equilibrium, mean, stdev and Q_out are required)");
  for (const void* ptr : {(const void*)a->s0, (const void*)a->target_position, (const void*)a->target_equilibrium, (const void*)a->L,
                          (const void*)a->previous_input, (const void*)a->mean, (const void*)a->stdev, (const void*)a->Q_out,
                          (const void*)a->S_out, (const void*)a->plan_out, (const void*)a->samples_out, (const void*)a->order_out})
    if (misaligned(ptr)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: misaligned pointer");
  if (reinterpret_cast<uintptr_t>(a->count_dev) & 7u) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: misaligned pointer (count_dev: 8 bytes)");
  if (a->iterations == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: iterations must be > 0");
  if (a->best_k == 0 || a->best_k > h->cfg.N) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: bad argument (0 < best_k <= N)");
  if (a->shift > h->cfg.H) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: shift exceeds the horizon");
  if (a->refine > CPMPPI_CEM_REFINE_ADAM) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_step: unknown refine kind");
  const bool refine = a->refine != CPMPPI_CEM_REFINE_NONE;
  if (const int rc = sweep_check_handle(h, "cpmppi_cem_step", CEM_WORDS)) return rc;
  if (const int rc = sweep_check_shape(h, "cpmppi_cem_step", CEM_WORDS, cem_lds_bytes(h, refine))) return rc;
  if (!pole_mass_rows_cover(h, a->E)) return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short("cpmppi_cem_step", h, a->E));
  if (const int rc = refuse_tuning_rows(h, "cpmppi_cem_step")) return rc;
  CPMPPI_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  if (h->cem_ws_floats < cem_floats(h, a->E, refine)) {
    if (const int rc = refuse_unreserved_capture(h, s, "cpmppi_cem_step", "cpmppi_cem_reserve")) return rc;
    if (const int rc = cpmppi_cem_reserve(h, a->E, a->refine)) return rc;
  }
  const uint32_t Nb = rpgd_block(h);
  const size_t plane = (size_t)h->cfg.H * a->E * Nb;           // one [E][H][block] array
  CemPtrs p{};
  p.s0 = a->s0; p.x_t = a->target_position; p.te = a->target_equilibrium; p.L = a->L; p.prev_in = a->previous_input;
  p.m_pole = h->m_pole_rows;
  p.mean = a->mean; p.stdev = a->stdev;
  p.samples = h->cem_ws;
  if (refine) { p.ckpt = h->cem_ws + plane; p.grad = h->cem_ws + 7 * plane; p.m = h->cem_ws + 8 * plane; p.v = h->cem_ws + 9 * plane; }
  p.count_dev = (const unsigned long long*)a->count_dev;
  p.seed = a->seed; p.offset = a->offset;
  p.iterations = a->iterations; p.best_k = a->best_k; p.adam = a->refine == CPMPPI_CEM_REFINE_ADAM; p.shift = a->shift;
  p.env_offset = a->env_offset;
  p.stdev_min = a->stdev_min; p.lr = a->learning_rate; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->epsilon;
  p.gradmax_clip = a->gradmax_clip; p.mean_fill = a->mean_fill; p.stdev_fill = a->stdev_fill;
  p.Q_out = a->Q_out; p.S_out = a->S_out; p.plan_out = a->plan_out; p.samples_out = a->samples_out; p.order_out = a->order_out;
  const bool cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
  const auto launch = refine ? (cromer ? launch_cem<PREDICTOR_ODE, true> : launch_cem<PREDICTOR_ODE_V0, true>)
                             : (cromer ? launch_cem<PREDICTOR_ODE, false> : launch_cem<PREDICTOR_ODE_V0, false>);
  launch(h->prm.cost_id, dim3(a->E), dim3(Nb), cem_lds_bytes(h, refine), s, h->prm, p);
  CPMPPI_HIP(h, hipGetLastError());
  if (a->count_dev) launch_step_count((unsigned long long*)a->count_dev, s);
  return launched(h);
}

int cpmppi_sgd_step(cpmppi_handle* h, uint32_t E, float* Q, const float* grad, float learning_rate, float gradmax_clip,
                    void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !Q || !grad) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_sgd_step: bad argument");
  CPMPPI_ON_DEVICE(h);
  const size_t rows = (size_t)E * h->cfg.N;
  hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)((rows + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                     rows, h->cfg.H, Q, grad, learning_rate, gradmax_clip, h->prm.lo, h->prm.hi);
  return launched(h);
}

int cpmppi_cem_sample(cpmppi_handle* h, uint32_t E, const float* mean, const float* stdev, uint64_t seed, uint64_t offset,
                      uint32_t env_offset, float* Q_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !mean || !stdev || !Q_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_sample: bad argument");
  CPMPPI_ON_DEVICE(h);
  const size_t rows = (size_t)E * h->cfg.N;
  hipLaunchKernelGGL(cem_sample_kernel, dim3((unsigned)((rows + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                     h->prm, E, mean, stdev, seed, offset, env_offset, Q_out);
  return launched(h);
}

int cpmppi_cem_gmm_sample(cpmppi_handle* h, uint32_t E, const float* centres, uint32_t K, const float* stdev, uint64_t seed,
                          uint64_t offset, uint32_t env_offset, float* Q_out, uint32_t* component_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !centres || K == 0 || !stdev || !Q_out)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_gmm_sample: bad argument");
  CPMPPI_ON_DEVICE(h);
  const size_t rows = (size_t)E * h->cfg.N;
  hipLaunchKernelGGL(cem_gmm_sample_kernel, dim3((unsigned)((rows + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                     h->prm, E, centres, K, stdev, seed, offset, env_offset, Q_out, component_out);
  return launched(h);
}

int cpmppi_cem_update(cpmppi_handle* h, uint32_t E, const float* S, const float* Q, uint32_t best_k, float stdev_min,
                      float* mean_out, float* stdev_out, uint32_t* elite_idx_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || !S || !Q || !mean_out || !stdev_out || best_k == 0 || best_k > h->cfg.N)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_update: bad argument (0 < best_k <= N)");
  uint32_t Np = 1;
  while (Np < h->cfg.N) Np <<= 1;
  if ((size_t)Np * 8 > 160 * 1024 - 1024) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_cem_update: N too large for the LDS sort (<= 16384)");
  CPMPPI_ON_DEVICE(h);
  hipLaunchKernelGGL(cem_update_kernel, dim3(E), dim3(BLOCK), (size_t)Np * 8, (hipStream_t)stream, h->prm, S, Q, best_k,
                     stdev_min, Np, mean_out, stdev_out, elite_idx_out);
  return launched(h);
}

}  // extern "C"
