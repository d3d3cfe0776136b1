// The pieces of the fused CEM control steps - cem_step_kernel (cpmppi_optim.hip; contract: cpmppi_cem_step in include/cpmppi.h),
// where one lane owns one sample of one env: it draws its row, refines it (the two hybrids), and costs it with adjoint_sweep
// (cpmppi_grad.hpp); and gru_cem_step_kernel (cpmppi_gru.hip; cpmppi_cem_step_gru), which costs the rows with the GRU rollout
// and shares the sampler's statement, the ranking and the refit.  The row lives in a workspace column of the env (lane-contiguous, the block's width as the
// stride), as the check-points and the gradient of the sweep do.
#pragma once
#include <hip/hip_runtime.h>
#include "cpmppi_params.hpp"
#include "cpmppi_philox.hpp"

namespace cpmppi {

// cem_sample_kernel's statement for row n of `env`: q[k] = clip(mean[k] + stdev[k] z), the normals of Philox pair k >> 1 (the odd
// tail of the horizon uses the first of its pair).  `m`, `sd`: the env's mean and stdev [H] (LDS); `q`: the lane's column.
__device__ __forceinline__ void cem_sample_row(const Params& p, const float* m, const float* sd, uint64_t seed, uint64_t offset,
                                               uint32_t env, uint32_t n, float* q, uint32_t stride) {
  for (uint32_t k = 0; k < p.H; k += 2) {
    float z0, z1;
    philox_normal_pair(seed, offset, env, n, k >> 1, z0, z1);
    q[(size_t)k * stride] = fminf(fmaxf(__builtin_fmaf(sd[k], z0, m[k]), p.lo), p.hi);
    if (k + 1 < p.H) q[(size_t)(k + 1) * stride] = fminf(fmaxf(__builtin_fmaf(sd[k + 1], z1, m[k + 1]), p.lo), p.hi);
  }
}

// The order of cem_update_kernel (cpmppi_optim.hip): numpy's -inf < finite < +inf < NaN, -0.0 == +0.0 (ties by index), padding
// after everything - so that idx[i] < N for every i < best_k <= N whatever S holds.  A float comparison is no order once a key is
// NaN (a sorting network would leave an arbitrary permutation, padded indices included), so the keys are order-preserving uint32
// images of the costs: -0.0 -> +0.0, every NaN -> 0x7FC00000, then all bits flipped if the sign bit is set, else the
// sign bit set; the padding is 0xFFFFFFFF, which no image equals (the canonical NaN maps to 0xFFC00000).
__device__ __forceinline__ uint32_t cem_sort_key(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;                          // -0.0 -> +0.0 (on the bits: independent of the denormal mode)
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;  // every NaN -> the canonical one, above +inf's image
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The same order inside one workgroup that holds the N costs of an env (the fused steps): the lane that holds sample n's cost S
// (`active`: it holds one, n < N) counts the (key, index) pairs below its own among the N keys in LDS and writes order[rank] = n -
// and, when `publish`, order_out[env][rank] (order_out: [E][N] or NULL).  Every lane of the block calls it (two barriers);
// order[] stands when it returns.  key, order: [N] at the least.
__device__ __forceinline__ void rank_costs_at(uint32_t* key, uint32_t* order, uint32_t n, float S, bool active, uint32_t N,
                                              uint32_t env, uint32_t* order_out, bool publish) {
  if (active) key[n] = cem_sort_key(S);
  __syncthreads();
  if (active) {
    const uint32_t mine = key[n];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < N; ++j) {
      const uint32_t kj = key[j];
      rank += (kj < mine || (kj == mine && j < n)) ? 1u : 0u;
    }
    order[rank] = n;
    if (publish && order_out) order_out[(size_t)env * N + rank] = n;
  }
  __syncthreads();
}

// ... for a block that holds one cost per lane, sample tid on lane tid (N <= blockDim.x; key, order: [blockDim.x])
__device__ __forceinline__ void rank_costs(uint32_t* key, uint32_t* order, float S, bool active, uint32_t N, uint32_t env,
                                           uint32_t* order_out, bool publish) {
  if (!active) key[threadIdx.x] = 0xFFFFFFFFu;
  rank_costs_at(key, order, threadIdx.x, S, active, N, env, order_out, publish);
}

// sgd_step_kernel's update of one row, row and gradient read from the lane's workspace columns.
__device__ __forceinline__ void cem_sgd_row(uint32_t H, float* Q, const float* grad, uint32_t stride, float lr, float gradmax_clip,
                                            float lo, float hi) {
  float ss = 0.0f;
  for (uint32_t k = 0; k < H; ++k) { const float g = grad[(size_t)k * stride]; ss = __builtin_fmaf(g, g, ss); }
  const float nrm = sqrtf(ss);
  const float sc = (gradmax_clip > 0.0f && nrm > gradmax_clip) ? gradmax_clip / nrm : 1.0f;
  for (uint32_t k = 0; k < H; ++k) {
    const size_t i = (size_t)k * stride;
    Q[i] = clamp_(Q[i] - lr * (grad[i] * sc), lo, hi);
  }
}

// cem_update_kernel's refit of time-step k: mean and population stdev of column k over the rows order[0 .. best_k), summed in
// that order, the stdev floored.  `col`: the env's samples of time-step k, one per lane.
__device__ __forceinline__ void cem_refit_column(const float* col, const uint32_t* order, uint32_t best_k, float stdev_min,
                                                 float& mean, float& stdev) {
  float m = 0.0f;
  for (uint32_t i = 0; i < best_k; ++i) m += col[order[i]];
  m /= (float)best_k;
  float v = 0.0f;
  for (uint32_t i = 0; i < best_k; ++i) { const float d = col[order[i]] - m; v = __builtin_fmaf(d, d, v); }
  mean = m;
  stdev = fmaxf(sqrtf(v / (float)best_k), stdev_min);
}

}  // namespace cpmppi
