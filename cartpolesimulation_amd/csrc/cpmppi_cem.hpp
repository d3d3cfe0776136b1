// The per-lane pieces of the fused CEM control step (cem_step_kernel, cpmppi_optim.hip; contract: cpmppi_cem_step in
// include/cpmppi.h): one lane owns one sample of one env - it draws its row, refines it (the two hybrids), and costs it with
// adjoint_sweep (cpmppi_grad.hpp).  The row lives in a workspace column of the env (lane-contiguous, the block's width as the
// stride), as the check-points and the gradient of the sweep do.
#pragma once
#include "cpmppi_philox.hpp"
#include "cpmppi_rpgd.hpp"

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
