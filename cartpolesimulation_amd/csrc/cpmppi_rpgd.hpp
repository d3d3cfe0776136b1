// The per-lane pieces of the fused rpgd / gradient-tf control step (rpgd_step_kernel, cpmppi_optim.hip; contract:
// cpmppi_rpgd_step in include/cpmppi.h) beside the adjoint sweep of cpmppi_grad.hpp: one lane owns one plan of one env and carries
// it through the sweep, the Adam update and the redraw.  The sweep's check-points and gradient are a workspace slice of the env,
// lane-contiguous with the block's width as the stride.
#pragma once
#include "cpmppi_philox.hpp"
#include "cpmppi_grad.hpp"

namespace cpmppi {

// Keras Adam's step length lr sqrt(1 - beta2^t) / (1 - beta1^t) at iteration t (counted from 1), in double and rounded once, as
// cpmppi_adam_step forms it on the host.  The powers are carried from iteration to iteration: pow() once per control step.
struct RpgdLr {
  double b1t, b2t;        // beta1^t, beta2^t of the iteration before the next
  __device__ __forceinline__ RpgdLr(float beta1, float beta2, uint64_t taken)
      : b1t(pow((double)beta1, (double)taken)), b2t(pow((double)beta2, (double)taken)) {}
  __device__ __forceinline__ float next(float lr, float beta1, float beta2) {
    b1t *= (double)beta1; b2t *= (double)beta2;
    return (float)((double)lr * sqrt(1.0 - b2t) / (1.0 - b1t));
  }
};

// adam_step_kernel's update of one row, the gradient read from the lane's workspace column (ROWSTRIDED: Q, m, v as well).
template <bool ROWSTRIDED = false>
__device__ __forceinline__ void rpgd_adam_row(uint32_t H, float* Q, float* m, float* v, const float* grad, uint32_t stride,
                                              float lr_t, float beta1, float beta2, float eps, float gradmax_clip, float lo,
                                              float hi) {
  float ss = 0.0f;
  for (uint32_t k = 0; k < H; ++k) { const float g = grad[(size_t)k * stride]; ss = __builtin_fmaf(g, g, ss); }
  const float nrm = sqrtf(ss);
  const float sc = (gradmax_clip > 0.0f && nrm > gradmax_clip) ? gradmax_clip / nrm : 1.0f;
  for (uint32_t k = 0; k < H; ++k) {
    const float gk = grad[(size_t)k * stride] * sc;
    const size_t i = ROWSTRIDED ? (size_t)k * stride : k;
    const float mk = beta1 * m[i] + (1.0f - beta1) * gk;
    const float vk = beta2 * v[i] + (1.0f - beta2) * gk * gk;
    m[i] = mk; v[i] = vk;
    Q[i] = clamp_(Q[i] - lr_t * mk / (sqrtf(vk) + eps), lo, hi);
  }
}

// The redraw of one plan: sample_kernel's delta_u[env, n, k] for Philox-drawn knots, evaluated on demand (the two knots around
// k are kept while k stays between them), then shaped and clipped as the optimizer shapes a fresh draw.
struct RpgdFresh {
  uint32_t j = 0xFFFFFFFFu;
  float zl = 0.0f, zh = 0.0f;
};
__device__ __forceinline__ float rpgd_fresh(RpgdFresh& f, const Params& p, uint64_t seed, uint64_t offset, uint32_t env,
                                            uint32_t n, uint32_t k, bool uniform, float mean, float ulo, float uhi) {
  const uint32_t j = k / p.period, i = k % p.period;
  if (j != f.j) {
    f.zl = (j == f.j + 1u && f.j != 0xFFFFFFFFu) ? f.zh : philox_knot(seed, offset, env, n, j, p.sigma);
    f.zh = philox_knot(seed, offset, env, n, j + 1u, p.sigma);
    f.j = j;
  }
  const float z = p.interp_f32 ? interp_from_slope32(knot_slope32(f.zl, f.zh, 1.0f / (float)p.period), f.zl, i)
                               : interp_knots(f.zl, f.zh, i, p.period);
  float q;
  if (uniform) {
#pragma clang fp contract(off)      // (the optimizer's torch expression rounds every operation)
    const float cdf2 = 1.0f + erff(z * 0.70710678118654752f);
    const float span = (uhi - ulo) * 0.5f;
    q = ulo + span * cdf2;
  } else {
    q = (mean != 0.0f) ? z + mean : z;
  }
  return clamp_(q, p.lo, p.hi);
}

}  // namespace cpmppi
