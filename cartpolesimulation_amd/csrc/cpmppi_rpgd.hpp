// The per-lane pieces of the fused rpgd / gradient-tf control steps (rpgd_step_kernel, cpmppi_optim.hip; contract:
// cpmppi_rpgd_step in include/cpmppi.h - and gru_rpgd_step_kernel, cpmppi_gru_rpgd.hip, over the GRU predictor: cpmppi_rpgd_step_gru) beside the adjoint sweep of cpmppi_grad.hpp: one lane owns one plan of one env and carries
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

// What follows the ranking in a fused rpgd / gradient step (rpgd_step_kernel; gru_rpgd_step_kernel, cpmppi_gru_rpgd.hip), for the
// lane that owns plan row `tid` of `env` (`active`: tid < N) - every lane of the block calls it.  `a`: the kernel's pointer block
// (Q, m, v, keep_k, resamp_per, shift, the redraw's fields as RpgdPtrs names them), `c` the control steps taken before this one,
// order[]: the ranking.  The survivor permutation, the redraw and the shift run column by column: every lane reads column
// k + shift of its SOURCE row, the block meets, every lane writes column k of its OWN row; columns <= k are never read again, so
// one barrier per column.  (Block-uniform: without a resampling and a shift nothing is done and no barrier is met.)
template <class Ptrs>
__device__ __forceinline__ void rpgd_permute_shift(const Params& p, const Ptrs& a, uint32_t env, uint32_t tid, bool active,
                                                   uint64_t c, const uint32_t* order) {
  const uint32_t N = p.N, H = p.H;
  const size_t row = ((size_t)env * N + tid) * H;
  const bool resample = a.resamp_per > 0 && a.keep_k < N && (c + 1) % a.resamp_per == 0;
  if (!resample && a.shift == 0) return;             // (block-uniform)
  const bool fresh = resample && tid >= a.keep_k;
  const size_t src = ((size_t)env * N + ((resample && tid < a.keep_k) ? order[tid] : tid)) * H;
  const uint64_t draw = a.draw_offset + (a.count_dev ? c / (a.resamp_per ? a.resamp_per : 1u) : 0ull);
  RpgdFresh fr;
  for (uint32_t k = 0; k < H; ++k) {
    const uint32_t kk = k + a.shift;
    const bool inside = kk < H;
    const uint32_t kq = inside ? kk : H - 1;         // Q repeats its last element
    float q = 0.0f, mk = 0.0f, vk = 0.0f;
    if (active) {
      if (fresh) {
        q = rpgd_fresh(fr, p, a.seed, draw, a.env_offset + env, tid, kq, a.uniform != 0u, a.sample_mean, a.uniform_lo, a.uniform_hi);
      } else {
        q = a.Q[src + kq];
        if (inside) { mk = a.m[src + kk]; vk = a.v[src + kk]; }
      }
    }
    __syncthreads();
    if (active) { a.Q[row + k] = q; a.m[row + k] = mk; a.v[row + k] = vk; }
  }
}

}  // namespace cpmppi
