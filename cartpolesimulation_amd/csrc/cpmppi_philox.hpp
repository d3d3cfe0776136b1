// cpmppi_philox.hpp — the library's own noise stream (Philox4x32-10, Box-Muller on the hardware transcendentals) and the
// interpolation between knots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpmppi {

// ------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 counter-based generator (Salmon et al. 2011).  Counter = (rollout, env, knot pair, offset lo),
// key = seed.  One call yields the two standard normals of one Box-Muller pair (knots 2j and 2j+1).
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // (the full 64-bit products: one v_mad_u64_u32 each instead of a v_mul_hi_u32 + v_mul_lo_u32 pair)
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// Two standard normals per Philox block (Box-Muller) on the hardware transcendentals: ln u1 = ln2 * v_log_f32(u1),
// v_sin_f32 / v_cos_f32 take their argument in revolutions, so sin(2 pi u2) is v_sin_f32(u2) (abs. error ~1e-6: this
// is the library's OWN noise stream, the same function feeds the sampler kernel and the in-kernel generation).
__device__ __forceinline__ void philox_normal_pair(uint64_t seed, uint64_t offset, uint32_t env, uint32_t rollout,
                                                   uint32_t pair, float& z0, float& z1) {
  uint32_t c0 = rollout, c1 = env, c2 = pair, c3 = (uint32_t)offset;
  philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32));
  const float u1 = (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f;   // (0, 1]
  const float u2 = (float)(c1 >> 8) * 5.9604644775390625e-8f;          // [0, 1)
  const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1)
  z0 = r * __builtin_amdgcn_cosf(u2);
  z1 = r * __builtin_amdgcn_sinf(u2);
}

// All four words of a Philox block: two Box-Muller pairs = the four consecutive knots 4q .. 4q+3 of (env, rollout).
// `second_pair` (wave-uniform) false - a consumer that walks the knots in order and knows where the sequence ends (the rollout
// kernel): knots 4q+2 and 4q+3 lie beyond it, their conversions, log, sqrt, sin and cos are skipped and z[2], z[3] come back as zero.
__device__ __forceinline__ void philox_normal_quad_upto(uint64_t seed, uint64_t offset, uint32_t env, uint32_t rollout,
                                                        uint32_t quad, bool second_pair, float z[4]) {
  uint32_t c0 = rollout, c1 = env, c2 = quad, c3 = (uint32_t)offset;
  philox4x32_10(c0, c1, c2, c3, (uint32_t)seed ^ 0x51ed270bu, (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32));
  const float ua = (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f, ub = (float)(c1 >> 8) * 5.9604644775390625e-8f;
  const float ra = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(ua));
  z[0] = ra * __builtin_amdgcn_cosf(ub);
  z[1] = ra * __builtin_amdgcn_sinf(ub);
  z[2] = 0.0f; z[3] = 0.0f;
  if (second_pair) {
    const float uc = (float)((c2 >> 8) + 1u) * 5.9604644775390625e-8f, ud = (float)(c3 >> 8) * 5.9604644775390625e-8f;
    const float rc = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(uc));
    z[2] = rc * __builtin_amdgcn_cosf(ud);
    z[3] = rc * __builtin_amdgcn_sinf(ud);
  }
}
// (every other consumer - the sampler kernels, philox_knot, the reduction's regeneration - takes the whole block: one body)
__device__ __forceinline__ void philox_normal_quad(uint64_t seed, uint64_t offset, uint32_t env, uint32_t rollout,
                                                   uint32_t quad, float z[4]) {
  philox_normal_quad_upto(seed, offset, env, rollout, quad, true, z);
}

// Knot j of (env, rollout) scaled by sigma (random access; sequential consumers keep the other three of the block).
__device__ __forceinline__ float philox_knot(uint64_t seed, uint64_t offset, uint32_t env, uint32_t rollout,
                                             uint32_t j, float sigma) {
  float z[4];
  philox_normal_quad(seed, offset, env, rollout, j >> 2, z);
  const uint32_t s = j & 3u;
  return sigma * (s == 0u ? z[0] : (s == 1u ? z[1] : (s == 2u ? z[2] : z[3])));
}

// Linear interpolation between knots as scipy interp1d does it at controller_mppi_cartpole.py:444-445:
// slope = float64(float32(hi - lo)) / period ; y = slope * i + float64(lo) ; stored as float32.
__device__ __forceinline__ float interp_knots(float z_lo, float z_hi, uint32_t i, uint32_t period) {
#pragma clang fp contract(off)
  if (i == 0) return z_lo;
  const float diff = z_hi - z_lo;                         // float32 difference, as numpy forms it
  const double slope = (double)diff / (double)period;
  const double prod = slope * (double)i;                  // two roundings (no FMA), as numpy
  return (float)(prod + (double)z_lo);
}

// The same value with the slope hoisted: slope changes only when the knots change (once per `period` steps).
__device__ __forceinline__ double knot_slope(float z_lo, float z_hi, uint32_t period) {
#pragma clang fp contract(off)      // (else sigma*z of philox_knot is fused into this subtraction and skips a rounding)
  const float diff = z_hi - z_lo;
  return (double)diff / (double)period;
}
// float32 form for the FAST path's own Philox noise: slope rounded to float, then ONE fma per control step.
__device__ __forceinline__ float knot_slope32(float z_lo, float z_hi, float inv_period) {
#pragma clang fp contract(off)      // same reason: the knots must be the rounded float32 values the sampler stores
  const float diff = z_hi - z_lo;
  return diff * inv_period;
}
__device__ __forceinline__ float interp_from_slope32(float slope, float z_lo, uint32_t i) {
  return __builtin_fmaf(slope, (float)i, z_lo);
}
__device__ __forceinline__ float interp_from_slope(double slope, float z_lo, uint32_t i) {
#pragma clang fp contract(off)
  if (i == 0) return z_lo;
  const double prod = slope * (double)i;
  return (float)(prod + (double)z_lo);
}

}  // namespace cpmppi
