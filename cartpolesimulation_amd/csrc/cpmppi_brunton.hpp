// cpmppi_brunton.hpp — the Brunton test's argument block and error statistics; included by the two units that hold its
// kernels (cpmppi_seams.hip, cpmppi_gru_seam.hip) and by nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cpmppi_wave.hpp"

namespace cpmppi {

// ---- Brunton test (cpmppi_brunton): what its ODE kernel (cpmppi_seams.hip) and its GRU kernel (cpmppi_gru_seam.hip) share ----------
// A start is row t = start + i of recording r; b = r * count + i numbers the starts.  partials[rows][horizon][6][3]: per horizon
// step and feature (sum |e|, sum e^2, max |e|) over the starts of one partial row - a workgroup of the ODE kernel, a wave of the
// GRU kernel - written with plain stores by the row's owner and reduced over the rows in a fixed order (brunton_finalize_kernel).
constexpr int BRUNTON_STATS = 18;
struct BruntonArgs {
  const float* states;   // [R,T,6]
  const float* Q;        // [R,T]
  const float* L;        // [R,T] or NULL (ODE only)
  const float* h_rows;   // [R,T,2,32] or NULL = 0 (GRU only)
  float* partials;       // [rows][horizon][6][3]
  float* pred;           // [R*count, horizon+1, 6] or NULL
  uint32_t R, T, start, count, horizon;
};

// e = predicted - recorded in float32, feature 0 (the angle) wrapped afterwards: e - 2 pi rint(e / 2 pi).  Every operation rounds
// once, wherever the function is inlined.
__device__ __forceinline__ void brunton_errors(const float pred[6], const float* __restrict__ rec, float e[6]) {
#pragma clang fp contract(off)
  constexpr float TWO_PI = 6.2831853071795864769f;
#pragma unroll
  for (int f = 0; f < 6; ++f) e[f] = pred[f] - rec[f];
  e[0] = e[0] - TWO_PI * rintf(e[0] / TWO_PI);
}

// The wave's (sum |e|, sum e^2, max |e|) per feature over the lanes that `counts`, stored to out[6][3] by the lane that `writes`,
// feature by feature (eighteen wave-uniform results held at once cost the ODE kernel SGPR spills).  Lanes that do not count
// enter as +0: no sum and no maximum of absolute values moves.
__device__ __forceinline__ void brunton_wave_stats(const float e[6], bool counts, bool writes, float* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const float a = counts ? fabsf(e[f]) : 0.0f;
    const float s1 = wave_sum(a), s2 = wave_sum(a * a), m = wave_max(a);
    if (writes) { out[3 * f + 0] = s1; out[3 * f + 1] = s2; out[3 * f + 2] = m; }
  }
}

}  // namespace cpmppi
