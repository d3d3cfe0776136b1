// cpmppi_train.hpp — what the three training units share (cpmppi_gru_train.hip, cpmppi_ode_fit.hip, cpmppi_dense.hip; nothing else includes it): Adam's
// update, the host check of a batch of windows, and the two refusals they word alike.
#pragma once
#include <math.h>
#include "cpmppi_internal.hpp"

// Adam at step t (cpmppi.h states the update): float64 arithmetic on float32 storage.
struct AdamStep {
  double b1, b2, c1, c2;
  float lr, eps;
  __device__ __forceinline__ AdamStep(float beta1, float beta2, float rate, float epsilon, unsigned long long t)
      : b1(beta1), b2(beta2), c1(1.0 - pow(b1, (double)t)), c2(1.0 - pow(b2, (double)t)), lr(rate), eps(epsilon) {}
  // One parameter x with the gradient g: both moments move on and are stored rounded; -> the new x, from the unrounded moments.
  // (x by reference: it is read behind the two stores, which it may alias for all the compiler knows - the order the kernels had)
  __device__ __forceinline__ double operator()(float& m, float& v, double g, const float& x) const {
    const double dm = b1 * (double)m + (1.0 - b1) * g;
    const double dv = b2 * (double)v + (1.0 - b2) * g * g;
    m = (float)dm;
    v = (float)dv;
    return (double)x - (double)lr * (dm / c1) / (sqrt(dv / c2) + (double)eps);
  }
};

// The host copy of a batch, which every call checks: window b = (r, t0) needs r < R and `rows` rows from t0 on inside the recording's
// T.  `rule`: the caller's words for that, the tail of the refusal.
inline int check_windows(cpmppi_handle* h, const char* who, const uint32_t* windows_host, uint32_t B, uint32_t R, uint32_t T,
                         uint64_t rows, const char* rule) {
  for (uint32_t b = 0; b < B; ++b) {
    const uint64_t r = windows_host[2 * b], t0 = windows_host[2 * b + 1];
    if (r >= R || t0 + rows > (uint64_t)T)
      return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": window " + std::to_string(b) + " = (" + std::to_string(r) + ", " +
                                             std::to_string(t0) + ") lies outside " + rule);
  }
  return CPMPPI_OK;
}

// loss_out, and the fit's grad_out, are float64 (misaligned() tests four bytes).
inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

inline int begun_or_refuse(cpmppi_handle* h, const char* who, bool begun, const char* begin) {
  return begun ? CPMPPI_OK : fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": call " + begin + " first");
}
