// The per-lane pieces of the fused rpgd / gradient-tf control step (rpgd_step_kernel, cpmppi_optim.hip; contract:
// cpmppi_rpgd_step in include/cpmppi.h): one lane owns one plan of one env and carries it through the adjoint sweep, the Adam
// update and the redraw.  The sweep is rollout_grad_kernel's, statement for statement, over the substep functions of
// cpmppi_grad.hpp / cpmppi_device.hpp; only where the check-points and the gradient go differs (a workspace slice of the env,
// lane-contiguous with the block's width as the stride).
#pragma once
#include "cpmppi_grad.hpp"

namespace cpmppi {

// What a lane's sweeps share within one control step.
struct RpgdLane {
  const float* s0;        // [6] the env's state
  const float* Q;         // [H] the lane's plan (QSTRIDED: [H][stride] + lane)
  float x_t, te, ub0;     // targets, the control applied before this step
  float cos0, sin0;
  float scale;
  bool clip;
  uint32_t stride;        // the block's width: stride of ckpt / grad / sub
  float* ckpt;            // [H][6][stride] + lane
  float* grad;            // [H][stride] + lane
  float* sub;             // LDS [S][6][stride] + lane
};

// Cost of the lane's plan; `backward`: also its gradient -> w.grad (a run-time flag, uniform over the launch: the final cost of a
// control step is the forward half of the one sweep the kernel holds).  `pi`: the block the integration computes with (the
// env's own pole mass under predictor_ODE), `p`: the launch's (costs).  QSTRIDED: the plan is a workspace column like the
// check-points (the fused CEM step), not a row.
template <int COST, int INTEG, bool QSTRIDED = false>
__device__ __forceinline__ float rpgd_sweep(const Params& p, const Params& pi, const EnvConst& ec, const RpgdLane& w,
                                            bool backward) {
  const uint32_t H = p.H, S = p.S, B = w.stride;
  auto plan = [&](uint32_t k) __attribute__((always_inline)) { return QSTRIDED ? w.Q[(size_t)k * B] : w.Q[k]; };
  const float t = p.t_step;
  auto forward_substep = [&](State<float>& s, float uK) __attribute__((always_inline)) {
    if constexpr (INTEG == PREDICTOR_ODE) substep_cromer_plain(s, uK, p.t_step, pi, ec);
    else substep_fast<float>(s, uK, p.t_step, p, ec, p.THL);
  };
  const float* __restrict__ s0 = w.s0;
  const float x_t = w.x_t, te = w.te, scale = w.scale;
  const bool clip = w.clip;

  // ---- forward, check-pointing every control step
  State<float> st{s0[0], s0[1], s0[2], s0[3], s0[4], s0[5]};
  float cost = 0.0f, cosang = w.cos0, u_before = w.ub0;
  for (uint32_t k = 0; k < H; ++k) {
    if (backward) {
      float* ck = w.ckpt + ((size_t)k * 6) * B;
      ck[0] = st.th; ck[B] = st.w; ck[2 * B] = st.c; ck[3 * B] = st.s; ck[4 * B] = st.x; ck[5 * B] = st.v;
    }
    float ur = plan(k);
    if (clip) ur = clamp_(ur, p.lo, p.hi);
    if constexpr (COST == COST_QBGM) cost += stage_qbgm<float, true>(p, st.x, cosang, st.w, ur, x_t, te);
    else if constexpr (COST == COST_DEFAULT) cost += stage_default<float, true>(p, st.x, cosang, ur, x_t, te);
    else cost += stage_qbg<float, true>(p, st.x, cosang, st.w, ur, u_before, x_t, te);
    u_before = ur;
    const float uK = ur * ec.uK_scale;
    for (uint32_t s = 0; s < S; ++s) forward_substep(st, uK);
    cosang = st.c;
  }
  const float term = (COST == COST_DEFAULT) ? terminal_indicator<float>(p, st.th, st.x, x_t) : 0.0f;
  const float total = (cost + term) * scale;
  if (!backward) return total;

  // ---- backward
  Adjoint lam{0.0f, 0.0f, 0.0f, 0.0f};
  float carry = 0.0f;
  for (uint32_t k = H; k-- > 0;) {
    const float* ck = w.ckpt + ((size_t)k * 6) * B;
    const State<float> st0{ck[0], ck[B], ck[2 * B], ck[3 * B], ck[4 * B], ck[5 * B]};
    const float q = plan(k);
    const bool clipped = clip && (q < p.lo || q > p.hi);
    const float ur = clip ? clamp_(q, p.lo, p.hi) : q;
    const float uK = ur * ec.uK_scale;
    State<float> s = st0;
    for (uint32_t i = 0; i < S; ++i) {
      float* d = w.sub + (size_t)i * 6 * B;
      d[0] = s.th; d[B] = s.w; d[2 * B] = s.c; d[3 * B] = s.s; d[4 * B] = s.x; d[5 * B] = s.v;
      forward_substep(s, uK);
    }
    float guK = 0.0f;
    for (uint32_t i = S; i-- > 0;) {
      const float* d = w.sub + (size_t)i * 6 * B;
      const State<float> si{d[0], d[B], d[2 * B], d[3 * B], d[4 * B], d[5 * B]};
      substep_reverse<(INTEG == PREDICTOR_ODE)>(si, uK, t, pi, ec, lam, guK);
    }
    const float ca = (k == 0) ? w.cos0 : st0.c, sa = (k == 0) ? w.sin0 : st0.s;
    float ub = w.ub0;
    if (COST == COST_QBG && k > 0) { ub = plan(k - 1); if (clip) ub = clamp_(ub, p.lo, p.hi); }
    StageGrad sg;
    if constexpr (COST == COST_QBGM) sg = stage_qbgm_grad(p, st0.x, ca, st0.w, ur, x_t, te);
    else if constexpr (COST == COST_DEFAULT) sg = stage_default_grad(p, st0.x, ca, ur, x_t, te);
    else sg = stage_qbg_grad(p, st0.x, ca, st0.w, ur, ub, x_t, te);
    lam.x = __builtin_fmaf(scale, sg.x, lam.x);
    lam.w = __builtin_fmaf(scale, sg.w, lam.w);
    lam.th = __builtin_fmaf(scale * sg.cosang, -sa, lam.th);
    const float gk = __builtin_fmaf(guK, ec.uK_scale, scale * sg.u + carry);
    carry = scale * sg.u_before;
    w.grad[(size_t)k * B] = clipped ? 0.0f : gk;
  }
  return total;
}

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
