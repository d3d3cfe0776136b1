// cpmppi_ode.hpp — the two in-tree ODE predictors as device functions: substeps and control steps of predictor_ODE_v0
// (simultaneous Euler, edge bounce) and predictor_ODE (Euler-Cromer), PRECISE and FAST, and the plant's substep.
//
// Arithmetic spec: SURVEY.md Appendix A, restating (reference checkout paths)
//   CartPole/cartpole_equations.py:44-105   _cartpole_ode
//   CartPole/cartpole_equations.py:356-364  cartpole_integration_numba (simultaneous forward Euler)
//   CartPole/cartpole_equations.py:341-347  edge_bounce
//   CartPole/_CartPole_mathematical_helpers.py:24-29  wrap_angle_rad_inplace
//   CartPole/cartpole_numba.py:55-78        cartpole_fine_integration_numba (the substep loop)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cpmppi_debug.hpp"
#include "cpmppi_params.hpp"

namespace cpmppi {

// ------------------------------------------------------------------------------------------------------------------
// sincos on [-pi_f32, pi_f32] (the angle is wrapped every substep, so the argument never leaves this range).
// No per-lane quadrant selects: reduce by multiples of pi to |r| <= pi/2 (q in {-1,0,1}, q*PI_HI exact),
// sin x = (-1)^q sin r, cos x = (-1)^q cos r; the sign is a multiply, so every instruction has a packed float2 form.
// Polynomials: sin r = r + r z P3(z), cos r = 1 + z Q4(z), z = r^2, fitted on [-pi/2, pi/2] (Lawson-weighted
// least squares, coefficients rounded to float32): relative error 1.2e-8 (sin), absolute 4.9e-9 (cos) before rounding.
template <class F>
__device__ __forceinline__ void sincos_pi_half(F x, F& sn, F& cs) {
  constexpr float INV_PI = 0.318309886183790672f;
  constexpr float PI_HI = 3.14159274101257324f;
  constexpr float PI_LO = -8.74227765734758577e-8f;
  const F q = rint_(x * splat<F>(INV_PI));
  F r = fma_(-q, splat<F>(PI_HI), x);
  r = fma_(-q, splat<F>(PI_LO), r);
  const F z = r * r;
  // (-1)^q for q in {-1, 0, 1}: 1 - 2|q|; packed float2 has no abs modifier, there q*q is one instruction instead of two
  F sg;
  if constexpr (Width<F>::value == 2) sg = fma_(q * q, splat<F>(-2.0f), splat<F>(1.0f));
  else sg = fma_(abs_(q), splat<F>(-2.0f), splat<F>(1.0f));
  F P = fma_(z, splat<F>(2.6056311526190257e-06f), splat<F>(-0.00019809538207482547f));
  P = fma_(P, z, splat<F>(0.008333065547049046f));
  P = fma_(P, z, splat<F>(-0.16666659712791443f));
  const F rs = r * sg;
  sn = fma_(rs * z, P, rs);
  F Q = fma_(z, splat<F>(-2.6075662162838853e-07f), splat<F>(2.476180816302076e-05f));
  Q = fma_(Q, z, splat<F>(-0.0013888402609154582f));
  Q = fma_(Q, z, splat<F>(0.04166664183139801f));
  Q = fma_(Q, z, splat<F>(-0.5f));
  cs = fma_(z * sg, Q, sg);
}

// _cartpole_ode with the reference's operand grouping (cartpole_equations.py:71-99), IEEE divides, no contraction.
__device__ __forceinline__ void ode_precise(float c, float s, float w, float v, float u, const Params& p,
                                            const EnvConst& e, float& aDD, float& xDD) {
#pragma clang fp contract(off)
  const float A = e.kp1_mt - p.m_pole * (c * c);
  const float F = -p.M_fric * v;
  const float T = -p.J_fric * w;
  const float Lh = e.Lh;
  xDD = (p.m_pole * p.g * s * c + ((T * c) / Lh) + e.kp1 * (-(p.m_pole * Lh * (w * w) * s) + F + u)) / A;
  aDD = (p.g * s + xDD * c + T / (p.m_pole * Lh)) / (e.kp1 * Lh);
}

// One Euler substep, PRECISE: the reference's operand grouping with IEEE divides, libm sincos and no FMA contraction.
__device__ __forceinline__ void substep_precise(State<float>& st, float u, float t, const Params& p,
                                                const EnvConst& e) {
#pragma clang fp contract(off)
  const float w = st.w, v = st.v;
  float aDD, xDD;
  ode_precise(st.c, st.s, w, v, u, p, e, aDD, xDD);
  float th1 = st.th + w * t;
  float w1 = w + aDD * t;
  float x1 = st.x + v * t;
  float v1 = v + xDD * t;
  if (x1 >= p.THL || -x1 >= p.THL) {
    const float cb = cosf(th1);
    w1 = w1 - 2.0f * (v1 * cb) / (0.5f * e.L);
    th1 = th1 + w1 * t;
    v1 = -v1;
    x1 = x1 + v1 * t;
  }
  const float m = fmodf(th1, TWO_PI_F);
  th1 = (m < -PI_F) ? (m + TWO_PI_F) : ((m > PI_F) ? (m - TWO_PI_F) : m);
  st.th = th1; st.w = w1; st.x = x1; st.v = v1;
  st.c = cosf(th1);
  st.s = sinf(th1);
}

// One simulation step of the PLANT (the caller side of the boundary): Euler-Cromer (cartpole_equations.py:367-378),
// edge bounce with cos of the integrated angle (CartPole/__init__.py:462-470), cos/sin (:329-331), wrap (:333-334).
__device__ __forceinline__ void plant_substep(State<float>& st, float aDD, float xDD, float t, const Params& p,
                                              const EnvConst& e) {
#pragma clang fp contract(off)
  float w1 = st.w + aDD * t;
  float v1 = st.v + xDD * t;
  float th1 = st.th + w1 * t;
  float x1 = st.x + v1 * t;
  if (x1 >= p.THL || -x1 >= p.THL) {
    const float cb = cosf(th1);
    w1 = w1 - 2.0f * (v1 * cb) / (0.5f * e.L);
    th1 = th1 + w1 * t;
    v1 = -v1;
    x1 = x1 + v1 * t;
  }
  st.c = cosf(th1);
  st.s = sinf(th1);
  const float m = fmodf(th1, TWO_PI_F);
  st.th = (m < -PI_F) ? (m + TWO_PI_F) : ((m > PI_F) ? (m - TWO_PI_F) : m);
  st.w = w1; st.x = x1; st.v = v1;
}

// ODE + simultaneous forward Euler of one substep with folded constants (FAST).  Outputs the un-wrapped new state.
//   A    = (k+1)(m_c+m_p) - m_p c^2
//   xDD  = [ c (m_p g s - J/Lh w) - (k+1) m_p Lh w^2 s - (k+1) M_fric v + (k+1) u ] / A
//   aDD  = g_i s + xDD c /((k+1)Lh) - cT w                                      (cartpole_equations.py:95-99)
template <class F>
__device__ __forceinline__ void ode_euler_fast(const State<F>& st, F uK, float t, const Params& p, const EnvConst& e,
                                               F& th1, F& w1, F& x1, F& v1, F* aDD_out = nullptr) {
  const F c = st.c, s = st.s, w = st.w, v = st.v;
  const F A = fma_(-(c * splat<F>(p.m_pole)), c, splat<F>(e.kp1_mt));
  const F t1 = fma_(splat<F>(e.mg), s, -(w * splat<F>(e.JinvLh)));
  F num = fma_(c, t1, uK);
  num = fma_(-((w * w) * splat<F>(e.kmLh)), s, num);
  num = fma_(splat<F>(-e.kM), v, num);
  const F r = rcp_(A);                                  // A in [0.33, 0.43]: no scaling needed
  const F xDD = num * r;                                // (<= 1.5 ulp; one Newton correction on top measured the identical deviation: removed, see history)
  const F tt = splat<F>(t);
  th1 = fma_(w, tt, st.th);
  // (do NOT fold "1 - cT*t" into one constant: its rounding error would bias w the same way every substep; measured against
  // the form that folded t into the three angleDD coefficients - one instruction fewer, 2.4x the deviation: removed, see history)
  // g s + T/(m_p Lh) is the bracket t1 = m_p g s - (J/Lh) w of xDD's numerator divided by m_p: one product instead of a
  // product and an FMA per substep (same formula, one rounding placed differently; -1 instruction per substep)
  const F aDD = fma_(xDD * c, splat<F>(e.inv_kLh), t1 * splat<F>(e.t1_i));
  w1 = fma_(aDD, tt, w);
  if (aDD_out) *aDD_out = aDD;
  x1 = fma_(v, tt, st.x);
  v1 = fma_(xDD, tt, v);
}

// Edge bounce of one lane (cartpole_equations.py:341-347), rare.  `cb` = cos of the integrated (un-wrapped) angle.
__device__ __forceinline__ void bounce_lane(float& thi, float& wi, float& xi, float& vi, float cb, float t, float inv_halfL) {
  wi = __builtin_fmaf(-(2.0f * (vi * cb)), inv_halfL, wi);
  thi = __builtin_fmaf(wi, t, thi);
  vi = -vi;
  xi = __builtin_fmaf(vi, t, xi);
}

// theta - 2pi*rint(theta/2pi): k*2pi_f32 is subtracted exactly for |k| <= 2 (Sterbenz), i.e. this IS fmod followed by the
// reference's two comparisons except when theta is within one ulp of +-pi, where both values are the same point of
// the circle; for absurd |theta| (> 4pi in one substep) it differs from the exact fmod by <= 0.5 ulp.
template <class F>
__device__ __forceinline__ F wrap_rint(F th) {
  return fma_(-rint_(th * splat<F>(0.159154943091895336f)), splat<F>(TWO_PI_F), th);
}

// ------------------------------------------------------------------------------------------------------------------
// Rotation by a small angle d: (cos d, sin d) from their Taylor polynomials.
//   rot_pair_lo: degree 5 / 4, |d| <= 0.125 (truncation < 1e-9): evaluated every substep by the one-rollout-per-lane path
//   rot_pair   : degree 7 / 6, |d| <= ROT_LIMIT = 0.25 (truncation 1e-11 / 4e-10): seeds the carried pair of the packed
//                path once per control step and serves every rare event (bounce, fast-spinning lane) of both paths
// |d| = |w t| > 0.25 means an angular velocity beyond 125 rad/s at t = 2 ms; such a lane is evaluated with the exact
// wrap + sincos on every substep (it practically never happens: a pole released from rest tops out near 20 rad/s).
// (ROT_LIMIT_LO = 0.125, ROT_LIMIT = 0.25: defined ahead of EnvConst, which carries the seed's limit as an angular velocity)
// Packed path: the range of |w t| within which a control step runs on the carried rotation pair is ROT_LIMIT_LO.  Seeded from
// rot_pair_lo (two instructions fewer per control step than the degree-7/6 pair; truncation below 1e-9 up to
// 0.125 rad per substep = 62 rad/s at t = 2 ms - a pole released from rest tops out near 20), lanes beyond take the exact sincos
// on every substep.

template <class F>
__device__ __forceinline__ void rot_pair_lo(F d, F& cd, F& sd) {
  const F d2 = d * d;
  sd = fma_(d * d2, fma_(d2, splat<F>(8.3333333e-3f), splat<F>(-1.6666667e-1f)), d);
  cd = fma_(d2, fma_(d2, splat<F>(4.1666667e-2f), splat<F>(-0.5f)), splat<F>(1.0f));
}

template <class F>
__device__ __forceinline__ void rot_pair(F d, F& cd, F& sd) {
  const F d2 = d * d;
  F ps = fma_(d2, splat<F>(-1.9841270e-4f), splat<F>(8.3333333e-3f));
  ps = fma_(ps, d2, splat<F>(-1.6666667e-1f));
  sd = fma_(d * d2, ps, d);
  F pc = fma_(d2, splat<F>(-1.3888889e-3f), splat<F>(4.1666667e-2f));
  pc = fma_(pc, d2, splat<F>(-0.5f));
  cd = fma_(d2, pc, splat<F>(1.0f));
}

// (cos, sin)(a + d) from (cos, sin)(a) and |d| <= ROT_LIMIT.
__device__ __forceinline__ void rotate_lane(float& c, float& s, float d) {
  float cd, sd;
  rot_pair<float>(d, cd, sd);
  const float c1 = __builtin_fmaf(c, cd, -(s * sd)), s1 = __builtin_fmaf(s, cd, c * sd);
  c = c1; s = s1;
}

// Rare event of ONE lane, shared by every FAST substep flavour.  On entry (thi, wi, xi, vi) is the Euler-advanced state
// (angle un-wrapped) and (ci, si) = (cos, sin) of thi if `have_cs`, else they are evaluated here: by rotating the
// previous substep's pair (c0, s0) through d0 = w_old t when |d0| <= ROT_LIMIT, exactly (wrap + polynomial sincos,
// the angle is stored wrapped) otherwise.  A lane beyond the track edge bounces (cartpole_equations.py:341-347: cos of
// the integrated angle, then the angle advances by the NEW angular velocity); (ci, si) follow by one more rotation.
// Returns false if the lane's angular velocity is beyond the rotation range (its caller then treats it exactly on
// every substep).  No libm call on this path: a wave that hits it pays ~40 instructions, about one substep.
__device__ __forceinline__ bool rare_lane(float& thi, float& wi, float& xi, float& vi, float& ci, float& si, bool have_cs,
                                          float c0, float s0, float d0, float t, float THL, float inv_halfL) {
  bool in_range = true;
  if (!have_cs) {
    if (__builtin_fabsf(d0) <= ROT_LIMIT) {
      ci = c0; si = s0;
      rotate_lane(ci, si, d0);
    } else {
      thi = fma_(-rint_(thi * 0.159154943091895336f), TWO_PI_F, thi);
      sincos_pi_half<float>(thi, si, ci);
      in_range = false;
    }
  }
  if (__builtin_fabsf(xi) >= THL) {
    bounce_lane(thi, wi, xi, vi, ci, t, inv_halfL);
    const float dl = wi * t;
    if (__builtin_fabsf(dl) <= ROT_LIMIT) {
      rotate_lane(ci, si, dl);
    } else {
      thi = fma_(-rint_(thi * 0.159154943091895336f), TWO_PI_F, thi);
      sincos_pi_half<float>(thi, si, ci);
      in_range = false;
    }
  }
  return in_range;
}

// The bounce of cartpole_equations.py:341-347 applied to ALL lanes of the wave under a 0/1 mask `m` (packed where F is
// float2): with one wave per SIMD the slowest wave sets a small launch's time, and a rollout that is caught beyond the
// edge bounces on EVERY substep (v flips sign whichever way it points; the oracle shows rollouts with > 100 consecutive
// bounces), so this event has to cost about as much as a substep, not the ~1000 cycles of per-lane divergent code.
// `c1` = cos of the integrated (un-wrapped) angle.  Returns dl = m * w_new * t, the extra angle a bounced lane advances by.
template <class F>
__device__ __forceinline__ F bounce_masked(F m, F c1, F& th1, F& w1, F& x1, F& v1, float t, float inv_halfL) {
  w1 = fma_(-(v1 * c1), m * splat<F>(2.0f * inv_halfL), w1);
  const F mt = m * splat<F>(t);
  th1 = fma_(mt, w1, th1);
  v1 = v1 * fma_(m, splat<F>(-2.0f), splat<F>(1.0f));
  x1 = fma_(mt, v1, x1);
  return mt * w1;
}

template <class F>
__device__ __forceinline__ void rotate_pair(F& c, F& s, F cd, F sd) {
  const F cn = fma_(c, cd, -(s * sd));
  s = fma_(s, cd, c * sd);
  c = cn;
}

// One Euler substep, FAST, with the reference's per-substep wrap and sin/cos evaluation (the control step's LAST
// substep of the rotating flavours, every substep of the plain one).
// `nearlim` <= THL (wave-uniform): the ONE pair of compares of the common path tests |x| against it instead of THL, and
// the return value says whether any lane of the wave ends the substep at or beyond it - the next stage's boundary cost
// (nonzero only for |x| > permissible_track_fraction * THL = nearlim) is evaluated only then.  The edge itself is tested
// behind that branch, so the common path costs what it did with the plain edge test.
// NEAR = false: `nearlim` is not used, the common path tests the edge itself (the latency build).
// INLINE_EVENTS: the bounce arithmetic is evaluated on every call under its mask instead of behind the wave-uniform branch
// (the eventful loop of the phased build: a wave that is there bounces on nearly every control step, and behind the branch
// the block costs ~500 cycles against ~150 inline).
template <class F, bool NEAR = true, bool INLINE_EVENTS = false>
__device__ __forceinline__ bool substep_fast(State<F>& st, F uK, float t, const Params& p, const EnvConst& e, float nearlim,
                                             bool check = true, bool* at_edge = nullptr) {
  constexpr int W = Width<F>::value;
  F th1, w1, x1, v1;
  ode_euler_fast<F>(st, uK, t, p, e, th1, w1, x1, v1);
  uint64_t near = 0, rare = 0;
  if constexpr (NEAR) {
    if (check) {
#pragma unroll
      for (int i = 0; i < W; ++i) near |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(x1, i)), nearlim, 11);   // 11 = unordered or >=
    }
    if (__builtin_expect(near != 0, 0)) {
#pragma unroll
      for (int i = 0; i < W; ++i) rare |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(x1, i)), p.THL, 3);
    }
  } else if (check) {
#pragma unroll
    for (int i = 0; i < W; ++i) rare |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(x1, i)), p.THL, 3);
    near = ~0ull;
  }
  if (at_edge) *at_edge = rare != 0;
  if (INLINE_EVENTS || __builtin_expect(rare != 0, 0)) {     // wave-uniform: no exec bookkeeping when cold
    CPMPPI_DBG(3, 1);
    // cos of the integrated angle by rotating the previous pair through d = w t; lanes beyond the rotation range (deep)
    const F d = st.w * splat<F>(t);
    F m;
    bool deep = false;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const bool hit = __builtin_fabsf(get(x1, i)) >= p.THL, far = __builtin_fabsf(get(d, i)) > ROT_LIMIT;
      put(m, i, (hit && !far) ? 1.0f : 0.0f);
      deep |= hit && far;
    }
    const F th0 = th1, w0 = w1, x0 = x1, v0 = v1;
    F cd, sd;
    rot_pair<F>(d, cd, sd);
    const F cb = fma_(st.c, cd, -(st.s * sd));
    bounce_masked<F>(m, cb, th1, w1, x1, v1, t, e.inv_halfL);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(deep) != 0, 0)) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        if (__builtin_fabsf(get(x0, i)) >= p.THL && __builtin_fabsf(get(d, i)) > ROT_LIMIT) {
          float thi = get(th0, i), wi = get(w0, i), xi = get(x0, i), vi = get(v0, i), ci, si;
          rare_lane(thi, wi, xi, vi, ci, si, false, get(st.c, i), get(st.s, i), get(d, i), t, p.THL, e.inv_halfL);
          put(th1, i, thi); put(w1, i, wi); put(x1, i, xi); put(v1, i, vi);
        }
      }
    }
  }
  th1 = wrap_rint<F>(th1);
  st.th = th1; st.w = w1; st.x = x1; st.v = v1;
  sincos_pi_half<F>(th1, st.s, st.c);
  return near != 0;
}

// Intermediate substep, FAST + ROTATE: the angle is left un-wrapped and (cos, sin) are advanced by the rotation
// through d = w*t, the exact increment of the angle, with sin d, cos d from their Taylor polynomials (|d| <= 0.125:
// truncation < 1e-9).  Rounding adds ~1 ulp per rotation; the control step's LAST substep re-synchronises with the full
// wrap + sincos (substep_fast), so the states observed at control-step granularity carry at most S-1 rotations of drift
// (~2e-7).  Lanes that bounce, or spin faster than 0.125 rad per substep, are re-evaluated in the cold branch
// (rare_lane: a higher-degree rotation up to 0.25 rad per substep, the exact wrap + sincos beyond).
// EVENTS: true = rare events behind a wave-uniform branch, false = none handled — only the wave mask of lanes that WOULD
// need it is returned (tools/dev/lone_wave.hip: the substep's own cost).
template <class F, bool EVENTS = true>
__device__ __forceinline__ uint64_t substep_fast_rot(State<F>& st, F uK, float t, const Params& p, const EnvConst& e) {
  constexpr int W = Width<F>::value;
  F th1, w1, x1, v1;
  const F d = st.w * splat<F>(t);
  ode_euler_fast<F>(st, uK, t, p, e, th1, w1, x1, v1);
  F cd, sd;
  rot_pair_lo<F>(d, cd, sd);
  F c1 = fma_(st.c, cd, -(st.s * sd));
  F s1 = fma_(st.s, cd, st.c * sd);
  uint64_t fired = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    fired |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(x1, i)), p.THL, 3);                        // 3 = ordered >=
    fired |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(d, i)), ROT_LIMIT_LO, 2);                  // 2 = ordered >
  }
  if (EVENTS && __builtin_expect(fired != 0, 0)) {
    CPMPPI_DBG(4, 1);
    // plain bounces of lanes inside the rotation range: masked, all lanes at once; everything else per lane (deep)
    F m;
    bool deep = false;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const bool hit = __builtin_fabsf(get(x1, i)) >= p.THL;
      const bool spin = __builtin_fabsf(get(d, i)) > ROT_LIMIT_LO;
      put(m, i, (hit && !spin) ? 1.0f : 0.0f);
      deep |= spin;
    }
    const F th0 = th1, w0 = w1, x0 = x1, v0 = v1, c0 = c1, s0 = s1;
    const F dl = bounce_masked<F>(m, c1, th1, w1, x1, v1, t, e.inv_halfL);
    F cdn, sdn;
    rot_pair<F>(dl, cdn, sdn);
    rotate_pair<F>(c1, s1, cdn, sdn);
#pragma unroll
    for (int i = 0; i < W; ++i) deep |= __builtin_fabsf(get(dl, i)) > ROT_LIMIT;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(deep) != 0, 0)) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const bool spin = __builtin_fabsf(get(d, i)) > ROT_LIMIT_LO;
        if (spin || __builtin_fabsf(get(dl, i)) > ROT_LIMIT) {
          float thi = get(th0, i), wi = get(w0, i), xi = get(x0, i), vi = get(v0, i), ci = get(c0, i), si = get(s0, i);
          rare_lane(thi, wi, xi, vi, ci, si, !spin, get(st.c, i), get(st.s, i), get(d, i), t, p.THL, e.inv_halfL);
          put(s1, i, si); put(c1, i, ci);
          put(th1, i, thi); put(w1, i, wi); put(x1, i, xi); put(v1, i, vi);
        }
      }
    }
  }
  st.th = th1; st.w = w1; st.x = x1; st.v = v1; st.c = c1; st.s = s1;
  return fired;
}

// Intermediate substep of the packed path with the rotation's (cos d, sin d) carried along: d = w t changes by
// eps = angleDD t^2 (up to ~1e-3 for a fast-spinning pole) per substep, so
//     (cd, sd) <- (cd - eps sd - eps^2/2, sd + eps cd)
// replaces the two Taylor polynomials (4 instead of 7 instructions; truncation O(eps^3) in cd, eps^2 sd / 2 in sd:
// <= 2e-7 at the range limit |sd| = 0.25, <= 1e-8 for ordinary angular velocities).  The pair is seeded from the
// degree-5/4 polynomials (rot_pair_lo) at every control step, and the control step's last substep re-synchronises (cos, sin) exactly
// as before.  Rare lanes are handled PER LANE in the wave-uniform cold branch (rare_lane) — a lane that hits the track
// edge bounces with the cosine it already carries, is rotated on by its new angular velocity and re-seeds its pair; a
// lane whose |w t| exceeded ROT_LIMIT at the start of the control step or after a bounce (`beyond`: its edge limit
// `xlim` is set to -1, so the one comparison per lane covers both events) gets the exact sincos on every substep — so a
// rollout's arithmetic never depends on what its wave partners do, and a wave that meets a rare lane pays about one
// extra substep for it (no libm call anywhere on the FAST path: with ONE wave per SIMD the slowest wave sets the
// kernel's time, and the first version's libm cosf + exact sincos per event made launches of the C3 / C4 size take
// between 80 and 180 us depending on the noise drawn).  The one-rollout-per-lane path keeps the per-substep
// polynomials: it is bound by the LATENCY of a single wave's dependency chain, and carrying the pair makes the next
// rotation wait for this substep's angleDD (measured: 79 us instead of 67 us per single-env step).
// BOUNCY = false: the event block sits behind a wave-uniform branch (cold).  BOUNCY = true: the same arithmetic inline,
// evaluated every substep under its mask — the loop a wave switches to for the rest of a control step once one of its
// lanes has bounced: a rollout caught beyond the edge bounces on EVERY substep, and behind the branch each of those
// costs ~500 cycles (exec-mask and SGPR shuffling around 45 instructions) against ~300 for the whole substep; inline
// and scheduled with the rest it costs ~100.  Returns whether an event occurred (wave-uniform).
// `check` (wave-uniform): false = the two compares and everything behind them are skipped with one scalar branch (no caller
// passes false at present: proving a control step clear of the edge beforehand was measured slower).
template <class F, bool BOUNCY, bool MASK_ONLY = false>
__device__ __forceinline__ uint64_t substep_fast_rot_carried(State<F>& st, F uK, float t, const Params& p, const EnvConst& e,
                                                             F& cd, F& sd, F& xlim, bool check = true, float* xmax = nullptr) {
  constexpr int W = Width<F>::value;
  F th1, w1, x1, v1, aDD;
  ode_euler_fast<F>(st, uK, t, p, e, th1, w1, x1, v1, &aDD);
  F c1 = fma_(st.c, cd, -(st.s * sd));
  F s1 = fma_(st.s, cd, st.c * sd);
  const F eps = aDD * splat<F>(t * t);
  F cd1 = fma_(-eps, fma_(eps, splat<F>(0.5f), sd), cd);            // cd - eps sd - eps^2/2  (cd ~ 1: the eps^2 term matters)
  F sd1 = fma_(cd, eps, sd);                                         // sd + eps cd
  uint64_t fired = 0;                                               // wave mask (a scalar register pair; the loops' exit tests read it)
  if (xmax != nullptr) {
    // (MASK_ONLY callers that test once per control step: the lane's largest |x| so far, one v_max3 instead of two compares)
    if constexpr (W == 2) *xmax = max3_abs2_(*xmax, get(x1, 0), get(x1, 1));
  } else if (check) {
#pragma unroll
    for (int i = 0; i < W; ++i)                                     // edge, or a lane flagged `beyond`  (3 = ordered >=)
      fired |= __builtin_amdgcn_fcmpf(__builtin_fabsf(get(x1, i)), get(xlim, i), 3);
  }
  if (!MASK_ONLY && (BOUNCY || __builtin_expect(fired != 0, 0))) {
    if (!BOUNCY) CPMPPI_DBG(0, 1);
    // plain bounces (lanes inside the rotation range): masked, both rollouts of all lanes at once — about one substep's
    // worth of packed instructions; lanes flagged `beyond`, or thrown beyond the range by this bounce, per lane (deep)
    F m;
    bool deep = false;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const bool hit = __builtin_fabsf(get(x1, i)) >= p.THL, beyond = get(xlim, i) < 0.0f;
      put(m, i, (hit && !beyond) ? 1.0f : 0.0f);
      deep |= beyond;
    }
    const F th0 = th1, w0 = w1, x0 = x1, v0 = v1, c0 = c1, s0 = s1;
    const F dl = bounce_masked<F>(m, c1, th1, w1, x1, v1, t, e.inv_halfL);
    F cdn, sdn;
    rot_pair<F>(dl, cdn, sdn);                       // lanes that did not bounce: dl = 0, the identity
    rotate_pair<F>(c1, s1, cdn, sdn);
#pragma unroll
    for (int i = 0; i < W; ++i) {
      if (get(m, i) != 0.0f) { put(cd1, i, get(cdn, i)); put(sd1, i, get(sdn, i)); }   // the pair of the new angular velocity
      deep |= __builtin_fabsf(get(dl, i)) > ROT_LIMIT;
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(deep) != 0, 0)) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const bool beyond = get(xlim, i) < 0.0f;
        if (beyond || __builtin_fabsf(get(dl, i)) > ROT_LIMIT) {
          float thi = get(th0, i), wi = get(w0, i), xi = get(x0, i), vi = get(v0, i), ci = get(c0, i), si = get(s0, i);
          rare_lane(thi, wi, xi, vi, ci, si, !beyond, get(st.c, i), get(st.s, i), ROT_LIMIT + 1.0f, t, p.THL, e.inv_halfL);
          put(s1, i, si); put(c1, i, ci);
          put(th1, i, thi); put(w1, i, wi); put(x1, i, xi); put(v1, i, vi);
          put(xlim, i, -1.0f);                        // exact on every substep until the next control step re-tests
        }
      }
    }
  }
  cd = cd1; sd = sd1;
  st.th = th1; st.w = w1; st.x = x1; st.v = v1; st.c = c1; st.s = s1;
  return fired;
}

// One control step of S substeps under a held control (FAST).
// Returns whether any lane of the wave ends the step with |x| >= nearlim (wave-uniform; always true where it is
// not tracked): the caller's next stage evaluates the boundary cost only then.
// SPIN_BRANCH (packed mapping, launches with several waves per SIMD): the once-per-control-step test "does a lane spin beyond
// the rotation range?" is ONE v_max of the lane's two |w| and one compare behind which a practically never taken wave-uniform
// branch flags the lanes, instead of a compare + select per rollout (two vector instructions per control step fewer).  Not for
// launches of one wave per SIMD: there the compare -> scalar-branch hand-over sits on the lone wave's critical path.
// ROLLBACK (packed builds, the reference's intermediate_steps = 10): the nine intermediate substeps run WITHOUT an event test of
// their own - each folds its two |x| into the lane's running maximum with one v_max3 instead of two compares, an s_or and a branch
// - as three straight-line triples, each on a fresh copy of the state (SSA renaming: no register moves), and ONE compare after
// substeps 3, 6 and 9 decides: no rollout of the wave reached the edge -> the copy is the state (the common case: 9 x 27 + 3
// vector instructions instead of 9 x 29); otherwise the triple is discarded and the loop with the per-substep test and the event
// arithmetic integrates from that triple's entry state to the end of the control step.  A rollout's arithmetic is the same on
// both routes (bit-identical results against the form with an edge test per substep; removed, see history).  Measured first with one test per control step: an event then wastes
// the whole step and SQ_INSTS_VALU did not move (profiles/HISTORY.md).
// `at_edge` (in/out; required with SPIN_BRANCH): a wave one of whose rollouts ENDED the previous control step at or beyond the edge
// does not speculate - a rollout caught there bounces on every substep, for tens of control steps (see bounce_masked).
template <class F, bool QUIET_UNROLL = false, bool SPIN_BRANCH = false, bool ROLLBACK = false>
__device__ __forceinline__ bool control_step_fast(State<F>& st, F uK, uint32_t S, float t, const Params& p,
                                                  const EnvConst& e, float nearlim, unsigned* sec = nullptr,
                                                  bool* at_edge = nullptr) {
  // `at_edge` (out, wave-uniform; the phased mid-size build passes it): does a rollout of this wave END the control step
  // at or beyond the track edge, or spin beyond the rotation range?  It bounces on the very next substep - and, caught
  // beyond the edge, on every one after it (cartpole_equations.py:341-347 flips v whichever way it points) - so the caller
  // integrates the next control step with the event arithmetic inline (control_step_fast_eventful).
  if constexpr (Width<F>::value == 1) {
    // one rollout per lane is the small-launch (latency-bound) mapping: there the per-substep test, which overlaps with
    // the arithmetic, is faster than the shorter loop with its test at the head (single env: 70 us vs 80 us)
    // (three substeps per loop iteration without event handling, under a rollback, as in the packed mid-size build, was
    // measured here twice: with three compare pairs or-ed (round 2: single env 63 -> 72 us) and with ONE test on v_max3 of
    // the positions and of the rotation angles (round 3: 56.6 -> 58.3 us; with section stamps: 1730 -> 1850 cycles for the
    // nine intermediate substeps) - this mapping gains nothing from it.  Nor from instruction order: the substep written
    // as ONE asm block with the links of the loop-carried chain spaced apart (tools/dev/lone_wave.hip, bit-identical) runs
    // at 61 ns against the compiler's 64 - a lone wave issues these three-operand instructions at ~4.5 cycles each
    // whatever their order, so only fewer instructions would help)
    if (sec) CPMPPI_SEC(sec, 2, st);
    if (S == 10u) {
      // the reference's intermediate_steps = 10 as straight-line code: a wave that has its SIMD to itself pays ~50 cycles
      // for every TAKEN branch (the instruction buffer refills from the cache; how many depends on where the target
      // falls, which is why this build's times moved by 10-25 % with unrelated changes of code layout), and the substep
      // loop's back edge is one per 190-cycle substep.  Unrolled, the nine substeps fall through their untaken event
      // branches: single env 56.3 -> 50.0 us, 256 x 20 27.9 -> 25.4 us, 3500 x 35 44.7 -> 39.1 us, 64 envs 62 -> 56 us.
      // (In this straight-line form too, one test per three substeps - rollback as in the mid-size build - is slower:
      // 49.9 -> 51.2 us.  The untaken event branch costs less than the rollback's copies.  Round 4 repeated it in the copy-free
      // form the packed builds now use - fresh State per triple, two running maxima instead of the two compares, one compare pair
      // and branch per triple: 48.9 -> 51.8 us, 256 x 20 24.7 -> 25.9, 64 envs 52.6 -> 56.5.  Not for one rollout per lane.)
#pragma unroll
      for (int sub = 0; sub < 9; ++sub) substep_fast_rot<F>(st, uK, t, p, e);
    } else {
      for (uint32_t sub = 0; sub + 1 < S; ++sub) substep_fast_rot<F>(st, uK, t, p, e);
    }
    if (sec) CPMPPI_SEC(sec, 3, st);
    const bool near_one = substep_fast<F, false>(st, uK, t, p, e, nearlim);     // (the edge itself: no coarser "near" limit)
    if (sec) CPMPPI_SEC(sec, 4, st);
    return near_one;
  }
  // The seed needs |w t| <= ROT_LIMIT_LO.  Tested once per control step: without a bounce w cannot leave the range within
  // one control step by more than the polynomials' margin, and a lane that bounces is re-tested.  Lanes beyond the
  // range are flagged and take the exact sincos on every substep.
  F xlim = splat<F>(p.THL);
  float xmax = 0.0f;                            // ROLLBACK: the lane's largest |x| over the substeps not yet tested
  const float wlim = e.wlim;                    // = ROT_LIMIT_LO / t: |w t| > the seed's range as one compare with a free abs modifier per lane
  uint64_t spinning = 0;      // wave mask of lanes beyond the rotation range: the same compare as the select's (one v_cmp)
  if constexpr (SPIN_BRANCH && Width<F>::value == 2) {
    const float wmax = max_abs2_(get(st.w, 0), get(st.w, 1));
    spinning = __builtin_amdgcn_fcmpf(wmax, wlim, 2);              // 2 = ordered >  (a NaN counts as within, as in the select form)
    // (ROLLBACK: the lanes are flagged BEHIND the triples - only the loop with the per-substep test reads xlim, and a wave with a
    // spinning lane never enters the triples, so st.w there is still the entry value: the common path no longer carries the
    // v_mov_b64 that formed xlim ahead of the branch)
    if (!ROLLBACK && __builtin_expect(spinning != 0, 0)) {
#pragma unroll
      for (int i = 0; i < Width<F>::value; ++i) put(xlim, i, !(__builtin_fabsf(get(st.w, i)) > wlim) ? p.THL : -1.0f);
    }
  } else {
#pragma unroll
    for (int i = 0; i < Width<F>::value; ++i) {
      const bool within = !(__builtin_fabsf(get(st.w, i)) > wlim);
      put(xlim, i, within ? p.THL : -1.0f);
      // (the select's own compare, in the sense the compiler emits it - v_cmp_ngt - so that no second compare is needed)
      if (at_edge != nullptr) spinning |= ~__builtin_amdgcn_ballot_w64(within) & __builtin_amdgcn_ballot_w64(true);
      if constexpr (ROLLBACK) xmax = within ? xmax : INFINITY;     // (no branch on the spin test here: such a lane fails the first edge test)
    }
  }
  F cd, sd;
  rot_pair_lo<F>(st.w * splat<F>(t), cd, sd);
  uint32_t left = S - 1u;                         // intermediate substeps the loop below still has to integrate
  if constexpr (ROLLBACK && Width<F>::value == 2) {
    // three tests per control step (after substeps 3, 6, 9; the reference's intermediate_steps = 10 only): an event discards at
    // most one triple, and the loop below takes over from that triple's entry state
    // (the phased mid-size build's quiet loop - no SPIN_BRANCH - enters with *at_edge false; a lane beyond the rotation range
    // carries xmax = inf into the first test)
    if (__builtin_expect(S == 10u && (!SPIN_BRANCH || (spinning == 0 && !*at_edge)), 1)) {
      State<F> a = st;
      F cda = cd, sda = sd;
#pragma unroll
      for (int sub = 0; sub < 3; ++sub) substep_fast_rot_carried<F, false, true>(a, uK, t, p, e, cda, sda, xlim, true, &xmax);
      if (__builtin_expect(__builtin_amdgcn_fcmpf(xmax, p.THL, 3) == 0, 1)) {         // 3 = ordered >=
        State<F> b = a;
        F cdb = cda, sdb = sda;
#pragma unroll
        for (int sub = 0; sub < 3; ++sub) substep_fast_rot_carried<F, false, true>(b, uK, t, p, e, cdb, sdb, xlim, true, &xmax);
        if (__builtin_expect(__builtin_amdgcn_fcmpf(xmax, p.THL, 3) == 0, 1)) {
          State<F> c = b;
          F cdc = cdb, sdc = sdb;
#pragma unroll
          for (int sub = 0; sub < 3; ++sub) substep_fast_rot_carried<F, false, true>(c, uK, t, p, e, cdc, sdc, xlim, true, &xmax);
          if (__builtin_expect(__builtin_amdgcn_fcmpf(xmax, p.THL, 3) == 0, 1)) {
            st = c;
            return substep_fast<F>(st, uK, t, p, e, nearlim, true, at_edge);
          }
          st = b; cd = cdb; sd = sdb; left = 3u;
        } else {
          st = a; cd = cda; sd = sda; left = 6u;
        }
      }
      asm volatile("; rollback: a rollout of this wave reached the track edge within the last three substeps");
    }
    if constexpr (SPIN_BRANCH) {
      if (__builtin_expect(spinning != 0, 0)) {
#pragma unroll
        for (int i = 0; i < Width<F>::value; ++i) put(xlim, i, !(__builtin_fabsf(get(st.w, i)) > wlim) ? p.THL : -1.0f);
      }
    }
  }
  // (Rounds 2 and 3 ran the packed mid-size build on three substeps at a time without event handling, under a rollback -
  // one v_max3 test per triple, the discarded triple redone substep by substep with the event arithmetic inline - until
  // section stamps showed that build's median wave 17 % slower per control step than this plain loop, in every section:
  // DESIGN.md §4.  The phased horizon loop replaced it; the code is in the history.)
  if (sec) { asm volatile("" : "+v"(cd), "+v"(sd), "+v"(xlim)); CPMPPI_SEC(sec, 2, st); }
  if (QUIET_UNROLL && !ROLLBACK && S == 10u) {
    // the quiet control step of the phased mid-size build in a launch of one wave per SIMD, the reference's
    // intermediate_steps = 10: the nine substeps as straight-line code - a lone wave pays ~50 cycles per taken branch
    // (see the one-rollout-per-lane mapping above), and the loop's back edge is one per substep
#pragma unroll
    for (int sub = 0; sub < 9; ++sub) substep_fast_rot_carried<F, false>(st, uK, t, p, e, cd, sd, xlim);
  } else if (QUIET_UNROLL && ROLLBACK && S == 10u) {
    // (the lone-wave build after a discarded triple: 9, 6 or 3 substeps left, whole triples as straight-line code)
    for (; left != 0u; left -= 3u) {
#pragma unroll
      for (int sub = 0; sub < 3; ++sub) substep_fast_rot_carried<F, false>(st, uK, t, p, e, cd, sd, xlim);
    }
  } else {
    for (; left != 0u; --left) substep_fast_rot_carried<F, false>(st, uK, t, p, e, cd, sd, xlim);
  }
  if (sec) CPMPPI_SEC(sec, 3, st);
  const bool near_end = substep_fast<F>(st, uK, t, p, e, nearlim, true, at_edge);
  // phased horizon loop: a wave with a lane beyond the rotation range (it takes the event path on every substep, ~500
  // cycles each behind the branch) goes to the loop with the event arithmetic inline like one with a rollout at the edge
  if (at_edge != nullptr) *at_edge = *at_edge || spinning != 0;
  if (sec) CPMPPI_SEC(sec, 4, st);
  return near_end;
}
// A control step of a wave one of whose rollouts ENDED the previous step at or beyond the track edge (`at_edge`): the
// event arithmetic inline on every intermediate substep, no test, no speculation (see control_step_fast).  Used by the
// phased horizon loop (cpmppi_rollout_kernel.inc), which keeps this code out of the loop the quiet control steps run in.
template <class F, bool UNROLL = false>
__device__ __forceinline__ bool control_step_fast_eventful(State<F>& st, F uK, uint32_t S, float t, const Params& p,
                                                           const EnvConst& e, float nearlim, bool* at_edge) {
  F xlim = splat<F>(p.THL);
  const float wlim = e.wlim;
  uint64_t spinning = 0;
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i) {
    const bool within = !(__builtin_fabsf(get(st.w, i)) > wlim);
    put(xlim, i, within ? p.THL : -1.0f);
    spinning |= ~__builtin_amdgcn_ballot_w64(within) & __builtin_amdgcn_ballot_w64(true);
  }
  F cd, sd;
  rot_pair_lo<F>(st.w * splat<F>(t), cd, sd);
  if (UNROLL && S == 10u) {                      // (launches of one wave per SIMD: no taken branch between the substeps)
#pragma unroll
    for (int sub = 0; sub < 9; ++sub) substep_fast_rot_carried<F, true>(st, uK, t, p, e, cd, sd, xlim);
  } else {
    uint32_t left = S - 1u;
    while (left >= 3u) {
      substep_fast_rot_carried<F, true>(st, uK, t, p, e, cd, sd, xlim);
      substep_fast_rot_carried<F, true>(st, uK, t, p, e, cd, sd, xlim);
      substep_fast_rot_carried<F, true>(st, uK, t, p, e, cd, sd, xlim);
      left -= 3u;
    }
    for (; left != 0u; --left) substep_fast_rot_carried<F, true>(st, uK, t, p, e, cd, sd, xlim);
  }
  const bool near_end = substep_fast<F, true, true>(st, uK, t, p, e, nearlim, true, at_edge);
  *at_edge = *at_edge || spinning != 0;          // (stays in this loop while the pole keeps spinning)
  return near_end;
}

// ------------------------------------------------------------------------------------------------------------------
// The OTHER in-tree ODE predictor: predictor_type "ODE" (SI_Toolkit_ASF/config_predictors.yml:22-26 - what the shipped
// config_controllers.yml:3,14 name as the mpc controllers' predictor_specification).  next_state_predictor_ODE
// (SI_Toolkit_ASF/ToolkitCustomization/predictors_customization.py:25-69) -> CartPoleEquations.cartpole_fine_integration
// (CartPole/cartpole_equations.py:181-259): per substep the same _cartpole_ode (:232), then EULER-CROMER (:293-304:
// velocities first, angle and position advance by the NEW velocities), NO edge bounce (:241-243 is commented out in the
// reference), cos / sin of the integrated angle (:245-246) and angle = atan2(sin, cos) (:248, 307-308).

// PRECISE: the reference's operand grouping with IEEE divides, libm cos / sin, no FMA contraction.  The angle this predictor
// re-derives on every substep, atan2(sin, cos), is evaluated in double and rounded once: the device's atan2f is a ~2 ulp
// function, and that noise - re-entering the state 500 times per rollout - moved a few rollouts of a full-width C4 launch
// (|w| = 11 rad/s) 2e-4 from the oracle where the oracle's own float32 realisations scatter by 2e-5; FAST, which never goes
// through atan2, was inside the band all along.
__device__ __forceinline__ void substep_precise_cromer(State<float>& st, float u, float t, const Params& p,
                                                       const EnvConst& e) {
#pragma clang fp contract(off)
  float aDD, xDD;
  ode_precise(st.c, st.s, st.w, st.v, u, p, e, aDD, xDD);
  const float w1 = st.w + aDD * t;
  const float v1 = st.v + xDD * t;
  const float th1 = st.th + w1 * t;
  const float x1 = st.x + v1 * t;
  const float c1 = cosf(th1), s1 = sinf(th1);
  st.th = (float)atan2((double)s1, (double)c1);
  st.w = w1; st.c = c1; st.s = s1; st.x = x1; st.v = v1;
}

// FAST: _cartpole_ode with the folded constants of ode_euler_fast (same formulas, same instruction sequence) followed by
// the Euler-Cromer update.  Outputs the un-wrapped new state and angleDD.
template <class F>
__device__ __forceinline__ void ode_cromer_fast(const State<F>& st, F uK, float t, const Params& p, const EnvConst& e,
                                                F& th1, F& w1, F& x1, F& v1, F& aDD) {
  const F c = st.c, s = st.s, w = st.w, v = st.v;
  const F A = fma_(-(c * splat<F>(p.m_pole)), c, splat<F>(e.kp1_mt));
  const F t1 = fma_(splat<F>(e.mg), s, -(w * splat<F>(e.JinvLh)));
  F num = fma_(c, t1, uK);
  num = fma_(-((w * w) * splat<F>(e.kmLh)), s, num);
  num = fma_(splat<F>(-e.kM), v, num);
  const F xDD = num * rcp_(A);
  aDD = fma_(xDD * c, splat<F>(e.inv_kLh), t1 * splat<F>(e.t1_i));
  const F tt = splat<F>(t);
  w1 = fma_(aDD, tt, w);
  v1 = fma_(xDD, tt, v);
  th1 = fma_(w1, tt, st.th);
  x1 = fma_(v1, tt, st.x);
}

// One control step of S Euler-Cromer substeps under a held control (FAST).  As in control_step_fast the angle is left
// un-wrapped inside the control step and (cos, sin) advance by ROTATION: a substep moves the angle by d' = w' t with the
// NEW angular velocity w' = w + angleDD t, i.e. by the previous substep's rotation angle plus eps = angleDD t^2, so the
// carried pair (cos d, sin d) - seeded from the degree-7/6 polynomials of d = w t once per control step - is advanced by
// eps FIRST and (cos, sin) are then rotated by it (substep_fast_rot_carried rotates first: simultaneous Euler moves the
// angle by the OLD velocity).  The control step's last substep re-synchronises with the exact wrap + polynomial sincos;
// theta - 2 pi rint(theta / 2 pi) is the value atan2(sin, cos) returns up to rounding (both in [-pi, pi]).  No edge
// test anywhere: this predictor does not bounce.  The carried pair is second order in eps: its truncation, eps^2 |sin d| / 2
// per substep, stays below 1e-7 while |d| = |w t| <= ~0.1 (the centrifugal term makes eps ~ 0.11 d^2 at worst: 0.006 d^5);
// a lane that starts a control step beyond CROMER_CARRY_LIMIT (45 rad/s at t = 2 ms - a pole released from rest tops out
// near 20) takes the exact wrap + sincos on every substep instead - per lane, so a rollout's arithmetic does not depend on
// its wave partners; the branch is wave-uniform and practically never taken.  (Found by the reference-generated "fastspin"
// fixture, 150 rad/s decaying through 100: with the limit at the polynomials' 0.25 every rollout left the band.)
constexpr float CROMER_CARRY_LIMIT = 0.09f;
template <class F, bool UNROLL = false>
__device__ __forceinline__ void control_step_cromer_fast(State<F>& st, F uK, uint32_t S, float t, const Params& p,
                                                         const EnvConst& e) {
  constexpr int W = Width<F>::value;
  const float wlim = CROMER_CARRY_LIMIT / t;
  bool beyond[W];
  bool any = false;
#pragma unroll
  for (int i = 0; i < W; ++i) { beyond[i] = __builtin_fabsf(get(st.w, i)) > wlim; any |= beyond[i]; }
  const bool any_beyond = __builtin_amdgcn_ballot_w64(any) != 0;
  F cd, sd;
  rot_pair<F>(st.w * splat<F>(t), cd, sd);
  const F tt2 = splat<F>(t * t);
  auto substep = [&]() __attribute__((always_inline)) {
    F th1, w1, x1, v1, aDD;
    ode_cromer_fast<F>(st, uK, t, p, e, th1, w1, x1, v1, aDD);
    const F eps = aDD * tt2;
    const F cd1 = fma_(-eps, fma_(eps, splat<F>(0.5f), sd), cd);     // cd - eps sd - eps^2/2
    const F sd1 = fma_(cd, eps, sd);                                  // sd + eps cd
    F c1 = fma_(st.c, cd1, -(st.s * sd1));
    F s1 = fma_(st.s, cd1, st.c * sd1);
    if (__builtin_expect(any_beyond, 0)) {
      const F thw = wrap_rint<F>(th1);
      F se, ce;
      sincos_pi_half<F>(thw, se, ce);
#pragma unroll
      for (int i = 0; i < W; ++i)
        if (beyond[i]) { put(th1, i, get(thw, i)); put(c1, i, get(ce, i)); put(s1, i, get(se, i)); }
    }
    cd = cd1; sd = sd1;
    st.th = th1; st.w = w1; st.x = x1; st.v = v1; st.c = c1; st.s = s1;
  };
  if (UNROLL && S == 10u) {                     // (a lone wave pays ~50 cycles per taken branch: control_step_fast)
#pragma unroll
    for (int sub = 0; sub < 9; ++sub) substep();
  } else {
    for (uint32_t sub = 0; sub + 1 < S; ++sub) substep();
  }
  F th1, w1, x1, v1, aDD;
  ode_cromer_fast<F>(st, uK, t, p, e, th1, w1, x1, v1, aDD);
  th1 = wrap_rint<F>(th1);
  st.th = th1; st.w = w1; st.x = x1; st.v = v1;
  sincos_pi_half<F>(th1, st.s, st.c);
}

}  // namespace cpmppi
