// cpmppi_cost.hpp — the four stage costs, the MPPI correction term, and the per-env folds of their wave-uniform factors
// (QbgmFolded, EnvFold).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cpmppi_params.hpp"

namespace cpmppi {

// ------------------------------------------------------------------------------------------------------------------
// Stage / terminal costs (generic over float / float2).  `x_t` target position, `te` target equilibrium, `u` the
// control applied at this stage.
// quadratic_boundary_grad_minimal.py:64-126; w = {dd, db, ep, ekp, cc, R, permissible_track_fraction}
// x / c for a wave-uniform c: the IEEE divide (PRECISE) or a multiply by the float32-rounded reciprocal (FAST; differs
// from the divide by <= 1 ulp).
template <bool FAST, class F>
__device__ __forceinline__ F div_uniform(F x, float c) {
  if constexpr (FAST) return x * splat<F>(1.0f / c);
  else return x / splat<F>(c);
}

// The wave-uniform factors of quadratic_boundary_grad_minimal's terms, formed once per kernel (or per env) in double.
// (c_dd = w_dd / (2 THL)^2 and c_cc = R w_cc served a FAST form of stage_qbgm that folded three terms - three instructions
// fewer per stage, each term within 2 ulp of the reference's grouping - until stage_qbgm_acc took the rollout kernel's FAST
// path over (removed, see history); the two words stay: they are part of EnvFold's layout, which the throughput kernels' scalar
// loads address - without them fold_env_kernel and three rollout kernels come out with other code and register counts.)
struct QbgmFolded {
  float c_dd, c_cc, neg_te;
  // stage_qbgm_acc (FAST, the rollout kernel): every term's weight with the horizon aggregation's scale (1 for sum, 1/(H+1)
  // for mean) folded in, and the MPPI correction's coefficients (controller_mppi_cartpole.py:261-263: cc_weight (0.5 (1 - 1/NU) R du^2 + R u du + 0.5 R u^2))
  float a_dd, a_ep, a_ekp, a_db, db_lim;   // db: b^2 w_db = (|x| - lim)^2 a_db for |x| > lim = permissible_track_fraction THL
  float a_u2;                              // u_run^2: w_cc R scale, + 0.5 cc_weight R when the correction takes u_run
  float k_a, k_b_run, k_b_nom;             // du (k_a du + k_b_run u_run + k_b_nom u_nom): one of the two k_b is zero
  float k_c_nom;                           // 0.5 cc_weight R when the correction takes u_nom: the (rollout-independent) term u_nom^2
};
// (`_lane`: every lane its own `te` - the per-env fold kernel; the rollout kernel's in-kernel form pins the fields to SGPRs)
__device__ __forceinline__ QbgmFolded make_qbgm_folded_lane(const Params& p, float te) {
  QbgmFolded f;
  const double two_thl = 2.0 * (double)p.THL;
  f.c_dd = (float)((double)p.w[0] / (two_thl * two_thl));
  f.c_cc = (float)((double)p.w[5] * (double)p.w[4]);
  f.neg_te = -te;
  const double scale = (p.horizon_reduce == 0u) ? 1.0 : 1.0 / (double)(p.H + 1u);      // CPMPPI_REDUCE_SUM = 0
  const double ptf = (double)p.w[6], span = (1.0 - ptf) * (double)p.THL;
  f.a_dd = (float)(scale * (double)p.w[0] / (two_thl * two_thl));
  f.a_ep = (float)(scale * (double)p.w[2]);
  f.a_ekp = (float)(scale * (double)p.w[3]);
  f.a_db = (float)(scale * (double)p.w[1] / (span * span));
  f.db_lim = (float)(ptf * (double)p.THL);
  const bool run = p.correction_u == 0u;                                                // CPMPPI_CORRECTION_U_RUN = 0
  const double half_r = (double)p.cc_weight * 0.5 * (double)p.R;
  f.a_u2 = (float)(scale * (double)p.w[5] * (double)p.w[4] + (run ? half_r : 0.0));
  f.k_a = (float)((double)p.cc_weight * 0.5 * (1.0 - 1.0 / (double)p.NU) * (double)p.R);
  f.k_b_run = run ? (float)((double)p.cc_weight * (double)p.R) : 0.0f;
  f.k_b_nom = run ? 0.0f : (float)((double)p.cc_weight * (double)p.R);
  f.k_c_nom = run ? 0.0f : (float)half_r;
  return f;
}
__device__ __forceinline__ QbgmFolded make_qbgm_folded(const Params& p, float te) {
  const QbgmFolded c = make_qbgm_folded_lane(p, te);
  QbgmFolded f;
  f.c_dd = uniform_(c.c_dd); f.c_cc = uniform_(c.c_cc); f.neg_te = uniform_(c.neg_te);
  f.a_dd = uniform_(c.a_dd); f.a_ep = uniform_(c.a_ep); f.a_ekp = uniform_(c.a_ekp); f.a_db = uniform_(c.a_db);
  f.db_lim = uniform_(c.db_lim); f.a_u2 = uniform_(c.a_u2); f.k_a = uniform_(c.k_a); f.k_b_run = uniform_(c.k_b_run);
  f.k_b_nom = uniform_(c.k_b_nom); f.k_c_nom = uniform_(c.k_c_nom);
  return f;
}

// Everything the throughput build's rollout kernel derives from (Params, L[env], target_equilibrium[env], s0[env]) alone, formed
// ONCE per env by fold_env_kernel (cpmppi.hip, the hot-path unit) instead of once per WAVE in the rollout kernel's prologue: ~300 vector instructions
// (double-precision folds, two IEEE divides, libm cosf) per wave of 128 rollouts = 1.5 % of the launch, read back with scalar loads.
// Same device functions, same values.  136 bytes per env.
struct EnvFold {
  EnvConst ec;          // 18 words
  QbgmFolded qf;        // 13 words
  float cos0;           // cosf(s0[0]): the cost plugins take cos(angle), not the stored angle_cos, at stage 0
  float inv_period;     // 1 / period_interpolation_inducing_points (the in-kernel interpolation's slope factor)
  float nearlim;        // min(permissible_track_fraction, 1) * THL: below it quadratic_boundary_grad_minimal's boundary term is zero
};
static_assert(sizeof(EnvFold) == 136, "EnvFold: 34 words per env");

// quadratic_boundary_grad_minimal's stage cost AND the MPPI correction term of one stage added to two running sums (FAST path of
// the rollout kernel).  Same terms as stage_qbgm + mppi_correction; what differs is the grouping: every term is accumulated
// with one FMA (weight folded into the constant) instead of formed, weighted, summed into the stage cost and added to the
// horizon's sum - 13 vector instructions instead of 20 per stage, each term within 2 ulp of the reference's grouping (PRECISE
// keeps that grouping operation for operation).  Two sums (`acc_a`: position and angle terms, `acc_b`: speed, control and
// correction terms) keep the dependent chain of a stage at two FMAs.  `b_nom` = k_b_nom * u_nom of this stage (wave-uniform; zero unless the correction takes
// u_nom); the rollout-independent term k_c_nom u_nom^2 of that mode is added by the caller once per rollout.
// near = false: |x| < permissible_track_fraction * THL for every lane, the boundary term is exactly zero and left out.
template <class F>
__device__ __forceinline__ void stage_qbgm_acc(const QbgmFolded& f, F x, F cosang, F w, F ur, F du, bool nom_mode, float b_nom,
                                               float x_t, bool near, F& acc_a, F& acc_b) {
  const F dx = x - splat<F>(x_t);
  acc_a = fma_(dx * dx, splat<F>(f.a_dd), acc_a);
  const F e1 = fma_(cosang, splat<F>(f.neg_te), splat<F>(1.0f));
  acc_a = fma_(e1 * e1, splat<F>(f.a_ep), acc_a);
  acc_b = fma_(w * w, splat<F>(f.a_ekp), acc_b);
  acc_b = fma_(ur * ur, splat<F>(f.a_u2), acc_b);
  const F lin = fma_(du, splat<F>(f.k_a), ur * splat<F>(f.k_b_run));
  acc_b = fma_(du, lin, acc_b);
  if (__builtin_expect(nom_mode, 0)) {
    asm volatile("; correction term on u_nom");    // (keeps this a branch: the common path carries no operand for it)
    acc_b = fma_(du, splat<F>(b_nom), acc_b);
  }
  if (__builtin_expect(near, 0)) {
    // (the asm statement keeps this a BRANCH: if-converted, the term's eight instructions would run on every stage)
    asm volatile("; quadratic_boundary_grad_minimal: boundary term");
    F over;
#pragma unroll
    for (int i = 0; i < Width<F>::value; ++i) put(over, i, max_abs_(get(x, i), f.db_lim));
    over = over - splat<F>(f.db_lim);
    acc_a = fma_(over * over, splat<F>(f.a_db), acc_a);
  }
}

// near = false: the caller knows |x| < permissible_track_fraction * THL for every lane, i.e. the boundary term is exactly
// zero and dd + 0 == dd: it is left out (wave-uniform branch), bit-identical.
template <class F, bool FAST = false>
__device__ __forceinline__ F stage_qbgm(const Params& p, F x, F cosang, F w_ang, F u, float x_t, float te, bool near = true) {
#pragma clang fp contract(off)     // every product and sum rounds once, wherever the function is inlined
  const float THL = p.THL;
  const F d = div_uniform<FAST, F>(x - splat<F>(x_t), 2.0f * THL);
  const F dd = (d * d) * splat<F>(p.w[0]);
  const F e1 = splat<F>(1.0f) - cosang * splat<F>(te);
  const F ep = (e1 * e1) * splat<F>(p.w[2]);
  const F cc = ((u * u) * splat<F>(p.w[5])) * splat<F>(p.w[4]);
  const F ekp = (w_ang * w_ang) * splat<F>(p.w[3]);
  if (!near) return dd + ep + ekp + cc;
  const float ptf = p.w[6];
  const F ax = abs_(x);
  // indicator(|x| > ptf THL) * b^2 == (max(|x| - ptf THL, 0) / ...)^2: the same value without compare + select
  F over = ax - splat<F>(ptf * THL);
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i) put(over, i, __builtin_fmaxf(get(over, i), 0.0f));
  const F b = div_uniform<FAST, F>(over, (1.0f - ptf) * THL);
  const F db = (b * b) * splat<F>(p.w[1]);
  return dd + db + ep + ekp + cc;
}

// quadratic_boundary_grad.py:64-232; w = {up: ddq, ddl, db, ep, ekp, cc, ccrc | down: the same 7 | tas_corr_up,
// tas_corr_down, permissible_track_fraction, cos(admissible_angle), R}; u_before = the control of the previous stage
// (previous_input at stage 0); terminal cost zero.
template <class F, bool FAST = false>
__device__ __forceinline__ F stage_qbg(const Params& p, F x, F cosang, F w_ang, F u, F u_before, float x_t, float te) {
#pragma clang fp contract(off)     // every product and sum rounds once, wherever the function is inlined
  const bool up = (te == 1.0f);
  const float* w = p.w + (up ? 0 : 7);
  const float corr = up ? p.w[14] : p.w[15];
  const float ptf = p.w[16], cos_adm = p.w[17], R = p.w[18], THL = p.THL;
  const F d = div_uniform<FAST, F>(x - splat<F>(x_t), 2.0f * THL);
  const F dd_quadratic = (d * d) * splat<F>(w[0]);
  const F dd_linear = abs_(d) * splat<F>(w[1]);
  const F ax = abs_(x);
  F over = ax - splat<F>(ptf * THL);
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i) put(over, i, __builtin_fmaxf(get(over, i), 0.0f));
  const F b = div_uniform<FAST, F>(over, (1.0f - ptf) * THL);
  const F db = (b * b) * splat<F>(w[2]);
  const F tc = cosang * splat<F>(te);
  const F e2 = splat<F>(2.0f) - tc;
  const F ep = (e2 * e2 - splat<F>(1.0f)) * splat<F>(w[3]);
  const float tas_max = __builtin_fabsf(120.0f * (1.0f + te) / 2.0f + corr);
  const F basic = (splat<F>(1.0f) - tc) * splat<F>(0.5f);
  F scaling;
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i)
    put(scaling, i, (te * (get(cosang, i) - cos_adm) > 0.0f) ? 0.0f : get(basic, i));
  const F ekp = abs_(w_ang * w_ang - scaling * splat<F>(tas_max)) * splat<F>(w[4]);
  const F cc = ((u * u) * splat<F>(R)) * splat<F>(w[5]);
  const F dc = u - u_before;
  const F ccrc = (dc * dc) * splat<F>(w[6]);
  return dd_linear + dd_quadratic + db + ep + ekp + cc + ccrc;
}

// default.py:23-88; w = {dd, ep, cc, R}.
// The same function serves the plugin's two siblings (p.qb_mode, wave-uniform; w = {dd, ep, cc, R, ccrc}):
//   1  quadratic_boundary.py:26-87 - the track-edge term is 1[|x| > 0.95 THL] 1e9 ((|x| - 0.95 THL) / (0.05 THL))^2 instead of
//      the 1e7 indicator at 0.9 THL, and a control-change-rate term ccrc_weight (u - u_before)^2 joins when the caller hands a
//      previous input over (`with_ccrc`; the reference adds the term only `if previous_input is not None`, :83-85);
//   2  quadratic_boundary_nonconvex.py:27-105 - the same plus the ripple -0.15 (cos(4 2 pi (x - x*) / (2 THL)) - 1) on the
//      position term (restated from the source text: the reference cannot import that module, oracle_np.qb_stage_cost).
// QB = false: compiled without the siblings (the predictor_ODE kernels: the plugins are built for predictor_ODE_v0 only).
template <class F, bool FAST = false, bool QB = true>
__device__ __forceinline__ F stage_default(const Params& p, F x, F cosang, F u, float x_t, float te, F u_before = splat<F>(0.0f),
                                           bool with_ccrc = false) {
#pragma clang fp contract(off)     // every product and sum rounds once, wherever the function is inlined
  const float THL = p.THL;
  const F d = div_uniform<FAST, F>(x - splat<F>(x_t), 2.0f * THL);
  F pos = d * d, edge;
  if (!QB || p.qb_mode == 0u) {
#pragma unroll
    for (int i = 0; i < Width<F>::value; ++i) put(edge, i, (__builtin_fabsf(get(x, i)) > 0.90f * THL) ? 1.0e7f : 0.0f);
  } else {
    const F b = div_uniform<FAST, F>(abs_(x) - splat<F>(0.95f * THL), 0.05f * THL);
    F ind;
#pragma unroll
    for (int i = 0; i < Width<F>::value; ++i) put(ind, i, (__builtin_fabsf(get(x, i)) > 0.95f * THL) ? 1.0e9f : 0.0f);
    edge = ind * (b * b);
    if (p.qb_mode == 2u) {
      const F arg = div_uniform<FAST, F>(splat<F>(25.132741228718345f) * (x - splat<F>(x_t)), 2.0f * THL);
      pos = pos - splat<F>(0.15f) * (cos_(arg) - splat<F>(1.0f));
    }
  }
  const F dd = (pos + edge) * splat<F>(p.w[0]);
  const F e1 = splat<F>(1.0f) - cosang;
  const F ep = ((e1 * e1) * splat<F>(0.25f) * splat<F>(te)) * splat<F>(p.w[1]);
  const F cc = ((u * u) * splat<F>(p.w[3])) * splat<F>(p.w[2]);
  if (QB && with_ccrc) {
    const F dc = u - u_before;
    return dd + ep + cc + (dc * dc) * splat<F>(p.w[4]);
  }
  return dd + ep + cc;
}

// default.py:55-63 and controller_mppi_cartpole.py:278-303 (phi): 10000 * 1[|angle| > 0.2 or |x - x*| > 0.1*THL]
template <class F>
__device__ __forceinline__ F terminal_indicator(const Params& p, F angle, F x, float x_t) {
  F out;
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i) {
    const bool bad = (__builtin_fabsf(get(angle, i)) > 0.2f) || (__builtin_fabsf(get(x, i) - x_t) > 0.1f * p.THL);
    put(out, i, bad ? 10000.0f : 0.0f);
  }
  return out;
}

// MPPI correction term, algebra of controller_mppi_cartpole.py:261-263
template <class F>
__device__ __forceinline__ F mppi_correction(const Params& p, F u, F du) {
  // cc_weight (0.5 (1 - 1/NU) R du^2 + R u du + 0.5 R u^2)  =  du (a du + b u) + c u^2   with the weight folded in
  const float a = p.cc_weight * (0.5f * (1.0f - 1.0f / p.NU) * p.R), b = p.cc_weight * p.R, c = p.cc_weight * (0.5f * p.R);
  return fma_(u * splat<F>(c), u, du * fma_(du, splat<F>(a), u * splat<F>(b)));
}

// controller_mppi_cartpole.py:227-275 (q); w = {dd, ep, ekp, ekc, cc, ccrc}; u = nominal control of the stage
template <class F, bool FAST = false>
__device__ __forceinline__ F stage_legacy(const Params& p, F x, F cosang, F w_ang, F v, float u, F du, float u_prev,
                                          float x_t) {
#pragma clang fp contract(off)     // every product and sum rounds once, wherever the function is inlined
  const float THL = p.THL;
  const F d = div_uniform<FAST, F>(x - splat<F>(x_t), 2.0f * THL);
  F ind;
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i) put(ind, i, (__builtin_fabsf(get(x, i)) > 0.95f * THL) ? 1.0e6f : 0.0f);
  const F dd = (d * d + ind) * splat<F>(p.w[0]);
  const F e1 = splat<F>(1.0f) - cosang;
  const F ep = ((e1 * e1) * splat<F>(0.25f)) * splat<F>(p.w[1]);
  const F ekp = (w_ang * w_ang) * splat<F>(p.w[2]);
  const F ekc = (v * v) * splat<F>(p.w[3]);
  const float half_nu = 0.5f * (1.0f - 1.0f / p.NU) * p.R;
  F cc = ((du * du) * splat<F>(half_nu) + du * splat<F>(p.R * u) + splat<F>(0.5f * p.R * (u * u))) * splat<F>(p.w[4]);
  const F ur = splat<F>(u) + du;
#pragma unroll
  for (int i = 0; i < Width<F>::value; ++i)
    if (__builtin_fabsf(get(ur, i)) > 1.0f) put(cc, i, 1.0e5f);
  const F dcr = ur - splat<F>(u_prev);
  const F ccrc = (dcr * dcr) * splat<F>(p.w[5]);
  return dd + ep + ekp + ekc + cc + ccrc;
}

}  // namespace cpmppi
