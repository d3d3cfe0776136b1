// cpmppi_params.hpp — what every kernel of the library is written over (gfx950 only): the kernel-argument block Params, the
// per-env constants EnvConst, the kernels' template-argument ids, the rollout state, and the float / float2 helpers.
// Everything is float32.  All per-env quantities are wave-uniform and end up in SGPRs (they are derived from kernel
// arguments and blockIdx only).
//
// Lane mapping.  A rollout is one serial dependency chain of ~30 000 VALU instructions.  Measured on MI355X
// (tools/valu_peak.hip): a dependent chain inside ONE wave issues at ~1.85 ns per wave64 instruction however many
// waves share the SIMD, two independent chains inside one wave at ~1.0 ns, and v_pk_fma_f32 performs two FMAs for the
// price of one instruction.  The FAST path is therefore written generically over F = float (one rollout per lane: the
// latency-optimal mapping when there are few rollouts) and F = float2 (two rollouts per lane: every arithmetic
// instruction is a packed v_pk_* op or one of two independent scalar ops; the throughput mapping).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpmppi {

constexpr float PI_F = 3.14159274101257324f;       // float32(np.pi)
constexpr float TWO_PI_F = 6.28318548202514648f;   // float32(2*np.pi)

enum : int { COST_QBGM = 0, COST_DEFAULT = 1, COST_LEGACY = 2, COST_QBG = 3 };
enum : int { NOISE_DELTA_U = 0, NOISE_KNOTS = 1, NOISE_PHILOX = 2, NOISE_TILED = 3 };
// INTEG, the in-tree ODE predictor a kernel integrates with (cpmppi_ode.hpp)
enum : int { PREDICTOR_ODE_V0 = 0, PREDICTOR_ODE = 1,
             PREDICTOR_ODE_ROWS = 2 };   // (the launch dispatch only: PREDICTOR_ODE with the pole mass read per env = rollout_cost_rows_kernel)

// Kernel-argument block (passed by value -> kernarg segment -> SGPRs).
struct Params {
  uint32_t E, N, H, S, P;            // P = number of knots = ceil(H/period)+1
  uint32_t period;
  float t_step;                      // dt / S
  float k, m_cart, m_pole, g, J_fric, M_fric, u_max, THL, L_default;
  uint32_t cost_id;
  float w[24];
  float R, LBD, NU, cc_weight, sigma;
  float lo, hi;
  float run_lo, run_hi;              // limits of the control a rollout applies: (lo, hi) when control_mode clips, (-inf, inf)
                                     // otherwise - the clamp is then unconditional (no select on the mode per control step)
  uint32_t horizon_reduce, control_mode, shift_mode, correction_u;
  uint32_t interp_f32;               // FAST + device-generated knots: interpolate with one float32 FMA (<= 1 ulp of the
                                     // float64 scipy form, which stays in force for caller-provided knots)
  uint32_t qb_mode;                  // cost_id == COST_DEFAULT only: 0 = default.py, 1 = quadratic_boundary.py, 2 = its
                                     // _nonconvex sibling (the public ids CPMPPI_COST_QB / _QB_NONCONVEX; same kernels)
};

// Per-env constants.  PRECISE keeps the reference's operands; FAST folds them (all wave-uniform).
constexpr float ROT_LIMIT_LO = 0.125f;
constexpr float ROT_LIMIT = 0.25f;

struct EnvConst {
  float L, Lh;
  float kp1, kp1_mt;                 // (k+1), (k+1)*(m_cart+m_pole)
  float mg, JinvLh, kmLh, kM, g_i, cT_i, inv_kLh, inv_halfL;
  float uK_scale;                    // (k+1) u_max: FAST forms (k+1) u = (k+1) u_max Q with one product
  float t1_i;                        // inv_kLh / m_pole: g_i s - cT_i w = t1_i (m_p g s - J/Lh w), the bracket xDD's numerator forms anyway
  float tg_i, tcT_i, tinv_kLh;       // the same three angleDD coefficients times the substep length t (no reader since the form
                                     // that folded t in was removed; kept: they are part of EnvFold's layout, which the
                                     // throughput kernels' scalar loads address - without them seven units' code moves)
  float wlim;                        // ROT_LIMIT_LO / t: |w| beyond it leaves the carried rotation pair's seed range (packed path)
};

__device__ __forceinline__ EnvConst make_env_const(const Params& p, float L) {
  EnvConst c;
  c.L = L;
  c.Lh = L / 2.0f;
  c.kp1 = p.k + 1.0f;
  c.kp1_mt = c.kp1 * (p.m_cart + p.m_pole);
  // folded constants are formed in double and rounded once
  const double Lh = (double)c.Lh, kp1 = (double)c.kp1;
  c.mg = (float)((double)p.m_pole * (double)p.g);
  c.JinvLh = (float)((double)p.J_fric / Lh);
  c.kmLh = (float)(kp1 * (double)p.m_pole * Lh);
  c.kM = (float)(kp1 * (double)p.M_fric);
  const double inv_kLh = 1.0 / (kp1 * Lh);
  c.inv_kLh = (float)inv_kLh;
  c.g_i = (float)((double)p.g * inv_kLh);
  c.cT_i = (float)((double)p.J_fric / ((double)p.m_pole * Lh) * inv_kLh);
  c.inv_halfL = (float)(1.0 / (0.5 * (double)L));
  c.t1_i = (float)(inv_kLh / (double)p.m_pole);
  c.uK_scale = (float)(kp1 * (double)p.u_max);
  const double t = (double)p.t_step;
  c.tg_i = (float)(t * (double)p.g * inv_kLh);
  c.tcT_i = (float)(t * ((double)p.J_fric / ((double)p.m_pole * Lh) * inv_kLh));
  c.tinv_kLh = (float)(t * inv_kLh);
  c.wlim = ROT_LIMIT_LO / p.t_step;
  return c;
}

// predictor_ODE's per-row controller-side pole mass (cpmppi_set_pole_mass_rows): the launch's argument block with the ROW's mass
// in the handle's place.  The copy then goes where the launch's own block went - make_env_const* and the substep functions - so a
// row computes, instruction for instruction, what a handle whose scalar mass is `m_pole` computes (only the fields those read
// survive the copy; the costs never read the mass and keep the launch's block).
__device__ __forceinline__ Params with_pole_mass(const Params& p, float m_pole) {
  Params q = p;
  q.m_pole = m_pole;
  return q;
}

// The per-env controller tuning (cpmppi_set_tuning_rows): one row of TUNING_ROW_FLOATS per env - the seven entries of
// quadratic_boundary_grad_minimal's cost vector in cpmppi_set_cost_weights order, LBD, sigma, padding to 64 bytes (a row's scalar
// loads never straddle a cache line).  with_tuning: the launch's argument block with the ROW's nine values in the handle's place.
// The copy then goes where the launch's own block went - the cost folds, the stage cost, the sampler's scale, the soft-min - so a
// row computes, instruction for instruction, what a handle with those scalars computes (only the fields those read survive the
// copy).  The row is read through the constant address space: wave-uniform scalar loads wherever in the kernel the copy is
// formed (the array is read-only for the launch); uniform_ pins the values as it does everywhere else.
constexpr uint32_t TUNING_ROW_FLOATS = 16, TUNING_LBD = 7, TUNING_SIGMA = 8;
__device__ __forceinline__ float uniform_(float x);
__device__ __forceinline__ Params with_tuning(const Params& p, const float* row) {
  const __attribute__((address_space(4))) float* r = (const __attribute__((address_space(4))) float*)(uintptr_t)row;
  Params q = p;
#pragma unroll
  for (int i = 0; i < 7; ++i) q.w[i] = uniform_(r[i]);
  q.LBD = uniform_(r[TUNING_LBD]);
  q.sigma = uniform_(r[TUNING_SIGMA]);
  return q;
}
// (`_lane`: every lane its own row - the per-env fold kernel of the throughput build)
__device__ __forceinline__ Params with_tuning_lane(const Params& p, const float* __restrict__ row) {
  Params q = p;
#pragma unroll
  for (int i = 0; i < 7; ++i) q.w[i] = row[i];
  q.LBD = row[TUNING_LBD];
  q.sigma = row[TUNING_SIGMA];
  return q;
}
// The per-env rows of the fused rpgd / gradient-tf step (cpmppi_rpgd_step_rows): the same 64-byte row and the same seven cost
// entries; where the MPPI row holds LBD and sigma this one holds Adam's learning rate and the gradient-norm clip, which are no
// fields of Params (rpgd_row_value reads them).  with_rpgd_row: the launch's block with the ROW's cost entries in the handle's
// place - all that with_tuning puts there for the cost; LBD (no soft-min in this step) and sigma (the redraw matches
// cpmppi_sample, which draws with the handle's) stay the launch's.  A sibling of with_tuning, which is left as it was.
constexpr uint32_t RPGD_ROW_LR = 7, RPGD_ROW_GRADMAX_CLIP = 8;
__device__ __forceinline__ float rpgd_row_value(const float* row, uint32_t i) {
  const __attribute__((address_space(4))) float* r = (const __attribute__((address_space(4))) float*)(uintptr_t)row;
  return uniform_(r[i]);
}
__device__ __forceinline__ Params with_rpgd_row(const Params& p, const float* row) {
  Params q = p;
#pragma unroll
  for (int i = 0; i < 7; ++i) q.w[i] = rpgd_row_value(row, i);
  return q;
}

// For kernels where the env (hence L) is the same for the whole wave: pin every field to an SGPR.  Field by field — the
// first version walked the struct through a float pointer, which kept it in a 28-byte private (scratch) slot per lane:
// 117 MB of scratch stores per 8192-env launch.
__device__ __forceinline__ float uniform_(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ EnvConst make_env_const_uniform(const Params& p, float L) {
  const EnvConst c = make_env_const(p, L);
  EnvConst u;
  u.L = uniform_(c.L); u.Lh = uniform_(c.Lh); u.kp1 = uniform_(c.kp1); u.kp1_mt = uniform_(c.kp1_mt);
  u.mg = uniform_(c.mg); u.JinvLh = uniform_(c.JinvLh); u.kmLh = uniform_(c.kmLh); u.kM = uniform_(c.kM);
  u.g_i = uniform_(c.g_i); u.cT_i = uniform_(c.cT_i); u.inv_kLh = uniform_(c.inv_kLh); u.inv_halfL = uniform_(c.inv_halfL);
  u.tg_i = uniform_(c.tg_i); u.tcT_i = uniform_(c.tcT_i); u.tinv_kLh = uniform_(c.tinv_kLh); u.t1_i = uniform_(c.t1_i);
  u.uK_scale = uniform_(c.uK_scale); u.wlim = uniform_(c.wlim);
  return u;
}

// ------------------------------------------------------------------------------------------------------------------
// float / float2 helpers
typedef float f2 __attribute__((ext_vector_type(2)));

template <int R> struct Lanes;
template <> struct Lanes<1> { using F = float; };
template <> struct Lanes<2> { using F = f2; };

template <class F> struct Width;
template <> struct Width<float> { static constexpr int value = 1; };
template <> struct Width<f2> { static constexpr int value = 2; };

__device__ __forceinline__ float get(float v, int) { return v; }
__device__ __forceinline__ float get(f2 v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ void put(float& v, int, float x) { v = x; }
__device__ __forceinline__ void put(f2& v, int i, float x) { if (i == 0) v.x = x; else v.y = x; }
template <class F> __device__ __forceinline__ F splat(float x);
template <> __device__ __forceinline__ float splat<float>(float x) { return x; }
template <> __device__ __forceinline__ f2 splat<f2>(float x) { return f2{x, x}; }

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ f2 fma_(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float rcp_(float a) { return __builtin_amdgcn_rcpf(a); }
__device__ __forceinline__ f2 rcp_(f2 a) { return f2{__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y)}; }
__device__ __forceinline__ float rint_(float a) { return __builtin_rintf(a); }
__device__ __forceinline__ f2 rint_(f2 a) { return f2{__builtin_rintf(a.x), __builtin_rintf(a.y)}; }
__device__ __forceinline__ float abs_(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ f2 abs_(f2 a) { return f2{__builtin_fabsf(a.x), __builtin_fabsf(a.y)}; }
__device__ __forceinline__ float clamp_(float a, float lo, float hi) { return __builtin_amdgcn_fmed3f(a, lo, hi); }
__device__ __forceinline__ f2 clamp_(f2 a, float lo, float hi) { return f2{clamp_(a.x, lo, hi), clamp_(a.y, lo, hi)}; }
// max(|a|, b) / max(|a|, |b|) as ONE v_max_f32 with source modifiers (fmaxf(fabsf(a), ...) comes out as three instructions: in
// IEEE mode the compiler canonicalises each operand of a maximum with a v_max x, x of its own; the operands here are results of
// arithmetic, never signalling NaNs)
__device__ __forceinline__ float max_abs_(float a, float b) {
  float r;
  asm("v_max_f32_e64 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float max_abs2_(float a, float b) {
  float r;
  asm("v_max_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// max(m, |a|, |b|) as ONE v_max3_f32 (m >= 0; a NaN operand is ignored, as by an ordered compare)
__device__ __forceinline__ float max3_abs2_(float m, float a, float b) {
  float r;
  asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float cos_(float a) { return cosf(a); }
__device__ __forceinline__ f2 cos_(f2 a) { return f2{cosf(a.x), cosf(a.y)}; }

template <class F>
struct State {
  F th, w, c, s, x, v;   // angle, angleD, angle_cos, angle_sin, position, positionD
};

}  // namespace cpmppi
