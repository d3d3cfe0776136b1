// cpmppi_ode_fit.hip — fitting the ODE predictor's physical parameters to recordings: the open-loop loss over windows, its
// derivative with respect to the parameters in forward mode, and Adam on the device.   Contract: include/cpmppi.h.
//
// Kernel inventory
//   ode_fit_kernel<FAST, INTEG, NT>   one lane = one window (r, t0), as in brunton_kernel: it starts at states[r,t0], integrates `horizon`
//                                     control steps on the recorded controls and carries, per trained parameter (NT register slots), the
//                                     tangents of (angle, angleD, position, positionD); every step's error enters the lane's loss and
//                                     its NT gradient sums as it is produced - no check-points, no LDS parking.  The workgroup's sums go
//                                     to its own row of the partials with plain stores.
//   ode_fit_finalize_kernel           the partial rows walked in a fixed order in float64: loss, d loss / d theta = p d loss / d p; with
//                                     `update` also Adam on theta and the rewrite of the float32 parameter block.
// Value path: the plain substep of the handle's math mode and predictor with wrap + sincos on every substep - substep_fast /
// substep_cromer_plain (FAST), substep_precise / substep_precise_cromer (PRECISE) - called unchanged on a copy of the launch's
// argument block that holds the fit's parameters (with_fit_block, after with_pole_mass).  The tangents are float32 and are formed
// from the state at the START of each substep with the partial derivatives cpmppi_grad.hpp's substep_reverse uses; non-smooth pieces
// by its rules (the branch taken through the bounce, derivative 1 through fmod / the wrap / atan2(sin, cos)).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_ode.hpp"
#include "cpmppi_grad.hpp"
#include "cpmppi_wave.hpp"
#include "cpmppi_train.hpp"

using namespace cpmppi_k;

// The handle's state of a fit.  block: p[8] | base[8] | theta[8] | m[8] | v[8] floats on the device; p is what the kernel reads.
struct OdeFit {
  float* ws = nullptr;                 // [rows][FIT_ROW] partial sums, one row per workgroup
  size_t ws_floats = 0;
  float* block = nullptr;
  double* grad = nullptr;              // [8] d loss / d theta of cpmppi_ode_fit_step
  unsigned long long* step = nullptr;
  float base_host[CPMPPI_ODE_FIT_PARAMS] = {};
  bool begun = false;
};

namespace {

constexpr int NP = (int)CPMPPI_ODE_FIT_PARAMS;
constexpr int FIT_ROW = 1 + NP;                                  // loss, then one column per parameter
constexpr uint32_t NO_PARAM = (uint32_t)NP;                      // the id of a slot that carries no parameter
enum : uint32_t { FIT_K = 0, FIT_M_CART, FIT_M_POLE, FIT_G, FIT_J_FRIC, FIT_M_FRIC, FIT_U_MAX, FIT_L };
enum : int { BLK_P = 0, BLK_BASE = NP, BLK_THETA = 2 * NP, BLK_M = 3 * NP, BLK_V = 4 * NP, BLK_FLOATS = 5 * NP };

struct OdeFitArgs {
  const float* states;     // [R,T,6]
  const float* Q;          // [R,T]
  const float* L;          // [R,T] or NULL
  const uint32_t* windows; // [B][2]
  const float* block;      // p[8], or NULL = the launch's own argument block
  float* partials;         // [gridDim.x][FIT_ROW]
  float* per_window;       // [B][FIT_ROW] or NULL
  uint32_t B, R, T, horizon;
  uint32_t id[NP];         // the parameter of each tangent slot (NO_PARAM: none), wave-uniform
  float scale[5];
};

// The launch's argument block with the fit's eight parameters in the handle's place, read through the constant address space
// (wave-uniform scalar loads, as with_tuning reads a row).  The copy then goes where the launch's own block went - make_env_const
// and the substep functions - unchanged.
__device__ __forceinline__ Params with_fit_block(const Params& p, const float* block) {
  const __attribute__((address_space(4))) float* r = (const __attribute__((address_space(4))) float*)(uintptr_t)block;
  Params q = p;
  q.k = uniform_(r[FIT_K]); q.m_cart = uniform_(r[FIT_M_CART]); q.m_pole = uniform_(r[FIT_M_POLE]); q.g = uniform_(r[FIT_G]);
  q.J_fric = uniform_(r[FIT_J_FRIC]); q.M_fric = uniform_(r[FIT_M_FRIC]); q.u_max = uniform_(r[FIT_U_MAX]);
  q.L_default = uniform_(r[FIT_L]);
  return q;
}

struct Tangent {
  float th, w, x, v;       // d (angle, angleD, position, positionD) / d parameter; angle_cos / angle_sin follow from th
};

// PRECISE: the position the simultaneous Euler step reaches, rounded as substep_precise rounds it (its bounce test reads this value).
__device__ __forceinline__ float euler_position_precise(float x, float v, float t) {
#pragma clang fp contract(off)
  return x + v * t;
}

// The tangents through one substep that starts at `st` under the control Qk (u = u_max Qk).  With Lh = L / 2:
//   A = (k+1)(m_c+m_p) - m_p c^2,  N = m_p g s c - J w c / Lh + (k+1)(-m_p Lh w^2 s - M v + u),  xDD = N / A,
//   B = g s + xDD c - J w / (m_p Lh),  D = (k+1) Lh,  aDD = B / D.
// d xDD = (d N - xDD d A) / A and d aDD = (d B - aDD d D) / D, each the state's part (substep_reverse's partials times the
// incoming tangent) plus the parameter's direct part, which the slot's wave-uniform id selects.
template <bool FAST, bool CROMER, int NT>
__device__ __forceinline__ void tangent_substep(const State<float>& st, float Qk, float t, const Params& p, const EnvConst& e,
                                                const uint32_t (&id)[NP], Tangent (&tg)[NT]) {
  const float c = st.c, s = st.s, w = st.w, v = st.v;
  const float A = __builtin_fmaf(-(c * p.m_pole), c, e.kp1_mt);
  const float r = 1.0f / A;
  const float t1 = __builtin_fmaf(e.mg, s, -(w * e.JinvLh));
  float num = __builtin_fmaf(c, t1, e.uK_scale * Qk);
  num = __builtin_fmaf(-((w * w) * e.kmLh), s, num);
  num = __builtin_fmaf(-e.kM, v, num);
  const float xDD = num * r;
  const float aDD = __builtin_fmaf(e.g_i, s, __builtin_fmaf(xDD * c, e.inv_kLh, -(w * e.cT_i)));
  // partial derivatives with respect to the state (cpmppi_grad.hpp, substep_reverse)
  const float dA_dth = 2.0f * p.m_pole * c * s;
  const float dnum_dth = __builtin_fmaf(-s, t1, c * (e.mg * c)) - e.kmLh * (w * w) * c;
  const float dx_dth = (dnum_dth - xDD * dA_dth) * r;
  const float dx_dw = -(__builtin_fmaf(c, e.JinvLh, 2.0f * e.kmLh * w * s)) * r;
  const float dx_dv = -e.kM * r;
  const float ic = e.inv_kLh * c;
  const float da_dth = __builtin_fmaf(e.g_i, c, e.inv_kLh * __builtin_fmaf(dx_dth, c, -(xDD * s)));
  const float da_dw = __builtin_fmaf(ic, dx_dw, -e.cT_i);
  const float da_dv = ic * dx_dv;
  // edge bounce (predictor_ODE_v0): the branch the value path takes - the same position, rounded the same way
  bool hit = false;
  float sb = 0.0f, cb = 0.0f, v1 = 0.0f;
  if constexpr (!CROMER) {
    const float x1 = FAST ? __builtin_fmaf(v, t, st.x) : euler_position_precise(st.x, v, t);
    hit = __builtin_fabsf(x1) >= p.THL;
    if (hit) {
      sincos_pi_half<float>(wrap_rint<float>(__builtin_fmaf(w, t, st.th)), sb, cb);   // of the integrated angle
      v1 = __builtin_fmaf(xDD, t, v);
    }
  }
  const float inv_Lh = 1.0f / e.Lh, w2s = (w * w) * s, jw = p.J_fric * w;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    float dN = 0.0f, dA = 0.0f, dB = 0.0f, dD = 0.0f;
    switch (id[i]) {                                                // wave-uniform
      case FIT_K:      dN = __builtin_fmaf(p.u_max, Qk, -(p.m_pole * e.Lh * w2s) - p.M_fric * v); dA = p.m_cart + p.m_pole; dD = e.Lh; break;
      case FIT_M_CART: dA = e.kp1; break;
      case FIT_M_POLE: dN = p.g * s * c - e.kp1 * e.Lh * w2s; dA = e.kp1 - c * c; dB = jw * inv_Lh / (p.m_pole * p.m_pole); break;
      case FIT_G:      dN = p.m_pole * s * c; dB = s; break;
      case FIT_J_FRIC: dN = -(w * c) * inv_Lh; dB = -(w * inv_Lh) / p.m_pole; break;
      case FIT_M_FRIC: dN = -e.kp1 * v; break;
      case FIT_U_MAX:  dN = e.kp1 * Qk; break;
      case FIT_L:      dN = 0.5f * (jw * c * inv_Lh * inv_Lh - e.kp1 * p.m_pole * w2s); dB = 0.5f * jw * inv_Lh * inv_Lh / p.m_pole;
                       dD = 0.5f * e.kp1; break;
      default: break;
    }
    Tangent g = tg[i];
    const float dx_dir = (dN - xDD * dA) * r;
    const float da_dir = __builtin_fmaf(ic, dx_dir, (dB - aDD * dD) * e.inv_kLh);
    const float dxDD = __builtin_fmaf(dx_dth, g.th, __builtin_fmaf(dx_dw, g.w, __builtin_fmaf(dx_dv, g.v, dx_dir)));
    const float daDD = __builtin_fmaf(da_dth, g.th, __builtin_fmaf(da_dw, g.w, __builtin_fmaf(da_dv, g.v, da_dir)));
    if constexpr (CROMER) {                                         // velocities first, angle and position by the NEW velocities
      g.w = __builtin_fmaf(daDD, t, g.w);
      g.v = __builtin_fmaf(dxDD, t, g.v);
      g.th = __builtin_fmaf(g.w, t, g.th);
      g.x = __builtin_fmaf(g.v, t, g.x);
    } else {
      g.th = __builtin_fmaf(g.w, t, g.th);
      g.x = __builtin_fmaf(g.v, t, g.x);
      g.w = __builtin_fmaf(daDD, t, g.w);
      g.v = __builtin_fmaf(dxDD, t, g.v);
      if (hit) {       // w2 = w1 - 2 v1 cos(th1) / (L/2); th2 = th1 + w2 t; v2 = -v1; x2 = x1 + v2 t   (the bounce reads L directly)
        float dw2 = g.w - 2.0f * e.inv_halfL * __builtin_fmaf(g.v, cb, -(v1 * sb * g.th));
        if (id[i] == FIT_L) dw2 = __builtin_fmaf(2.0f * (v1 * cb), e.inv_halfL / e.L, dw2);
        g.w = dw2;
        g.th = __builtin_fmaf(g.w, t, g.th);
        g.v = -g.v;
        g.x = __builtin_fmaf(g.v, t, g.x);
      }
    }
    tg[i] = g;
  }
}

template <bool FAST, int INTEG, int NT>
__global__ __launch_bounds__(BLOCK) void ode_fit_kernel(const Params p0, const OdeFitArgs a) {
  constexpr bool CROMER = INTEG == PREDICTOR_ODE;
  __shared__ float red[WAVES][1 + NT];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t b_raw = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = b_raw < a.B;
  const size_t b = live ? b_raw : (size_t)a.B - 1;               // (idle lanes of the last workgroup shadow the last window)
  // (the host copy of the windows is what every call checks; the device copy is clamped into the recordings, so that one that differs
  // from it - a stale buffer - costs a wrong number, never a read outside `states`)
  const uint32_t wr = min(a.windows[2 * b], a.R - 1u), wt = min(a.windows[2 * b + 1], a.T - 1u - a.horizon);
  const size_t row = (size_t)wr * a.T + wt;
  Params p = p0;                                                 // (by value: a reference chosen at run time keeps both blocks in scratch)
  if (a.block) p = with_fit_block(p0, a.block);
  const EnvConst ec = make_env_const(p, a.L ? a.L[row] : p.L_default);
  const float* s = a.states + row * 6;
  State<float> st{s[0], s[1], s[2], s[3], s[4], s[5]};
  Tangent tg[NT];
  float grad[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) { tg[i] = Tangent{0.0f, 0.0f, 0.0f, 0.0f}; grad[i] = 0.0f; }
  float loss = 0.0f;
  const float t = p.t_step;
  for (uint32_t k = 0; k < a.horizon; ++k) {
    const float Qk = a.Q[row + k];
    const float uK = ec.uK_scale * Qk, u = p.u_max * Qk;
    for (uint32_t sub = 0; sub < p.S; ++sub) {
      tangent_substep<FAST, CROMER, NT>(st, Qk, t, p, ec, a.id, tg);
      if constexpr (CROMER) {
        if constexpr (FAST) substep_cromer_plain(st, uK, t, p, ec);
        else substep_precise_cromer(st, u, t, p, ec);
      } else {
        if constexpr (FAST) substep_fast<float>(st, uK, t, p, ec, p.THL);
        else substep_precise(st, u, t, p, ec);
      }
    }
    const float* rec = a.states + (row + k + 1) * 6;
    const float pred[5] = {st.w, st.c, st.s, st.x, st.v};
    float e2[5];                                                    // 2 scale^2 (predicted - recorded)
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const float e = (pred[f] - rec[1 + f]) * a.scale[f];
      loss = __builtin_fmaf(e, e, loss);
      e2[f] = 2.0f * e * a.scale[f];
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const Tangent& g = tg[i];
      float d = e2[0] * g.w;
      d = __builtin_fmaf(__builtin_fmaf(e2[2], st.c, -(e2[1] * st.s)), g.th, d);   // d cos = -sin d angle, d sin = cos d angle
      d = __builtin_fmaf(e2[3], g.x, d);
      d = __builtin_fmaf(e2[4], g.v, d);
      grad[i] += d;
    }
  }
  if (a.per_window && live) {
    float* o = a.per_window + b * FIT_ROW;
    o[0] = loss;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      float gj = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) gj = (a.id[i] == (uint32_t)j) ? grad[i] : gj;
      o[1 + j] = gj;
    }
  }
  // wave_sum, then the four waves through LDS as (w0 + w1) + (w2 + w3); idle lanes enter as zeros
  const float wl = wave_sum(live ? loss : 0.0f);
  if (lane == 0) red[wave][0] = wl;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const float wg = wave_sum(live ? grad[i] : 0.0f);
    if (lane == 0) red[wave][1 + i] = wg;
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)FIT_ROW) {
    const uint32_t col = threadIdx.x;
    int slot = col == 0 ? 0 : -1;                                   // the column of red that holds this column's sums
    if (col != 0) {
#pragma unroll
      for (int i = 0; i < NT; ++i) slot = (a.id[i] == col - 1u) ? 1 + i : slot;
    }
    a.partials[(size_t)blockIdx.x * FIT_ROW + col] =
        slot < 0 ? 0.0f : (red[0][slot] + red[1][slot]) + (red[2][slot] + red[3][slot]);
  }
}

// ONE workgroup of 64 lanes; lane 0 owns the loss, lane 1 + i parameter i.  Each walks its column of the partial rows first to last
// in float64.  d loss / d theta_i = p_i d loss / d p_i.  update != 0: Adam on theta with t = *step + 1 (cpmppi.h states the update;
// float64 arithmetic, moments and theta stored as float32) for the parameters of `trainable`, p = (float)(base exp(theta)) rewritten,
// then *step = t.  repack != 0 (cpmppi_ode_fit_begin / _set_theta): p from base and theta alone, nothing else is read or written.
__global__ __launch_bounds__(64) void ode_fit_finalize_kernel(const float* __restrict__ partials, uint32_t rows, double count,
                                                              const Params p0, float* block, uint32_t trainable,
                                                              double* __restrict__ loss_out, double* __restrict__ grad_out,
                                                              unsigned long long* step, float lr, float beta1, float beta2, float eps,
                                                              int update, int repack) {
  const uint32_t tid = threadIdx.x;
  if (repack) {
    if (tid < (uint32_t)NP) block[BLK_P + tid] = (float)((double)block[BLK_BASE + tid] * exp((double)block[BLK_THETA + tid]));
    return;
  }
  const unsigned long long t = update ? *step + 1 : 0;
  __syncthreads();                                                  // every lane has read *step
  if (tid >= (uint32_t)FIT_ROW) return;
  double acc = 0.0;
  for (uint32_t r = 0; r < rows; ++r) acc += (double)partials[(size_t)r * FIT_ROW + tid];
  acc /= count;
  if (tid == 0) {
    *loss_out = acc;
    if (update) *step = t;
    return;
  }
  const uint32_t i = tid - 1;
  const float own[NP] = {p0.k, p0.m_cart, p0.m_pole, p0.g, p0.J_fric, p0.M_fric, p0.u_max, p0.L_default};
  float pi = own[0];
#pragma unroll
  for (int j = 1; j < NP; ++j) pi = (i == (uint32_t)j) ? own[j] : pi;
  if (block) pi = block[BLK_P + i];
  const bool trained = (trainable >> i) & 1u;
  const double g = trained ? (double)pi * acc : 0.0;
  if (grad_out) grad_out[i] = g;
  if (update && trained) {
    const AdamStep adam(beta1, beta2, lr, eps, t);
    const float theta = (float)adam(block[BLK_M + i], block[BLK_V + i], g, block[BLK_THETA + i]);
    block[BLK_THETA + i] = theta;
    block[BLK_P + i] = (float)((double)block[BLK_BASE + i] * exp((double)theta));
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
template <bool FAST, int INTEG>
void launch_fit(int slots, dim3 grid, hipStream_t s, const Params& p, const OdeFitArgs& a) {
  if (slots <= 1) hipLaunchKernelGGL((ode_fit_kernel<FAST, INTEG, 1>), grid, dim3(BLOCK), 0, s, p, a);
  else if (slots <= 4) hipLaunchKernelGGL((ode_fit_kernel<FAST, INTEG, 4>), grid, dim3(BLOCK), 0, s, p, a);
  else hipLaunchKernelGGL((ode_fit_kernel<FAST, INTEG, 8>), grid, dim3(BLOCK), 0, s, p, a);
}

size_t fit_rows(uint32_t B) { return ((size_t)B + BLOCK - 1) / BLOCK; }

// The handle's fit state with partial rows for B windows: allocated on first use, never inside a capture.
int ensure(cpmppi_handle* h, uint32_t B, hipStream_t s, const char* who) {
  const size_t need = fit_rows(B) * FIT_ROW;
  OdeFit* st = h->ode_fit;
  if (st && st->block && st->grad && st->step && st->ws_floats >= need) return CPMPPI_OK;
  if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_ode_fit_reserve")) return rc;
  if (!st) st = h->ode_fit = new OdeFit();
  if (!st->block) {
    CPMPPI_HIP(h, hipMalloc(&st->block, BLK_FLOATS * sizeof(float)));
    CPMPPI_HIP(h, hipMemset(st->block, 0, BLK_FLOATS * sizeof(float)));
  }
  if (!st->grad) CPMPPI_HIP(h, hipMalloc(&st->grad, NP * sizeof(double)));
  if (!st->step) {
    CPMPPI_HIP(h, hipMalloc(&st->step, sizeof(unsigned long long)));
    CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  }
  return grow_workspace(h, st->ws, st->ws_floats, need);
}

void own_parameters(const cpmppi_handle* h, float out[NP]) {
  const cpmppi_config& c = h->cfg;
  out[FIT_K] = c.k; out[FIT_M_CART] = c.m_cart; out[FIT_M_POLE] = c.m_pole; out[FIT_G] = c.g;
  out[FIT_J_FRIC] = c.J_fric; out[FIT_M_FRIC] = c.M_fric; out[FIT_U_MAX] = c.u_max; out[FIT_L] = c.L_default;
}

// What cpmppi_ode_fit_loss_grad refuses before it launches (cpmppi.h lists it), in `who`'s name.
int check_args(cpmppi_handle* h, const cpmppi_ode_fit_args* a, const char* who) {
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": " + why); };
  if (!a->states || !a->Q || !a->windows || !a->windows_host || !a->loss_out)
    return refuse("states, Q, windows, windows_host and loss_out are required");
  if (a->B == 0 || a->R == 0 || a->T == 0 || a->horizon == 0) return refuse("B, R, T and horizon must be at least 1");
  if (a->horizon > h->cfg.H)
    return refuse("horizon " + std::to_string(a->horizon) + " is longer than the handle's (" + std::to_string(h->cfg.H) + ")");
  if (a->trainable == 0 || a->trainable >= (1u << NP))
    return refuse("trainable = " + std::to_string(a->trainable) + ": a non-empty mask of the " + std::to_string(NP) +
                  " parameters k, m_cart, m_pole, g, J_fric, M_fric, u_max, L");
  if (h->m_pole_rows) return refuse("per-row pole masses are registered (cpmppi_set_pole_mass_rows): the fit has one pole mass");
  if (((a->trainable >> FIT_L) & 1u) && a->L) return refuse("L is trainable and L rows are given: the rows would replace the parameter");
  float base[NP];
  own_parameters(h, base);
  const float* b = (h->ode_fit && h->ode_fit->begun) ? h->ode_fit->base_host : base;
  static const char* const names[NP] = {"k", "m_cart", "m_pole", "g", "J_fric", "M_fric", "u_max", "L"};
  for (int i = 0; i < NP; ++i)
    if (((a->trainable >> i) & 1u) && !(b[i] > 0.0f))
      return refuse(std::string("trainable parameter ") + names[i] + " has the base value " + std::to_string(b[i]) +
                    ": p = base exp(theta) needs base > 0");
  if (misaligned(a->states) || misaligned(a->Q) || misaligned(a->L) || misaligned(a->windows) || misaligned(a->windows_host) ||
      misaligned(a->per_window_out) || misaligned8(a->loss_out) || misaligned8(a->grad_out))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  return check_windows(h, who, a->windows_host, a->B, a->R, a->T, (uint64_t)a->horizon + 1, "r < R, t0 + horizon <= T - 1");
}

void launch_finalize(cpmppi_handle* h, uint32_t rows, double count, float* block, uint32_t trainable, double* loss_out,
                     double* grad_out, float lr, float beta1, float beta2, float eps, int update, int repack, hipStream_t s) {
  OdeFit* st = h->ode_fit;
  hipLaunchKernelGGL(ode_fit_finalize_kernel, dim3(1), dim3(64), 0, s, (const float*)st->ws, rows, count, h->prm, block, trainable,
                     loss_out, grad_out, st->step, lr, beta1, beta2, eps, update, repack);
}

// The loss and d loss / d theta (into `grad`, or NULL) on `s`; `update`: and Adam.  Checks, workspace, the two launches.
int loss_grad_impl(cpmppi_handle* h, const cpmppi_ode_fit_args* a, double* grad, int update, float lr, float beta1, float beta2,
                   float eps, hipStream_t s, const char* who) {
  if (const int rc = check_args(h, a, who)) return rc;
  if (const int rc = ensure(h, a->B, s, who)) return rc;
  OdeFit* st = h->ode_fit;
  float* block = st->begun ? st->block : nullptr;
  OdeFitArgs k{a->states, a->Q, a->L, a->windows, block, st->ws, a->per_window_out, a->B, a->R, a->T, a->horizon, {}, {}};
  int slots = 0;
  for (int i = 0; i < NP; ++i) {
    k.id[i] = NO_PARAM;
    if ((a->trainable >> i) & 1u) k.id[slots++] = (uint32_t)i;
  }
  for (int f = 0; f < 5; ++f) k.scale[f] = a->feature_scale[f];
  const bool fast = h->cfg.math_mode == CPMPPI_MATH_FAST, cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
  const auto launch = fast ? (cromer ? launch_fit<true, PREDICTOR_ODE> : launch_fit<true, PREDICTOR_ODE_V0>)
                           : (cromer ? launch_fit<false, PREDICTOR_ODE> : launch_fit<false, PREDICTOR_ODE_V0>);
  const uint32_t rows = (uint32_t)fit_rows(a->B);
  launch(slots, dim3(rows), s, h->prm, k);
  CPMPPI_HIP(h, hipGetLastError());
  launch_finalize(h, rows, (double)a->B * a->horizon * 5.0, block, a->trainable, a->loss_out, grad, lr, beta1, beta2, eps, update, 0, s);
  return launched(h);
}

int not_begun(cpmppi_handle* h, const char* who) {
  return begun_or_refuse(h, who, h->ode_fit && h->ode_fit->begun, "cpmppi_ode_fit_begin");
}

// p = (float)(base exp(theta)) on the device, synchronously (cpmppi_ode_fit_begin, cpmppi_ode_fit_set_theta).
int repack(cpmppi_handle* h) {
  launch_finalize(h, 0, 1.0, h->ode_fit->block, 0, nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0, 1, nullptr);
  CPMPPI_HIP(h, hipGetLastError());
  CPMPPI_HIP(h, hipDeviceSynchronize());
  return CPMPPI_OK;
}

}  // namespace

void ode_fit_destroy(cpmppi_handle* h) {
  OdeFit* st = h->ode_fit;
  if (!st) return;
  if (st->ws) (void)hipFree(st->ws);
  if (st->block) (void)hipFree(st->block);
  if (st->grad) (void)hipFree(st->grad);
  if (st->step) (void)hipFree(st->step);
  delete st;
  h->ode_fit = nullptr;
}

extern "C" {

int cpmppi_ode_fit_reserve(cpmppi_handle* h, uint32_t B) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (B == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_reserve: B must be at least 1");
  CPMPPI_ON_DEVICE(h);
  return ensure(h, B, nullptr, "cpmppi_ode_fit_reserve");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

int cpmppi_ode_fit_loss_grad(cpmppi_handle* h, const cpmppi_ode_fit_args* a, void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_loss_grad: no argument block");
  CPMPPI_ON_DEVICE(h);
  return loss_grad_impl(h, a, a->grad_out, 0, 0.0f, 0.0f, 0.0f, 0.0f, (hipStream_t)stream, "cpmppi_ode_fit_loss_grad");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_ode_fit_begin(cpmppi_handle* h) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (h->m_pole_rows)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_begin: per-row pole masses are registered (cpmppi_set_pole_mass_rows): the fit has one pole mass");
  CPMPPI_ON_DEVICE(h);
  if (const int rc = ensure(h, 1, nullptr, "cpmppi_ode_fit_begin")) return rc;
  OdeFit* st = h->ode_fit;
  float blk[BLK_FLOATS] = {};
  own_parameters(h, st->base_host);
  for (int i = 0; i < NP; ++i) blk[BLK_P + i] = blk[BLK_BASE + i] = st->base_host[i];
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemcpy(st->block, blk, sizeof(blk), hipMemcpyHostToDevice));
  CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  if (const int rc = repack(h)) return rc;
  st->begun = true;
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_ode_fit_set_theta(cpmppi_handle* h, const float* theta_host) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!theta_host) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_set_theta: theta_host is required");
  if (const int rc = not_begun(h, "cpmppi_ode_fit_set_theta")) return rc;
  for (int i = 0; i < NP; ++i)
    if (!(fabsf(theta_host[i]) < INFINITY)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_set_theta: theta must be finite");
  CPMPPI_ON_DEVICE(h);
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemcpy(h->ode_fit->block + BLK_THETA, theta_host, NP * sizeof(float), hipMemcpyHostToDevice));
  return repack(h);
}

int cpmppi_ode_fit_step(cpmppi_handle* h, const cpmppi_ode_fit_args* a, float lr, float beta1, float beta2, float eps,
                        void* stream) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_ode_fit_step: no argument block");
  if (const int rc = not_begun(h, "cpmppi_ode_fit_step")) return rc;
  CPMPPI_ON_DEVICE(h);
  return loss_grad_impl(h, a, h->ode_fit->grad, 1, lr, beta1, beta2, eps, (hipStream_t)stream, "cpmppi_ode_fit_step");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_ode_fit_get(cpmppi_handle* h, float* params_host, float* theta_host) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (const int rc = not_begun(h, "cpmppi_ode_fit_get")) return rc;
  CPMPPI_ON_DEVICE(h);
  CPMPPI_HIP(h, hipDeviceSynchronize());
  if (params_host) CPMPPI_HIP(h, hipMemcpy(params_host, h->ode_fit->block + BLK_P, NP * sizeof(float), hipMemcpyDeviceToHost));
  if (theta_host) CPMPPI_HIP(h, hipMemcpy(theta_host, h->ode_fit->block + BLK_THETA, NP * sizeof(float), hipMemcpyDeviceToHost));
  return CPMPPI_OK;
}

}  // extern "C"
