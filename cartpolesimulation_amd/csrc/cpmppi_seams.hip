// cpmppi_seams.hip — the seams of the reference's MPPI loop as kernels of their own: the sampler, the perturbation tiling,
// the predictor, the cost on materialised trajectories and the reward-weighted average.   Contract: include/cpmppi.h.
//
// Kernel inventory
//   sample_kernel                         a17: Philox knots and / or interpolated delta_u (scipy-interp1d-compatible);
//                                         also the interpolation of given knots (cpmppi_sample, cpmppi_interpolate).
//   sample_tiled_kernel                   a17 straight into the TILED perturbation layout (cpmppi_sample_tiled).
//   tile_kernel                           delta_u in the reference layout -> tiled (cpmppi_tile_delta_u).
//   predict_kernel<FAST, STAGED, INTEG>   predictor seam: trajectories [B,H+1,6] (stores staged through LDS for large launches).
//   brunton_kernel<FAST, INTEG>           Brunton test (cpmppi_brunton): every start row of the recordings rolled forward on the recorded
//                                         controls with predict_kernel's control step; per-workgroup error statistics per horizon step.
//   brunton_finalize_kernel               the partial statistics of the ODE or the GRU kernel (cpmppi_gru_seam.hip) reduced in float64.
//   trajectory_cost_kernel                cost seam on materialised trajectories.
//   rwa_kernel                            a16 on given (S, delta_u).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_ode.hpp"
#include "cpmppi_cost.hpp"
#include "cpmppi_philox.hpp"
#include "cpmppi_wave.hpp"
#include "cpmppi_brunton.hpp"

using namespace cpmppi_k;

namespace {

// a17: knots[E,N,P] and/or delta_u[E,N,H].  One lane draws (or loads) the knots of one rollout into LDS; the wave then
// writes its 64 delta_u rows with lane = time-step, i.e. whole 256-byte row segments per store instruction.
__global__ __launch_bounds__(BLOCK) void sample_kernel(const Params p, uint32_t E, uint64_t seed, uint64_t offset,
                                                       uint32_t env_offset, const float* __restrict__ knots_in,
                                                       float* __restrict__ knots_out, float* __restrict__ du_out) {
  extern __shared__ float kn_lds[];                               // [WAVES][64][P+1]
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t total = (size_t)E * p.N;
  const size_t wave_row0 = ((size_t)blockIdx.x * WAVES + wave) * 64;
  const size_t r = wave_row0 + lane;                              // flat (env, rollout)
  const uint32_t stride = p.P + 1;
  float* __restrict__ mine = kn_lds + (wave * 64 + lane) * stride;
  if (r < total) {
    const uint32_t env = (uint32_t)(r / p.N), n = (uint32_t)(r % p.N);
    for (uint32_t j0 = 0; j0 < p.P; j0 += 4) {
      float zq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!knots_in) philox_normal_quad(seed, offset, env_offset + env, n, j0 >> 2, zq);
#pragma unroll
      for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t j = j0 + s;
        if (j < p.P) {
          const float z = knots_in ? knots_in[r * p.P + j] : p.sigma * zq[s];
          mine[j] = z;
          if (knots_out) knots_out[r * p.P + j] = z;
        }
      }
    }
  }
  if (!du_out) return;
  __syncthreads();
  const float* __restrict__ wk = kn_lds + wave * 64 * stride;
  for (uint32_t row = 0; row < 64 && wave_row0 + row < total; ++row) {
    for (uint32_t k = lane; k < p.H; k += 64) {
      const uint32_t j = k / p.period, i = k % p.period;
      const float zl = wk[row * stride + j], zh = wk[row * stride + j + 1];
      du_out[(wave_row0 + row) * p.H + k] = (p.interp_f32 && !knots_in)
          ? interp_from_slope32(knot_slope32(zl, zh, 1.0f / (float)p.period), zl, i)      // what the FAST Philox kernel forms
          : interp_knots(zl, zh, i, p.period);
    }
  }
}

// ---- the TILED perturbation layout --------------------------------------------------------------------------------
// delta_u_tiled[E][G = ceil(N/64)][Hq = ceil(H/4)][64 rows][4 steps]: element (env, n, k) lives at
//   ((((env * G + n / 64) * Hq + k / 4) * 64 + n % 64) * 4 + k % 4;   rows >= N and steps >= H are zero.
// A wave of the rollout kernel reads it with one 16-byte load per lane per four control steps: 1 KB of contiguous memory
// per wave-instruction, every byte used once per pass (the rollout-major reference layout delta_u[E,N,H] gives 200-byte
// rows, of which a time tile touches 32 bytes: 5.9x the algorithmic traffic).

// a17 straight into the tiled layout: one wave per (env, row group); lane = row; knots staged per lane in LDS.
__global__ __launch_bounds__(BLOCK) void sample_tiled_kernel(const Params p, uint32_t E, uint64_t seed, uint64_t offset,
                                                             uint32_t env_offset, const float* __restrict__ knots_in,
                                                             float* __restrict__ tiled_out) {
  extern __shared__ float kn_lds[];                               // [WAVES][64][P+1]
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t G = (p.N + 63u) >> 6, Hq = (p.H + 3u) >> 2;
  const size_t grp = (size_t)blockIdx.x * WAVES + wave;           // flat (env, group)
  if (grp >= (size_t)E * G) return;
  const uint32_t env = (uint32_t)(grp / G), n = (uint32_t)(grp % G) * 64u + lane;
  const uint32_t stride = p.P + 1;
  float* __restrict__ mine = kn_lds + (wave * 64 + lane) * stride;
  const bool valid = n < p.N;
  for (uint32_t j0 = 0; j0 < p.P; j0 += 4) {
    float zq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid && !knots_in) philox_normal_quad(seed, offset, env_offset + env, n, j0 >> 2, zq);
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
      const uint32_t j = j0 + s;
      if (j < p.P) mine[j] = !valid ? 0.0f : (knots_in ? knots_in[((size_t)env * p.N + n) * p.P + j] : p.sigma * zq[s]);
    }
  }
  float4* __restrict__ out = reinterpret_cast<float4*>(tiled_out) + grp * Hq * 64u + lane;
  const float inv_period = 1.0f / (float)p.period;
  for (uint32_t q = 0; q < Hq; ++q) {
    float v[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint32_t k = 4u * q + c;
      if (k < p.H && valid) {
        const uint32_t j = k / p.period, i = k % p.period;
        const float zl = mine[j], zh = mine[j + 1];
        v[c] = (p.interp_f32 && !knots_in) ? interp_from_slope32(knot_slope32(zl, zh, inv_period), zl, i)
                                           : interp_knots(zl, zh, i, p.period);
      } else {
        v[c] = 0.0f;
      }
    }
    out[(size_t)q * 64u] = float4{v[0], v[1], v[2], v[3]};
  }
}

// delta_u[E,N,H] (reference layout) -> tiled: one wave per (env, row group); 64 x 64 sub-blocks through LDS (rows of the
// sub-block are 256 contiguous bytes of the source; the destination quads are written 1 KB per wave-instruction).
__global__ __launch_bounds__(BLOCK) void tile_kernel(const Params p, uint32_t E, const float* __restrict__ du,
                                                     float* __restrict__ tiled_out) {
  __shared__ float blk[WAVES][64][65];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t G = (p.N + 63u) >> 6, Hq = (p.H + 3u) >> 2;
  const size_t grp = (size_t)blockIdx.x * WAVES + wave;
  if (grp >= (size_t)E * G) return;
  const uint32_t env = (uint32_t)(grp / G), n0 = (uint32_t)(grp % G) * 64u;
  const float* __restrict__ src = du + ((size_t)env * p.N + n0) * p.H;
  float4* __restrict__ out = reinterpret_cast<float4*>(tiled_out) + grp * Hq * 64u + lane;
  for (uint32_t k0 = 0; k0 < p.H; k0 += 64) {
    for (uint32_t r0 = 0; r0 < 64; r0 += 16) {                             // row r: steps k0 .. k0+63, lane = step
      float v[16];                                                         // sixteen row segments in flight
#pragma unroll
      for (uint32_t u = 0; u < 16; ++u)
        v[u] = (n0 + r0 + u < p.N && k0 + lane < p.H) ? src[(size_t)(r0 + u) * p.H + k0 + lane] : 0.0f;
#pragma unroll
      for (uint32_t u = 0; u < 16; ++u) blk[wave][r0 + u][lane] = v[u];
    }
    // (one wave owns blk[wave]: no block barrier; the wave's own LDS writes are ordered before its reads)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (uint32_t c = 0; c < 16 && k0 + 4u * c < p.H; ++c)
      out[(size_t)((k0 >> 2) + c) * 64u] = float4{blk[wave][lane][4 * c], blk[wave][lane][4 * c + 1],
                                                 blk[wave][lane][4 * c + 2], blk[wave][lane][4 * c + 3]};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
}

// predictor seam.  traj[B,H+1,6] is the reference's tensor (row-major per rollout, 24 bytes per state): a lane integrates
// one rollout, the states of PRED_KS control steps are parked in LDS (odd row stride: conflict-free) and then written by
// the whole wave with consecutive lanes on consecutive floats of a row's 192-byte segment — whole sectors per store
// instead of 64 scattered 4-byte pieces 1224 bytes apart (0.9 TB/s at 262144 rollouts before).
constexpr int PRED_KS = 8;
constexpr int PRED_ROW = PRED_KS * 6 + 1;
// STAGED = false: every lane stores its own states directly — the shorter path for launches that do not fill the chip
// (1024 rollouts: 59 us against 82 us staged; 262144 rollouts: 416 us against 280 us staged).
// INTEG: the in-tree ODE predictor (cpmppi_params.hpp: PREDICTOR_ODE_V0 | PREDICTOR_ODE).
template <bool FAST, bool STAGED, int INTEG = PREDICTOR_ODE_V0>
__device__ __forceinline__ void predict_control_step(State<float>& st, float Qk, const Params& p, const EnvConst& ec) {
  if constexpr (INTEG == PREDICTOR_ODE) {
    if constexpr (FAST) control_step_cromer_fast<float>(st, ec.uK_scale * Qk, p.S, p.t_step, p, ec);
    else for (uint32_t sub = 0; sub < p.S; ++sub) substep_precise_cromer(st, p.u_max * Qk, p.t_step, p, ec);
  } else {
    if constexpr (FAST) control_step_fast<float>(st, ec.uK_scale * Qk, p.S, p.t_step, p, ec, p.THL);
    else for (uint32_t sub = 0; sub < p.S; ++sub) substep_precise(st, p.u_max * Qk, p.t_step, p, ec);
  }
}

template <bool FAST, bool STAGED, int INTEG = PREDICTOR_ODE_V0>
__global__ __launch_bounds__(BLOCK) void predict_kernel(const Params p0, uint32_t B, uint32_t H,
                                                        const float* __restrict__ s0, const float* __restrict__ Q,
                                                        const float* __restrict__ Lp, float* __restrict__ traj,
                                                        const float* __restrict__ Mp) {
  // Mp[B]: predictor_ODE's pole mass per row (cpmppi_set_pole_mass_rows; NULL = the handle's) - a row integrates with its own
  // copy of the argument block (with_pole_mass); predictor_ODE_v0 does not read the mass attribute
  if constexpr (!STAGED) {
    const size_t b = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (b >= B) return;
    Params pm_;
    if constexpr (INTEG == PREDICTOR_ODE) pm_ = with_pole_mass(p0, Mp ? Mp[b] : p0.m_pole);
    const Params& p = (INTEG == PREDICTOR_ODE) ? pm_ : p0;
    const EnvConst ec = make_env_const(p, Lp ? Lp[b] : p.L_default);
    const float* s = s0 + b * 6;
    State<float> st{s[0], s[1], s[2], s[3], s[4], s[5]};
    float* o = traj + b * (size_t)(H + 1) * 6;
    o[0] = st.th; o[1] = st.w; o[2] = st.c; o[3] = st.s; o[4] = st.x; o[5] = st.v;
    for (uint32_t k = 0; k < H; ++k) {
      predict_control_step<FAST, STAGED, INTEG>(st, Q[b * H + k], p, ec);
      o += 6;
      o[0] = st.th; o[1] = st.w; o[2] = st.c; o[3] = st.s; o[4] = st.x; o[5] = st.v;
    }
    return;
  }
  __shared__ float park[STAGED ? WAVES : 1][STAGED ? 64 * PRED_ROW : 1];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t b_raw = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool valid = b_raw < B;
  const size_t b = valid ? b_raw : (size_t)B - 1;                 // (idle lanes of the last block shadow the last rollout)
  const size_t wave_b0 = (size_t)blockIdx.x * BLOCK + (size_t)wave * 64;
  Params pm_;
  if constexpr (INTEG == PREDICTOR_ODE) pm_ = with_pole_mass(p0, Mp ? Mp[b] : p0.m_pole);
  const Params& p = (INTEG == PREDICTOR_ODE) ? pm_ : p0;
  const EnvConst ec = make_env_const(p, Lp ? Lp[b] : p.L_default);
  const float* s = s0 + b * 6;
  State<float> st{s[0], s[1], s[2], s[3], s[4], s[5]};
  if (valid) {
    float* o = traj + b * (size_t)(H + 1) * 6;
    o[0] = st.th; o[1] = st.w; o[2] = st.c; o[3] = st.s; o[4] = st.x; o[5] = st.v;
  }
  float* __restrict__ mine = park[wave] + lane * PRED_ROW;
  for (uint32_t k0 = 0; k0 < H; k0 += PRED_KS) {
    const uint32_t kn = (H - k0 < (uint32_t)PRED_KS) ? H - k0 : (uint32_t)PRED_KS;
    for (uint32_t kk = 0; kk < kn; ++kk) {
      predict_control_step<FAST, STAGED, INTEG>(st, Q[b * H + k0 + kk], p, ec);
      float* m = mine + kk * 6;
      m[0] = st.th; m[1] = st.w; m[2] = st.c; m[3] = st.s; m[4] = st.x; m[5] = st.v;
    }
    __syncthreads();
    const uint32_t seg = kn * 6;                                  // floats per row in this chunk
    for (uint32_t idx = lane; idx < 64u * seg; idx += 64u) {
      const uint32_t row = idx / seg, col = idx - row * seg;
      if (wave_b0 + row < B)
        traj[((wave_b0 + row) * (size_t)(H + 1) + k0 + 1) * 6 + col] = park[wave][row * PRED_ROW + col];
    }
    __syncthreads();
  }
}

// Brunton test with an in-tree ODE predictor: the open-loop prediction error over recordings, per horizon step.  One lane per
// start (r, t): it begins at states[r,t], integrates `horizon` control steps on the RECORDED controls Q[r,t+k] - read where the
// series lies, no window tensor - with predict_kernel's own control step (predict_control_step: the two kernels agree by
// construction), and after step k compares with states[r,t+k+1] (brunton_errors).  The workgroup's (sum |e|, sum e^2, max |e|)
// per feature - wave_sum / wave_max, then the four waves through LDS as (w0 + w1) + (w2 + w3) - go to its own row of the
// partials with plain stores: no atomics, the same bits run to run.  `red` is double-buffered by the parity of k, so one barrier
// per step orders both the waves' stores before the combining read and that read before the stores of step k + 2.  Idle lanes
// of the last workgroup shadow the last start (they stay for the barriers) and enter the statistics as zeros.
// The pole mass is the handle's: per-row masses (cpmppi_set_pole_mass_rows) are the predict seam's.
template <bool FAST, int INTEG>
__global__ __launch_bounds__(BLOCK) void brunton_kernel(const Params p, const BruntonArgs a) {
  __shared__ float red[2][WAVES][BRUNTON_STATS];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t starts = (size_t)a.R * a.count;
  const size_t b_raw = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = b_raw < starts;
  const size_t b = live ? b_raw : starts - 1;
  const size_t row = (b / a.count) * a.T + a.start + b % a.count;          // (r, t) in the series
  const EnvConst ec = make_env_const(p, a.L ? a.L[row] : p.L_default);
  const float* s = a.states + row * 6;
  State<float> st{s[0], s[1], s[2], s[3], s[4], s[5]};
  float* o = a.pred ? a.pred + b * (size_t)(a.horizon + 1) * 6 : nullptr;
  if (o && live) { o[0] = st.th; o[1] = st.w; o[2] = st.c; o[3] = st.s; o[4] = st.x; o[5] = st.v; }
  float* __restrict__ out = a.partials + (size_t)blockIdx.x * a.horizon * BRUNTON_STATS;
  for (uint32_t k = 0; k < a.horizon; ++k) {
    predict_control_step<FAST, false, INTEG>(st, a.Q[row + k], p, ec);
    const float pred[6] = {st.th, st.w, st.c, st.s, st.x, st.v};
    if (o && live) {
      o += 6;
#pragma unroll
      for (int f = 0; f < 6; ++f) o[f] = pred[f];
    }
    float e[6];
    brunton_errors(pred, a.states + (row + k + 1) * 6, e);
    brunton_wave_stats(e, live, lane == 0, red[k & 1u][wave]);
    __syncthreads();
    if (threadIdx.x < (uint32_t)BRUNTON_STATS) {
      const float (*r)[BRUNTON_STATS] = red[k & 1u];
      const uint32_t i = threadIdx.x;
      out[(size_t)k * BRUNTON_STATS + i] = (i % 3u == 2u) ? fmaxf(fmaxf(r[0][i], r[1][i]), fmaxf(r[2][i], r[3][i]))
                                                          : (r[0][i] + r[1][i]) + (r[2][i] + r[3][i]);
    }
  }
}

// partials[rows][horizon][6][3] -> stats[horizon][6][3]: one thread per statistic walks the partial rows first to last in
// float64 (sums) or takes their maximum - a fixed order, whatever the launch's shape.
__global__ __launch_bounds__(BLOCK) void brunton_finalize_kernel(const float* __restrict__ partials, uint32_t rows,
                                                                 uint32_t per_row, double* __restrict__ stats) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= per_row) return;
  const bool is_max = i % 3u == 2u;
  double acc = 0.0;
  for (uint32_t r = 0; r < rows; ++r) {
    const double v = (double)partials[(size_t)r * per_row + i];
    acc = is_max ? fmax(acc, v) : acc + v;
  }
  stats[i] = acc;
}

// cost seam on materialised trajectories
// Cost seam.  traj[B,H+1,6] and inputs[B,H] are the reference's tensors (row-major per rollout): lane = time-step, a
// wave walks its rows — a row's 24(H+1) bytes are read by consecutive lanes (coalesced) instead of 64 rows 1224 bytes
// apart per load as in the first version (0.59 TB/s at 262144 rows) — and sums a row's stage costs by wave reduction.
__global__ __launch_bounds__(BLOCK) void trajectory_cost_kernel(const Params p, uint32_t B, uint32_t H, uint32_t rows_per_wave,
                                                                const float* __restrict__ traj,
                                                                const float* __restrict__ inputs, float x_t, float te,
                                                                const float* __restrict__ u_nom,
                                                                const float* __restrict__ u_prev,
                                                                float* __restrict__ stage_out,
                                                                float* __restrict__ terminal_out,
                                                                float* __restrict__ total_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t wave = ((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const size_t b0 = wave * rows_per_wave;
  for (size_t b = b0; b < b0 + rows_per_wave && b < B; ++b) {
    const float* __restrict__ row = traj + b * (size_t)(H + 1) * 6;
    float sum = 0.0f;
    for (uint32_t k0 = 0; k0 < H; k0 += 64) {
      const uint32_t k = k0 + lane;
      float c = 0.0f;
      if (k < H) {
        const float* __restrict__ t = row + (size_t)k * 6;
        const float in = inputs[b * H + k];
        const float cosang = cosf(t[0]);
        if (p.cost_id == CPMPPI_COST_QBGM) c = stage_qbgm<float>(p, t[4], cosang, t[1], in, x_t, te);
        else if (p.cost_id == CPMPPI_COST_DEFAULT)      // (default.py and, by p.qb_mode, quadratic_boundary / _nonconvex: ccrc only with a previous input)
          c = stage_default<float>(p, t[4], cosang, in, x_t, te, k == 0 ? (u_prev ? u_prev[0] : 0.0f) : inputs[b * H + k - 1],
                                   p.qb_mode != 0u && u_prev != nullptr);
        else if (p.cost_id == CPMPPI_COST_QBG)
          c = stage_qbg<float>(p, t[4], cosang, t[1], in, k == 0 ? (u_prev ? u_prev[0] : 0.0f) : inputs[b * H + k - 1], x_t, te);
        else c = stage_legacy<float>(p, t[4], cosang, t[1], t[5], u_nom[k], in, u_prev ? u_prev[k] : 0.0f, x_t);
        if (stage_out) stage_out[b * H + k] = c;
      }
      sum += wave_sum(c);
    }
    if (lane == 0) {
      const float* __restrict__ tl = row + (size_t)H * 6;
      const float term = (p.cost_id == CPMPPI_COST_QBGM || p.cost_id == CPMPPI_COST_QBG) ? 0.0f : terminal_indicator<float>(p, tl[0], tl[4], x_t);
      if (terminal_out) terminal_out[b] = term;
      if (total_out)
        total_out[b] = (p.cost_id == CPMPPI_COST_LEGACY || p.horizon_reduce == CPMPPI_REDUCE_SUM)
                           ? (sum + term) : (sum + term) / (float)(H + 1);
    }
  }
}

// a16 on given (S, delta_u): one block per env
__global__ __launch_bounds__(BLOCK) void rwa_kernel(const Params p, const float* __restrict__ S,
                                                    const float* __restrict__ du, float* __restrict__ out) {
  __shared__ float red[WAVES];
  __shared__ float sh_m, sh_a;
  const uint32_t env = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const float* Se = S + (size_t)env * p.N;
  const float* de = du + (size_t)env * p.N * p.H;
  float m = INFINITY;
  for (uint32_t n = tid; n < p.N; n += BLOCK) m = fminf(m, Se[n]);
  m = wave_min(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) { float v = red[0]; for (int w = 1; w < WAVES; ++w) v = fminf(v, red[w]); sh_m = v; }
  __syncthreads();
  m = sh_m;
  float a = 0.0f;
  for (uint32_t n = tid; n < p.N; n += BLOCK) a += expf((-1.0f / p.LBD) * (Se[n] - m));
  a = wave_sum(a);
  __syncthreads();
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (tid == 0) { float v = red[0]; for (int w = 1; w < WAVES; ++w) v += red[w]; sh_a = v; }
  __syncthreads();
  a = sh_a;
  // lane = column, one wave = every WAVES-th row: rows are read coalesced and a row's weight is formed once per wave (the
  // first version evaluated expf N x H times from H threads); the waves' sums meet in LDS
  __shared__ float part[WAVES][64];
  for (uint32_t k0 = 0; k0 < p.H; k0 += 64) {
    const uint32_t k = k0 + lane;
    float acc = 0.0f;
    const uint32_t kk = k < p.H ? k : 0u;
    uint32_t n = wave;
    for (; n + 7 * WAVES < p.N; n += 8 * WAVES) {           // eight rows in flight: the pass is bound by load latency
      float x[8], e[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { x[u] = de[(size_t)(n + u * WAVES) * p.H + kk]; e[u] = Se[n + u * WAVES]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = __builtin_fmaf(expf((-1.0f / p.LBD) * (e[u] - m)), x[u], acc);
    }
    for (; n < p.N; n += WAVES) acc = __builtin_fmaf(expf((-1.0f / p.LBD) * (Se[n] - m)), de[(size_t)n * p.H + kk], acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && k < p.H) {
      float v = part[0][lane];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) v += part[w][lane];
      out[(size_t)env * p.H + k] = v / a;
    }
    __syncthreads();
  }
}

// What the three sampler entry points check, in this order: E within the handle's and the buffers (`args_ok`, else `bad_arg`),
// the alignment (`aligned`, else `unaligned`), and the knots of a rollout within the sampler's LDS ([256][P+1] floats).
int check_sampler(cpmppi_handle* h, const std::string& fn, uint32_t E, bool args_ok, const char* bad_arg, bool aligned,
                  const char* unaligned) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !args_ok) return fail(h, CPMPPI_ERR_BAD_ARG, fn + bad_arg);
  if (!aligned) return fail(h, CPMPPI_ERR_ALIGN, fn + unaligned);
  if ((size_t)BLOCK * (h->prm.P + 1) * sizeof(float) > SAMPLER_LDS_MAX)
    return fail(h, CPMPPI_ERR_BAD_ARG, fn + ": more than " + std::to_string(SAMPLER_LDS_MAX / (BLOCK * sizeof(float)) - 1) +
                                           " knots per rollout are not supported");
  return CPMPPI_OK;
}

// sample_kernel over E envs: Philox knots (knots_in == NULL) or the given ones, stored and / or interpolated
int launch_sample(cpmppi_handle* h, uint32_t E, uint64_t seed, uint64_t offset, uint32_t env_offset, const float* knots_in,
                  float* knots_out, float* delta_u_out, void* stream) {
  CPMPPI_ON_DEVICE(h);
  const size_t rows = (size_t)E * h->cfg.N;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((rows + BLOCK - 1) / BLOCK)), dim3(BLOCK),
                     (size_t)BLOCK * (h->prm.P + 1) * sizeof(float), (hipStream_t)stream, h->prm, E, seed, offset,
                     env_offset, knots_in, knots_out, delta_u_out);
  return launched(h);
}

template <bool FAST, int INTEG>
void launch_predict(bool staged, dim3 grid, hipStream_t st, const Params& p, uint32_t B, uint32_t H, const float* s0,
                    const float* Q, const float* L, float* traj, const float* m_pole) {
  if (staged) hipLaunchKernelGGL((predict_kernel<FAST, true, INTEG>), grid, dim3(BLOCK), 0, st, p, B, H, s0, Q, L, traj, m_pole);
  else hipLaunchKernelGGL((predict_kernel<FAST, false, INTEG>), grid, dim3(BLOCK), 0, st, p, B, H, s0, Q, L, traj, m_pole);
}

template <bool FAST, int INTEG>
void launch_brunton(dim3 grid, hipStream_t st, const Params& p, const BruntonArgs& a) {
  hipLaunchKernelGGL((brunton_kernel<FAST, INTEG>), grid, dim3(BLOCK), 0, st, p, a);
}

}  // namespace

void allow_large_lds_seams() {
  allow_large_lds(&sample_kernel);
  allow_large_lds(&sample_tiled_kernel);
}

extern "C" {

int cpmppi_sample(cpmppi_handle* h, uint32_t E, uint64_t seed, uint64_t offset, uint32_t env_offset, float* knots_out,
                  float* delta_u_out, void* stream) {
  if (const int rc = check_sampler(h, "cpmppi_sample", E, knots_out || delta_u_out, ": E out of range or no output buffer",
                                   !misaligned(knots_out) && !misaligned(delta_u_out), ": misaligned"); rc != CPMPPI_OK)
    return rc;
  if (const int rc = refuse_tuning_rows(h, "cpmppi_sample")) return rc;       // (it would draw with the handle's sigma, not the rows')
  return launch_sample(h, E, seed, offset, env_offset, nullptr, knots_out, delta_u_out, stream);
}

int cpmppi_interpolate(cpmppi_handle* h, uint32_t E, const float* knots, float* delta_u_out, void* stream) {
  if (const int rc = check_sampler(h, "cpmppi_interpolate", E, knots && delta_u_out, ": bad argument",
                                   !misaligned(knots) && !misaligned(delta_u_out), ": misaligned"); rc != CPMPPI_OK)
    return rc;
  return launch_sample(h, E, 0, 0, 0, knots, nullptr, delta_u_out, stream);
}

size_t cpmppi_tiled_floats(const cpmppi_handle* h, uint32_t E) {
  if (!h) return 0;
  return (size_t)E * ((h->cfg.N + 63u) / 64u) * ((h->cfg.H + 3u) / 4u) * 256u;
}

int cpmppi_sample_tiled(cpmppi_handle* h, uint32_t E, uint64_t seed, uint64_t offset, uint32_t env_offset,
                        const float* knots_in, float* tiled_out, void* stream) {
  if (const int rc = check_sampler(h, "cpmppi_sample_tiled", E, tiled_out != nullptr, ": bad argument",
                                   (reinterpret_cast<uintptr_t>(tiled_out) & 15u) == 0 && !misaligned(knots_in),
                                   ": tiled_out must be 16-byte aligned"); rc != CPMPPI_OK)
    return rc;
  if (!knots_in)                                   // (given knots are only interpolated and tiled: no sigma is read)
    if (const int rc = refuse_tuning_rows(h, "cpmppi_sample_tiled")) return rc;
  CPMPPI_ON_DEVICE(h);
  const size_t groups = (size_t)E * ((h->cfg.N + 63u) / 64u);
  hipLaunchKernelGGL(sample_tiled_kernel, dim3((unsigned)((groups + WAVES - 1) / WAVES)), dim3(BLOCK),
                     (size_t)BLOCK * (h->prm.P + 1) * sizeof(float), (hipStream_t)stream, h->prm, E, seed, offset,
                     env_offset, knots_in, tiled_out);
  return launched(h);
}

int cpmppi_tile_delta_u(cpmppi_handle* h, uint32_t E, const float* delta_u, float* tiled_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || E > h->cfg.E || !delta_u || !tiled_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_tile_delta_u: bad argument");
  if ((reinterpret_cast<uintptr_t>(tiled_out) & 15u) != 0 || misaligned(delta_u))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_tile_delta_u: tiled_out must be 16-byte aligned");
  CPMPPI_ON_DEVICE(h);
  const size_t groups = (size_t)E * ((h->cfg.N + 63u) / 64u);
  hipLaunchKernelGGL(tile_kernel, dim3((unsigned)((groups + WAVES - 1) / WAVES)), dim3(BLOCK), 0, (hipStream_t)stream,
                     h->prm, E, delta_u, tiled_out);
  return launched(h);
}

int cpmppi_predict(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* s0, const float* Q, const float* L,
                   float* traj_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (horizon == 0) horizon = h->cfg.H;
  if (B == 0 || !s0 || !Q || !traj_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_predict: bad argument");
  if (misaligned(s0) || misaligned(Q) || misaligned(L) || misaligned(traj_out))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_predict: misaligned pointer");
  if (!pole_mass_rows_cover(h, B)) return fail(h, CPMPPI_ERR_BAD_ARG, pole_mass_rows_short("cpmppi_predict", h, B));
  if (const int rc = refuse_tuning_rows(h, "cpmppi_predict")) return rc;
  CPMPPI_ON_DEVICE(h);
  // stores staged through LDS once the launch puts more than one wave on every SIMD (below that the direct stores'
  // shorter path wins: measured 59 vs 82 us at 1024 rollouts, 416 vs 280 us at 262144)
  const bool staged = (uint64_t)B > 65536ull;
  const bool fast = h->cfg.math_mode == CPMPPI_MATH_FAST, cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
  const auto launch = fast ? (cromer ? launch_predict<true, PREDICTOR_ODE> : launch_predict<true, PREDICTOR_ODE_V0>)
                           : (cromer ? launch_predict<false, PREDICTOR_ODE> : launch_predict<false, PREDICTOR_ODE_V0>);
  launch(staged, dim3((B + BLOCK - 1) / BLOCK), (hipStream_t)stream, h->prm, B, horizon, s0, Q, L, traj_out, h->m_pole_rows);
  return launched(h);
}

int cpmppi_brunton(cpmppi_handle* h, const cpmppi_brunton_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_brunton: " + why); };
  if (!a) return refuse("no argument block");
  if (!a->states || !a->Q || !a->stats_out) return refuse("states, Q, stats_out are required");
  if (a->R == 0 || a->count == 0 || a->horizon == 0) return refuse("R, count and horizon must be at least 1");
  if (a->horizon > h->cfg.H)
    return refuse("horizon " + std::to_string(a->horizon) + " is longer than the handle's (" + std::to_string(h->cfg.H) + ")");
  if ((uint64_t)a->start + a->count + a->horizon > (uint64_t)a->T)
    return refuse("start + count + horizon = " + std::to_string((uint64_t)a->start + a->count + a->horizon) +
                  " rows, a recording has T = " + std::to_string(a->T));
  const bool gru = a->predictor == CPMPPI_PREDICTOR_GRU;
  if (!gru && a->predictor != CPMPPI_PREDICTOR_ODE_V0) return refuse("unknown predictor " + std::to_string(a->predictor));
  if (gru && !h->gru_image) return refuse("no model set (cpmppi_set_gru)");
  if (gru && a->L) return refuse("the GRU predictor takes no L: the network is the plant model");
  if (!gru && a->h_rows) return refuse("h_rows is the memory of the GRU predictor");
  const size_t starts = (size_t)a->R * a->count;
  const size_t rows = gru ? brunton_gru_rows(starts) : (starts + BLOCK - 1) / BLOCK;
  if (rows > 0x7fffffffull) return refuse("too many starts for one launch");
  if (misaligned(a->states) || misaligned(a->Q) || misaligned(a->L) || misaligned(a->h_rows) || misaligned(a->pred_out) ||
      (reinterpret_cast<uintptr_t>(a->stats_out) & 7u) != 0)
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_brunton: misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  // one partial row per workgroup (ODE) or wave (GRU); allocated on first use and grown on demand, never inside a capture
  const size_t per_row = (size_t)a->horizon * BRUNTON_STATS, need = rows * per_row;
  if (h->brunton_ws_floats < need) {
    if (const int rc = refuse_unreserved_capture(h, (hipStream_t)stream, "cpmppi_brunton", "cpmppi_brunton once")) return rc;
    if (const int rc = grow_workspace(h, h->brunton_ws, h->brunton_ws_floats, need)) return rc;
  }
  const BruntonArgs k{a->states, a->Q, a->L, a->h_rows, h->brunton_ws, a->pred_out, a->R, a->T, a->start, a->count, a->horizon};
  if (gru) {
    launch_gru_brunton(h, k, (hipStream_t)stream);
  } else {
    const bool fast = h->cfg.math_mode == CPMPPI_MATH_FAST, cromer = h->cfg.ode_predictor == CPMPPI_ODE_CROMER;
    const auto launch = fast ? (cromer ? launch_brunton<true, PREDICTOR_ODE> : launch_brunton<true, PREDICTOR_ODE_V0>)
                             : (cromer ? launch_brunton<false, PREDICTOR_ODE> : launch_brunton<false, PREDICTOR_ODE_V0>);
    launch(dim3((unsigned)rows), (hipStream_t)stream, h->prm, k);
  }
  CPMPPI_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(brunton_finalize_kernel, dim3((unsigned)((per_row + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                     (const float*)h->brunton_ws, (uint32_t)rows, (uint32_t)per_row, a->stats_out);
  return launched(h);
}

int cpmppi_trajectory_cost(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* traj, const float* inputs,
                           float target_position, float target_equilibrium, const float* u_nom, const float* u_prev,
                           float* stage_out, float* terminal_out, float* total_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (horizon == 0) horizon = h->cfg.H;
  if (B == 0 || !traj || !inputs || (!stage_out && !terminal_out && !total_out))
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_trajectory_cost: bad argument");
  if (h->prm.cost_id == CPMPPI_COST_LEGACY && !u_nom)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_trajectory_cost: legacy cost needs u_nom");
  if (const int rc = refuse_tuning_rows(h, "cpmppi_trajectory_cost")) return rc;
  CPMPPI_ON_DEVICE(h);
  // rows per wave: one for the reference's call shape (a few thousand rollouts: spread them over the chip), up to 64
  // once there are more rows than ~8 waves per SIMD can take one each
  uint32_t rpw = (uint32_t)(((uint64_t)B + 8191) / 8192);
  rpw = rpw < 1 ? 1 : (rpw > 64 ? 64 : rpw);
  const uint32_t waves = (B + rpw - 1) / rpw;
  hipLaunchKernelGGL(trajectory_cost_kernel, dim3((waves + WAVES - 1) / WAVES), dim3(BLOCK), 0, (hipStream_t)stream, h->prm,
                     B, horizon, rpw, traj, inputs, target_position, target_equilibrium, u_nom, u_prev, stage_out,
                     terminal_out, total_out);
  return launched(h);
}

int cpmppi_reward_weighted_average(cpmppi_handle* h, uint32_t E, const float* S, const float* delta_u, float* out,
                                   void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || !S || !delta_u || !out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_reward_weighted_average: bad argument");
  if (const int rc = refuse_tuning_rows(h, "cpmppi_reward_weighted_average")) return rc;   // (the soft-min with the handle's LBD)
  CPMPPI_ON_DEVICE(h);
  hipLaunchKernelGGL(rwa_kernel, dim3(E), dim3(BLOCK), 0, (hipStream_t)stream, h->prm, S, delta_u, out);
  return launched(h);
}

}  // extern "C"
