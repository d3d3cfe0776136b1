// cpmppi_gru_reverse.hpp — the reverse sweep through the GRU predictor for the wave's 32 rollouts, as the two kernels that run it
// share it: gru_grad_reverse_kernel (cpmppi_gru_adjoint.hip: the second launch of cpmppi_rollout_cost_grad_gru) and
// gru_rpgd_step_kernel (cpmppi_gru_rpgd.hip: the fused rpgd / gradient control step, where it runs between the forward sweep and
// the Adam row of every iteration).  Exact-f32 MFMA in both math modes, on the forward f32 image `lds` (the gates are recomputed)
// and the transposed image `ldst` (cpmppi_gru.hpp).  Neither function holds a barrier or leaves early: a caller with barriers
// behind the sweep calls both for every wave, and H = 1 runs no step.
#pragma once
#include "cpmppi_gru.hpp"        // (and cpmppi_internal.hpp)
#include "cpmppi_grad.hpp"       // (stage_qbgm_grad, stage_default_grad)

namespace cpmppi {

// One GRU layer of the reverse sweep for the wave's 32 rollouts.  Recomputes the layer's gates (exact f32, the order of gru_layer)
// from its input tile x (KX k-steps) and the hidden tile hp the step began with, then turns dh - in: the adjoint of the step's
// new hidden state, out: the direct part z * dh of the adjoint of hp - into the adjoints of the four pre-activation tiles: r, z,
// n's input part and n's hidden part.
template <int KX>
__device__ __forceinline__ void gru_layer_reverse(const float* lds, int fx, int fh, int b0, const f16v& x, const f16v& hp,
                                                  uint32_t lane, f16v& dh, f16v& dar, f16v& daz, f16v& danx, f16v& danh) {
  f16v ar = gru_mm<KX>(gru_bias_v(lds, b0 + 0, lane), lds + (fx + 0 * KX) * 64, x, lane);
  f16v az = gru_mm<KX>(gru_bias_v(lds, b0 + 1, lane), lds + (fx + 1 * KX) * 64, x, lane);
  const f16v anx = gru_mm<KX>(gru_bias_v(lds, b0 + 2, lane), lds + (fx + 2 * KX) * 64, x, lane);
  ar = gru_mm<16>(ar, lds + (fh + 0) * 64, hp, lane);
  az = gru_mm<16>(az, lds + (fh + 16) * 64, hp, lane);
  const f16v anh = gru_mm<16>(gru_bias_v(lds, b0 + 3, lane), lds + (fh + 32) * 64, hp, lane);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float r = gru_sigmoid(ar[v]);
    const float z = gru_sigmoid(az[v]);
    const float n = gru_tanh(__builtin_fmaf(r, anh[v], anx[v]));
    const float d = dh[v];
    const float dn = d * (1.0f - z);                          // h = (1 - z) n + z hp
    const float dz = d * (hp[v] - n);
    const float dan = dn * __builtin_fmaf(-n, n, 1.0f);       // n = tanh(anx + r anh)
    danx[v] = dan;
    danh[v] = dan * r;
    dar[v] = (dan * anh[v]) * (r * (1.0f - r));
    daz[v] = dz * (z * (1.0f - z));
    dh[v] = d * z;
  }
}

// What a rollout's reverse sweep reads and writes, per lane: lanes c and c + 32 of a wave hold rollout `nn` of the env.
struct GruReverseLane {
  const float* s0;         // the env's state [6]
  const float* h0;         // the memory of all envs [E][2][32] or NULL = 0
  uint32_t env;
  const float* in;         // the rollout's inputs [H]
  float* g;                // its gradient [H] (written by the owner lane)
  const float* ckpt;       // its check-point of step 0; step k lies k * ck_step floats on (GRU_CKPT_FLOATS each)
  size_t ck_step;
  float x_t, te, scale;    // the env's targets; the horizon reduction's factor
  uint32_t lane, c;
  bool half1, owner, clip;
};

// d stage / d u: the direct control term
template <int COST>
__device__ __forceinline__ float gru_stage_u(const Params& p, float u, float x_t, float te) {
  if constexpr (COST == COST_QBGM) return stage_qbgm_grad(p, 0.0f, 1.0f, 0.0f, u, x_t, te).u;
  else return stage_default_grad(p, 0.0f, 1.0f, u, x_t, te).u;
}

// The last input: its cell is never costed, g[H - 1] is the direct control term alone.
template <int COST>
__device__ __forceinline__ void gru_reverse_last_input(const Params& p, const GruReverseLane& w) {
  const float q = w.in[p.H - 1];
  const bool clipped = w.clip && (q < p.lo || q > p.hi);
  if (w.owner) w.g[p.H - 1] = clipped ? 0.0f : w.scale * gru_stage_u<COST>(p, q, w.x_t, w.te);
}

// The steps of the reverse sweep: per control step k = H-2 .. 0 (the cell of step H-1 feeds no cost; H = 1: none), from the
// check-points of steps k (outputs, layer-1 hidden tile) and k-1 (both hidden tiles, outputs = the input features; k = 0: the
// env's memory and state): head adjoint, layer-2 cell, layer-1 cell, each layer's gates recomputed right before its adjoint.
// Row 5 of the input adjoint is d/dQ[k]; rows 0..4 are the feedback into the outputs of step k-1, which also collect the
// partials of stage k through the de-normalisation.
template <int COST>
__device__ __forceinline__ void gru_reverse_steps(const Params& p, const GruNorm& nm, const float* lds, const float* ldst,
                                                  const GruReverseLane& w) {
  const uint32_t H = p.H, lane = w.lane, c = w.c;
  const bool half1 = w.half1, owner = w.owner, clip = w.clip;
  const float x_t = w.x_t, te = w.te, scale = w.scale;
  const float* __restrict__ s0 = w.s0;
  const float* __restrict__ in = w.in;
  float* __restrict__ g = w.g;
  const size_t ck_step = w.ck_step;
  const uint32_t hoff = half1 ? 16u : 0u;                  // the lane's 16 slots inside a hidden tile
  f16v dh1, dh2;                                           // adjoints of the hidden tiles behind step k
#pragma unroll
  for (int v = 0; v < 16; ++v) { dh1[v] = 0.0f; dh2[v] = 0.0f; }
  float dfb[4] = {0.0f, 0.0f, 0.0f, 0.0f};                 // feedback: adjoint of step k's outputs through the input tile of step k + 1
  const float* ck = w.ckpt + (size_t)(H - 2) * ck_step;    // check-point of step k (H = 1: never read)
  for (uint32_t k = H - 1; k-- > 0; ck -= ck_step) {
    const float* ckp = ck - ck_step;                       // check-point of step k - 1 (k = 0: not read)
    const float q = in[k];
    const bool clipped = clip && (q < p.lo || q > p.hi);
    const float ur = clip ? clamp_(q, p.lo, p.hi) : q;
    // ---- outputs of step k = state of stage k + 1: its partials through the de-normalisation, plus the feedback
    f16v gout;
#pragma unroll
    for (int v = 0; v < 16; ++v) gout[v] = 0.0f;
    {
      const f4v o = *reinterpret_cast<const f4v*>(ck + 64);
      const float w_ang = __builtin_fmaf(o.x, nm.out_scale[0], nm.out_shift[0]);
      const float ca = __builtin_fmaf(o.y, nm.out_scale[1], nm.out_shift[1]);
      const float sa = __builtin_fmaf(o.z, nm.out_scale[2], nm.out_shift[2]);
      const float x = __builtin_fmaf(o.w, nm.out_scale[3], nm.out_shift[3]);
      const float rr = __builtin_fmaf(ca, ca, sa * sa);
      const float ir = rr > 0.0f ? __builtin_amdgcn_rsqf(rr) : 0.0f;
      const float cosang = rr > 0.0f ? ca * ir : 1.0f;     // cos(atan2(s, c)) = c / |(c, s)|, differentiated through both
      const float ir3 = ir * ir * ir;
      StageGrad sg;
      if constexpr (COST == COST_QBGM) sg = stage_qbgm_grad(p, x, cosang, w_ang, 0.0f, x_t, te);
      else sg = stage_default_grad(p, x, cosang, 0.0f, x_t, te);
      const float gc = scale * sg.cosang;
      if (!half1) {
        gout[0] = __builtin_fmaf(scale * sg.w, nm.out_scale[0], dfb[0]);
        gout[1] = __builtin_fmaf(gc * (sa * sa * ir3), nm.out_scale[1], dfb[1]);
        gout[2] = __builtin_fmaf(gc * (-(ca * sa) * ir3), nm.out_scale[2], dfb[2]);
        gout[3] = __builtin_fmaf(scale * sg.x, nm.out_scale[3], dfb[3]);
      } else {
        gout[0] = dfb[0];                                  // positionD (row 4): no stage costs it
      }
    }
    f16v dar, daz, danx, danh;
    // ---- head adjoint, then the layer-2 cell: input = the layer-1 hidden tile of step k, hidden = layer 2's of step k - 1
    {
      const f16v h1 = gru_fetch_tile(ck + hoff);
      const f16v h2p = k ? gru_fetch_tile(ckp + 32 + hoff) : gru_load_hidden(w.h0 ? w.h0 + (size_t)w.env * 64 + 32 : nullptr, lane);
      dh2 = gru_mm<4>(dh2, ldst + GT_HEAD * 64, gout, lane);
      gru_layer_reverse<16>(lds, GF_L2X, GF_L2H, 4, h1, h2p, lane, dh2, dar, daz, danx, danh);
    }
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 0) * 64, dar, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 16) * 64, daz, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L2X + 32) * 64, danx, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 0) * 64, dar, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 16) * 64, daz, lane);
    dh2 = gru_mm<16>(dh2, ldst + (GT_L2H + 32) * 64, danh, lane);
    __builtin_amdgcn_sched_barrier(0);
    // ---- the layer-1 cell: input = the step's feature tile, hidden = layer 1's of step k - 1
    {
      f16v xt;
      if (k == 0) {
        xt = gru_input_tile(nm, s0, ur, lane);
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) xt[v] = 0.0f;
        if (!half1) {
          const f4v o = *reinterpret_cast<const f4v*>(ckp + 64);
          xt[0] = o.x; xt[1] = o.y; xt[2] = o.z; xt[3] = o.w;
        } else {
          xt[0] = ckp[68];
          xt[1] = __builtin_fmaf(ur, nm.in_scale[0], nm.in_shift[0]);
        }
      }
      const f16v h1p = k ? gru_fetch_tile(ckp + hoff) : gru_load_hidden(w.h0 ? w.h0 + (size_t)w.env * 64 : nullptr, lane);
      gru_layer_reverse<4>(lds, GF_L1X, GF_L1H, 0, xt, h1p, lane, dh1, dar, daz, danx, danh);
    }
    // ---- the input adjoint (rows 0..4: feedback, row 5: d/dQ) and the hidden adjoint
    f16v dx;
#pragma unroll
    for (int v = 0; v < 16; ++v) dx[v] = 0.0f;
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 0) * 64, dar, lane);
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 16) * 64, daz, lane);
    dx = gru_mm<16>(dx, ldst + (GT_L1X + 32) * 64, danx, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 0) * 64, dar, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 16) * 64, daz, lane);
    dh1 = gru_mm<16>(dh1, ldst + (GT_L1H + 32) * 64, danh, lane);
    dfb[0] = dx[0]; dfb[1] = dx[1]; dfb[2] = dx[2]; dfb[3] = dx[3];          // (lane-half 1: [0] = row 4; [1..3] are not read)
    const float dq = __shfl(dx[1], (int)(c + 32u), 64);                       // row 5 lives on the partner lane-half
    if (owner) g[k] = clipped ? 0.0f : __builtin_fmaf(dq, nm.in_scale[0], scale * gru_stage_u<COST>(p, ur, x_t, te));
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace cpmppi
