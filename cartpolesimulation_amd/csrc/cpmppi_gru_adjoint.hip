// cpmppi_gru_adjoint.hip — the reverse sweep of cpmppi_rollout_cost_grad_gru (the forward sweep is cpmppi_gru.hip's gru_grad_forward_kernel).
//   gru_grad_reverse_kernel<COST>           the reverse sweep through head, layer 2 and layer 1 (exact f32 MFMA on a transposed weights
//                                           image): d cost / d inputs of GIVEN plans - the building block of gradient, rpgd and the
//                                           CEM + gradient hybrids over the GRU (gru_adjoint=True).  Launched by launch_gru_grad_reverse.
#include "cpmppi_gru.hpp"        // (and cpmppi_internal.hpp)
#include "cpmppi_grad.hpp"       // (stage_qbgm_grad, stage_default_grad)

using namespace cpmppi_k;

namespace {

constexpr size_t GRU_GRAD_REVERSE_LDS = ((size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS) * sizeof(float);   // 98 208 B: opt-in

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

// Reverse sweep, exact-f32 MFMA in both math modes.  Per control step k = H-2 .. 0 (the cell of step H-1 feeds no cost), from the
// check-points of steps k (outputs, layer-1 hidden tile) and k-1 (both hidden tiles, outputs = the input features; k = 0: the
// env's memory and state): head adjoint, layer-2 cell, layer-1 cell, each layer's gates recomputed right before its adjoint.
// Row 5 of the input adjoint is d/dQ[k]; rows 0..4 are the feedback into the outputs of step k-1, which also collect the
// partials of stage k through the de-normalisation.  LDS: the forward f32 image (gates) and the transposed one.  A column
// beyond N repeats the env's rollout 0 and is never written.
template <int COST>
__global__ __launch_bounds__(BLOCK, 1) void gru_grad_reverse_kernel(const Params p, const GruGradPtrs a, const GruNorm nm,
                                                                    const float* __restrict__ image,
                                                                    const float* __restrict__ image_t) {
  extern __shared__ float lds[];                           // forward f32 image, then the transposed image
  float* ldst = lds + GRU_IMAGE_FLOATS;
  for (int i = threadIdx.x; i < GRU_T_IMAGE_FLOATS; i += BLOCK) ldst[i] = image_t[i];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);            // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool live = n < p.N, half1 = lane >= 32, owner = !half1 && live;
  const uint32_t nn = live ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  float* __restrict__ g = a.grad + ((size_t)env * p.N + nn) * H;
  const size_t ck_step = a.rows * GRU_CKPT_FLOATS;
  const uint32_t hoff = half1 ? 16u : 0u;                  // the lane's 16 slots inside a hidden tile
  const float scale = (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? 1.0f : 1.0f / (float)(p.H + 1);
  const bool clip = p.control_mode == CPMPPI_CONTROL_CLIP;
  auto stage_u = [&](float u) __attribute__((always_inline)) -> float {      // d stage / d u: the direct control term
    if constexpr (COST == COST_QBGM) return stage_qbgm_grad(p, 0.0f, 1.0f, 0.0f, u, x_t, te).u;
    else return stage_default_grad(p, 0.0f, 1.0f, u, x_t, te).u;
  };
  {                                                        // the last input: its cell is never costed
    const float q = in[H - 1];
    const bool clipped = clip && (q < p.lo || q > p.hi);
    if (owner) g[H - 1] = clipped ? 0.0f : scale * stage_u(q);
  }
  if (H < 2) return;

  f16v dh1, dh2;                                           // adjoints of the hidden tiles behind step k
#pragma unroll
  for (int v = 0; v < 16; ++v) { dh1[v] = 0.0f; dh2[v] = 0.0f; }
  float dfb[4] = {0.0f, 0.0f, 0.0f, 0.0f};                 // feedback: adjoint of step k's outputs through the input tile of step k + 1
  const float* ck = a.ckpt + ((size_t)env * p.N + nn) * GRU_CKPT_FLOATS + (size_t)(H - 2) * ck_step;   // check-point of step k
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
      const f16v h2p = k ? gru_fetch_tile(ckp + 32 + hoff) : gru_load_hidden(a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr, lane);
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
      const f16v h1p = k ? gru_fetch_tile(ckp + hoff) : gru_load_hidden(a.h0 ? a.h0 + (size_t)env * 64 : nullptr, lane);
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
    if (owner) g[k] = clipped ? 0.0f : __builtin_fmaf(dq, nm.in_scale[0], scale * stage_u(ur));
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace

void launch_gru_grad_reverse(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* x_t, const float* te,
                             const float* h0, float* grad, hipStream_t s) {
  const GruGradPtrs a = gru_grad_ptrs(h, E, s0, inputs, x_t, te, h0, nullptr, grad);
  const auto kernel = h->prm.cost_id == CPMPPI_COST_QBGM ? &gru_grad_reverse_kernel<COST_QBGM> : &gru_grad_reverse_kernel<COST_DEFAULT>;
  hipLaunchKernelGGL(kernel, dim3(E * a.nb), dim3(BLOCK), GRU_GRAD_REVERSE_LDS, s, h->prm, a, h->gru_norm, (const float*)h->gru_image,
                     (const float*)h->gru_t_image);
}

void allow_large_lds_gru_adjoint() {
  allow_large_lds(&gru_grad_reverse_kernel<COST_QBGM>);      // both images in LDS: beyond the default 64 KB
  allow_large_lds(&gru_grad_reverse_kernel<COST_DEFAULT>);
}
