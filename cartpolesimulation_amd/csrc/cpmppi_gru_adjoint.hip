// cpmppi_gru_adjoint.hip — the reverse sweep of cpmppi_rollout_cost_grad_gru (the forward sweep is cpmppi_gru.hip's gru_grad_forward_kernel).
//   gru_grad_reverse_kernel<COST>           the reverse sweep through head, layer 2 and layer 1 (exact f32 MFMA on a transposed weights
//                                           image): d cost / d inputs of GIVEN plans - the building block of gradient, rpgd and the
//                                           CEM + gradient hybrids over the GRU (gru_adjoint=True).  Launched by launch_gru_grad_reverse.
#include "cpmppi_gru_reverse.hpp"   // the sweep itself, shared with cpmppi_gru_rpgd.hip (and cpmppi_gru.hpp, cpmppi_grad.hpp, cpmppi_internal.hpp)

using namespace cpmppi_k;

namespace {

constexpr size_t GRU_GRAD_REVERSE_LDS = ((size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS) * sizeof(float);   // 98 208 B: opt-in

// Reverse sweep, exact-f32 MFMA in both math modes: gru_reverse_last_input, then gru_reverse_steps (cpmppi_gru_reverse.hpp) for the
// wave's 32 rollouts.  LDS: the forward f32 image (gates) and the transposed one.  A column beyond N repeats the env's rollout 0
// and is never written.
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
  GruReverseLane w;
  w.s0 = a.s0 + (size_t)env * 6;
  w.h0 = a.h0; w.env = env;
  w.in = a.inputs + ((size_t)env * p.N + nn) * H;
  w.g = a.grad + ((size_t)env * p.N + nn) * H;
  w.ckpt = a.ckpt + ((size_t)env * p.N + nn) * GRU_CKPT_FLOATS;
  w.ck_step = a.rows * GRU_CKPT_FLOATS;
  w.x_t = a.x_t[env]; w.te = a.te[env];
  w.scale = (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? 1.0f : 1.0f / (float)(p.H + 1);
  w.lane = lane; w.c = c; w.half1 = half1; w.owner = owner;
  w.clip = p.control_mode == CPMPPI_CONTROL_CLIP;
  gru_reverse_last_input<COST>(p, w);
  if (H < 2) return;
  gru_reverse_steps<COST>(p, nm, lds, ldst, w);
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
