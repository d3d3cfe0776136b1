// cpmppi_gru_rpgd.hip — the fused rpgd / gradient-tf control step over the GRU predictor (cpmppi_rpgd_step_gru, cpmppi_rpgd_gru_reserve).
//   gru_rpgd_step_kernel<COST,F16>          the whole control step, one workgroup per env: over the network what rpgd_step_kernel
//                                           (cpmppi_optim.hip) is over the ODE.
// It composes what the staged step launches one by one and shares every body with it: the rollout of gru_grad_forward_kernel
// (GruRollout and its parking, cpmppi_gru_rollout.hpp), the reverse sweep of gru_grad_reverse_kernel (cpmppi_gru_reverse.hpp), the
// Adam row, the learning-rate carry, the redraw and the permutation + shift of rpgd_step_kernel (cpmppi_rpgd.hpp), the ranking of the
// CEM steps (cpmppi_cem.hpp).  The memory is read; cpmppi_gru_advance (cpmppi_gru_seam.hip) hands it on.
#include "cpmppi_cem.hpp"           // rank_costs_at
#include "cpmppi_rpgd.hpp"          // RpgdLr, rpgd_adam_row, rpgd_fresh, rpgd_permute_shift
#include "cpmppi_gru_rollout.hpp"   // GruRollout, gru_dispatch (and cpmppi_gru16.hpp, cpmppi_gru.hpp, cpmppi_internal.hpp)
#include "cpmppi_gru_reverse.hpp"   // gru_reverse_last_input, gru_reverse_steps

using namespace cpmppi_k;

namespace {

// Plan n lives on lanes (c, c + 32) of wave n / 32, c = n % 32, as in every GRU rollout kernel; the block is one wave per 32 plans.
// The reverse sweep needs one wave per SIMD (the staged kernel takes about 350 of the 512 unified registers, this one 412 - 434), so
// a workgroup - one per env, one per compute unit - is at most four waves: N <= GRU_RPGD_ROLLOUTS.  No wave leaves before the last barrier; the lanes of a tile
// beyond N roll out plan 0 unaccounted (they write nothing).
//
// Per iteration i = 1 .. iterations:
//   forward sweep in the handle's math mode from h0[env], the check-points parked as gru_grad_forward_kernel parks them ([H][E N][72]);
//   barrier (A);  reverse sweep: d cost / d inputs into the env's gradient rows [N][H];  the owner lane's Adam row (Q, m, v in
//   place, step length from RpgdLr);  barrier (B).
// then one forward-only pass (the final costs), rank_costs_at, the outputs, rpgd_permute_shift on lane n = plan row n.
// What crosses lanes goes through global memory, and a workgroup barrier orders every hand-over:
//   (A) orders the check-points: a lane-half parks its 16 slots of each hidden tile and its share of the outputs, the reverse sweep
//       reads the outputs of both halves, and the lanes beyond N read the check-points of plan 0, which wave 0 parked;
//   (B) orders the plan rows: the owner lane (lane-half 0) wrote Q[n], its partner and the lanes beyond N read it in the next
//       forward sweep; it also keeps the next sweep's check-points from overtaking this reverse sweep's reads.
//   The gradient row is written and read by the owner lane alone (program order).  The barriers of the ranking order the last
//   Adam rows, which (B) already ordered, against the permutation, which reads other lanes' rows.
// Dynamic LDS: f32 image | transposed image | FAST: the f16 rollout image | key[128] | order[128] - all resident for the whole
// step (the register budget already limits a compute unit to this one workgroup, so the LDS costs no occupancy).
constexpr int GRU_RPGD_ROLLOUTS = 128;
constexpr int GRU_RPGD_BLOCK = 2 * GRU_RPGD_ROLLOUTS;
template <bool F16>
constexpr size_t GRU_RPGD_LDS = ((size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS) * sizeof(float) + (F16 ? (size_t)G16_IMAGE_BYTES : 0) +
                                2 * (size_t)GRU_RPGD_ROLLOUTS * sizeof(uint32_t);
// (the size does not depend on the horizon: it holds at CPMPPI_MAX_HORIZON as at every other)
static_assert(GRU_RPGD_LDS<true> <= SAMPLER_LDS_MAX && GRU_RPGD_LDS<false> <= SAMPLER_LDS_MAX,
              "the three images and the ranking keys stay under the LDS opt-in (147 488 B, FAST) at every allowed horizon");
static_assert(((size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS) * sizeof(float) % 16 == 0, "the f16 image is read 16 bytes at a time");

struct GruRpgdPtrs {
  const float* s0; const float* x_t; const float* te;
  const float* h0;        // [E,2,32] or NULL = 0
  float* Q; float* m; float* v;
  float* ckpt;            // [H][rows][GRU_CKPT_FLOATS]
  float* grad;            // [E][N][H]
  size_t rows;            // E N of this launch
  const unsigned long long* count_dev;
  unsigned long long count, seed, draw_offset;
  uint32_t iterations, adam_iteration, keep_k, resamp_per, shift, uniform, env_offset;
  float lr, beta1, beta2, eps, gradmax_clip, sample_mean, uniform_lo, uniform_hi;
  float* Q_out; float* S_out; float* plan_out; uint32_t* order_out;
};

template <int COST, bool F16>
__global__ __launch_bounds__(GRU_RPGD_BLOCK, 1) void gru_rpgd_step_kernel(const Params p, const GruRpgdPtrs a, const GruNorm nm,
                                                                         const float* __restrict__ image,
                                                                         const float* __restrict__ image_t,
                                                                         const float* __restrict__ image16) {
  extern __shared__ float lds[];                           // the f32 image first: the reverse sweep's gates, PRECISE: the rollout's too
  float* ldst = lds + GRU_IMAGE_FLOATS;
  float* lds16 = ldst + GRU_T_IMAGE_FLOATS;
  const uint32_t tid = threadIdx.x, Nt = blockDim.x, env = blockIdx.x, N = p.N, H = p.H;
  uint32_t* key = reinterpret_cast<uint32_t*>(lds16 + (F16 ? G16_IMAGE_BYTES / 4 : 0));
  uint32_t* order = key + GRU_RPGD_ROLLOUTS;
  for (uint32_t i = tid; i < (uint32_t)GRU_IMAGE_FLOATS; i += Nt) lds[i] = image[i];
  for (uint32_t i = tid; i < (uint32_t)GRU_T_IMAGE_FLOATS; i += Nt) ldst[i] = image_t[i];
  if constexpr (F16)
    for (uint32_t i = tid; i < (uint32_t)(G16_IMAGE_BYTES / 4); i += Nt) lds16[i] = image16[i];
  const float* ldsf = F16 ? lds16 : lds;                   // the rollout's image
  const uint32_t lane = tid & 63u, c = lane & 31u;
  const uint32_t n = (tid >> 6) * 32 + c;                  // the plan of this lane pair
  const bool live = n < N, half1 = lane >= 32, owner = !half1 && live;
  const uint32_t nn = live ? n : 0;
  const uint64_t cnt = a.count_dev ? (uint64_t)*a.count_dev : (uint64_t)a.count;
  const uint64_t it0 = a.count_dev ? cnt * a.iterations : (uint64_t)a.adam_iteration;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* s0 = a.s0 + (size_t)env * 6;
  const float* h1src = a.h0 ? a.h0 + (size_t)env * 64 : nullptr;
  const size_t row = ((size_t)env * N + nn) * H;
  const float* in = a.Q + row;
  const size_t ck_step = a.rows * GRU_CKPT_FLOATS;
  GruReverseLane w;
  w.s0 = s0; w.h0 = a.h0; w.env = env; w.in = in; w.g = a.grad + row;
  w.ckpt = a.ckpt + ((size_t)env * N + nn) * GRU_CKPT_FLOATS;
  w.ck_step = ck_step;
  w.x_t = x_t; w.te = te;
  w.scale = (p.horizon_reduce == CPMPPI_REDUCE_SUM) ? 1.0f : 1.0f / (float)(H + 1);
  w.lane = lane; w.c = c; w.half1 = half1; w.owner = owner;
  w.clip = p.control_mode == CPMPPI_CONTROL_CLIP;
  GruStamps none;
  RpgdLr lr(a.beta1, a.beta2, it0);
  float S = 0.0f;
  __syncthreads();                                         // the images stand
  for (uint32_t i = 1; i <= a.iterations + 1; ++i) {
    const bool descend = i <= a.iterations;                // the last pass is the final cost: forward only, nothing parked
    {
      GruRollout ro;
      gru_rollout_init<F16>(ro, ldsf, s0, lane, h1src, h1src ? h1src + 32 : nullptr);
      float* ck = a.ckpt + ((size_t)env * N + nn) * GRU_CKPT_FLOATS;       // the plan's check-point of step 0
      float u_next = in[0];
      for (uint32_t k = 0; k < H; ++k) {
        const float ur = u_next;
        if (k + 1 < H) u_next = in[k + 1];                 // in flight during this step's cell
        gru_rollout_step<COST, F16>(ro, ldsf, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
        if (descend && k + 1 < H && live) gru_rollout_park<F16>(ro, ck, half1);   // rows >= N are never written
        ck += ck_step;
      }
      S = gru_rollout_total<COST>(ro, x_t, p);
    }
    if (!descend) break;                                   // (block-uniform)
    __syncthreads();                                       // (A) every check-point stands
    gru_reverse_last_input<COST>(p, w);
    gru_reverse_steps<COST>(p, nm, lds, ldst, w);
    const float lr_t = lr.next(a.lr, a.beta1, a.beta2);
    if (owner) rpgd_adam_row(H, a.Q + row, a.m + row, a.v + row, w.g, 1u, lr_t, a.beta1, a.beta2, a.eps, a.gradmax_clip, p.lo, p.hi);
    __syncthreads();                                       // (B) every plan row stands; the check-points are read
  }
  if (a.S_out && owner) a.S_out[(size_t)env * N + n] = S;
  rank_costs_at(key, order, n, S, owner, N, env, a.order_out, true);
  const float* best = a.Q + ((size_t)env * N + order[0]) * H;
  if (tid == 0) a.Q_out[env] = best[0];
  if (a.plan_out) for (uint32_t k = tid; k < H; k += Nt) a.plan_out[(size_t)env * H + k] = best[k];
  // from here lane tid is plan row tid (the block holds at least N lanes), as in rpgd_step_kernel
  rpgd_permute_shift(p, a, env, tid, tid < N, cnt, order);
}

inline size_t gru_ckpt_floats(const cpmppi_handle* h) { return (size_t)h->cfg.H * GRU_CKPT_FLOATS * (size_t)h->cfg.E * h->cfg.N; }
// the staged adjoint's check-points (cpmppi_rollout_cost_grad_gru's workspace, of the handle's largest launch), the gradient behind them
inline size_t gru_rpgd_floats(const cpmppi_handle* h) { return gru_ckpt_floats(h) + (size_t)h->cfg.H * h->cfg.E * h->cfg.N; }

// what both entry points refuse about the handle
int gru_rpgd_check_handle(cpmppi_handle* h, const char* who) {
  if (h->cfg.N > (uint32_t)GRU_RPGD_ROLLOUTS)
    return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": one workgroup per env holds at most " + std::to_string(GRU_RPGD_ROLLOUTS) +
                                           " plans (N = " + std::to_string(h->cfg.N) + ")");
  return CPMPPI_OK;
}

}  // namespace

void allow_large_lds_gru_rpgd() {
  allow_large_lds(&gru_rpgd_step_kernel<COST_QBGM, true>);      // two or three images in LDS: beyond the default 64 KB
  allow_large_lds(&gru_rpgd_step_kernel<COST_DEFAULT, true>);
  allow_large_lds(&gru_rpgd_step_kernel<COST_QBGM, false>);
  allow_large_lds(&gru_rpgd_step_kernel<COST_DEFAULT, false>);
}

extern "C" {

int cpmppi_rpgd_gru_reserve(cpmppi_handle* h, uint32_t E) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_rpgd_gru_reserve";
  if (const int rc = gru_refusal(h, who, E != 0 && E <= h->cfg.E, "bad argument (0 < E <= config.E)", true, "", true)) return rc;
  if (const int rc = gru_rpgd_check_handle(h, who)) return rc;
  CPMPPI_ON_DEVICE(h);
  return grow_workspace(h, h->gru_grad_ws, h->gru_grad_ws_floats, gru_rpgd_floats(h));
}

// the whole rpgd / gradient-tf control step over the network: gru_rpgd_step_kernel, then the step counter
int cpmppi_rpgd_step_gru(cpmppi_handle* h, const cpmppi_rpgd_gru_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_rpgd_step_gru";
  const std::string w = std::string(who) + ": ";
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, w + "null argument block");
  if (const int rc = refuse_tuning_rows(h, who)) return rc;
  if (const int rc = gru_refusal(h, who, a->E != 0 && a->E <= h->cfg.E, "bad argument (0 < E <= config.E)",
                                 a->s0 && a->target_position && a->target_equilibrium && a->Q && a->m && a->v && a->Q_out,
                                 "null pointer (s0, target_position, target_equilibrium, Q, m, v and Q_out are required)", true))
    return rc;
  for (const void* ptr : {(const void*)a->s0, (const void*)a->target_position, (const void*)a->target_equilibrium, (const void*)a->h0,
                          (const void*)a->Q, (const void*)a->m, (const void*)a->v, (const void*)a->Q_out, (const void*)a->S_out,
                          (const void*)a->plan_out, (const void*)a->order_out})
    if (misaligned(ptr)) return fail(h, CPMPPI_ERR_BAD_ARG, w + "misaligned pointer");
  if (reinterpret_cast<uintptr_t>(a->count_dev) & 7u) return fail(h, CPMPPI_ERR_BAD_ARG, w + "misaligned pointer (count_dev: 8 bytes)");
  if (a->iterations == 0) return fail(h, CPMPPI_ERR_BAD_ARG, w + "iterations must be > 0");
  if (a->keep_k == 0 || a->keep_k > h->cfg.N) return fail(h, CPMPPI_ERR_BAD_ARG, w + "bad argument (0 < keep_k <= N)");
  if (a->shift > h->cfg.H) return fail(h, CPMPPI_ERR_BAD_ARG, w + "shift exceeds the horizon");
  if (a->distribution > CPMPPI_RPGD_UNIFORM) return fail(h, CPMPPI_ERR_BAD_ARG, w + "unknown distribution");
  if (const int rc = gru_rpgd_check_handle(h, who)) return rc;
  CPMPPI_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  if (h->gru_grad_ws_floats < gru_rpgd_floats(h)) {
    if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_rpgd_gru_reserve")) return rc;
    if (const int rc = grow_workspace(h, h->gru_grad_ws, h->gru_grad_ws_floats, gru_rpgd_floats(h))) return rc;
  }
  GruRpgdPtrs p{};
  p.s0 = a->s0; p.x_t = a->target_position; p.te = a->target_equilibrium; p.h0 = a->h0;
  p.Q = a->Q; p.m = a->m; p.v = a->v;
  p.ckpt = h->gru_grad_ws; p.grad = h->gru_grad_ws + gru_ckpt_floats(h); p.rows = (size_t)a->E * h->cfg.N;
  p.count_dev = (const unsigned long long*)a->count_dev;
  p.count = a->count; p.seed = a->seed; p.draw_offset = a->draw_offset;
  p.iterations = a->iterations; p.adam_iteration = a->adam_iteration; p.keep_k = a->keep_k; p.resamp_per = a->resamp_per;
  p.shift = a->shift; p.uniform = a->distribution == CPMPPI_RPGD_UNIFORM; p.env_offset = a->env_offset;
  p.lr = a->learning_rate; p.beta1 = a->beta1; p.beta2 = a->beta2; p.eps = a->epsilon; p.gradmax_clip = a->gradmax_clip;
  p.sample_mean = a->sample_mean; p.uniform_lo = a->uniform_lo; p.uniform_hi = a->uniform_hi;
  p.Q_out = a->Q_out; p.S_out = a->S_out; p.plan_out = a->plan_out; p.order_out = a->order_out;
  const uint32_t threads = 64u * ((h->cfg.N + 31u) / 32u);     // one wave per 32 plans: <= GRU_RPGD_BLOCK
  gru_dispatch(h, [&](auto cost, auto f16) {
    constexpr int COST = decltype(cost)::value; constexpr bool F16 = decltype(f16)::value;
    hipLaunchKernelGGL((gru_rpgd_step_kernel<COST, F16>), dim3(a->E), dim3(threads), GRU_RPGD_LDS<F16>, s, h->prm, p, h->gru_norm,
                       (const float*)h->gru_image, (const float*)h->gru_t_image, (const float*)h->gru16_image);
  });
  CPMPPI_HIP(h, hipGetLastError());
  if (a->count_dev) launch_step_count((unsigned long long*)a->count_dev, s);
  return launched(h);
}

}  // extern "C"
