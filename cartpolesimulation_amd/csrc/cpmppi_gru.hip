// cpmppi_gru.hip — the GRU predictor (BASELINE configs[4]) inside the optimizers: the kernels that share one rollout, GruRollout.
// The cell and its mapping onto the matrix cores: cpmppi_gru.hpp (exact f32 MFMA chains) and cpmppi_gru16.hpp (f16 split).
// The model upload is cpmppi_gru_model.hip, the exact-cell seams are cpmppi_gru_seam.hip, the reverse sweep is cpmppi_gru_adjoint.hip.
//   gru_rollout_cost_kernel<COST,NOISE,F16> the fused MPPI step with the GRU predictor: same contract as rollout_cost_kernel
//                                           (plugin costs); launched by step_impl through launch_gru_rollout.
//   gru_cost_only_kernel<COST,F16>          costs of GIVEN input plans under the GRU predictor, nothing of the MPPI update: the
//                                           building block of the sampling optimizers (cem, cem-gmm, random-action).
//   gru_grad_forward_kernel<COST,F16>       the cost-only rollout that also parks, per control step, what the reverse sweep
//                                           (gru_grad_reverse_kernel, cpmppi_gru_adjoint.hip) needs.
//   gru_cem_step_kernel<COST,F16>           the whole cem control step over the network, one workgroup per env: the cost-only
//                                           rollout between cem_step_kernel's sampler, ranking and refit (cpmppi_cem.hpp).
// They share one rollout (GruRollout: gru_rollout_init, gru_rollout_step, gru_rollout_total - cpmppi_gru_rollout.hpp, which the fused
// rpgd step of cpmppi_gru_rpgd.hip includes as well) and differ in where a step's input
// comes from and in what becomes of the costs.  Entry points: cpmppi_rollout_cost_gru, cpmppi_rollout_cost_grad_gru, cpmppi_cem_step_gru;
// -DCPMPPI_GRU_STAMPS: cpmppi_debug_gru_stamps (the kernels that write g_gru_stamp_sum are this unit's).
#include "cpmppi_philox.hpp"
#include "cpmppi_wave.hpp"
#include "cpmppi_cem.hpp"        // the sampler's statement, the ranking and the refit of the fused CEM step
#include "cpmppi_gru_rollout.hpp"   // GruRollout, gru_dispatch (and cpmppi_cost.hpp, cpmppi_gru16.hpp, cpmppi_gru.hpp, cpmppi_internal.hpp)

using namespace cpmppi_k;

namespace {

// development aid (-DCPMPPI_GRU_STAMPS): the stamp sums the fused MPPI kernel publishes (GruStamps: cpmppi_gru_rollout.hpp)
#ifdef CPMPPI_GRU_STAMPS
__device__ unsigned long long g_gru_stamp_sum[8];
#endif

// Fused MPPI step with the GRU predictor: same contract as rollout_cost_kernel (plugin costs), h0[E,2,32] or NULL.
template <int COST, int NOISE, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_rollout_cost_kernel(const Params p, const StepPtrs a, const GruNorm nm,
                                                                 const float* __restrict__ image,
                                                                 const float* __restrict__ h0) {
  extern __shared__ float lds[];                           // GRU image, then [WAVES][W] weighted sums
  __shared__ float red[2 * WAVES];
  constexpr int IMAGE_FLOATS = GRU_ROLLOUT_IMAGE_FLOATS<F16>;
  gru_load_image(lds, image, IMAGE_FLOATS);
  float* bsum = lds + IMAGE_FLOATS;
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  const uint32_t n = row0 + c;
  const bool owner = lane < 32 && n < p.N;                 // the lane that accounts for rollout n
  const uint32_t nn = n < p.N ? n : 0;
  const uint32_t H = p.H;
  const uint64_t step_offset = a.offset_dev ? (uint64_t)*a.offset_dev : a.offset;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ un = a.u_nom + (size_t)env * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, h0 ? h0 + (size_t)env * 64 : nullptr, h0 ? h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;

  auto knot = [&](uint32_t j) __attribute__((always_inline)) -> float {
    if constexpr (NOISE == NOISE_KNOTS) return a.noise[((size_t)env * p.N + nn) * p.P + j];
    else return philox_knot(a.seed, step_offset, a.env_offset + env, nn, j, p.sigma);
  };
  float z_lo = 0.0f, z_hi = 0.0f;
  if constexpr (NOISE != NOISE_DELTA_U) { z_lo = knot(0); z_hi = knot(1); }
  uint32_t ii = 0, j = 0;
  float corr = 0.0f;
  GruStamps stamps;
#ifdef CPMPPI_GRU_STAMPS
  stamps.prev = __builtin_amdgcn_s_memtime();
#endif
  for (uint32_t k = 0; k < H; ++k) {
    float du;
    if constexpr (NOISE == NOISE_DELTA_U) du = a.noise[((size_t)env * p.N + nn) * H + k];
    else if constexpr (F16 && NOISE == NOISE_PHILOX)      // FAST + own noise: one float32 FMA, as the ODE kernel and the sampler
      du = interp_from_slope32(knot_slope32(z_lo, z_hi, 1.0f / (float)p.period), z_lo, ii);
    else du = interp_knots(z_lo, z_hi, ii, p.period);
    const float uk = shifted_nominal(p, un, k);
    float ur = uk + du;
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, stamps, [&](float u) __attribute__((always_inline)) {
      corr += mppi_correction<float>(p, p.correction_u == CPMPPI_CORRECTION_U_RUN ? u : uk, du);
    });
    if constexpr (NOISE != NOISE_DELTA_U) {
      if (++ii == p.period) {
        ii = 0; ++j;
        z_lo = z_hi;
        if (j + 1 < p.P) z_hi = knot(j + 1);
      }
    }
  }
#ifdef CPMPPI_GRU_STAMPS
  if (lane == 0)
    for (int i = 0; i < 6; ++i) atomicAdd(&g_gru_stamp_sum[i], stamps.acc[i]);
  if (lane == 0) atomicAdd(&g_gru_stamp_sum[6], 1ull);
#endif
  const float S_total = gru_rollout_total<COST>(ro, x_t, p) + corr;
  if (a.S_out && owner) a.S_out[(size_t)env * p.N + n] = S_total;

  const float m_w = wave_min(owner ? S_total : INFINITY);
  if (lane == 0) red[wave] = m_w;
  __syncthreads();
  float m_b = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) m_b = fminf(m_b, red[w]);
  const float e = owner ? expf((-1.0f / p.LBD) * (S_total - m_b)) : 0.0f;
  const float a_w = wave_sum(e);
  if (lane == 0) red[WAVES + wave] = a_w;
  const uint32_t W = a.W;
  float* __restrict__ my_bsum = bsum + wave * W;
  if constexpr (NOISE == NOISE_PHILOX) {
    for (uint32_t jj = 0; jj < W; ++jj) {
      const float v = wave_sum(e * philox_knot(a.seed, step_offset, a.env_offset + env, nn, jj, p.sigma));
      if (lane == 0) my_bsum[jj] = v;
    }
  } else {
    const float* __restrict__ src = a.noise + ((size_t)env * p.N + row0) * W;
    const uint32_t rows = (row0 < p.N) ? ((p.N - row0 < 32u) ? p.N - row0 : 32u) : 0u;
    for (uint32_t c0 = 0; c0 < W; c0 += 64) {
      const uint32_t col = c0 + lane;
      float acc = 0.0f;
      const float* __restrict__ colp = src + (col < W ? col : 0u);
      uint32_t r = 0;
      for (; r + 8 <= rows; r += 8) {                      // eight independent row loads in flight (latency-bound pass)
        float xr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xr[u] = colp[(size_t)(r + u) * W];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), r + u)), xr[u], acc);
      }
      for (; r < rows; ++r)
        acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), r)), colp[(size_t)r * W], acc);
      if (col < W) my_bsum[col] = acc;
    }
  }
  __syncthreads();
  float* __restrict__ outp = a.partial + ((size_t)env * a.nb + blk) * (2 + W);
  if (tid == 0) {
    float a_b = red[WAVES];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) a_b += red[WAVES + w];
    outp[0] = m_b;
    outp[1] = a_b;
  }
  for (uint32_t cc = tid; cc < W; cc += BLOCK) {
    float v = bsum[cc];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += bsum[w * W + cc];
    outp[2 + cc] = v;
  }
}

// Cost-only rollout with the GRU predictor: S[env][n] = get_trajectory_cost(predict_core_GRU(s0[env], inputs[env][n]), inputs[env][n]).
// What gru_rollout_cost_kernel<COST, NOISE_DELTA_U, F16> computes for a zero nominal sequence, no shift and cc_weight = 0 - same
// tile mapping (32 rollouts per wave, GRU_ROLLOUTS_PER_BLOCK per workgroup, grid E x nb) and the same GruRollout set-up, step and
// epilogue - without anything that serves the MPPI update: no block minimum, no weights, no weighted sums of the noise, no
// partials.  Dynamic LDS holds the weights image only, and after its load no wave depends on another: a wave whose 32 rollouts
// all lie beyond N leaves at once, and there is no barrier behind the one of the image load.
// The lane's next input does not depend on the state: it is loaded one control step ahead, off the recurrent chain.
template <int COST, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_cost_only_kernel(const Params p, const GruCostPtrs a, const GruNorm nm,
                                                                              const float* __restrict__ image) {
  extern __shared__ float lds[];                           // GRU image only
  gru_load_image(lds, image, GRU_ROLLOUT_IMAGE_FLOATS<F16>);   // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool owner = lane < 32 && n < p.N;                 // the lane that accounts for rollout n
  const uint32_t nn = n < p.N ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, a.h0 ? a.h0 + (size_t)env * 64 : nullptr, a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;
  GruStamps none;
  float u_next = in[0];
  for (uint32_t k = 0; k < H; ++k) {
    const float ur = u_next;
    if (k + 1 < H) u_next = in[k + 1];                     // in flight during this step's cell
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
  }
  const float S_total = gru_rollout_total<COST>(ro, x_t, p);
  if (owner) a.S_out[(size_t)env * p.N + n] = S_total;
}

// Forward sweep of cpmppi_rollout_cost_grad_gru: gru_cost_only_kernel (same set-up, step and epilogue, in the handle's math mode) that
// parks, after every control step but the last, what the reverse sweep (gru_grad_reverse_kernel, cpmppi_gru_adjoint.hip) starts from -
// the last step's cell produces a state that no stage costs.  Two launches rather than one kernel that swaps its LDS image between the
// sweeps: each keeps the cost-only kernel's shape, and the sweeps meet in global memory either way.
// (A copy of the kernel above and not one body under `if constexpr`: behind two wrappers the hidden-state loads of the prologue
// compile to other code, and the FAST cost-only launch measured 0.4 - 0.5 % slower at its three smallest shapes: profiles/HISTORY.md, r15.)
template <int COST, bool F16>
__global__ __launch_bounds__(BLOCK, GRU_MIN_WAVES) void gru_grad_forward_kernel(const Params p, const GruGradPtrs a, const GruNorm nm,
                                                                                 const float* __restrict__ image) {
  extern __shared__ float lds[];                           // GRU image only
  gru_load_image(lds, image, GRU_ROLLOUT_IMAGE_FLOATS<F16>);   // the kernel's only barrier
  const uint32_t env = blockIdx.x / a.nb, blk = blockIdx.x % a.nb;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, c = lane & 31u;
  const uint32_t row0 = blk * GRU_ROLLOUTS_PER_BLOCK + wave * 32;
  if (row0 >= p.N) return;                                 // (wave-uniform) a tile without a rollout
  const uint32_t n = row0 + c;
  const bool live = n < p.N, owner = lane < 32 && live;
  const uint32_t nn = live ? n : 0;
  const uint32_t H = p.H;
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* __restrict__ in = a.inputs + ((size_t)env * p.N + nn) * H;
  GruRollout ro;
  gru_rollout_init<F16>(ro, lds, s0, lane, a.h0 ? a.h0 + (size_t)env * 64 : nullptr, a.h0 ? a.h0 + (size_t)env * 64 + 32 : nullptr);
  const bool half1 = lane >= 32;
  float* ck = a.ckpt + ((size_t)env * p.N + nn) * GRU_CKPT_FLOATS;        // the rollout's check-point of step 0
  const size_t ck_step = a.rows * GRU_CKPT_FLOATS;
  GruStamps none;
  float u_next = in[0];
  for (uint32_t k = 0; k < H; ++k) {
    const float ur = u_next;
    if (k + 1 < H) u_next = in[k + 1];                     // in flight during this step's cell
    gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
    if (k + 1 < H && live) gru_rollout_park<F16>(ro, ck, half1);   // rows >= N are never written
    ck += ck_step;
  }
  const float S_total = gru_rollout_total<COST>(ro, x_t, p);
  if (a.S_out && owner) a.S_out[(size_t)env * p.N + n] = S_total;
}

// The fused CEM control step over the GRU predictor (cpmppi_cem_step_gru): what cem_step_kernel (cpmppi_optim.hip) is over the
// ODE, with gru_cost_only_kernel's rollout in the place of the forward sweep.  One workgroup = one env, all outer iterations in
// the one launch; the block is one wave per 32 samples (N <= GRU_CEM_ROLLOUTS: at most 8 waves, two per SIMD - the register
// budget GRU_MIN_WAVES compiles these bodies for), so every wave has a rollout and the whole population runs in one pass.
// Per iteration: lane n < N draws row n (cem_sample_row: cem_sample_kernel's statement) into the env's workspace column n,
// lane-contiguous as cem_step_kernel's; the block meets; rollout n runs on lanes (c, c + 32) of wave n / 32 from h0[env] - the
// calls gru_cost_only_kernel makes, the next input loaded one control step ahead - ; the owner lanes rank the costs
// (rank_costs_at: cem_update_kernel's stable order, the keys in LDS); lanes k < H refit time-step k (cem_refit_column).  The
// barrier that opens an iteration closes the refit of the one before.  Mean and stdev live in LDS for the whole step.
// Dynamic LDS: the weights image | key[256] | order[256] | mean[H] | stdev[H].  Unlike the cost-only kernel this one has barriers
// behind the image load: no wave leaves before the end, and the lanes of a wave's tile beyond N roll out sample 0 unaccounted.
constexpr int GRU_CEM_ROLLOUTS = 256;
constexpr int GRU_CEM_BLOCK = 2 * GRU_CEM_ROLLOUTS;
struct GruCemPtrs {
  const float* s0; const float* x_t; const float* te;
  const float* h0;                 // [E,2,32] or NULL = 0
  float* mean; float* stdev;       // [E][H], in place
  float* samples;                  // [E][H][stride]
  const unsigned long long* count_dev;
  unsigned long long seed, offset;
  uint32_t iterations, best_k, shift, env_offset, stride;
  float stdev_min, mean_fill, stdev_fill;
  float* Q_out; float* S_out; float* plan_out; float* samples_out; uint32_t* order_out;
};

template <int COST, bool F16>
__global__ __launch_bounds__(GRU_CEM_BLOCK, GRU_MIN_WAVES) void gru_cem_step_kernel(const Params p, const GruCemPtrs a, const GruNorm nm,
                                                                                     const float* __restrict__ image) {
  extern __shared__ float lds[];
  constexpr int IMAGE_FLOATS = GRU_ROLLOUT_IMAGE_FLOATS<F16>;
  const uint32_t tid = threadIdx.x, Nt = blockDim.x, env = blockIdx.x, N = p.N, H = p.H, Nb = a.stride;
  uint32_t* key = reinterpret_cast<uint32_t*>(lds + IMAGE_FLOATS);
  uint32_t* order = key + GRU_CEM_ROLLOUTS;
  float* mu = reinterpret_cast<float*>(order + GRU_CEM_ROLLOUTS);
  float* sd = mu + H;
  for (uint32_t i = tid; i < (uint32_t)IMAGE_FLOATS; i += Nt) lds[i] = image[i];
  for (uint32_t k = tid; k < H; k += Nt) { mu[k] = a.mean[(size_t)env * H + k]; sd[k] = a.stdev[(size_t)env * H + k]; }
  const uint32_t lane = tid & 63u, c = lane & 31u;
  const uint32_t n = (tid >> 6) * 32 + c;                  // the rollout of this lane pair
  const bool owner = lane < 32 && n < N;                   // the lane that accounts for rollout n
  const uint32_t nn = n < N ? n : 0;
  const bool half1 = lane >= 32;
  const uint64_t base = a.offset + (a.count_dev ? (uint64_t)*a.count_dev * a.iterations : 0ull);
  const float x_t = a.x_t[env], te = a.te[env];
  const float* __restrict__ s0 = a.s0 + (size_t)env * 6;
  const float* h1src = a.h0 ? a.h0 + (size_t)env * 64 : nullptr;
  float* cols = a.samples + (size_t)env * H * Nb;          // the env's samples [H][Nb]
  const float* in = cols + nn;
  GruStamps none;

  for (uint32_t it = 0; it < a.iterations; ++it) {
    const bool last = it + 1 == a.iterations;
    __syncthreads();                                       // image, mean / stdev of this iteration stand; the refit before is through
    if (tid < N) {
      cem_sample_row(p, mu, sd, a.seed, base + it, a.env_offset + env, tid, cols + tid, Nb);
      if (last && a.samples_out) {
        float* out = a.samples_out + ((size_t)env * N + tid) * H;
        for (uint32_t k = 0; k < H; ++k) out[k] = cols[(size_t)k * Nb + tid];
      }
    }
    __syncthreads();                                       // every row stands (global memory, block scope)
    GruRollout ro;
    gru_rollout_init<F16>(ro, lds, s0, lane, h1src, h1src ? h1src + 32 : nullptr);
    float u_next = in[0];
    for (uint32_t k = 0; k < H; ++k) {
      const float ur = u_next;
      if (k + 1 < H) u_next = in[(size_t)(k + 1) * Nb];    // in flight during this step's cell
      gru_rollout_step<COST, F16>(ro, lds, s0, x_t, te, lane, c, half1, p, nm, k, ur, none, [](float) {});
    }
    const float S_total = gru_rollout_total<COST>(ro, x_t, p);
    if (last && a.S_out && owner) a.S_out[(size_t)env * N + n] = S_total;
    rank_costs_at(key, order, n, S_total, owner, N, env, a.order_out, last);
    for (uint32_t k = tid; k < H; k += Nt) cem_refit_column(cols + (size_t)k * Nb, order, a.best_k, a.stdev_min, mu[k], sd[k]);
  }
  __syncthreads();
  if (tid == 0) a.Q_out[env] = mu[0];
  for (uint32_t k = tid; k < H; k += Nt) {
    if (a.plan_out) a.plan_out[(size_t)env * H + k] = mu[k];
    const uint32_t kk = k + a.shift;
    a.mean[(size_t)env * H + k] = kk < H ? mu[kk] : a.mean_fill;
    a.stdev[(size_t)env * H + k] = kk < H ? sd[kk] : a.stdev_fill;
  }
}

// One launch of a rollout kernel (Params, ptrs, GruNorm, image, tail...) on the weights image of its math mode, with `lds_extra`
// bytes of dynamic LDS behind the image.
template <bool F16, class Kernel, class Ptrs, class... Tail>
void launch_gru_kernel(cpmppi_handle* h, Kernel kernel, uint32_t blocks, size_t lds_extra, hipStream_t s, const Ptrs& a, Tail... tail) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), GRU_ROLLOUT_IMAGE_FLOATS<F16> * sizeof(float) + lds_extra, s, h->prm, a,
                     h->gru_norm, (const float*)(F16 ? h->gru16_image : h->gru_image), tail...);
}

}  // namespace

void launch_gru_rollout(cpmppi_handle* h, const cpmppi_step_args* a, const StepPtrs& p, hipStream_t s) {
  const size_t sums = (size_t)WAVES * p.W * sizeof(float);   // [WAVES][W] weighted sums behind the image
  gru_dispatch(h, [&](auto cost, auto f16) {
    constexpr int COST = decltype(cost)::value; constexpr bool F16 = decltype(f16)::value;
    auto launch = [&](auto kernel) {   // (the opt-in: host code that no allowed H reaches - H = 1024 needs 64 640 B (FAST), 64 416 B)
      if (GRU_ROLLOUT_IMAGE_FLOATS<F16> * sizeof(float) + sums > 64 * 1024) allow_large_lds(kernel);
      launch_gru_kernel<F16>(h, kernel, a->E * p.nb, sums, s, p, a->h0);
    };
    if (a->noise_kind == CPMPPI_NOISE_DELTA_U) launch(&gru_rollout_cost_kernel<COST, NOISE_DELTA_U, F16>);
    else if (a->noise_kind == CPMPPI_NOISE_KNOTS) launch(&gru_rollout_cost_kernel<COST, NOISE_KNOTS, F16>);
    else launch(&gru_rollout_cost_kernel<COST, NOISE_PHILOX, F16>);
  });
}

extern "C" {

int cpmppi_rollout_cost_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                            const float* target_equilibrium, const float* h0, float* S_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (const int rc = refuse_tuning_rows(h, "cpmppi_rollout_cost_gru")) return rc;      // (before the model is looked for, as cpmppi_step)
  if (const int rc = gru_refusal(h, "cpmppi_rollout_cost_gru", E != 0 && E <= h->cfg.E, "E out of range",
                                 s0 && inputs && target_position && target_equilibrium && S_out,
                                 "s0, inputs, target_position, target_equilibrium, S_out are required", true)) return rc;
  CPMPPI_ON_DEVICE(h);
  // (one launch, nothing allocated, nothing awaited: the call can be captured; no pole mass and no L - the network is the plant model)
  const GruCostPtrs a{{s0, inputs, target_position, target_equilibrium, h0, S_out},
                      (h->cfg.N + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK};
  gru_dispatch(h, [&](auto cost, auto f16) {
    launch_gru_kernel<f16.value>(h, &gru_cost_only_kernel<cost.value, f16.value>, E * a.nb, 0, (hipStream_t)stream, a);
  });
  return launched(h);
}

// cost and gradient: gru_grad_forward_kernel, then gru_grad_reverse_kernel (cpmppi_gru_adjoint.hip), on one stream
int cpmppi_rollout_cost_grad_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                                 const float* target_equilibrium, const float* h0, float* S_out, float* grad_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_rollout_cost_grad_gru";
  if (const int rc = refuse_tuning_rows(h, who)) return rc;
  if (const int rc = gru_refusal(h, who, E != 0 && E <= h->cfg.E, "E out of range",
                                 s0 && inputs && target_position && target_equilibrium && grad_out,
                                 "s0, inputs, target_position, target_equilibrium, grad_out are required", true)) return rc;
  CPMPPI_ON_DEVICE(h);
  // check-points of the handle's largest launch; allocated on first use, never inside a capture
  const size_t need = (size_t)h->cfg.H * GRU_CKPT_FLOATS * (size_t)h->cfg.E * h->cfg.N;
  if (h->gru_grad_ws_floats < need) {
    if (const int rc = refuse_unreserved_capture(h, (hipStream_t)stream, who, "cpmppi_rollout_cost_grad_gru once")) return rc;
    if (const int rc = grow_workspace(h, h->gru_grad_ws, h->gru_grad_ws_floats, need)) return rc;
  }
  const GruGradPtrs a = gru_grad_ptrs(h, E, s0, inputs, target_position, target_equilibrium, h0, S_out, grad_out);
  gru_dispatch(h, [&](auto cost, auto f16) {
    launch_gru_kernel<f16.value>(h, &gru_grad_forward_kernel<cost.value, f16.value>, E * a.nb, 0, (hipStream_t)stream, a);
  });
  launch_gru_grad_reverse(h, E, s0, inputs, target_position, target_equilibrium, h0, grad_out, (hipStream_t)stream);
  return launched(h);
}

// the whole cem control step over the network: gru_cem_step_kernel, then the step counter
int cpmppi_cem_step_gru(cpmppi_handle* h, const cpmppi_cem_gru_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const char* who = "cpmppi_cem_step_gru";
  const std::string w = std::string(who) + ": ";
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, w + "null argument block");
  if (const int rc = refuse_tuning_rows(h, who)) return rc;
  if (const int rc = gru_refusal(h, who, a->E != 0 && a->E <= h->cfg.E, "bad argument (0 < E <= config.E)",
                                 a->s0 && a->target_position && a->target_equilibrium && a->mean && a->stdev && a->Q_out,
                                 "null pointer (s0, target_position, target_equilibrium, mean, stdev and Q_out are required)", true))
    return rc;
  for (const void* ptr : {(const void*)a->s0, (const void*)a->target_position, (const void*)a->target_equilibrium, (const void*)a->h0,
                          (const void*)a->mean, (const void*)a->stdev, (const void*)a->Q_out, (const void*)a->S_out,
                          (const void*)a->plan_out, (const void*)a->samples_out, (const void*)a->order_out})
    if (misaligned(ptr)) return fail(h, CPMPPI_ERR_BAD_ARG, w + "misaligned pointer");
  if (reinterpret_cast<uintptr_t>(a->count_dev) & 7u) return fail(h, CPMPPI_ERR_BAD_ARG, w + "misaligned pointer (count_dev: 8 bytes)");
  if (a->iterations == 0) return fail(h, CPMPPI_ERR_BAD_ARG, w + "iterations must be > 0");
  if (a->best_k == 0 || a->best_k > h->cfg.N) return fail(h, CPMPPI_ERR_BAD_ARG, w + "bad argument (0 < best_k <= N)");
  if (a->shift > h->cfg.H) return fail(h, CPMPPI_ERR_BAD_ARG, w + "shift exceeds the horizon");
  if (h->cfg.N > (uint32_t)GRU_CEM_ROLLOUTS)
    return fail(h, CPMPPI_ERR_BAD_ARG, w + "one workgroup per env holds at most " + std::to_string(GRU_CEM_ROLLOUTS) +
                                           " samples (N = " + std::to_string(h->cfg.N) + ")");
  CPMPPI_ON_DEVICE(h);
  hipStream_t s = (hipStream_t)stream;
  const size_t need = cem_floats(h, a->E, false);              // cpmppi_cem_reserve(h, E, CPMPPI_CEM_REFINE_NONE)'s
  if (h->cem_ws_floats < need) {
    if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_cem_reserve")) return rc;
    if (const int rc = grow_workspace(h, h->cem_ws, h->cem_ws_floats, need)) return rc;
  }
  GruCemPtrs p{};
  p.s0 = a->s0; p.x_t = a->target_position; p.te = a->target_equilibrium; p.h0 = a->h0;
  p.mean = a->mean; p.stdev = a->stdev; p.samples = h->cem_ws;
  p.count_dev = (const unsigned long long*)a->count_dev;
  p.seed = a->seed; p.offset = a->offset;
  p.iterations = a->iterations; p.best_k = a->best_k; p.shift = a->shift; p.env_offset = a->env_offset; p.stride = rpgd_block(h);
  p.stdev_min = a->stdev_min; p.mean_fill = a->mean_fill; p.stdev_fill = a->stdev_fill;
  p.Q_out = a->Q_out; p.S_out = a->S_out; p.plan_out = a->plan_out; p.samples_out = a->samples_out; p.order_out = a->order_out;
  const uint32_t threads = 64u * ((h->cfg.N + 31u) / 32u);     // one wave per 32 samples: <= GRU_CEM_BLOCK
  const size_t tail = (2 * (size_t)GRU_CEM_ROLLOUTS + 2 * (size_t)h->cfg.H) * sizeof(float);   // key, order | mean, stdev
  gru_dispatch(h, [&](auto cost, auto f16) {
    constexpr int COST = decltype(cost)::value; constexpr bool F16 = decltype(f16)::value;
    const size_t lds = GRU_ROLLOUT_IMAGE_FLOATS<F16> * sizeof(float) + tail;
    static_assert(GRU_ROLLOUT_IMAGE_FLOATS<F16> * sizeof(float) + (2 * GRU_CEM_ROLLOUTS + 2 * CPMPPI_MAX_HORIZON) * sizeof(float) <=
                  64 * 1024, "the step's LDS stays under the default limit at every allowed H (58 496 B at H = 1024, FAST)");
    hipLaunchKernelGGL((gru_cem_step_kernel<COST, F16>), dim3(a->E), dim3(threads), lds, s, h->prm, p, h->gru_norm,
                       (const float*)(F16 ? h->gru16_image : h->gru_image));
  });
  CPMPPI_HIP(h, hipGetLastError());
  if (a->count_dev) launch_step_count((unsigned long long*)a->count_dev, s);
  return launched(h);
}

#ifdef CPMPPI_GRU_STAMPS
int cpmppi_debug_gru_stamps(unsigned long long out[8], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gru_stamp_sum), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gru_stamp_sum), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

}  // extern "C"
