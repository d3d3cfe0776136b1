// cpmppi_replay.hip - cpmppi_replay_step: control along recorded trajectories (gfx950 only).  The reference computes a controller's
// output along recordings that exist already (SI_Toolkit_ASF/Run/PreprocessData_Add_Control_Along_Trajectories.py, one CPU job per
// file); here the recordings lie on the device and this launch stands where the plant stands in the device loop: it hands the
// controller the recorded row where the plant would hand it the simulated one, and reduces the evaluations of a row to one number.
// Contract: include/cpmppi.h, cpmppi_replay_args.
#include <string>
#include "cpmppi_internal.hpp"

namespace {

// Two kinds of workgroup in ONE launch, told apart by the block index (block-uniform):
//   env blocks      one env per lane: publish the row the next controller call reads, keep Q (Q_all_out), zero the plans
//   collect blocks  one recording per wave: the mean (and standard deviation) of its K controls in float64
// No block reads what another writes.
constexpr uint32_t REPLAY_BLOCK = 256, REPLAY_WAVES = REPLAY_BLOCK / 64;

struct ReplayDev {
  uint32_t R, T, K, H, E, env_blocks, prime;
  uint64_t period;
  const unsigned long long* period_dev;
  const uint32_t* rows;
  const float *states, *tp, *te, *L, *prev, *Q;
  float *mean_out, *std_out, *all_out;
  float *s_out, *tp_out, *te_out, *L_out, *prev_out, *u_nom_reset;
};

// the sum over the wave of a float64, every lane with the same bits: lane l adds lane l^32's, then l^16's, ... l^1's
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(REPLAY_BLOCK) void replay_kernel(const ReplayDev a) {
  // the period: the host's, or the device counter's (already advanced by the step); a counter still 0 names no period: prime
  uint64_t c = a.period;
  bool prime = a.prime != 0u;
  if (a.period_dev) {
    const uint64_t cnt = (uint64_t)*a.period_dev;
    prime = prime || cnt == 0u;
    c = cnt ? cnt - 1u : 0u;
  }
  if (blockIdx.x >= a.env_blocks) {                                     // ---- collect: wave w of the block has recording r
    if (prime) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t r = (blockIdx.x - a.env_blocks) * REPLAY_WAVES + wave;
    if (r >= a.R) return;
    const uint32_t n = min(a.rows[r], a.T);
    if (c >= n) return;                                                 // (past this recording's end: no row is written)
    const float* __restrict__ q = a.Q + (size_t)r * a.K;
    double sum = 0.0;
    for (uint32_t k = lane; k < a.K; k += 64u) sum += (double)q[k];
    const double mean = wave_sum_f64(sum) / (double)a.K;
    double sd = 0.0;
    if (a.std_out && a.K > 1u) {                                        // two passes: the squares of the deviations from that mean
      double sq = 0.0;
      for (uint32_t k = lane; k < a.K; k += 64u) { const double d = (double)q[k] - mean; sq += d * d; }
      sd = sqrt(wave_sum_f64(sq) / (double)(a.K - 1u));
    }
    if (lane == 0u) {
      const size_t at = (size_t)r * a.T + (size_t)c;
      if (a.mean_out) a.mean_out[at] = (float)mean;
      if (a.std_out) a.std_out[at] = (float)sd;
    }
    return;
  }
  const uint32_t gid = blockIdx.x * REPLAY_BLOCK + threadIdx.x;         // ---- env blocks
  if (a.u_nom_reset) {                                                  // every row starts from a cold plan
    const size_t total = (size_t)a.E * a.H, stride = (size_t)a.env_blocks * REPLAY_BLOCK;
    for (size_t i = gid; i < total; i += stride) a.u_nom_reset[i] = 0.0f;
  }
  const uint32_t env = gid;
  if (env >= a.E) return;
  const uint32_t r = env / a.K;
  const uint32_t n = max(min(a.rows[r], a.T), 1u);
  if (a.all_out && !prime && c < n) a.all_out[(size_t)c * a.E + env] = a.Q[env];
  // what the next controller call reads: the next row, the last one at (and past) the recording's end
  const uint32_t p = prime ? 0u : (uint32_t)(c + 1u < (uint64_t)n ? c + 1u : (uint64_t)(n - 1u));
  const size_t row = (size_t)r * a.T + p;
  if (a.s_out) {
    const float* __restrict__ s = a.states + row * CPMPPI_STATE_DIM;
    float* __restrict__ o = a.s_out + (size_t)env * CPMPPI_STATE_DIM;
#pragma unroll
    for (uint32_t i = 0; i < CPMPPI_STATE_DIM; ++i) o[i] = s[i];
  }
  if (a.tp_out) a.tp_out[env] = a.tp[row];
  if (a.te_out) a.te_out[env] = a.te[row];
  if (a.L_out) a.L_out[env] = a.L[row];
  if (a.prev_out) a.prev_out[env] = a.prev[row];
}

}  // namespace

int cpmppi_replay_step(cpmppi_handle* h, const cpmppi_replay_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_replay_step: " + why); };
  if (!a) return refuse("no argument block");
  if (!a->states || !a->Q || !a->rows || !a->rows_host) return refuse("states, Q, rows and rows_host are required");
  if (a->R == 0 || a->T == 0 || a->K == 0) return refuse("R, T and K must be at least 1");
  const uint64_t E = (uint64_t)a->R * a->K;
  if (E > h->cfg.E)
    return refuse(std::to_string(a->R) + " recordings x " + std::to_string(a->K) + " evaluations = " + std::to_string(E) +
                  " envs, the handle has " + std::to_string(h->cfg.E));
  for (uint32_t r = 0; r < a->R; ++r)
    if (a->rows_host[r] == 0 || a->rows_host[r] > a->T)
      return refuse("rows[" + std::to_string(r) + "] = " + std::to_string(a->rows_host[r]) + " must lie in 1.." + std::to_string(a->T));
  if (!a->Q_mean_out && !a->Q_std_out && !a->Q_all_out && !a->s_out && !a->target_position_out && !a->target_equilibrium_out &&
      !a->L_out && !a->previous_input_out && !a->u_nom_reset)
    return refuse("no output at all");
  if (a->target_position_out && !a->target_position) return refuse("target_position_out without the target_position column");
  if (a->target_equilibrium_out && !a->target_equilibrium) return refuse("target_equilibrium_out without the target_equilibrium column");
  if (a->L_out && !a->L) return refuse("L_out without the L column");
  if (a->previous_input_out && !a->previous_input) return refuse("previous_input_out without the previous_input column");
  if (a->u_nom_reset && a->H == 0) return refuse("u_nom_reset needs H (the columns of the plans)");
  if (misaligned(a->states) || misaligned(a->target_position) || misaligned(a->target_equilibrium) || misaligned(a->L) ||
      misaligned(a->previous_input) || misaligned(a->Q) || misaligned(a->rows) || misaligned(a->Q_mean_out) ||
      misaligned(a->Q_std_out) || misaligned(a->Q_all_out) || misaligned(a->s_out) || misaligned(a->target_position_out) ||
      misaligned(a->target_equilibrium_out) || misaligned(a->L_out) || misaligned(a->previous_input_out) ||
      misaligned(a->u_nom_reset) || (a->period_dev && ((uintptr_t)a->period_dev & 7u)))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_replay_step: misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  ReplayDev d{};
  d.R = a->R; d.T = a->T; d.K = a->K; d.H = a->H; d.E = (uint32_t)E; d.prime = a->prime;
  d.env_blocks = (d.E + REPLAY_BLOCK - 1u) / REPLAY_BLOCK;
  d.period = a->period; d.period_dev = (const unsigned long long*)a->period_dev;
  d.rows = a->rows;
  d.states = a->states; d.tp = a->target_position; d.te = a->target_equilibrium; d.L = a->L; d.prev = a->previous_input; d.Q = a->Q;
  d.mean_out = a->Q_mean_out; d.std_out = a->Q_std_out; d.all_out = a->Q_all_out;
  d.s_out = a->s_out; d.tp_out = a->target_position_out; d.te_out = a->target_equilibrium_out; d.L_out = a->L_out;
  d.prev_out = a->previous_input_out; d.u_nom_reset = a->u_nom_reset;
  const bool collects = a->Q_mean_out || a->Q_std_out;
  const uint32_t blocks = d.env_blocks + (collects ? (a->R + REPLAY_WAVES - 1u) / REPLAY_WAVES : 0u);
  hipLaunchKernelGGL(replay_kernel, dim3(blocks), dim3(REPLAY_BLOCK), 0, (hipStream_t)stream, d);
  return launched(h);
}
