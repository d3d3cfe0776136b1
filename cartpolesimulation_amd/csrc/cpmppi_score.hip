// cpmppi_score.hip - cpmppi_score_runs: the score of a recording per env, reduced on the device (gfx950 only).  The reference judges
// a controller setting by the two numbers its simulator prints after an experiment - mean |position - target_position| and mean
// |angle| in degrees (CartPole/__init__.py:727-729) - for one cartpole at a time; here they come, with three more, for every env of
// a device loop's logs in one launch, so that a sweep over controller settings never copies a recording to the host.
#include <string>
#include "cpmppi_internal.hpp"

namespace {

// Lanes run along envs: a row of the logs is env-contiguous, so a wave reads 64 neighbouring envs of one row.  The rows of the
// window are dealt to the SCORE_WAVES waves of a workgroup round robin, and wave 0 adds the waves' sums in wave order: a fixed
// order whatever the placement, no atomics.  Sums are float64 (a recording has thousands of rows; the kernel waits for memory).
constexpr uint32_t SCORE_WAVES = 8, SCORE_BLOCK = 64 * SCORE_WAVES;
constexpr float STABLE_ANGLE = (float)(3.14159265358979323846 / 5.0);   // float32(np.pi / 5): CartPole/CheckStabilized.py:7,24
constexpr uint32_t SCORE_MAX_ROWS = 1u << 24;                           // row numbers are reported as floats

struct ScoreArgs {
  const float* states;
  const float* table;
  const float* target;
  const float* Q;
  float* out;
  uint64_t sched_rows;
  uint32_t E, row_envs, rows, first_row, last_row, q_first, q_last, save_every, sched_stride;
  float target_value;
  uint32_t narrow;      // rows * save_every < 2^32: the table row of a saved row is computed in 32 bits
};

__global__ __launch_bounds__(SCORE_BLOCK) void score_runs_kernel(const ScoreArgs a) {
  __shared__ double sums[SCORE_WAVES][3][64];       // distance, |angle|, Q^2
  __shared__ uint32_t counts[SCORE_WAVES][2][64];   // rows inside the angle, 1 + the last row outside it
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t env = blockIdx.x * 64u + lane;
  const bool live = env < a.E;
  const uint32_t e = live ? env : a.E - 1u;         // (lanes past the last env read its logs and store nothing)
  const float target_env = a.table ? 0.0f : (a.target ? a.target[e] : a.target_value);

  double dist = 0.0, angle_abs = 0.0, q_sq = 0.0;
  uint32_t inside = 0u, after = a.first_row;
#pragma unroll 4
  for (uint32_t r = a.first_row + wave; r < a.last_row; r += SCORE_WAVES) {
    const float* __restrict__ s = a.states + ((size_t)r * a.row_envs + e) * CPMPPI_STATE_DIM;
    const float angle = s[0], position = s[4];
    float target = target_env;
    if (a.table) {                                  // the table row of simulation step r * save_every (cpmppi_plant_step's rule)
      // (r is wave-uniform: scalar arithmetic; in 32 bits whenever the recording's last simulation step fits, which the host checks)
      uint64_t tr = a.narrow ? (uint64_t)(r * a.save_every / a.sched_stride) : (uint64_t)r * a.save_every / a.sched_stride;
      tr = tr < a.sched_rows ? tr : a.sched_rows - 1u;
      target = a.table[(size_t)tr * a.row_envs + e];
    }
    dist += __builtin_fabs((double)position - (double)target);
    angle_abs += (double)__builtin_fabsf(angle);
    const bool ok = __builtin_fabsf(angle) < STABLE_ANGLE;     // (false for a NaN)
    inside += ok ? 1u : 0u;
    after = ok ? after : r + 1u;
  }
  if (a.Q) {
#pragma unroll 4
    for (uint32_t c = a.q_first + wave; c < a.q_last; c += SCORE_WAVES) {
      const double q = (double)a.Q[(size_t)c * a.row_envs + e];
      q_sq += q * q;
    }
  }
  sums[wave][0][lane] = dist; sums[wave][1][lane] = angle_abs; sums[wave][2][lane] = q_sq;
  counts[wave][0][lane] = inside; counts[wave][1][lane] = after;
  __syncthreads();
  if (wave != 0u || !live) return;
  for (uint32_t w = 1; w < SCORE_WAVES; ++w) {
    dist += sums[w][0][lane]; angle_abs += sums[w][1][lane]; q_sq += sums[w][2][lane];
    inside += counts[w][0][lane];
    after = after > counts[w][1][lane] ? after : counts[w][1][lane];
  }
  const double n = (double)(a.last_row - a.first_row);
  float* __restrict__ out = a.out + (size_t)env * CPMPPI_SCORE_FLOATS;
  out[CPMPPI_SCORE_MEAN_ABS_DISTANCE] = (float)(dist / n);
  out[CPMPPI_SCORE_MEAN_ABS_ANGLE_DEG] = (float)(angle_abs / n * (180.0 / 3.14159265358979323846));
  out[CPMPPI_SCORE_MEAN_Q_SQUARED] = a.Q ? (float)(q_sq / (double)(a.q_last - a.q_first)) : 0.0f;
  out[CPMPPI_SCORE_STABLE_SHARE] = (float)((double)inside / n);
  out[CPMPPI_SCORE_FIRST_STABLE_ROW] = (float)(after < a.last_row ? after : a.rows);
}

}  // namespace

int cpmppi_score_runs(cpmppi_handle* h, const cpmppi_score_args* a, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  const auto refuse = [&](const std::string& why) { return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_score_runs: " + why); };
  if (!a) return refuse("no argument block");
  if (!a->states || !a->score_out) return refuse("states and score_out are required");
  if (a->E == 0 || a->rows == 0) return refuse("E and rows must be at least 1");
  if (a->rows > SCORE_MAX_ROWS) return refuse(std::to_string(a->rows) + " rows: at most 2^24 (a row number is reported as a float)");
  const uint32_t row_envs = a->row_envs ? a->row_envs : a->E;
  if (row_envs < a->E) return refuse("row_envs " + std::to_string(row_envs) + " is fewer than the " + std::to_string(a->E) + " envs scored");
  const uint32_t last_row = a->last_row ? a->last_row : a->rows;
  if (a->first_row >= last_row || last_row > a->rows)
    return refuse("the window of rows [" + std::to_string(a->first_row) + ", " + std::to_string(last_row) +
                  ") must be non-empty and lie inside the recording's " + std::to_string(a->rows) + " rows");
  const uint32_t q_last = a->q_last ? a->q_last : a->q_rows;
  if (a->Q && (a->q_first >= q_last || q_last > a->q_rows))
    return refuse("the window of controller calls [" + std::to_string(a->q_first) + ", " + std::to_string(q_last) +
                  ") must be non-empty and lie inside Q's " + std::to_string(a->q_rows) + " rows");
  if (a->target_position_table && a->sched_rows == 0) return refuse("target_position_table needs sched_rows");
  if (misaligned(a->states) || misaligned(a->score_out) || misaligned(a->target_position_table) || misaligned(a->target_position) ||
      misaligned(a->Q))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_score_runs: misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  const uint32_t save_every = a->save_every ? a->save_every : 1u;
  const ScoreArgs k{a->states, a->target_position_table, a->target_position, a->Q, a->score_out, a->sched_rows,
                    a->E, row_envs, a->rows, a->first_row, last_row, a->q_first, q_last,
                    save_every, a->sched_stride ? a->sched_stride : 1u, a->target_position_value,
                    (uint64_t)a->rows * save_every <= 0xFFFFFFFFull ? 1u : 0u};
  hipLaunchKernelGGL(score_runs_kernel, dim3((a->E + 63u) / 64u), dim3(SCORE_BLOCK), 0, (hipStream_t)stream, k);
  return launched(h);
}
