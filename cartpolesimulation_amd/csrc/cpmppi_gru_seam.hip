// cpmppi_gru_seam.hip — the seams of the GRU predictor (BASELINE configs[4]): the kernels of the exact f32 cell (gru_step, cpmppi_gru.hpp).
//   gru_predict_kernel                      predictor seam with the neural predictor: trajectories [B,H+1,6], hidden states.
//   gru_advance_kernel                      one exact cell step on (state seen, control chosen), in place on h[E,2,32]: the memory
//                                           hand-over between two control periods of the device loop.
//   gru_washout_kernel                      that step along whole recordings, every row's memory kept: h_rows[R,T,2,32] (cpmppi_gru_washout).
//   gru_brunton_kernel                      Brunton test with the neural predictor (cpmppi_brunton, cpmppi_seams.hip): gru_predict_kernel's
//                                           rollout from every start row of the recordings, per-wave error statistics per horizon step.
// The four share their start (gru_seam_begin).  predict and brunton each keep their rollout loop, predict and advance their memory
// stores: one loop with a per-step sink, gru_store_memory in all three and one tile set-up were measured and not kept - each moved
// the code of kernels it did not touch, and cpmppi_gru_advance went from 12.4 to 14.5 us (profiles/HISTORY.md, r15).
// Entry points: cpmppi_gru_predict, cpmppi_gru_advance, cpmppi_gru_washout; launch_gru_brunton for cpmppi_brunton (cpmppi_seams.hip).
#include "cpmppi_brunton.hpp"
#include "cpmppi_gru.hpp"        // (and cpmppi_internal.hpp)

using namespace cpmppi_k;

namespace {

// How every kernel here begins: the image into LDS (its only barrier), and the mapping - the wave's tile (`tile` of the grid) is
// rows first .. first + 31 of `rows`, row first + c on lanes c and c + 32.  A lane beyond the end repeats row 0 and stores nothing:
// what it computes is never looked at, and an MFMA column depends on its own column only, so it reaches no live row either.
// (`rows` in the caller's own type: widened here, three of the kernels took other scalar registers.)
struct GruSeamLane {
  uint32_t lane;
  size_t tile, first, row;
  bool valid;
};
template <class Count>
__device__ __forceinline__ GruSeamLane gru_seam_begin(float* lds, const float* __restrict__ image, Count rows) {
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u;
  const size_t tile = (size_t)blockIdx.x * WAVES + wave, first = tile * 32;
  const bool valid = first + c < rows;
  return {lane, tile, first, valid ? first + c : 0, valid};
}

// predictor seam with the neural predictor: s0[B,6], Q[B,H], h0[2,B,32] or NULL -> traj[B,H+1,6], h_out[2,B,32] or NULL
// (one wave per SIMD: the exact-f32 MFMA chain of gru_step with all its fragment loads in flight wants more than 256 registers -
// compiled for two waves per SIMD it spilled 38 of them to a 156-byte scratch slot; the seam is bound by the matrix pipe either way)
__global__ __launch_bounds__(BLOCK, 1) void gru_predict_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t B,
                                                            uint32_t H, const float* __restrict__ s0,
                                                            const float* __restrict__ Q, const float* __restrict__ h0,
                                                            float* __restrict__ traj, float* __restrict__ h_out) {
  extern __shared__ float lds[];
  const GruSeamLane m = gru_seam_begin(lds, image, B);
  const bool valid = m.valid;                              // (a local: read through m, the operands of the last test's s_and_b64 swap)
  const float* s = s0 + m.row * 6;
  f16v h1 = gru_load_hidden(h0 ? h0 + m.row * 32 : nullptr, m.lane);
  f16v h2 = gru_load_hidden(h0 ? h0 + ((size_t)B + m.row) * 32 : nullptr, m.lane);
  f16v x = gru_input_tile(nm, s, Q[m.row * H], m.lane);
  float* o = traj + m.row * (size_t)(H + 1) * 6;
  if (valid && m.lane < 32) for (int i = 0; i < 6; ++i) o[i] = s[i];
  for (uint32_t k = 0; k < H; ++k) {
    const f16v out = gru_step(lds, x, h1, h2, m.lane);
    float st[6];
    gru_output_state(nm, out, m.lane, st);
    if (valid && m.lane < 32) {
      o += 6;
      for (int i = 0; i < 6; ++i) o[i] = st[i];
    }
    x = out;                                               // normalised outputs are fed back unchanged
    if (m.lane >= 32 && k + 1 < H) x[1] = __builtin_fmaf(Q[m.row * H + k + 1], nm.in_scale[0], nm.in_shift[0]);
  }
  if (h_out && valid) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      h_out[m.row * 32 + gru_tile_row(v, m.lane >> 5)] = h1[v];
      h_out[((size_t)B + m.row) * 32 + gru_tile_row(v, m.lane >> 5)] = h2[v];
    }
  }
}

// The memory hand-over of the device loop: h_io[E,2,32] (the rollout kernels' layout) <- hidden states after ONE exact cell step
// on (s[E,6], Q[E]), in place.  gru_predict_kernel's mapping (env e on lanes c and c + 32 of a wave, one wave per SIMD for the
// same reason) and its cell, so what it stores is what that kernel writes to h_out for B = E, H = 1; the head's result is
// dropped, nothing is de-normalised.  In place is safe: all of a live env's loads precede its stores in its own wave, and no
// other wave stores to its rows.  A lane beyond E repeats row 0, which block 0 may be rewriting at that moment: what it then
// computes is undefined but never stored (an MFMA column depends on its own column only, so it reaches no live env either).
__global__ __launch_bounds__(BLOCK, 1) void gru_advance_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t E,
                                                            const float* __restrict__ s, const float* __restrict__ Q,
                                                            float* h_io) {
  extern __shared__ float lds[];
  const GruSeamLane m = gru_seam_begin(lds, image, E);
  float* hrow = h_io + m.row * 64;
  f16v h1 = gru_load_hidden(hrow, m.lane);
  f16v h2 = gru_load_hidden(hrow + 32, m.lane);
  const f16v x = gru_input_tile(nm, s + m.row * 6, Q[m.row], m.lane);
  (void)gru_step(lds, x, h1, h2, m.lane);
  if (m.valid) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      hrow[gru_tile_row(v, m.lane >> 5)] = h1[v];
      hrow[32 + gru_tile_row(v, m.lane >> 5)] = h2[v];
    }
  }
}

// A lane's registers of both hidden tiles -> one memory row [2,32] (the layout of cpmppi_step_args.h0).
__device__ __forceinline__ void gru_store_memory(float* hrow, const f16v& h1, const f16v& h2, uint32_t lane) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    hrow[gru_tile_row(v, lane >> 5)] = h1[v];
    hrow[32 + gru_tile_row(v, lane >> 5)] = h2[v];
  }
}

// The memory along recordings (update_before_predicting of the reference's Brunton test): h_rows[r,0] = h0[r] (NULL: zeros),
// h_rows[r,t+1] = the memory after ONE exact cell step on (states[r,t], Q[r,t]) from h_rows[r,t] - what T-1 successive
// cpmppi_gru_advance calls leave, bit for bit: gru_advance_kernel's mapping (recording r on lanes c and c + 32 of a wave, one wave
// per SIMD) and its cell, with the memory kept in registers between the rows instead of going through h_io.  The next row's state
// and control do not depend on the cell: they are loaded one row ahead.  A wave without a recording leaves behind the image
// load's barrier, the kernel's only one; a lane beyond R in a live wave repeats recording 0 and stores nothing.
__global__ __launch_bounds__(BLOCK, 1) void gru_washout_kernel(const GruNorm nm, const float* __restrict__ image, uint32_t R,
                                                            uint32_t T, const float* __restrict__ states,
                                                            const float* __restrict__ Q, const float* __restrict__ h0,
                                                            float* __restrict__ h_rows) {
  extern __shared__ float lds[];
  const GruSeamLane m = gru_seam_begin(lds, image, R);
  if (m.first >= R) return;                                // (wave-uniform) a tile without a recording
  f16v h1 = gru_load_hidden(h0 ? h0 + m.row * 64 : nullptr, m.lane);
  f16v h2 = gru_load_hidden(h0 ? h0 + m.row * 64 + 32 : nullptr, m.lane);
  const float* __restrict__ s = states + m.row * T * 6;
  const float* __restrict__ q = Q + m.row * T;
  float* hrow = h_rows + m.row * T * 64;
  if (m.valid) gru_store_memory(hrow, h1, h2, m.lane);
  float sn[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
  float qn = q[0];
  for (uint32_t t = 0; t + 1 < T; ++t) {
    const f16v x = gru_input_tile(nm, sn, qn, m.lane);
    if (t + 2 < T) {                                       // in flight during this row's cell
#pragma unroll
      for (int i = 0; i < 6; ++i) sn[i] = s[(size_t)(t + 1) * 6 + i];
      qn = q[t + 1];
    }
    (void)gru_step(lds, x, h1, h2, m.lane);
    hrow += 64;
    if (m.valid) gru_store_memory(hrow, h1, h2, m.lane);
  }
}

// Brunton test with the neural predictor: gru_predict_kernel's mapping (32 starts per wave on lanes c and c + 32, one wave per
// SIMD) and its exact-f32 cell, begun at states[r,t] with the memory h_rows[r,t] (NULL: zeros) and fed the RECORDED controls
// Q[r,t+k]; after step k the de-normalised state (gru_output_state: angle = atan2(sin, cos), as in the seam) is compared with
// states[r,t+k+1] (brunton_errors).  The states live on lanes 0..31; the other half and the lanes beyond the last start enter the
// statistics as zeros.  One partial row per WAVE, written by its lane 0 with plain stores: after the image load no wave depends
// on another, so a wave whose 32 starts all lie beyond the last one leaves at once - there is no second barrier it could be
// missed at, and no row of the partials for it (brunton_gru_rows counts the live waves, which are the first ones).
__global__ __launch_bounds__(BLOCK, 1) void gru_brunton_kernel(const GruNorm nm, const float* __restrict__ image,
                                                            const BruntonArgs a) {
  extern __shared__ float lds[];
  const size_t starts = (size_t)a.R * a.count;
  const GruSeamLane m = gru_seam_begin(lds, image, starts);
  if (m.first >= starts) return;                           // (wave-uniform) a tile without a start
  const size_t row = (m.row / a.count) * a.T + a.start + m.row % a.count;          // (r, t) in the series
  const float* s = a.states + row * 6;
  f16v h1 = gru_load_hidden(a.h_rows ? a.h_rows + row * 64 : nullptr, m.lane);
  f16v h2 = gru_load_hidden(a.h_rows ? a.h_rows + row * 64 + 32 : nullptr, m.lane);
  f16v x = gru_input_tile(nm, s, a.Q[row], m.lane);
  const bool owner = m.valid && m.lane < 32;                   // the lane that accounts for start m.row
  float* o = a.pred ? a.pred + m.row * (size_t)(a.horizon + 1) * 6 : nullptr;
  if (o && owner) for (int i = 0; i < 6; ++i) o[i] = s[i];
  float* __restrict__ out = a.partials + m.tile * a.horizon * BRUNTON_STATS;
  for (uint32_t k = 0; k < a.horizon; ++k) {
    const f16v y = gru_step(lds, x, h1, h2, m.lane);
    float st[6];
    gru_output_state(nm, y, m.lane, st);
    if (o && owner) {
      o += 6;
      for (int i = 0; i < 6; ++i) o[i] = st[i];
    }
    float e[6];
    brunton_errors(st, a.states + (row + k + 1) * 6, e);
    brunton_wave_stats(e, owner, m.lane == 0, out + (size_t)k * BRUNTON_STATS);
    x = y;                                                 // normalised outputs are fed back unchanged
    if (m.lane >= 32 && k + 1 < a.horizon) x[1] = __builtin_fmaf(a.Q[row + k + 1], nm.in_scale[0], nm.in_shift[0]);
  }
}

// one launch of an exact-cell kernel over `rows` rows: nothing allocated, nothing awaited, so the call can be captured
template <class... Params, class... Args>
void launch_gru_seam(cpmppi_handle* h, void (*kernel)(GruNorm, const float*, Params...), size_t rows, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK)), dim3(BLOCK),
                     (size_t)GRU_IMAGE_FLOATS * sizeof(float), s, h->gru_norm, (const float*)h->gru_image, args...);
}

}  // namespace

void launch_gru_brunton(cpmppi_handle* h, const BruntonArgs& a, hipStream_t s) {
  launch_gru_seam(h, gru_brunton_kernel, (size_t)a.R * a.count, s, a);   // brunton_gru_rows live waves
}

extern "C" {

int cpmppi_gru_predict(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* s0, const float* Q, const float* h0,
                       float* traj_out, float* h_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (const int rc = gru_refusal(h, "cpmppi_gru_predict", B != 0 && s0 && Q && traj_out, "bad argument", true, "")) return rc;
  if (horizon == 0) horizon = h->cfg.H;
  CPMPPI_ON_DEVICE(h);
  launch_gru_seam(h, gru_predict_kernel, B, (hipStream_t)stream, B, horizon, s0, Q, h0, traj_out, h_out);
  return launched(h);
}

int cpmppi_gru_advance(cpmppi_handle* h, uint32_t E, const float* s, const float* Q, float* h_io, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (const int rc = gru_refusal(h, "cpmppi_gru_advance", E != 0 && E <= h->cfg.E, "E out of range", s && Q && h_io,
                                 "s, Q, h_io are required")) return rc;
  CPMPPI_ON_DEVICE(h);
  launch_gru_seam(h, gru_advance_kernel, E, (hipStream_t)stream, E, s, Q, h_io);
  return launched(h);
}

int cpmppi_gru_washout(cpmppi_handle* h, uint32_t R, uint32_t T, const float* states, const float* Q, const float* h0,
                       float* h_rows_out, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (const int rc = gru_refusal(h, "cpmppi_gru_washout", R != 0 && T != 0, "R and T must be at least 1", states && Q && h_rows_out,
                                 "states, Q, h_rows_out are required")) return rc;
  if (misaligned(states) || misaligned(Q) || misaligned(h0) || misaligned(h_rows_out))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_gru_washout: misaligned pointer");
  CPMPPI_ON_DEVICE(h);
  launch_gru_seam(h, gru_washout_kernel, R, (hipStream_t)stream, R, T, states, Q, h0, h_rows_out);
  return launched(h);
}

}  // extern "C"
