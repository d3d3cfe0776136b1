// cpmppi_gru_train.hip — training the GRU predictor on recordings (cpmppi_gru_loss_grad, cpmppi_gru_rollout_loss_grad,
// cpmppi_gru_train_*): the loss over windows of recordings - teacher-forced, or through the open-loop rollout the predictor is used
// in -, its gradient with respect to the weights by back-propagation through time, Adam and the rebuild of the two float32 weight
// images on the device.  Small kernels, one job each, no float atomics; every sum runs in a fixed order.
//   gru_train_forward_kernel<STORE, ROLLOUT>
//                                     gru_washout_kernel's mapping (32 windows per wave on lanes c and c + 32, one wave per SIMD, the
//                                     exact-f32 gru_step cell) from a zero memory over the window's W + P rows: recorded rows, or
//                                     (ROLLOUT) behind row W the head's outputs of the row before with the recorded control.  Per
//                                     wave a partial loss; STORE: per (row, window) a check-point - both hidden tiles, the head adjoint
//                                     2 (y - label) / (B P 5) (0 on wash-out rows) and the input tile the cell consumed.
//   gru_loss_finalize_kernel          the waves' partial losses summed in float64 -> loss_out.
//   gru_train_reverse_kernel<ROLLOUT> rows last to first: gru_layer_reverse per layer on both images in LDS (98 208 B, opt-in); there
//                                     is no cost stage.  Writes the eight pre-activation adjoint tiles per (row, window).  ROLLOUT:
//                                     the feedback path of gru_reverse_steps - rows 0..4 of the input adjoint of a fed-back row join
//                                     the head adjoint of the row before, in the check-point.
//   gru_wgrad_kernel                  dW = sum over (row, window) of da (x) input per matrix and gate on v_mfma_f32_32x32x2_f32 with
//                                     the WINDOW as the contraction index: check-points and adjoints lie [row][window][unit], so a
//                                     lane loads its A and B operands as they stand.  One wave per (product, slice of the (row, window
//                                     tile) sequence), rows and window tiles in ascending order; a bias gradient is the same product
//                                     against ones.
//   gru_wgrad_reduce_kernel           the slices' partial products added in ascending order, scattered to the flat parameter order.
//   gru_adam_repack_kernel            Adam on the master copy (float64 arithmetic, float32 storage, step counter on the device), then
//                                     both images rebuilt from a table of source indices that cpmppi_gru_model.hip reads off its own
//                                     packers; one workgroup, its barrier orders the two halves.
// The forward kernel stores the head ADJOINT where the issue that asked for it suggested the head output: the reverse sweep and the
// head's weight gradient need nothing else of the output, and the label is then formed once.
#include "cpmppi_gru_reverse.hpp"   // (and cpmppi_gru.hpp, cpmppi_grad.hpp, cpmppi_internal.hpp)
#include "cpmppi_train.hpp"

using namespace cpmppi_k;

// What training keeps on the device between calls.
struct GruTrain {
  float* ws = nullptr;                 // [loss partials | partial products | check-points | adjoints] of one call
  size_t ws_floats = 0;
  int32_t* tables = nullptr;           // image sources [2 * (GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS)], then gradient sources [CPMPPI_GRU_PARAMS]
  float* master = nullptr;             // [4][CPMPPI_GRU_PARAMS]: master copy, Adam's m and v, the gradient of cpmppi_gru_train_step
  unsigned long long* step = nullptr;  // Adam's t so far
  bool begun = false;                  // cpmppi_gru_train_begin has run
};

namespace {

constexpr int CK = 80;                 // check-point floats per (row, window): h1[32] h2[32] head adjoint[8] input tile[8], natural row order
constexpr int CK_H2 = 32, CK_DY = 64, CK_X = 72;
constexpr int ADJ = 256;               // adjoint floats per (row, window): layer 1 r, z, n_x, n_h [32 each], then layer 2's
constexpr int WG_TASKS = 22;           // products of gru_wgrad_kernel: 4 matrices x 3 gates, the head, 8 gate-bias sums, the head's bias
constexpr int WG_MAX_SLICES = 64;      // ... each cut into at most this many slices of the (row, window tile) sequence
constexpr int WG_MIN_TILES = 8;        // ... of at least this many tiles (16 MFMAs each)
constexpr size_t N_IMG = (size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS;
constexpr size_t REVERSE_LDS = N_IMG * sizeof(float);          // 98 208 B: opt-in
constexpr int REPACK_BLOCK = 1024;

struct GruTrainArgs {
  const float* states;   // [R,T,6]
  const float* Q;        // [R,T]
  const uint32_t* windows;   // [B][2]
  uint32_t B, Bp, T, W, L, shift;   // windows, rounded up to whole waves; rows of a recording; wash-out rows, all rows of a window
  float scale;           // 2 / (B P 5)
  float* ckpt;           // [L][Bp][CK]
  float* adj;            // [L][Bp][ADJ]
  double* loss_part;     // [Bp / 32]
};

// A lane's 16 registers of a tile <-> the tile's rows in natural order: registers 4q .. 4q+3 are rows 8q + 4 hf .. + 3.
__device__ __forceinline__ void park_rows(float* dst, const f16v& h, uint32_t hf) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<cpmppi::f4v*>(dst + 8 * q + 4 * hf) = cpmppi::f4v{h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]};
}
__device__ __forceinline__ f16v fetch_rows(const float* src, uint32_t hf) {
  f16v h;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const cpmppi::f4v t = *reinterpret_cast<const cpmppi::f4v*>(src + 8 * q + 4 * hf);
    h[4 * q] = t.x; h[4 * q + 1] = t.y; h[4 * q + 2] = t.z; h[4 * q + 3] = t.w;
  }
  return h;
}
__device__ __forceinline__ f16v zero_tile() {
  f16v z;
#pragma unroll
  for (int v = 0; v < 16; ++v) z[v] = 0.0f;
  return z;
}

// Window first + c of the wave's tile on lanes c and c + 32; a lane beyond B repeats window 0, adds nothing to the loss and parks a
// zero head adjoint (its adjoints are stored as zeros by the reverse sweep, so the contraction may read whole tiles).
// ROLLOUT: rows j > W take input rows 0..4 from the head's normalised output of row j - 1, unchanged (gru_predict_kernel's rule), and
// row 5 from the recorded Q[t0 + j]; the check-point's input tile is the tile the cell consumed.
template <bool STORE, bool ROLLOUT>
__global__ __launch_bounds__(BLOCK, 1) void gru_train_forward_kernel(const cpmppi::GruNorm nm, const float* __restrict__ image,
                                                                     const GruTrainArgs a) {
  extern __shared__ float lds[];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);            // the kernel's only barrier
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u, hf = lane >> 5;
  const size_t tile = (size_t)blockIdx.x * WAVES + wave, first = tile * 32;
  if (first >= a.B) return;                                // (wave-uniform) a tile without a window
  const bool valid = first + c < a.B;
  const size_t win = valid ? first + c : 0;
  const size_t base = (size_t)a.windows[2 * win] * a.T + a.windows[2 * win + 1];
  const float* __restrict__ s = a.states + base * 6;
  const float* __restrict__ q = a.Q + base;
  f16v h1 = zero_tile(), h2 = zero_tile();
  float acc = 0.0f;
  float* ck = STORE ? a.ckpt + (first + c) * CK : nullptr;
  f16v fed = zero_tile();                                  // ROLLOUT: the outputs of the row before
  for (uint32_t j = 0; j < a.L; ++j) {
    f16v x;
    if (ROLLOUT && j > a.W) {                              // (wave-uniform)
      x = fed;
      if (hf) x[1] = __builtin_fmaf(q[j], nm.in_scale[0], nm.in_shift[0]);
    } else {
      x = cpmppi::gru_input_tile(nm, s + (size_t)j * 6, q[j], lane);
    }
    const f16v y = cpmppi::gru_step(lds, x, h1, h2, lane);
    if constexpr (ROLLOUT) fed = y;
    cpmppi::f4v d = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j >= a.W && valid) {
      const float* __restrict__ lab = s + (size_t)(j + a.shift) * 6;
      if (!hf) {
        const float e0 = y[0] - (lab[1] - nm.out_shift[0]) / nm.out_scale[0];
        const float e1 = y[1] - (lab[2] - nm.out_shift[1]) / nm.out_scale[1];
        const float e2 = y[2] - (lab[3] - nm.out_shift[2]) / nm.out_scale[2];
        const float e3 = y[3] - (lab[4] - nm.out_shift[3]) / nm.out_scale[3];
        acc = __builtin_fmaf(e0, e0, acc); acc = __builtin_fmaf(e1, e1, acc);
        acc = __builtin_fmaf(e2, e2, acc); acc = __builtin_fmaf(e3, e3, acc);
        d = cpmppi::f4v{a.scale * e0, a.scale * e1, a.scale * e2, a.scale * e3};
      } else {
        const float e4 = y[0] - (lab[5] - nm.out_shift[4]) / nm.out_scale[4];   // row 4 lives on lane-half 1
        acc = __builtin_fmaf(e4, e4, acc);
        d.x = a.scale * e4;
      }
    }
    if (STORE) {
      park_rows(ck, h1, hf);
      park_rows(ck + CK_H2, h2, hf);
      *reinterpret_cast<cpmppi::f4v*>(ck + CK_DY + 4 * hf) = d;
      *reinterpret_cast<cpmppi::f4v*>(ck + CK_X + 4 * hf) = cpmppi::f4v{x[0], x[1], x[2], x[3]};
      ck += (size_t)a.Bp * CK;
    }
  }
  double sum = (double)acc;                                // the wave's partial loss: a butterfly, the same order every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) a.loss_part[tile] = sum;
}

// One wave: lane l adds partials l, l + 64, ... in ascending order, the lanes' sums meet in a butterfly; / (B P 5).
__global__ __launch_bounds__(64) void gru_loss_finalize_kernel(const double* __restrict__ part, uint32_t tiles, double count,
                                                               double* __restrict__ loss_out) {
  double sum = 0.0;
  for (uint32_t t = threadIdx.x; t < tiles; t += 64) sum += part[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (threadIdx.x == 0) *loss_out = sum / count;
}

// The forward kernel's mapping.  Per row, last to first: head adjoint (parked by the forward sweep) -> layer 2 -> layer 1, each
// layer's gates recomputed from its check-pointed input and previous hidden tile (zeros before row 0) right before its adjoint.
// ROLLOUT: the feedback adjoint as gru_reverse_steps forms it - behind a row j > W the input adjoint dx = W_ih0^T (da_r, da_z, da_nx),
// whose rows 0..4 (lane-half 0 carries rows 0..3, lane-half 1 row 4) join the head adjoint of row j - 1; the sum is parked in the
// check-point, where gru_wgrad_kernel reads the head adjoint.  The input adjoints of rows <= W and the Q row are dropped.
template <bool ROLLOUT>
__global__ __launch_bounds__(BLOCK, 1) void gru_train_reverse_kernel(const float* __restrict__ image, const float* __restrict__ image_t,
                                                                     const GruTrainArgs a) {
  extern __shared__ float lds[];                           // forward f32 image, then the transposed image
  float* ldst = lds + GRU_IMAGE_FLOATS;
  for (int i = threadIdx.x; i < GRU_T_IMAGE_FLOATS; i += BLOCK) ldst[i] = image_t[i];
  gru_load_image(lds, image, GRU_IMAGE_FLOATS);            // the kernel's only barrier
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, c = lane & 31u, hf = lane >> 5;
  const size_t first = ((size_t)blockIdx.x * WAVES + wave) * 32;
  if (first >= a.B) return;                                // (wave-uniform) a tile without a window
  const bool valid = first + c < a.B;
  const size_t col = first + c;
  f16v dh1 = zero_tile(), dh2 = zero_tile();               // adjoints of the hidden tiles behind row j
  const f16v zero = zero_tile();
  float dfb[4] = {0.0f, 0.0f, 0.0f, 0.0f};                 // ROLLOUT: adjoint of row j's outputs through the input tile of row j + 1
  for (uint32_t j = a.L; j-- > 0;) {
    const float* ck = a.ckpt + ((size_t)j * a.Bp + col) * CK;
    const float* ckp = ck - (size_t)a.Bp * CK;             // row j - 1 (j = 0: not read)
    float* ad = a.adj + ((size_t)j * a.Bp + col) * ADJ;
    f16v gout = zero;
    {
      const cpmppi::f4v d = *reinterpret_cast<const cpmppi::f4v*>(ck + CK_DY + 4 * hf);
      gout[0] = d.x; gout[1] = d.y; gout[2] = d.z; gout[3] = d.w;
      if constexpr (ROLLOUT) {
        gout[0] += dfb[0];                                 // (lane-half 1: [0] = row 4; [1..3] are not read)
        if (!hf) { gout[1] += dfb[1]; gout[2] += dfb[2]; gout[3] += dfb[3]; }
        *reinterpret_cast<cpmppi::f4v*>(a.ckpt + ((size_t)j * a.Bp + col) * CK + CK_DY + 4 * hf) =
            cpmppi::f4v{gout[0], gout[1], gout[2], gout[3]};
      }
    }
    f16v dar, daz, danx, danh;
    {
      const f16v h1 = fetch_rows(ck, hf);
      const f16v h2p = j ? fetch_rows(ckp + CK_H2, hf) : zero;
      dh2 = cpmppi::gru_mm<4>(dh2, ldst + cpmppi::GT_HEAD * 64, gout, lane);
      cpmppi::gru_layer_reverse<16>(lds, cpmppi::GF_L2X, cpmppi::GF_L2H, 4, h1, h2p, lane, dh2, dar, daz, danx, danh);
    }
    park_rows(ad + 128, valid ? dar : zero, hf);
    park_rows(ad + 160, valid ? daz : zero, hf);
    park_rows(ad + 192, valid ? danx : zero, hf);
    park_rows(ad + 224, valid ? danh : zero, hf);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L2X + 0) * 64, dar, lane);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L2X + 16) * 64, daz, lane);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L2X + 32) * 64, danx, lane);
    dh2 = cpmppi::gru_mm<16>(dh2, ldst + (cpmppi::GT_L2H + 0) * 64, dar, lane);
    dh2 = cpmppi::gru_mm<16>(dh2, ldst + (cpmppi::GT_L2H + 16) * 64, daz, lane);
    dh2 = cpmppi::gru_mm<16>(dh2, ldst + (cpmppi::GT_L2H + 32) * 64, danh, lane);
    __builtin_amdgcn_sched_barrier(0);
    {
      f16v xt = zero;
      const cpmppi::f4v xr = *reinterpret_cast<const cpmppi::f4v*>(ck + CK_X + 4 * hf);
      xt[0] = xr.x; xt[1] = xr.y; xt[2] = xr.z; xt[3] = xr.w;
      const f16v h1p = j ? fetch_rows(ckp, hf) : zero;
      cpmppi::gru_layer_reverse<4>(lds, cpmppi::GF_L1X, cpmppi::GF_L1H, 0, xt, h1p, lane, dh1, dar, daz, danx, danh);
    }
    park_rows(ad + 0, valid ? dar : zero, hf);
    park_rows(ad + 32, valid ? daz : zero, hf);
    park_rows(ad + 64, valid ? danx : zero, hf);
    park_rows(ad + 96, valid ? danh : zero, hf);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L1H + 0) * 64, dar, lane);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L1H + 16) * 64, daz, lane);
    dh1 = cpmppi::gru_mm<16>(dh1, ldst + (cpmppi::GT_L1H + 32) * 64, danh, lane);
    if constexpr (ROLLOUT) {
      f16v dx = zero;
      if (j > a.W) {                                       // (wave-uniform) the row's input tile was fed back
        dx = cpmppi::gru_mm<16>(dx, ldst + (cpmppi::GT_L1X + 0) * 64, dar, lane);
        dx = cpmppi::gru_mm<16>(dx, ldst + (cpmppi::GT_L1X + 16) * 64, daz, lane);
        dx = cpmppi::gru_mm<16>(dx, ldst + (cpmppi::GT_L1X + 32) * 64, danx, lane);
      }
      dfb[0] = dx[0]; dfb[1] = dx[1]; dfb[2] = dx[2]; dfb[3] = dx[3];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// D[i][n] = sum over (row j, window b) of A[j,b][i] * B[j,b][n], one product (blockIdx.y) and one slice (blockIdx.x) per wave.
// An MFMA contracts two windows: lane-half hf supplies window 2 s + hf of the tile at k-step s, lane % 32 is the A operand's row i
// and the B operand's column n.  Products 0..11: matrix = task / 3 (w_ih0, w_hh0, w_ih1, w_hh1), gate = task % 3 (r, z, n) - the
// layer's adjoint of that gate (n: its input part for w_ih, its hidden part for w_hh) against the input tile, the layer-1 hidden
// tile of the row before, the layer-1 tile, the layer-2 tile of the row before (`prev`: row 0 has zeros there and is skipped);
// 12: the head adjoint against the layer-2 tile; 13..20: the eight adjoint tiles against ones (bias sums, every column alike);
// 21: the head adjoint against ones.  partial[slice][task][i][n].
__global__ __launch_bounds__(64) void gru_wgrad_kernel(const GruTrainArgs a, float* __restrict__ partial, uint32_t tiles,
                                                       uint32_t per_slice) {
  const uint32_t task = blockIdx.y, slice = blockIdx.x, lane = threadIdx.x, m = lane & 31u, hf = lane >> 5;
  const float* A = a.adj;
  size_t as = ADJ;
  uint32_t am = 32, bn = 32, prev = 0;
  const float* Bm = nullptr;                               // NULL: ones
  if (task < 12) {
    const uint32_t mat = task / 3, g = task % 3;
    const bool hidden = mat & 1u;                          // w_hh: the n gate's hidden part, the tile of the row before
    A += (mat >> 1) * 128 + (g < 2 ? g * 32 : (hidden ? 96 : 64));
    Bm = a.ckpt + (mat == 0 ? CK_X : (mat == 3 ? CK_H2 : 0));
    if (mat == 0) bn = 8;
    prev = hidden ? 1u : 0u;
  } else if (task == 12 || task == 21) {
    A = a.ckpt + CK_DY; as = CK; am = 8;
    if (task == 12) Bm = a.ckpt + CK_H2;
  } else {
    A += (task - 13) * 32;
  }
  f16v acc = zero_tile();
  const uint32_t tpr = a.Bp / 32;                          // window tiles per row
  const uint32_t t0 = slice * per_slice, t1 = min(t0 + per_slice, tiles);
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t j = t / tpr, wt = t % tpr;
    if (prev && j == 0) continue;                          // (wave-uniform)
    const size_t rec = (size_t)j * a.Bp + (size_t)wt * 32 + hf;
    const float* ap = A + rec * as + m;
    const float* bp = Bm ? Bm + (rec - (size_t)prev * a.Bp) * CK + m : nullptr;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float av = m < am ? ap[(size_t)(2 * s) * as] : 0.0f;
      const float bv = Bm ? (m < bn ? bp[(size_t)(2 * s) * CK] : 0.0f) : 1.0f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }
  float* out = partial + ((size_t)slice * WG_TASKS + task) * 1024;
#pragma unroll
  for (int v = 0; v < 16; ++v) out[cpmppi::gru_tile_row(v, hf) * 32 + m] = acc[v];
}

// grad[p] = the slices' partials of parameter p's entry (src[p] = task * 1024 + i * 32 + n), slice 0 first.
__global__ __launch_bounds__(BLOCK) void gru_wgrad_reduce_kernel(const float* __restrict__ partial, uint32_t slices,
                                                                 const int32_t* __restrict__ src, float* __restrict__ grad) {
  const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= CPMPPI_GRU_PARAMS) return;
  const uint32_t at = (uint32_t)src[p];
  const float* in = partial + (size_t)(at >> 10) * 1024 + (at & 1023u);
  float sum = 0.0f;
  for (uint32_t sl = 0; sl < slices; ++sl) sum += in[(size_t)sl * WG_TASKS * 1024];
  grad[p] = sum;
}

// ONE workgroup.  update != 0: Adam on the master copy with t = *step + 1 (cpmppi.h states the update; float64 arithmetic, the moments
// and the weights stored as float32), then *step = t.  Then every float of both images from the master copy: src[2 i], src[2 i + 1]
// name the parameters it is the sum of (-1: none), as gru_image_sources read them off the host packers.
__global__ __launch_bounds__(REPACK_BLOCK) void gru_adam_repack_kernel(float* master, float* mom1, float* mom2, const float* grad,
                                                                       unsigned long long* step, float lr, float beta1, float beta2,
                                                                       float eps, int update, const int32_t* __restrict__ src,
                                                                       float* image, float* image_t) {
  const uint32_t tid = threadIdx.x;
  unsigned long long t = 0;
  if (update) {
    t = *step + 1;
    const AdamStep adam(beta1, beta2, lr, eps, t);
    for (uint32_t p = tid; p < CPMPPI_GRU_PARAMS; p += REPACK_BLOCK)
      master[p] = (float)adam(mom1[p], mom2[p], (double)grad[p], master[p]);
  }
  __syncthreads();                                         // the master copy is whole; every lane has read *step
  if (update && tid == 0) *step = t;
  for (uint32_t i = tid; i < N_IMG; i += REPACK_BLOCK) {
    const int32_t s0 = src[2 * i], s1 = src[2 * i + 1];
    float w = s0 < 0 ? 0.0f : master[s0];
    if (s1 >= 0) w = w + master[s1];
    if (i < (uint32_t)GRU_IMAGE_FLOATS) image[i] = w;
    else image_t[i - GRU_IMAGE_FLOATS] = w;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
uint32_t round32(uint32_t B) { return (B + 31u) & ~31u; }
size_t header_floats(uint32_t Bp) { return (((size_t)Bp / 32 * 2 + 63) & ~(size_t)63) + (size_t)WG_MAX_SLICES * WG_TASKS * 1024; }
size_t need_floats(uint32_t B, uint32_t rows, bool grad) {
  const uint32_t Bp = round32(B);
  return header_floats(Bp) + (grad ? (size_t)rows * Bp * (CK + ADJ) : 0);
}

// src[p] = task * 1024 + i * 32 + n of gru_wgrad_kernel's output for parameter p of the flat order.  Columns of w_ih0 follow xcol of
// cpmppi_gru_model.hip (input 0 = Q is tile row 5, inputs 1..5 rows 0..4); b_ih and b_hh of the r and z gates read the same sum,
// b_in the n gate's input part, b_hn its hidden part.
void gradient_sources(int32_t* src) {
  size_t p = 0;
  const auto put = [&](int task, int i, int n) { src[p++] = task * 1024 + i * 32 + n; };
  for (int l = 0; l < 2; ++l) {
    const int K = l == 0 ? 6 : 32;
    for (int u = 0; u < 96; ++u)
      for (int k = 0; k < K; ++k) put(6 * l + u / 32, u % 32, l == 0 ? (k == 0 ? 5 : k - 1) : k);
    for (int u = 0; u < 96; ++u)
      for (int k = 0; k < 32; ++k) put(6 * l + 3 + u / 32, u % 32, k);
    for (int u = 0; u < 96; ++u) put(13 + 4 * l + u / 32, u % 32, 0);
    for (int u = 0; u < 96; ++u) put(13 + 4 * l + (u / 32 == 2 ? 3 : u / 32), u % 32, 0);
  }
  for (int o = 0; o < 5; ++o)
    for (int k = 0; k < 32; ++k) put(12, o, k);
  for (int o = 0; o < 5; ++o) put(21, o, 0);
}

// The handle's training state with a workspace of `need` floats: allocated on first use, never inside a capture.
int ensure(cpmppi_handle* h, size_t need, hipStream_t s, const char* who) {
  if (h->gru_train && h->gru_train->tables && h->gru_train->ws_floats >= need) return CPMPPI_OK;
  if (const int rc = refuse_unreserved_capture(h, s, who, "cpmppi_gru_train_reserve")) return rc;
  if (!h->gru_train) h->gru_train = new GruTrain();
  GruTrain* st = h->gru_train;
  if (!st->tables) {
    std::vector<int32_t> tab;
    gru_image_sources(tab);
    tab.resize(2 * N_IMG + CPMPPI_GRU_PARAMS);
    gradient_sources(tab.data() + 2 * N_IMG);
    CPMPPI_HIP(h, hipMalloc(&st->tables, tab.size() * sizeof(int32_t)));
    CPMPPI_HIP(h, hipMemcpy(st->tables, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    allow_large_lds(&gru_train_reverse_kernel<false>);
    allow_large_lds(&gru_train_reverse_kernel<true>);
  }
  return grow_workspace(h, st->ws, st->ws_floats, need);
}

// What cpmppi_gru_loss_grad refuses before it launches (cpmppi.h lists it), in `who`'s name; `rollout`: and a label that is not the
// next row, which could not be fed back.
int check_loss_args(cpmppi_handle* h, const cpmppi_gru_loss_args* a, bool rollout, const char* who) {
  if (const int rc = gru_refusal(h, who, a->B != 0 && a->R != 0 && a->T != 0 && a->post_wash_out != 0,
                                 "B, R, T and post_wash_out must be at least 1",
                                 a->states && a->Q && a->windows && a->windows_host && a->loss_out,
                                 "states, Q, windows, windows_host and loss_out are required")) return rc;
  if (rollout && a->shift_labels != 1)
    return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": shift_labels must be 1 (the output of a row is the input of the next), got " +
                                           std::to_string(a->shift_labels));
  if (misaligned(a->states) || misaligned(a->Q) || misaligned(a->windows) || misaligned(a->windows_host) || misaligned(a->grad_out) ||
      misaligned8(a->loss_out))
    return fail(h, CPMPPI_ERR_ALIGN, std::string(who) + ": misaligned pointer");
  // rows from t0 to the last label, inclusive (every window fits, so wash_out + post_wash_out <= T: no overflow below)
  return check_windows(h, who, a->windows_host, a->B, a->R, a->T, (uint64_t)a->wash_out + a->post_wash_out + a->shift_labels,
                       "r < R, t0 + wash_out + post_wash_out - 1 + shift_labels <= T - 1");
}

// The launches of one loss (and gradient into `grad`, or NULL) on `s`, teacher-forced or through the open-loop `rollout`; the
// arguments are checked and the workspace is large enough.
void launch_loss_grad(cpmppi_handle* h, const cpmppi_gru_loss_args* a, float* grad, bool rollout, hipStream_t s) {
  GruTrain* st = h->gru_train;
  const uint32_t Bp = round32(a->B), L = a->wash_out + a->post_wash_out, wave_tiles = Bp / 32;
  double* loss_part = reinterpret_cast<double*>(st->ws);
  float* partial = st->ws + (header_floats(Bp) - (size_t)WG_MAX_SLICES * WG_TASKS * 1024);
  float* ckpt = st->ws + header_floats(Bp);
  const double count = (double)a->B * a->post_wash_out * 5.0;
  const GruTrainArgs k{a->states, a->Q, a->windows, a->B, Bp, a->T, a->wash_out, L, a->shift_labels, (float)(2.0 / count),
                       grad ? ckpt : nullptr, grad ? ckpt + (size_t)L * Bp * CK : nullptr, loss_part};
  const dim3 grid((a->B + GRU_ROLLOUTS_PER_BLOCK - 1) / GRU_ROLLOUTS_PER_BLOCK);
  const size_t lds = (size_t)GRU_IMAGE_FLOATS * sizeof(float);
  const auto forward = rollout ? (grad ? &gru_train_forward_kernel<true, true> : &gru_train_forward_kernel<false, true>)
                               : (grad ? &gru_train_forward_kernel<true, false> : &gru_train_forward_kernel<false, false>);
  hipLaunchKernelGGL(forward, grid, dim3(BLOCK), lds, s, h->gru_norm, (const float*)h->gru_image, k);
  hipLaunchKernelGGL(gru_loss_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)loss_part, (a->B + 31u) / 32u, count, a->loss_out);
  if (!grad) return;
  hipLaunchKernelGGL(rollout ? &gru_train_reverse_kernel<true> : &gru_train_reverse_kernel<false>, grid, dim3(BLOCK), REVERSE_LDS, s,
                     (const float*)h->gru_image, (const float*)h->gru_t_image, k);
  const uint64_t tiles = (uint64_t)L * wave_tiles;
  uint64_t per_slice = (tiles + WG_MAX_SLICES - 1) / WG_MAX_SLICES;
  if (per_slice < WG_MIN_TILES) per_slice = WG_MIN_TILES;
  const uint32_t slices = (uint32_t)((tiles + per_slice - 1) / per_slice);
  hipLaunchKernelGGL(gru_wgrad_kernel, dim3(slices, WG_TASKS), dim3(64), 0, s, k, partial, (uint32_t)tiles, (uint32_t)per_slice);
  hipLaunchKernelGGL(gru_wgrad_reduce_kernel, dim3((CPMPPI_GRU_PARAMS + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, (const float*)partial,
                     slices, (const int32_t*)(st->tables + 2 * N_IMG), grad);
}

int loss_grad_impl(cpmppi_handle* h, const cpmppi_gru_loss_args* a, float* grad, bool rollout, hipStream_t s, const char* who) {
  if (const int rc = check_loss_args(h, a, rollout, who)) return rc;
  const uint64_t tiles = (uint64_t)(a->wash_out + a->post_wash_out) * (round32(a->B) / 32);
  if (tiles > 0xffffffffull) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": too many (row, window) tiles");
  if (const int rc = ensure(h, need_floats(a->B, a->wash_out + a->post_wash_out, grad != nullptr), s, who)) return rc;
  launch_loss_grad(h, a, grad, rollout, s);
  return launched(h);
}

// cpmppi_gru_loss_grad and cpmppi_gru_rollout_loss_grad, in `who`'s name.
int loss_grad_entry(cpmppi_handle* h, const cpmppi_gru_loss_args* a, bool rollout, void* stream, const char* who) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": null argument block");
  CPMPPI_ON_DEVICE(h);
  return loss_grad_impl(h, a, a->grad_out, rollout, (hipStream_t)stream, who);
}

void launch_adam_repack(cpmppi_handle* h, float lr, float beta1, float beta2, float eps, int update, hipStream_t s) {
  GruTrain* st = h->gru_train;
  float* p = st->master;
  hipLaunchKernelGGL(gru_adam_repack_kernel, dim3(1), dim3(REPACK_BLOCK), 0, s, p, p + CPMPPI_GRU_PARAMS, p + 2 * CPMPPI_GRU_PARAMS,
                     (const float*)(p + 3 * CPMPPI_GRU_PARAMS), st->step, lr, beta1, beta2, eps, update, (const int32_t*)st->tables,
                     h->gru_image, h->gru_t_image);
}

// cpmppi_gru_train_step and cpmppi_gru_rollout_train_step, in `who`'s name.
int train_step_entry(cpmppi_handle* h, const cpmppi_gru_loss_args* a, bool rollout, float lr, float beta1, float beta2, float eps,
                     void* stream, const char* who) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a) return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": null argument block");
  if (const int rc = begun_or_refuse(h, who, h->gru_train && h->gru_train->begun, "cpmppi_gru_train_begin")) return rc;
  CPMPPI_ON_DEVICE(h);
  if (const int rc = loss_grad_impl(h, a, h->gru_train->master + 3 * (size_t)CPMPPI_GRU_PARAMS, rollout, (hipStream_t)stream, who))
    return rc;
  launch_adam_repack(h, lr, beta1, beta2, eps, 1, (hipStream_t)stream);
  return launched(h);
}

}  // namespace

void gru_train_destroy(cpmppi_handle* h) {
  GruTrain* st = h->gru_train;
  if (!st) return;
  if (st->ws) (void)hipFree(st->ws);
  if (st->tables) (void)hipFree(st->tables);
  if (st->master) (void)hipFree(st->master);
  if (st->step) (void)hipFree(st->step);
  delete st;
  h->gru_train = nullptr;
}

void gru_train_end(cpmppi_handle* h) {
  if (h->gru_train) h->gru_train->begun = false;           // the workspace and the tables stay: they do not depend on the model
}

extern "C" {

int cpmppi_gru_train_reserve(cpmppi_handle* h, uint32_t B, uint32_t rows) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (B == 0 || rows == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_train_reserve: B and rows must be at least 1");
  CPMPPI_ON_DEVICE(h);
  return ensure(h, need_floats(B, rows, true), nullptr, "cpmppi_gru_train_reserve");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

int cpmppi_gru_loss_grad(cpmppi_handle* h, const cpmppi_gru_loss_args* a, void* stream) try {
  return loss_grad_entry(h, a, false, stream, "cpmppi_gru_loss_grad");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_gru_rollout_loss_grad(cpmppi_handle* h, const cpmppi_gru_loss_args* a, void* stream) try {
  return loss_grad_entry(h, a, true, stream, "cpmppi_gru_rollout_loss_grad");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_gru_train_begin(cpmppi_handle* h) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!h->gru_image || h->gru_params.size() != CPMPPI_GRU_PARAMS)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_train_begin: no model set (cpmppi_set_gru)");
  CPMPPI_ON_DEVICE(h);
  if (const int rc = ensure(h, 0, nullptr, "cpmppi_gru_train_begin")) return rc;
  GruTrain* st = h->gru_train;
  const size_t bytes = (size_t)CPMPPI_GRU_PARAMS * sizeof(float);
  if (!st->master) CPMPPI_HIP(h, hipMalloc(&st->master, 4 * bytes));
  if (!st->step) CPMPPI_HIP(h, hipMalloc(&st->step, sizeof(unsigned long long)));
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemset(st->master, 0, 4 * bytes));
  CPMPPI_HIP(h, hipMemset(st->step, 0, sizeof(unsigned long long)));
  CPMPPI_HIP(h, hipMemcpy(st->master, h->gru_params.data(), bytes, hipMemcpyHostToDevice));
  launch_adam_repack(h, 0.0f, 0.0f, 0.0f, 0.0f, 0, nullptr);
  CPMPPI_HIP(h, hipGetLastError());
  CPMPPI_HIP(h, hipDeviceSynchronize());
  st->begun = true;
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_gru_train_step(cpmppi_handle* h, const cpmppi_gru_loss_args* a, float lr, float beta1, float beta2, float eps,
                          void* stream) try {
  return train_step_entry(h, a, false, lr, beta1, beta2, eps, stream, "cpmppi_gru_train_step");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_gru_rollout_train_step(cpmppi_handle* h, const cpmppi_gru_loss_args* a, float lr, float beta1, float beta2, float eps,
                                  void* stream) try {
  return train_step_entry(h, a, true, lr, beta1, beta2, eps, stream, "cpmppi_gru_rollout_train_step");
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }

int cpmppi_gru_train_get(cpmppi_handle* h, float* params_host) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!params_host) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_gru_train_get: params_host is required");
  if (const int rc = begun_or_refuse(h, "cpmppi_gru_train_get", h->gru_train && h->gru_train->begun, "cpmppi_gru_train_begin")) return rc;
  CPMPPI_ON_DEVICE(h);
  CPMPPI_HIP(h, hipDeviceSynchronize());
  CPMPPI_HIP(h, hipMemcpy(params_host, h->gru_train->master, (size_t)CPMPPI_GRU_PARAMS * sizeof(float), hipMemcpyDeviceToHost));
  return CPMPPI_OK;
}

}  // extern "C"
