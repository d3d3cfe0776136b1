// cpmppi_gru_model.hip — host code only: cpmppi_set_gru packs a GRU-6IN-32H1-32H2-5OUT model into the three weight images of the
// GRU kernels - the exact f32 fragments + plain vectors (cpmppi_gru.hpp, GF_* / GV_*), the f16 split (cpmppi_gru16.hpp, HF_*) and
// the transposed fragments of the reverse sweep (cpmppi_gru.hpp, GT_*), one function each over a plain host buffer - and uploads them.
#include <math.h>
#include <exception>
#include <vector>
#include "cpmppi_gru16.hpp"      // (and cpmppi_gru.hpp, cpmppi_internal.hpp)

using namespace cpmppi_k;

namespace {

// x-tile row r -> network input column: rows 0..4 = the 5 state features (inputs 1..5), row 5 = Q (input 0)
int xcol(int r) { return r < 5 ? r + 1 : (r == 5 ? 0 : -1); }

// The exact f32 image: A fragments (fragment f = 64 floats, one per lane), then the plain vectors of the fused rollout kernel
// (biases as accumulator tiles, dense head on the VALU).
void pack_f32_image(const cpmppi_gru_model* m, float* img) {
  auto frag = [&](int f) { return img + (size_t)f * 64; };
  for (int g = 0; g < 3; ++g) {
    for (int s = 0; s < 4; ++s)
      for (int l = 0; l < 64; ++l) {
        const int col = xcol(gru_tile_row(s, l >> 5));
        frag(GF_L1X + g * 4 + s)[l] = col < 0 ? 0.0f : m->w_ih[0][(size_t)(g * 32 + (l & 31)) * 6 + col];
      }
    for (int s = 0; s < 16; ++s)
      for (int l = 0; l < 64; ++l) {
        const int k = gru_tile_row(s, l >> 5);
        const size_t row = (size_t)(g * 32 + (l & 31));
        frag(GF_L1H + g * 16 + s)[l] = m->w_hh[0][row * 32 + k];
        frag(GF_L2X + g * 16 + s)[l] = m->w_ih[1][row * 32 + k];
        frag(GF_L2H + g * 16 + s)[l] = m->w_hh[1][row * 32 + k];
      }
  }
  // the four gate biases of a layer - r (b_ir + b_hr), z (b_iz + b_hz), n_x (b_in), n_h (b_hn) - of unit j, once as a fragment
  // (lane-half 0 carries the bias, k = 0; half 1 zeros) and once as the vector [lane half][register] that holds unit j there
  for (int layer = 0; layer < 2; ++layer)
    for (int hf = 0; hf < 2; ++hf)
      for (int v = 0; v < 16; ++v) {
        const int j = gru_tile_row(v, hf);
        const float *bi = m->b_ih[layer], *bh = m->b_hh[layer];
        const float b[4] = {bi[j] + bh[j], bi[32 + j] + bh[32 + j], bi[64 + j], bh[64 + j]};
        for (int kind = 0; kind < 4; ++kind) {
          frag((layer == 0 ? GF_L1B : GF_L2B) + kind)[j] = b[kind];
          img[GV_BIAS + (size_t)(layer * 4 + kind) * 32 + hf * 16 + v] = b[kind];
        }
      }
  for (int s = 0; s < 16; ++s)
    for (int l = 0; l < 64; ++l)
      frag(GF_DW + s)[l] = (l & 31) < 5 ? m->w_out[(size_t)(l & 31) * 32 + gru_tile_row(s, l >> 5)] : 0.0f;
  for (int l = 0; l < 5; ++l) frag(GF_DB)[l] = m->b_out[l];
  for (int hf = 0; hf < 2; ++hf)
    for (int o = 0; o < 5; ++o)
      for (int v = 0; v < 16; ++v)
        img[GV_HEAD + (size_t)hf * 80 + o * 16 + v] = m->w_out[(size_t)o * 32 + gru_tile_row(v, hf)];
  for (int o = 0; o < 5; ++o) img[GV_HEADB + o] = m->b_out[o];
}

// The f16 split image (cpmppi_gru16.hpp): fragment f holds, for lane l and t = 0..7, the weight of output row l%32 against k-slot
// (block b, lane half l/32, t) = tile register v = 8b + t of that half; its gate biases are those of the f32 image `img`.
// false: a weight lies beyond the f16 range.
bool pack_f16_image(const cpmppi_gru_model* m, const float* img, unsigned char* img16) {
  bool in_range = true;
  auto put16 = [&](int f, int lane, int t, float w) {
    const _Float16 hi = (_Float16)w;
    const _Float16 lo = (_Float16)(w - (float)hi);
    if (!(fabsf(w) < 60000.0f)) in_range = false;
    reinterpret_cast<_Float16*>(img16 + (size_t)f * G16_FRAG_BYTES + lane * 16)[t] = hi;
    reinterpret_cast<_Float16*>(img16 + (size_t)(f + 1) * G16_FRAG_BYTES + lane * 16)[t] = lo;
  };
  // gate rows pre-scaled so that the gates need no multiply before v_exp_f32 (gru16_gates_overlapped): r, z by -log2(e), n by 2 log2(e)
  const double LOG2E = 1.4426950408889634;
  const double gate_scale[3] = {-LOG2E, -LOG2E, 2.0 * LOG2E};
  auto sc = [&](int g, float w) { return (float)(gate_scale[g] * (double)w); };
  for (int g = 0; g < 3; ++g)
    for (int l = 0; l < 64; ++l)
      for (int tt = 0; tt < 8; ++tt) {
        const size_t row = (size_t)(g * 32 + (l & 31));
        const int col = xcol(gru_tile_row(tt, l >> 5));                       // x tile registers 0..7
        put16(HF_L1X + g * 2, l, tt, (col < 0 || tt >= 4) ? 0.0f : sc(g, m->w_ih[0][row * 6 + col]));
        for (int b = 0; b < 2; ++b) {
          const int k = gru_tile_row(8 * b + tt, l >> 5);
          put16(HF_L1H + (g * 2 + b) * 2, l, tt, sc(g, m->w_hh[0][row * 32 + k]));
          put16(HF_L2X + (g * 2 + b) * 2, l, tt, sc(g, m->w_ih[1][row * 32 + k]));
          put16(HF_L2H + (g * 2 + b) * 2, l, tt, sc(g, m->w_hh[1][row * 32 + k]));
        }
      }
  for (int b = 0; b < 2; ++b)
    for (int l = 0; l < 64; ++l)
      for (int tt = 0; tt < 8; ++tt)
        put16(HF_HEAD + b * 2, l, tt, (l & 31) < 5 ? m->w_out[(size_t)(l & 31) * 32 + gru_tile_row(8 * b + tt, l >> 5)] : 0.0f);
  float* bv = reinterpret_cast<float*>(img16 + G16_BIAS_OFF);
  for (int i = 0; i < 8 * 32; ++i) {                                          // the same 8 gate-bias tiles, scaled alike
    const int kind = (i / 32) % 4;                                            // r, z, n_x, n_h
    bv[i] = (float)(gate_scale[kind < 2 ? kind : 2] * (double)img[GV_BIAS + i]);
  }
  for (int hf = 0; hf < 2; ++hf)
    for (int v = 0; v < 16; ++v) {
      const int r = gru_tile_row(v, hf);
      bv[8 * 32 + hf * 16 + v] = r < 5 ? m->b_out[r] : 0.0f;
    }
  return in_range;
}

// The transposed image of the reverse sweep (cpmppi_gru.hpp, GT_*): fragment s of W^T holds W[unit(s, lane half)][lane % 32].
void pack_transposed_image(const cpmppi_gru_model* m, float* imgt) {
  auto fragt = [&](int f) { return imgt + (size_t)f * 64; };
  for (int g = 0; g < 3; ++g)
    for (int s = 0; s < 16; ++s)
      for (int l = 0; l < 64; ++l) {
        const size_t unit = (size_t)(g * 32 + gru_tile_row(s, l >> 5));
        const int mrow = l & 31;
        const int col = mrow < 8 ? xcol(mrow) : -1;
        fragt(GT_L1X + g * 16 + s)[l] = col < 0 ? 0.0f : m->w_ih[0][unit * 6 + col];
        fragt(GT_L1H + g * 16 + s)[l] = m->w_hh[0][unit * 32 + mrow];
        fragt(GT_L2X + g * 16 + s)[l] = m->w_ih[1][unit * 32 + mrow];
        fragt(GT_L2H + g * 16 + s)[l] = m->w_hh[1][unit * 32 + mrow];
      }
  for (int s = 0; s < 4; ++s)
    for (int l = 0; l < 64; ++l) {
      const int o = gru_tile_row(s, l >> 5);
      fragt(GT_HEAD + s)[l] = o < 5 ? m->w_out[(size_t)o * 32 + (l & 31)] : 0.0f;
    }
}

// The flat parameter vector (CPMPPI_GRU_PARAMS, the order of cpmppi_gru_model's fields) and a model that points into one.
constexpr size_t FLAT_SIZES[10] = {96 * 6, 96 * 32, 96, 96, 96 * 32, 96 * 32, 96, 96, 5 * 32, 5};
cpmppi_gru_model flat_model(const float* p) {
  cpmppi_gru_model m{};
  m.inputs = 6; m.hidden = 32; m.layers = 2; m.outputs = 5;
  for (int l = 0; l < 2; ++l) {
    m.w_ih[l] = p; p += FLAT_SIZES[4 * l + 0];
    m.w_hh[l] = p; p += FLAT_SIZES[4 * l + 1];
    m.b_ih[l] = p; p += FLAT_SIZES[4 * l + 2];
    m.b_hh[l] = p; p += FLAT_SIZES[4 * l + 3];
  }
  m.w_out = p; p += FLAT_SIZES[8];
  m.b_out = p;
  return m;
}
void flatten_model(const cpmppi_gru_model* m, std::vector<float>& flat) {
  const float* src[10] = {m->w_ih[0], m->w_hh[0], m->b_ih[0], m->b_hh[0], m->w_ih[1], m->w_hh[1], m->b_ih[1], m->b_hh[1], m->w_out, m->b_out};
  flat.clear();
  for (int i = 0; i < 10; ++i) flat.insert(flat.end(), src[i], src[i] + FLAT_SIZES[i]);
}

}  // namespace

// The two packers run twice over weights that name themselves - parameter i holds i + 1 (exact in float32), once with every b_hh
// zero and once with the b_hh alone - so a float of an image reads back which parameter it is (0: none), and a gate bias that is
// the sum b_ih + b_hh reads back one term per run.
void gru_image_sources(std::vector<int32_t>& src) {
  const size_t P = CPMPPI_GRU_PARAMS, n = (size_t)GRU_IMAGE_FLOATS + GRU_T_IMAGE_FLOATS;
  std::vector<float> flat[2] = {std::vector<float>(P, 0.0f), std::vector<float>(P, 0.0f)};
  size_t at = 0;
  for (int i = 0; i < 10; ++i) {
    const bool hh = i == 3 || i == 7;                      // b_hh0, b_hh1
    for (size_t k = 0; k < FLAT_SIZES[i]; ++k, ++at) flat[hh ? 1 : 0][at] = (float)(at + 1);
  }
  std::vector<float> img[2];
  for (int run = 0; run < 2; ++run) {
    img[run].assign(n, 0.0f);
    const cpmppi_gru_model m = flat_model(flat[run].data());
    pack_f32_image(&m, img[run].data());
    pack_transposed_image(&m, img[run].data() + GRU_IMAGE_FLOATS);
  }
  src.assign(2 * n, -1);
  for (size_t i = 0; i < n; ++i) {
    int k = 0;
    for (int run = 0; run < 2; ++run)
      if (img[run][i] != 0.0f) src[2 * i + k++] = (int32_t)img[run][i] - 1;
  }
}

extern "C" {

int cpmppi_set_gru(cpmppi_handle* h, const cpmppi_gru_model* m) try {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!m || m->hidden != 32 || m->layers != 2 || m->inputs != 6 || m->outputs != 5)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: only GRU-6IN-32H1-32H2-5OUT is built");
  for (int l = 0; l < 2; ++l)
    if (!m->w_ih[l] || !m->w_hh[l] || !m->b_ih[l] || !m->b_hh[l]) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: null weights");
  if (!m->w_out || !m->b_out) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: null head weights");
  // Everything that can refuse the model comes first and touches locals only: a refused call leaves the handle - the three images,
  // the normalisation, gru_params and a training run - exactly as it found them.  (The normalisation vectors may be NULL: identity.)
  const struct { const char* name; const float* p; size_t n; } tensors[14] = {
      {"w_ih0", m->w_ih[0], 96 * 6}, {"w_hh0", m->w_hh[0], 96 * 32}, {"b_ih0", m->b_ih[0], 96},
      {"b_hh0", m->b_hh[0], 96},     {"w_ih1", m->w_ih[1], 96 * 32}, {"w_hh1", m->w_hh[1], 96 * 32},
      {"b_ih1", m->b_ih[1], 96},     {"b_hh1", m->b_hh[1], 96},     {"w_out", m->w_out, 5 * 32},
      {"b_out", m->b_out, 5},        {"in_scale", m->in_scale, 6},   {"in_shift", m->in_shift, 6},
      {"out_scale", m->out_scale, 5}, {"out_shift", m->out_shift, 5}};
  for (const auto& t : tensors)
    for (size_t i = 0; t.p && i < t.n; ++i)
      if (!isfinite(t.p[i])) return fail(h, CPMPPI_ERR_BAD_ARG, std::string("cpmppi_set_gru: non-finite value in ") + t.name);
  cpmppi::GruNorm norm;
  for (int i = 0; i < 6; ++i) {
    norm.in_scale[i] = m->in_scale ? m->in_scale[i] : 1.0f;
    norm.in_shift[i] = m->in_shift ? m->in_shift[i] : 0.0f;
  }
  for (int i = 0; i < 5; ++i) {
    norm.out_scale[i] = m->out_scale ? m->out_scale[i] : 1.0f;
    norm.out_shift[i] = m->out_shift ? m->out_shift[i] : 0.0f;
  }
  std::vector<float> img((size_t)GRU_IMAGE_FLOATS, 0.0f), imgt((size_t)GRU_T_IMAGE_FLOATS, 0.0f), flat;
  std::vector<unsigned char> img16((size_t)G16_IMAGE_BYTES, 0);
  pack_f32_image(m, img.data());
  if (!pack_f16_image(m, img.data(), img16.data())) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_set_gru: weights beyond the f16 range");
  pack_transposed_image(m, imgt.data());
  flatten_model(m, flat);
  CPMPPI_ON_DEVICE(h);
  // ... then the device buffers a first call needs, all three or none: `gru_image` is what every entry point reads as "a model is set"
  void* fresh[3] = {nullptr, nullptr, nullptr};
  const size_t bytes[3] = {img.size() * sizeof(float), imgt.size() * sizeof(float), img16.size()};
  const bool have[3] = {h->gru_image != nullptr, h->gru_t_image != nullptr, h->gru16_image != nullptr};
  for (int i = 0; i < 3; ++i)
    if (!have[i]) {
      const hipError_t e = hipMalloc(&fresh[i], bytes[i]);
      if (e != hipSuccess) {
        for (int k = 0; k < i; ++k)
          if (fresh[k]) (void)hipFree(fresh[k]);
        return fail(h, CPMPPI_ERR_HIP, std::string("cpmppi_set_gru: hipMalloc: ") + hipGetErrorString(e));
      }
    }
  // ... and only now the handle changes: buffers, uploads, normalisation, the flat copy and the end of a training run together
  if (!have[0]) h->gru_image = (float*)fresh[0];
  if (!have[1]) h->gru_t_image = (float*)fresh[1];
  if (!have[2]) h->gru16_image = fresh[2];
  CPMPPI_HIP(h, hipMemcpy(h->gru_image, img.data(), bytes[0], hipMemcpyHostToDevice));
  CPMPPI_HIP(h, hipMemcpy(h->gru_t_image, imgt.data(), bytes[1], hipMemcpyHostToDevice));
  CPMPPI_HIP(h, hipMemcpy(h->gru16_image, img16.data(), bytes[2], hipMemcpyHostToDevice));
  allow_large_lds_gru_adjoint();      // (both images in LDS: beyond the default 64 KB)
  allow_large_lds_gru_rpgd();         // (... and the fused rpgd step keeps the rollout's image beside them)
  h->gru_norm = norm;
  h->gru_params.swap(flat);           // (what cpmppi_gru_train_begin starts from)
  gru_train_end(h);                   // (a master copy of the model before this one must not be stepped on: cpmppi_gru_train_begin again)
  return CPMPPI_OK;
} catch (const std::exception&) { return CPMPPI_ERR_NOMEM; }   // (no C++ exception leaves the C ABI)

}  // extern "C"
