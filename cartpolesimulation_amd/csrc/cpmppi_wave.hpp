// cpmppi_wave.hpp — wave64 reductions on the DPP lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace cpmppi {

// ------------------------------------------------------------------------------------------------------------------
// wave64 reductions
// Wave-wide reductions on the VALU's data-parallel-primitive lanes (no LDS round trips: a __shfl_xor butterfly is six
// DEPENDENT ds_bpermute_b32: single env 61.0 -> 60.1 us, C4 93.6 -> 91.5 us, neutral at 8192 envs).  Four DPP steps
// leave every lane of a 16-lane row with its row's result (quad swaps, half-row mirror, row mirror), the four row
// results are combined through scalar registers.  The result is wave-uniform.
template <int CTRL>
__device__ __forceinline__ float dpp_(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_lane_(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wave_min(float v) {
  v = fminf(v, dpp_<0xB1>(v));      // quad_perm [1,0,3,2]
  v = fminf(v, dpp_<0x4E>(v));      // quad_perm [2,3,0,1]
  v = fminf(v, dpp_<0x141>(v));     // row_half_mirror
  v = fminf(v, dpp_<0x140>(v));     // row_mirror
  return fminf(fminf(row_lane_(v, 0), row_lane_(v, 16)), fminf(row_lane_(v, 32), row_lane_(v, 48)));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_<0xB1>(v);
  v += dpp_<0x4E>(v);
  v += dpp_<0x141>(v);
  v += dpp_<0x140>(v);
  return (row_lane_(v, 0) + row_lane_(v, 16)) + (row_lane_(v, 32) + row_lane_(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_<0xB1>(v));
  v = fmaxf(v, dpp_<0x4E>(v));
  v = fmaxf(v, dpp_<0x141>(v));
  v = fmaxf(v, dpp_<0x140>(v));
  return fmaxf(fmaxf(row_lane_(v, 0), row_lane_(v, 16)), fmaxf(row_lane_(v, 32), row_lane_(v, 48)));
}

}  // namespace cpmppi
