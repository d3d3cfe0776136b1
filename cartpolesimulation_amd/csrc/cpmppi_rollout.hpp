// cpmppi_rollout.hpp — the hot path: rollout_cost_kernel.  A header because the kernel is instantiated in several
// translation units compiled with different instruction-scheduling strategies (cpmppi_rollout_latency.hip /
// cpmppi_rollout_throughput.hip / ...): a launch of at most one wave per SIMD is bound by the latency of a single wave's
// instruction stream, larger ones by issue throughput, and the compiler's schedulers differ measurably on the two.
// Included by the cpmppi_rollout_*.hip units, which instantiate the kernel, and by cpmppi.hip, which launches it and sets
// CPMPPI_ROLLOUT_DECLARATIONS_ONLY first; what the other units share about a step is in cpmppi_step.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cpmppi_params.hpp"
#include "cpmppi_step.hpp"

namespace cpmppi_k {
using namespace cpmppi;

// The hot path.  R = rollouts per lane (1: latency mapping, 2: packed float2 throughput mapping, FAST only).
// A block of 256 threads owns 256*R consecutive rollouts of one env; wave w owns rows [w*64*R, (w+1)*64*R) and lane l
// integrates rows l (component 0) and l+64 (component 1).
// VARIANT selects the translation unit (hence the scheduling strategy) an instantiation is compiled in:
// 0 = latency build (one rollout per lane, launches of at most one wave per SIMD), 1 = throughput build, 2 = packed
// mapping for mid-sized launches (same code except where the loop constants live, see below).
// INTEG selects the in-tree ODE predictor the rollouts are integrated with: PREDICTOR_ODE_V0 (predictor_ODE_v0: simultaneous
// Euler, edge bounce, fmod wrap - the north-star path) or PREDICTOR_ODE (predictor_ODE: Euler-Cromer, no bounce, atan2 wrap;
// cpmppi_ode.hpp).  The second has no events, hence no phased loop: it is built in the latency and throughput forms only.
// The definition lives in cpmppi_rollout_kernel.inc and is compiled under TWO names: rollout_cost_kernel, and - predictor_ODE with
// the pole mass read PER ENV (cpmppi_set_pole_mass_rows) - rollout_cost_rows_kernel, launched only while an array is registered:
// with the pointer unset a handle launches the very code it launched before the per-env mass existed.  (First built as a run-time
// null test inside the PREDICTOR_ODE kernels: the pointer's two scalars live in the prologue moved the lone-wave Philox kernel from
// 22 to 31 spilled scalars, and C4 on predictor_ODE from 58.7 to 59.8 us - profiles/HISTORY.md.  Not a shared __device__ body
// either: as an inlined function the same text compiles to other code in every unit - one kernel with a scratch slot.)
// (the declarations: all that cpmppi.hip sees of the kernels, and the one place INTEG's default is written)
template <int COST, bool FAST, int NOISE, int R, int VARIANT, int INTEG = PREDICTOR_ODE_V0>
__global__ void rollout_cost_kernel(const Params p, const StepPtrs a);
template <int COST, bool FAST, int NOISE, int R, int VARIANT, int INTEG = PREDICTOR_ODE>
__global__ void rollout_cost_rows_kernel(const Params p, const StepPtrs a);
// ... and a third: rollout_cost_tuned_kernel, the cost weights, LBD and sigma read PER ENV (cpmppi_set_tuning_rows), launched only
// while such rows are registered - quadratic_boundary_grad_minimal with Philox noise, both ODE predictors.
template <int COST, bool FAST, int NOISE, int R, int VARIANT, int INTEG = PREDICTOR_ODE_V0>
__global__ void rollout_cost_tuned_kernel(const Params p, const StepPtrs a);

}  // namespace cpmppi_k

#ifndef CPMPPI_ROLLOUT_DECLARATIONS_ONLY
#include <type_traits>
#include "cpmppi_debug.hpp"
#include "cpmppi_ode.hpp"
#include "cpmppi_cost.hpp"
#include "cpmppi_philox.hpp"
#include "cpmppi_wave.hpp"

namespace cpmppi_k {

// 16 bytes per lane from a per-lane global address straight into LDS at (wave-uniform `lds`) + 16 * lane - gfx950's
// global_load_lds_dwordx4; tracked by vmcnt.  (The builtin exists in the device pass only; the host pass, which merely
// emits the kernel's launch stub, sees an empty body.)
__device__ __forceinline__ void load16_to_lds(const float* gptr, float* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(gptr, lds, 16, 0, 0);
#else
  (void)gptr; (void)lds;
#endif
}

// The StepPtrs kernel argument re-read from the kernarg segment at the point of call (the kernels here take
// (const Params, const StepPtrs): the second argument sits at the first 8-byte boundary after the first).
__device__ __forceinline__ StepPtrs late_step_ptrs() {
  typedef const __attribute__((address_space(4))) char* kptr;
  kptr k = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  static_assert(alignof(StepPtrs) == 8 && sizeof(StepPtrs) % 8 == 0, "kernarg layout");
  const __attribute__((address_space(4))) uint64_t* w =
      (const __attribute__((address_space(4))) uint64_t*)(k + ((sizeof(Params) + 7u) & ~(size_t)7u));
  union { StepPtrs s; uint64_t w[sizeof(StepPtrs) / 8]; } u;
#pragma unroll
  for (size_t i = 0; i < sizeof(StepPtrs) / 8; ++i) u.w[i] = w[i];       // (only the words of fields used later survive)
  return u.s;
}

// ... and the Params argument likewise: the fields a late use names are loaded there and then instead of being kept (or spilled
// and reloaded) through the horizon loop.  Params is the FIRST argument of the (const Params, const StepPtrs) signature, i.e. at
// offset 0 of the kernarg segment (late_step_ptrs above relies on the same layout for the second), and what comes back is the
// launch's argument as passed: a kernel that computes with a modified copy (predictor_ODE's `pi`, the pole mass per env) must not
// take that copy's fields from here.  (Beside late_step_ptrs rather than in cpmppi_params.hpp: both are statements about this
// header's kernel signature.)
__device__ __forceinline__ Params late_params() {
  typedef const __attribute__((address_space(4))) char* kptr;
  kptr k = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  static_assert(sizeof(Params) % 4 == 0, "kernarg layout");
  const __attribute__((address_space(4))) uint32_t* w = (const __attribute__((address_space(4))) uint32_t*)k;
  union { Params s; uint32_t w[sizeof(Params) / 4]; } u;
#pragma unroll
  for (size_t i = 0; i < sizeof(Params) / 4; ++i) u.w[i] = w[i];
  return u.s;
}

#define CPMPPI_ROLLOUT_KERNEL rollout_cost_kernel
#define CPMPPI_ROLLOUT_MASS_ROWS false
#define CPMPPI_ROLLOUT_TUNING_ROWS false
#include "cpmppi_rollout_kernel.inc"
#undef CPMPPI_ROLLOUT_KERNEL
#undef CPMPPI_ROLLOUT_MASS_ROWS
#define CPMPPI_ROLLOUT_KERNEL rollout_cost_rows_kernel
#define CPMPPI_ROLLOUT_MASS_ROWS true
#include "cpmppi_rollout_kernel.inc"
#undef CPMPPI_ROLLOUT_KERNEL
#undef CPMPPI_ROLLOUT_MASS_ROWS
#undef CPMPPI_ROLLOUT_TUNING_ROWS
#define CPMPPI_ROLLOUT_KERNEL rollout_cost_tuned_kernel
#define CPMPPI_ROLLOUT_MASS_ROWS false
#define CPMPPI_ROLLOUT_TUNING_ROWS true
#include "cpmppi_rollout_kernel.inc"
#undef CPMPPI_ROLLOUT_KERNEL
#undef CPMPPI_ROLLOUT_MASS_ROWS
#undef CPMPPI_ROLLOUT_TUNING_ROWS

}  // namespace cpmppi_k
#endif  // CPMPPI_ROLLOUT_DECLARATIONS_ONLY

// Every instantiation of rollout_cost_kernel, by the translation unit that compiles it.  X(COST, FAST, NOISE, R, VARIANT).
// The units define them with CPMPPI_DEFINE_ROLLOUT, cpmppi.hip (the hot-path unit, the only one that launches them) declares
// ALL of them extern with CPMPPI_DECLARE_ROLLOUT and generates its kernel lookup from these same lists; an instantiation listed
// in two units is a duplicate case of that lookup.
// Structural: cpmppi.hip includes this header with CPMPPI_ROLLOUT_DECLARATIONS_ONLY, so the definition is not in that unit at
// all - it cannot instantiate the kernel a second time with its own flags (the runtime would launch whichever copy registered
// last); a lookup case that names an instantiation no rollout unit defines fails at link time.  No other unit includes this
// header (they share cpmppi_step.hpp), and tests/test_headers_host.py holds the include graph to that.
// Still a convention: a cpmppi_rollout_*.hip unit sees the definition, so nothing but these lists keeps it from
// instantiating a kernel that belongs to another unit - each such unit defines exactly the instances of its own list.
#define CPMPPI_FOR_COSTS(X, FAST, NOISE, R, V) \
  X(COST_QBGM, FAST, NOISE, R, V) X(COST_DEFAULT, FAST, NOISE, R, V) X(COST_LEGACY, FAST, NOISE, R, V) X(COST_QBG, FAST, NOISE, R, V)
#define CPMPPI_FOR_NOISES(X, FAST, R, V)                                                        \
  CPMPPI_FOR_COSTS(X, FAST, NOISE_DELTA_U, R, V) CPMPPI_FOR_COSTS(X, FAST, NOISE_KNOTS, R, V)   \
  CPMPPI_FOR_COSTS(X, FAST, NOISE_PHILOX, R, V) CPMPPI_FOR_COSTS(X, FAST, NOISE_TILED, R, V)
// (the latency build is two units: the reference-layout buffer kernel schedules best with iterative-ilp, the others with
// max-memory-clause - single env 1024 x 50 on MI355X: Philox 59.2 vs 56.2 us, knots 59.6 vs 58.2, buffer 61.8 vs 68.0)
#define CPMPPI_LATENCY_INSTANCES(X)                                                                                     \
  CPMPPI_FOR_COSTS(X, true, NOISE_KNOTS, 1, 0) CPMPPI_FOR_COSTS(X, true, NOISE_TILED, 1, 0)                              \
  X(COST_QBGM, true, NOISE_PHILOX, 1, 0) X(COST_LEGACY, true, NOISE_PHILOX, 1, 0) X(COST_QBG, true, NOISE_PHILOX, 1, 0)
// (... and the `default`-cost Philox kernel, which max-memory-clause leaves with a 20-byte scratch slot for two spilled
// scalar registers - tests/test_abi_and_host.py keeps scratch out of every instantiation)
#define CPMPPI_LATENCY_BUFFER_INSTANCES(X) CPMPPI_FOR_COSTS(X, true, NOISE_DELTA_U, 1, 0) X(COST_DEFAULT, true, NOISE_PHILOX, 1, 0)
// (the mid-size build is two units as well, for compile time: 32 kernels each; VARIANT 3 = the build for launches of at
// most one wave per SIMD)
#define CPMPPI_MID_INSTANCES(X) CPMPPI_FOR_COSTS(X, true, NOISE_KNOTS, 2, 2) CPMPPI_FOR_COSTS(X, true, NOISE_PHILOX, 2, 2) \
  CPMPPI_FOR_COSTS(X, true, NOISE_KNOTS, 2, 3) CPMPPI_FOR_COSTS(X, true, NOISE_PHILOX, 2, 3)
#define CPMPPI_MID_BUFFER_INSTANCES(X) CPMPPI_FOR_COSTS(X, true, NOISE_DELTA_U, 2, 2) CPMPPI_FOR_COSTS(X, true, NOISE_TILED, 2, 2) \
  CPMPPI_FOR_COSTS(X, true, NOISE_DELTA_U, 2, 3) CPMPPI_FOR_COSTS(X, true, NOISE_TILED, 2, 3)
#define CPMPPI_THROUGHPUT_INSTANCES(X) \
  CPMPPI_FOR_NOISES(X, true, 1, 1) CPMPPI_FOR_NOISES(X, false, 1, 1) CPMPPI_FOR_NOISES(X, true, 2, 1)
// predictor_ODE (INTEG = PREDICTOR_ODE): latency build (one rollout per lane) and throughput build (both lane mappings, PRECISE)
#define CPMPPI_ODE_LATENCY_INSTANCES(X) CPMPPI_FOR_NOISES(X, true, 1, 0)
#define CPMPPI_ODE_THROUGHPUT_INSTANCES(X) \
  CPMPPI_FOR_NOISES(X, true, 1, 1) CPMPPI_FOR_NOISES(X, false, 1, 1) CPMPPI_FOR_NOISES(X, true, 2, 1)
// (two rollouts per lane in a launch of at most one wave per SIMD: the substeps as straight-line code, raised wave priority)
#define CPMPPI_ODE_LONE_INSTANCES(X) CPMPPI_FOR_NOISES(X, true, 2, 3)
// the tuned kernel (cpmppi_set_tuning_rows): quadratic_boundary_grad_minimal x Philox in every build the plan can select, three
// units with the flags of the untuned units of the same builds.  X(COST, FAST, NOISE, R, VARIANT, INTEG)
#define CPMPPI_TUNED_LATENCY_INSTANCES(X) \
  X(COST_QBGM, true, NOISE_PHILOX, 1, 0, PREDICTOR_ODE_V0) X(COST_QBGM, true, NOISE_PHILOX, 1, 0, PREDICTOR_ODE)
#define CPMPPI_TUNED_MID_INSTANCES(X) \
  X(COST_QBGM, true, NOISE_PHILOX, 2, 2, PREDICTOR_ODE_V0) X(COST_QBGM, true, NOISE_PHILOX, 2, 3, PREDICTOR_ODE_V0)
#define CPMPPI_TUNED_THROUGHPUT_INSTANCES(X)                                                                        \
  X(COST_QBGM, true, NOISE_PHILOX, 1, 1, PREDICTOR_ODE_V0) X(COST_QBGM, false, NOISE_PHILOX, 1, 1, PREDICTOR_ODE_V0) \
  X(COST_QBGM, true, NOISE_PHILOX, 2, 1, PREDICTOR_ODE_V0)                                                           \
  X(COST_QBGM, true, NOISE_PHILOX, 1, 1, PREDICTOR_ODE) X(COST_QBGM, false, NOISE_PHILOX, 1, 1, PREDICTOR_ODE)       \
  X(COST_QBGM, true, NOISE_PHILOX, 2, 1, PREDICTOR_ODE) X(COST_QBGM, true, NOISE_PHILOX, 2, 3, PREDICTOR_ODE)
#define CPMPPI_DEFINE_ROLLOUT_TUNED(COST, FAST, NOISE, R, V, INTEG) \
  template __global__ void rollout_cost_tuned_kernel<COST, FAST, NOISE, R, V, INTEG>(const Params, const StepPtrs);
#define CPMPPI_DECLARE_ROLLOUT_TUNED(COST, FAST, NOISE, R, V, INTEG) \
  extern template __global__ void rollout_cost_tuned_kernel<COST, FAST, NOISE, R, V, INTEG>(const Params, const StepPtrs);
#define CPMPPI_DEFINE_ROLLOUT_ODE(COST, FAST, NOISE, R, V) \
  template __global__ void rollout_cost_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>(const Params, const StepPtrs);
#define CPMPPI_DECLARE_ROLLOUT_ODE(COST, FAST, NOISE, R, V) \
  extern template __global__ void rollout_cost_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>(const Params, const StepPtrs);
#define CPMPPI_DEFINE_ROLLOUT_ODE_ROWS(COST, FAST, NOISE, R, V) \
  template __global__ void rollout_cost_rows_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>(const Params, const StepPtrs);
#define CPMPPI_DECLARE_ROLLOUT_ODE_ROWS(COST, FAST, NOISE, R, V) \
  extern template __global__ void rollout_cost_rows_kernel<COST, FAST, NOISE, R, V, PREDICTOR_ODE>(const Params, const StepPtrs);
#define CPMPPI_DEFINE_ROLLOUT(COST, FAST, NOISE, R, V) \
  template __global__ void rollout_cost_kernel<COST, FAST, NOISE, R, V>(const Params, const StepPtrs);
#define CPMPPI_DECLARE_ROLLOUT(COST, FAST, NOISE, R, V) \
  extern template __global__ void rollout_cost_kernel<COST, FAST, NOISE, R, V>(const Params, const StepPtrs);
