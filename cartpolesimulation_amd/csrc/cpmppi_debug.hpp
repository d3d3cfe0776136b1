// cpmppi_debug.hpp — the diagnostic builds' per-wave counters and stamps (-DCPMPPI_DEBUG_COUNTERS, -DCPMPPI_SECTION_STAMPS), their
// readers, and the macros the kernels mark their events and sections with: no-ops in the product build.
#pragma once
#include <hip/hip_runtime.h>

namespace cpmppi {

// Diagnostic build only (-DCPMPPI_DEBUG_COUNTERS, tools/dev/cold_counts.py): per-translation-unit event counters and
// per-wave lifetimes of the rollout kernel.  No counter exists in the product build.
#ifdef CPMPPI_DEBUG_COUNTERS
static __device__ unsigned long long g_dbg[8];        // unused slots kept for ad-hoc counters
static __device__ unsigned long long g_wave_cycles[16384];
static __device__ unsigned int g_wave_cold[16384];    // cold-branch entries of each wave (all substep flavours)
static __device__ unsigned long long g_wave_t[16384][4];   // s_memrealtime (100 MHz, chip-wide): entry, loop end, partials written, exit
// -DCPMPPI_SECTION_STAMPS on top (tools/dev/sections.py): s_memtime at the section boundaries of a control step, summed per
// wave.  `sec[0..6]` accumulate shader cycles per section, `sec[7]` holds the previous stamp.
static __device__ unsigned int g_wave_sec[16384][8];
// where a wave runs (tools/dev/placement.py): HW_REG_HW_ID (wave / SIMD / CU / shader array / shader engine) and HW_REG_XCC_ID
static __device__ unsigned int g_wave_hw[16384][2];
#define CPMPPI_DBG_STAMP(slot)                                                                       \
  do {                                                                                               \
    const unsigned wv_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                        \
    if ((threadIdx.x & 63u) == 0u && wv_ < 16384u) {                                                 \
      cpmppi::g_wave_t[wv_][slot] = __builtin_amdgcn_s_memrealtime();                                \
      if ((slot) == 0) {                                                                             \
        unsigned hw_, xcc_;                                                                          \
        asm volatile("s_getreg_b32 %0, hwreg(4)" : "=s"(hw_));                                       \
        asm volatile("s_getreg_b32 %0, hwreg(20)" : "=s"(xcc_));                                     \
        cpmppi::g_wave_hw[wv_][0] = hw_; cpmppi::g_wave_hw[wv_][1] = xcc_;                           \
      }                                                                                              \
    }                                                                                                \
  } while (0)
#define CPMPPI_HW_READER(NAME)                                                                                          \
  extern "C" int NAME(unsigned int* hw, unsigned n_waves) {                                                            \
    return hipMemcpyFromSymbol(hw, HIP_SYMBOL(cpmppi::g_wave_hw), (size_t)n_waves * 8) == hipSuccess ? 0 : -1;         \
  }
// one reader per translation unit (the arrays are per unit): extern "C" int NAME(cold, cycles, stamps, n_waves, reset)
#define CPMPPI_DEBUG_READER(NAME)                                                                                      \
  extern "C" int NAME(unsigned int* wave_cold, unsigned long long* wave_cycles, unsigned long long* stamps,            \
                      unsigned n_waves, int reset) {                                                                   \
    if (wave_cold && hipMemcpyFromSymbol(wave_cold, HIP_SYMBOL(cpmppi::g_wave_cold), (size_t)n_waves * 4) != hipSuccess) return -1; \
    if (wave_cycles && hipMemcpyFromSymbol(wave_cycles, HIP_SYMBOL(cpmppi::g_wave_cycles), (size_t)n_waves * 8) != hipSuccess) return -1; \
    if (stamps && hipMemcpyFromSymbol(stamps, HIP_SYMBOL(cpmppi::g_wave_t), (size_t)n_waves * 32) != hipSuccess) return -1; \
    if (reset) {                                                                                                       \
      static unsigned int z[16384];                                                                                    \
      if (hipMemcpyToSymbol(HIP_SYMBOL(cpmppi::g_wave_cold), z, sizeof(z)) != hipSuccess) return -1;                   \
    }                                                                                                                  \
    return 0;                                                                                                          \
  }
#define CPMPPI_SECTION_READER(NAME)                                                                                     \
  extern "C" int NAME(unsigned int* sections, unsigned n_waves) {                                                      \
    return hipMemcpyFromSymbol(sections, HIP_SYMBOL(cpmppi::g_wave_sec), (size_t)n_waves * 32) == hipSuccess ? 0 : -1; \
  }
#define CPMPPI_DBG(i, n)                                                                             \
  do {                                                                                               \
    const unsigned wv_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                        \
    if ((i) != 1 && (i) != 2 && (threadIdx.x & 63u) == (unsigned)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)) && wv_ < 16384u) \
      atomicAdd(&cpmppi::g_wave_cold[wv_], 1u);                                                      \
  } while (0)
#else
#define CPMPPI_DBG(i, n) ((void)0)
#define CPMPPI_DBG_STAMP(slot) ((void)0)
#endif
// -DCPMPPI_SECTION_STAMPS on top of -DCPMPPI_DEBUG_COUNTERS: the stamp at a section boundary of a control step (g_wave_sec above)
#if defined(CPMPPI_DEBUG_COUNTERS) && defined(CPMPPI_SECTION_STAMPS)
// the state is pinned in front of the stamp (an opaque asm it passes through), so a section's arithmetic cannot drift
// across its boundary
#define CPMPPI_SEC(sec, i, ST)                                                                                          \
  do {                                                                                                                 \
    asm volatile("" : "+v"((ST).th), "+v"((ST).w), "+v"((ST).c), "+v"((ST).s), "+v"((ST).x), "+v"((ST).v));           \
    const unsigned now_ = (unsigned)__builtin_amdgcn_s_memtime();                                                      \
    (sec)[i] += now_ - (sec)[7];                                                                                       \
    (sec)[7] = now_;                                                                                                   \
  } while (0)
#else
#define CPMPPI_SEC(sec, i, ST) ((void)0)
#endif

}  // namespace cpmppi
