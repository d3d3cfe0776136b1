// cpmppi_step.hpp — what the units of the library share about a step: the workgroup constants, the pointer block of a
// rollout launch (StepPtrs), the device-side ordering with the all-gather (GatherSync), the nominal-sequence shift and
// the per-env finalize.  No kernel is declared or defined here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cpmppi.h"
#include "cpmppi_params.hpp"

namespace cpmppi {
struct EnvFold;     // cpmppi_cost.hpp (StepPtrs carries a pointer)
}

namespace cpmppi_k {
using namespace cpmppi;

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int GRU_MIN_WAVES = 2;                 // waves per SIMD the GRU kernels are compiled for (register budget 512 / this)
constexpr int MIN_WAVES = 1;                     // ... and the rollout kernels
constexpr uint32_t DMA_TK_DEFAULT = 8;           // control steps per direct-to-LDS tile (two tiles per wave)
constexpr uint32_t DMA_TK_THROUGHPUT = 16;       // ... in the throughput build (one tile per wave)
constexpr size_t SAMPLER_LDS_MAX = 159 * 1024;   // gfx950: 160 KB of LDS per workgroup (sampler: [256][P+1] floats)

// Device-side ordering between a step and the all-gather of its result (cpmppi_step_gather, cpmppi_comm.hip) without any
// packet on the launch stream: flags[0] envs finalized by this launch, flags[1] steps published (read by the fallback
// waiter kernel), flags[2] gathers completed (written by the side stream), flags[3] a wait gave up (sticky until
// cpmppi_comm_sync: while it is set nothing waits and nothing is stored).
struct GatherSync {
  uint32_t* flags;          // NULL = no gather follows this step.  The block also holds what only the slow paths need, so that
                            // the kernel argument stays four words: [4,5] pointer to the signal memory the side stream's
                            // hipStreamWaitValue32 watches (0: the waiter kernel polls flags[1]), [6,7] pointer to the pinned
                            // host word that mirrors the error, [8,9] the 100 MHz ticks a wait may last (~0 = for ever), [10,11]
                            // pointer to the communicator's other flag block (env groups; 0: none)
  uint32_t publish;         // the step number every env of this launch publishes once its nominal sequence is written
  uint32_t need;            // flags[2] must have reached this before the output buffer may be overwritten (0 = no wait)
  uint32_t envs;            // envs in this launch
};
constexpr int GS_PUBLISHED = 4, GS_ERR_HOST = 6, GS_TIMEOUT = 8, GS_OTHER = 10, GS_WORDS = 16;
__device__ __forceinline__ uint64_t gs_word64(const uint32_t* flags, int i) {
  return (uint64_t)flags[i] | ((uint64_t)flags[i + 1] << 32);
}

// flag >= need (wrap-safe), polled with system-scope loads (the side stream's hipStreamWriteValue32 is a write of the command
// processor: not through this XCD's L2).  Returns false - after raising the error for device and host - when the wait
// outlasts `timeout_ticks` or the error is already up: the caller then does NOT proceed to the stores the wait guards.
// (Env groups: the error goes into BOTH flag blocks, so that the next step - of the other parity - drops its stores too.)
__device__ __forceinline__ bool spin_until_reached(uint32_t* flag, uint32_t need, const GatherSync& gs) {
  uint32_t* err = gs.flags + 3;
  if ((int32_t)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - need) >= 0)
    return __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  for (;;) {
    __builtin_amdgcn_s_sleep(4);
    if ((int32_t)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - need) >= 0)
      return __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
    if (__builtin_amdgcn_s_memrealtime() - t0 > gs_word64(gs.flags, GS_TIMEOUT)) {
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t* other = reinterpret_cast<uint32_t*>(gs_word64(gs.flags, GS_OTHER));
      if (other) __hip_atomic_store(other + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t* err_host = reinterpret_cast<uint32_t*>(gs_word64(gs.flags, GS_ERR_HOST));
      if (err_host) __hip_atomic_store(err_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
  }
}

struct StepPtrs {
  const float* s0;
  const float* u_nom;
  const float* u_prev;
  const float* x_t;
  const float* te;
  const float* L;
  const float* noise;
  const float* prev_in; // [E] control applied before this step (quadratic_boundary_grad ccrc) or NULL
  uint64_t seed, offset;
  const unsigned long long* offset_dev;   // if set: the Philox step counter lives in device memory (graph replay)
  uint32_t stash;       // NOISE_PHILOX: the generated knots are parked in LDS ([P][R][BLOCK] after the weighted sums) for the reduction
  uint32_t env_offset;
  uint32_t nb;          // blocks per env
  uint32_t W;           // width of the weighted-sum vector (H in delta_u space, P in knot space)
  float* S_out;
  float* partial;       // [E][nb][2 + W]
  uint32_t* counter;    // [E] arrival tickets of the env's blocks (0 between launches); NULL = separate finalize kernel
  float* u_nom_out;     // fused finalize: where the updated nominal sequence goes (u_nom itself, or the caller's second buffer)
  float* Q_out;
  uint32_t* host_ticket; // cpmppi_step_host: counter in pinned host memory, +1 (system scope) per finalized env; NULL otherwise
  GatherSync gs;
  const EnvFold* env_fold;   // [envs of this launch] per-env constants (throughput build, FAST, predictor_ODE_v0: launch_rollout fills it first;
                             // behind the fields the latency builds were tuned with: they keep their kernarg offsets)
  union {                    // (one slot: the two registrations exclude each other, and a block that grew would move the kernel
                             // arguments BEHIND it - the GRU kernels' - and with them those kernels' code)
  const float* m_pole;       // [envs of this launch] predictor_ODE: the pole mass each env's rollouts are integrated with
                             // (cpmppi_set_pole_mass_rows); launch_rollout fills it.  Read by rollout_cost_rows_kernel only, which is
                             // launched only when it is set
  const float* tuning;       // [envs of this launch][TUNING_ROW_FLOATS] the per-env controller tuning (cpmppi_set_tuning_rows);
                             // launch_rollout fills it.  Read by rollout_cost_tuned_kernel only, launched only when it is set
  };
};

// Nominal control for stage k after the configured shift (a18).
__device__ __forceinline__ float shifted_nominal(const Params& p, const float* __restrict__ un, uint32_t k) {
  if (p.shift_mode == CPMPPI_SHIFT_NONE) return un[k];
  if (k + 1 < p.H) return un[k + 1];
  return (p.shift_mode == CPMPPI_SHIFT_REPEAT_LAST) ? un[p.H - 1] : 0.0f;
}

// Merge the per-block partials of one env (rescaled to the env-wide minimum), apply shift / update / clip, write u_nom
// and Q.  Executed by one whole block.  COHERENT = the partials were written by other workgroups of THIS launch: read
// them with agent-scope (sc1) loads that bypass this CU's L1.
template <bool KNOT_SPACE, bool COHERENT>
__device__ __forceinline__ void finalize_env(const Params& p, const float* partial, uint32_t nb, uint32_t W,
                                             const float* u_nom_in, float* u_nom_out, float* __restrict__ Q_out,
                                             uint32_t env, uint32_t* host_ticket = nullptr,
                                             const GatherSync gs = GatherSync{nullptr, 0u, 0u, 0u}) {
  __shared__ float u_new[CPMPPI_MAX_HORIZON];
  __shared__ float bz[KNOT_SPACE ? (CPMPPI_MAX_HORIZON + 2) : 1];
  const uint32_t tid = threadIdx.x, H = p.H;
  const float* pe = partial + (size_t)env * nb * (2 + W);
  auto ld = [&](size_t i) -> float {
    if constexpr (COHERENT) return __hip_atomic_load(pe + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return pe[i];
  };
  // One memory round trip per batch of eight blocks: the minimum, the weight sum and this thread's column of every block are
  // requested together (the loads do not depend on each other; issued one after the other as written they were three
  // dependent L2 round trips at the tail of every launch), then merged with the running minimum (identical arithmetic
  // to a min-first pass when nb <= 8).
  constexpr int NBB = 8;
  float a = 0.0f;
  auto merged = [&](uint32_t c) {
    float M = INFINITY, v = 0.0f;
    a = 0.0f;
    for (uint32_t b0 = 0; b0 < nb; b0 += NBB) {
      float mb[NBB], ab[NBB], vb[NBB];
#pragma unroll
      for (int u = 0; u < NBB; ++u) {
        const uint32_t b = (b0 + u < nb) ? b0 + u : nb - 1u;
        mb[u] = ld((size_t)b * (2 + W));
        ab[u] = ld((size_t)b * (2 + W) + 1);
        vb[u] = ld((size_t)b * (2 + W) + 2 + c);
      }
      float Mn = M;
#pragma unroll
      for (int u = 0; u < NBB; ++u) Mn = fminf(Mn, mb[u]);
      if (b0 != 0) {
        const float sc = expf((-1.0f / p.LBD) * (M - Mn));
        a *= sc;
        v *= sc;
      }
      M = Mn;
#pragma unroll
      for (int u = 0; u < NBB; ++u) {
        if (b0 + u < nb) {
          const float w = expf((-1.0f / p.LBD) * (mb[u] - M));
          a += ab[u] * w;
          v = __builtin_fmaf(vb[u], w, v);
        }
      }
    }
    return v;
  };
  if constexpr (KNOT_SPACE) {
    // every thread merges one column (clamped), so that every thread also holds the weight sum `a`
    const float v0 = merged(tid < W ? tid : W - 1u);
    if (tid < W) bz[tid] = v0;
    for (uint32_t c = tid + BLOCK; c < W; c += BLOCK) bz[c] = merged(c);
    __syncthreads();
  }
  const float* un = u_nom_in + (size_t)env * H;       // (may alias the output: every read precedes the barrier below)
  float* uo = u_nom_out + (size_t)env * H;
  for (uint32_t k = tid; k < H; k += BLOCK) {
    float bk;
    if constexpr (KNOT_SPACE) {
      const uint32_t j = k / p.period, i = k % p.period;
      bk = bz[j] + (bz[j + 1] - bz[j]) * ((float)i / (float)p.period);
    } else {
      bk = merged(k);
    }
    float v = shifted_nominal(p, un, k) + bk / a;
    if (p.control_mode == CPMPPI_CONTROL_CLIP) v = fminf(fmaxf(v, p.lo), p.hi);
    u_new[k] = v;
  }
  __syncthreads();                          // every read of the old nominal sequence is done
  bool store = true;
  if (gs.flags && gs.need) {
    // the all-gather that still reads the buffer written next (two steps back with alternating buffers) must be complete:
    // by now it has had a whole step to run, so this practically never spins.  A wait that gives up (a peer rank stalled
    // beyond cpmppi_comm_set_timeout) must NOT fall through to the stores - the gather would send a half-overwritten
    // buffer to every rank: this step's result is dropped instead, the error is raised for the host, and the launch still
    // publishes so that nothing behind it wedges.
    __shared__ uint32_t may_store;
    if (tid == 0) may_store = spin_until_reached(gs.flags + 2, gs.need, gs) ? 1u : 0u;
    __syncthreads();
    store = may_store != 0u;
  }
  if (store) {
    for (uint32_t k = tid; k < H; k += BLOCK) uo[k] = u_new[k];
    if (tid == 0 && Q_out) Q_out[env] = u_new[0];
  }
  if (tid == 0 && host_ticket) {
    // the simulator's host thread spins on this counter instead of waiting on the stream (cpmppi_step_host): Q_out lives
    // in the same pinned, fine-grained block; system-scope release so that the control is visible before the ticket
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_fetch_add(host_ticket, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (gs.flags) {
    // publish "every env of this step has written its sequence" to the side stream's waiter: stores drained, block
    // barrier, one lane's agent-scope release + arrival count; the last env's block publishes the step number
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const uint32_t arrived = __hip_atomic_fetch_add(gs.flags, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (arrived == gs.envs - 1u) {
        __hip_atomic_store(gs.flags, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the side stream waits for this number: hipStreamWaitValue32 on signal memory (a one-lane blit kernel of the runtime's,
        // as the round-6 kernel trace shows), or - env groups; devices without stream memory operations - our one-lane kernel polling flags[1]
        uint32_t* published = reinterpret_cast<uint32_t*>(gs_word64(gs.flags, GS_PUBLISHED));
        if (published) __hip_atomic_store(published, gs.publish, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        else __hip_atomic_store(gs.flags + 1, gs.publish, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
}  // namespace cpmppi_k
