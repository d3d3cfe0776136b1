// cpmppi_internal.hpp — where the translation units of libcpmppi.so meet beside the public header: the handle's layout, the
// error and device helpers of every entry point, and the few host functions one unit calls in another.
//   cpmppi.hip            the hot path: handle lifecycle, cpmppi_step / _step_gather / _step_host, the rollout kernel lookup and
//                         launch, profiling, streams
//   cpmppi_launch_plan.hpp  the launch policy (which build of the rollout kernel, block split, LDS): one pure host function
//   cpmppi_seams.hip      sampler, tiling, predictor, trajectory cost and reward-weighted-average seams
//   cpmppi_plant.hip      the simulated plant (cpmppi_plant_*)
//   cpmppi_optim.hip      cost-only rollouts, the adjoint, Adam / SGD steps and CEM
//   cpmppi_score.hip      the score of a recording per env (cpmppi_score_runs)
//   cpmppi_replay.hip     control along recorded trajectories: the recorded row in the plant's place (cpmppi_replay_step)
//   cpmppi_gru.hip        the GRU predictor in the optimizers: the fused MPPI step, cost-only rollouts, the gradient's forward sweep,
//                         the fused CEM step (cpmppi_cem_step_gru)
//   cpmppi_gru_seam.hip   its exact-cell seams: predict, advance, washout, the Brunton test's kernel
//   cpmppi_gru_adjoint.hip  the gradient's reverse sweep
//   cpmppi_gru_rpgd.hip   the fused rpgd / gradient-tf step over the GRU predictor (cpmppi_rpgd_step_gru): forward sweep, reverse sweep,
//                         Adam, ranking, resampling and shift in one kernel
//   cpmppi_gru_train.hip  training on recordings: teacher-forced loss, BPTT weight gradient, Adam and the image rebuild on the device
//                         (cpmppi_gru_loss_grad, cpmppi_gru_train_*)
//   cpmppi_ode_fit.hip    fitting the ODE predictor's physical parameters to recordings: open-loop loss, forward-mode gradient, Adam
//                         on the device (cpmppi_ode_fit_*)
//   cpmppi_dense.hip      the neural imitator (Dense-7IN-32H1-32H2-1OUT): the control kernel, loss and gradient over recordings with the
//                         batch contraction on MFMA, Adam on the device (cpmppi_set_dense, cpmppi_dense_*); the DAgger control period
//                         on the same forward body (cpmppi_dagger_step)
//   cpmppi_gru_model.hip  host code only: cpmppi_set_gru packs and uploads the three weight images
//   cpmppi_comm.hip, cpmppi_groups.hip, cpmppi_io.hip   host code only: the collective, env groups, the recording writer
//   cpmppi_rollout_*.hip  the instances of rollout_cost_kernel, each unit with its own compiler flags
// The headers underneath, one per subject, each included by name where it is used (there is no umbrella header):
//   cpmppi_params.hpp     Params, EnvConst, the kernels' template-argument ids, State, the float / float2 helpers
//   cpmppi_step.hpp       what the units share about a step: BLOCK / WAVES, StepPtrs, GatherSync, shifted_nominal, finalize_env
//   cpmppi_rollout.hpp    the rollout kernel (+ cpmppi_rollout_kernel.inc): the cpmppi_rollout_*.hip units, and - declarations and
//                         instance lists only - cpmppi.hip; no other unit includes it
//   cpmppi_ode.hpp, cpmppi_cost.hpp, cpmppi_philox.hpp, cpmppi_wave.hpp   the integrators, the stage costs and their folds, the noise
//                         stream and knot interpolation, the wave reductions: the kernel units that use them, never the host-only ones
//   cpmppi_brunton.hpp    the Brunton test's arguments and statistics: cpmppi_seams.hip and cpmppi_gru_seam.hip only
//   cpmppi_debug.hpp      the diagnostic builds' counters and stamps (no-ops in the product build)
//   cpmppi_grad.hpp, cpmppi_rpgd.hpp (cpmppi_optim.hip, cpmppi_gru_rpgd.hip), cpmppi_cem.hpp (cpmppi_optim.hip and - sampler, ranking,
//   refit - cpmppi_gru.hip, cpmppi_gru_rpgd.hip), cpmppi_gru.hpp, cpmppi_gru16.hpp (the GRU units), cpmppi_gru_rollout.hpp (GruRollout:
//   cpmppi_gru.hip, cpmppi_gru_rpgd.hip), cpmppi_gru_reverse.hpp (the reverse sweep: cpmppi_gru_adjoint.hip, cpmppi_gru_rpgd.hip)
// This header includes cpmppi_params.hpp and cpmppi_step.hpp, and forward-declares what the handle only points to.
// Kernels stay in an anonymous namespace of the unit that launches them; units call each other through host functions only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "cpmppi.h"
#include "cpmppi_params.hpp"
#include "cpmppi_step.hpp"         // (no kernel: cpmppi_rollout.hpp is for the units that instantiate or launch rollout_cost_kernel)
#include "cpmppi_launch_plan.hpp"

namespace cpmppi_comm {
struct CommState;                                        // cpmppi_comm.hip
void destroy(CommState* c);                              // called by cpmppi_destroy

// cpmppi_step_gather = begin_step_gather (numbers the gather, says what the step's finalize must publish / await) ->
// the step launch -> enqueue_gather (side stream: wait for the published step, ncclAllGather, post completion)
struct GatherTicket {
  unsigned* flags;        // device words: [0] envs finalized, [1] steps published, [2] gathers completed, [3] error, [4..9] the
                          // slow paths' pointers and the timeout (GatherSync, cpmppi_step.hpp)
  unsigned publish, need;
  unsigned envs;          // envs that publish the step together: 0 = the launch's own (one handle); env groups: all groups' envs
};
void begin_step_gather(CommState* c, const float* out_buffer, GatherTicket* out);
int share_between_groups(CommState* c);      // the communicator serves env groups: steps alternate between two flag blocks
void abort_step_gather(CommState* c);
int enqueue_gather(cpmppi_handle* h, const float* send, float* recv_all, size_t count);
int enqueue_guard(cpmppi_handle* h, const GatherTicket& t, unsigned envs, void* stream);   // launch stream: gather_guard_kernel (many envs only)
void poison(CommState* c);                   // a partly enqueued step-gather: error state until cpmppi_comm_sync (which resets the counters)
int comm_error_pending(cpmppi_handle* h);    // a device-side wait timed out or a step-gather was poisoned (sticky until cpmppi_comm_sync)
}  // namespace cpmppi_comm

namespace cpmppi {
struct EnvFold;          // cpmppi_cost.hpp
struct BruntonArgs;      // cpmppi_brunton.hpp

// The GRU predictor's input / output normalisation (cpmppi_gru.hpp); here because the handle holds one by value.
struct GruNorm {         // normalised = x*scale + shift ; order Q, angleD, angle_cos, angle_sin, position, positionD
  float in_scale[6], in_shift[6], out_scale[5], out_shift[5];
};
}  // namespace cpmppi

struct cpmppi_handle {
  cpmppi_config cfg;
  cpmppi::Params prm;
  int device;
  float* workspace;
  size_t workspace_floats;
  uint32_t nb;
  std::string err;
  // optional per-kernel timing with HIP events recorded on the launch stream (cpmppi_set_profiling)
  uint32_t* counters = nullptr;        // [cfg.E] block-arrival tickets of the fused finalize
  cpmppi::EnvFold* env_fold = nullptr; // [cfg.E] per-env constants of the throughput build (fold_env_kernel, rewritten before every such launch)
  float* zeros_H = nullptr;            // [cfg.E, cfg.H] zeros: the nominal sequence of a cost-only launch
  float* host_stage = nullptr;         // pinned [cfg.E * 10 + 16]: staging of cpmppi_step_host (state 6, target, equilibrium, L | Q | ticket)
  uint32_t host_ticket_value = 0;      // what the ticket in that block reads once every launch so far has delivered
  double host_t[4] = {0, 0, 0, 0};     // development aid (cpmppi_debug_host_times): sums of staging / launch / wait seconds, calls
  uint32_t host_zero_copy_max = 64;    // up to this many envs cpmppi_step_host runs without copies and stream waits (CPMPPI_HOST_ZERO_COPY_MAX)
  float* dev_stage = nullptr;          // device [cfg.E * 10], allocated on first use
  float* gru_image = nullptr;          // device copy of the LDS fragment image (cpmppi_set_gru)
  void* gru16_image = nullptr;         // device copy of the f16 split image (cpmppi_gru16.hpp)
  float* gru_t_image = nullptr;        // device copy of the transposed fragment image (the reverse sweep of cpmppi_rollout_cost_grad_gru)
  float* gru_grad_ws = nullptr;        // [H][GRU_CKPT_FLOATS][E*N] check-points of cpmppi_rollout_cost_grad_gru (allocated on first use);
                                       // cpmppi_rpgd_gru_reserve: the same, then the gradient [E*N][H] of cpmppi_rpgd_step_gru
  size_t gru_grad_ws_floats = 0;
  float* brunton_ws = nullptr;         // [rows][horizon][6][3] partial statistics of cpmppi_brunton (allocated on first use, grown on demand)
  size_t brunton_ws_floats = 0;
  float* grad_ckpt = nullptr;          // [H][6][E*N] check-points of cpmppi_rollout_cost_grad (allocated on first use)
  size_t grad_ckpt_floats = 0;
  float* rpgd_ws = nullptr;            // cpmppi_rpgd_step: check-points [E][H][6][block] then gradients [E][H][block] (cpmppi_rpgd_reserve)
  size_t rpgd_ws_floats = 0;
  float* cem_ws = nullptr;             // cpmppi_cem_step: samples [E][H][block]; refining, + check-points, gradients, Adam moments (cpmppi_cem_reserve)
  size_t cem_ws_floats = 0;
  cpmppi::GruNorm gru_norm;
  std::vector<float> gru_params;       // the weights of the last cpmppi_set_gru in the flat order of CPMPPI_GRU_PARAMS (cpmppi_gru_train_begin)
  struct GruTrain* gru_train = nullptr;  // training on recordings (cpmppi_gru_train.hip): workspace, master copy, moments; or none yet
  struct OdeFit* ode_fit = nullptr;    // fitting the physical parameters (cpmppi_ode_fit.hip): partial rows, parameter block, Adam state; or none yet
  struct DenseNet* dense = nullptr;    // the neural imitator (cpmppi_dense.hip): parameter vector, normalisation, partial rows, Adam state; or none yet
  bool fuse_finalize = true;           // ODE path: the env's last block finalizes in-kernel (CPMPPI_FUSE_FINALIZE=0 disables)
  uint32_t profile_every = 0;          // 0 = off, 1 = every rollout kernel bracketed, n > 1 = one bracket around n steps
  uint32_t profile_count = 0;
  bool group_open = false;             // n > 1: the current group's closing event is still to come
  std::vector<hipEvent_t> ev;          // triples per sampled step: before rollout, after it, after the trailing kernels
  std::vector<uint8_t> ev_tail;        // per triple: was the third event recorded (a separate finalize / counter kernel ran)
  size_t ev_used = 0;
  cpmppi_comm::CommState* comm = nullptr;   // RCCL communicator + side stream of cpmppi_comm_* (cpmppi_comm.hip)
  const float* m_pole_rows = nullptr;  // cpmppi_set_pole_mass_rows: the caller's DEVICE array of per-row controller-side pole masses (predictor_ODE), or NULL
  uint32_t m_pole_rows_n = 0;          // ... and how many rows it holds
  const float* tuning_rows = nullptr;  // cpmppi_set_tuning_rows: the caller's DEVICE array [n][CPMPPI_TUNING_ROW_FLOATS] of per-env controller tunings, or NULL
  uint32_t tuning_rows_n = 0;          // ... and how many rows it holds
  float plant_m_pole = 0.0f;           // the pole mass of the simulated PLANT (cfg.m_pole at creation; cpmppi_set_pole_mass does not touch it)
  cpmppi_launch_info last_launch = {0, 0, 0, 0, 0, 0, 0};   // cpmppi_last_launch: the instantiation the last rollout launch used
};

// Sets the call's error message and returns `code`.  h == NULL: the calling thread's creation error, which
// cpmppi_last_error(NULL) reads - one object, so this is defined once (cpmppi.hip).
int fail(cpmppi_handle* h, int code, const std::string& msg);

#define CPMPPI_HIP(h, call)                                                                        \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail((h), CPMPPI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));         \
  } while (0)

// Every entry point runs on the handle's device and leaves the CALLER's current device as it found it (a process that
// shares the HIP runtime with torch must not have its later raw HIP calls retargeted).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = (err == hipSuccess);
    }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define CPMPPI_ON_DEVICE(h)                                                                        \
  DeviceGuard device_guard_((h)->device);                                                          \
  if (device_guard_.err != hipSuccess)                                                             \
    return fail((h), CPMPPI_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err))

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// cpmppi_set_pole_mass_rows: does the registered array (if any) hold a mass for every row of a launch of `rows` rows?  Every entry
// point that integrates predictor_ODE asks before it launches; the second function words the refusal.
inline bool pole_mass_rows_cover(const cpmppi_handle* h, uint32_t rows) { return !h->m_pole_rows || rows <= h->m_pole_rows_n; }
inline std::string pole_mass_rows_short(const char* who, const cpmppi_handle* h, uint32_t rows) {
  return std::string(who) + ": " + std::to_string(rows) + " rows, but cpmppi_set_pole_mass_rows registered " +
         std::to_string(h->m_pole_rows_n) + " pole masses";
}

// cpmppi_set_tuning_rows: the rows are read by the fused ODE MPPI step alone (and the finalize kernel behind it); every other entry
// point whose kernels read the cost vector, LBD or sigma of the handle's block refuses by name while rows are registered (it would
// silently compute with the handle's scalars): the list is in cpmppi.h.
inline int refuse_tuning_rows(cpmppi_handle* h, const char* who) {
  if (!h->tuning_rows) return CPMPPI_OK;
  return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": per-env tuning rows are registered (cpmppi_set_tuning_rows), which only the "
                                         "fused ODE cpmppi_step reads; unregister them first (NULL)");
}

// the end of an entry point that has just launched a kernel: CPMPPI_OK, or the launch's error
inline int launched(cpmppi_handle* h) {
  CPMPPI_HIP(h, hipGetLastError());
  return CPMPPI_OK;
}

// Grows a device workspace of the handle to `need` floats (the contents are not kept).
inline int grow_workspace(cpmppi_handle* h, float*& ws, size_t& floats, size_t need) {
  if (floats >= need) return CPMPPI_OK;
  if (ws) (void)hipFree(ws);
  ws = nullptr; floats = 0;
  CPMPPI_HIP(h, hipMalloc(&ws, need * sizeof(float)));
  floats = need;
  return CPMPPI_OK;
}

// No allocation inside a capture: a step whose workspace is not reserved (`reserve`: the call that does it) is refused there.
inline int refuse_unreserved_capture(cpmppi_handle* h, hipStream_t s, const char* who, const char* reserve) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  if (!capturing) return CPMPPI_OK;
  return fail(h, CPMPPI_ERR_BAD_ARG, std::string(who) + ": the stream is being captured and the workspace is not reserved (call " +
                                         reserve + " before the capture)");
}

// a kernel whose dynamic LDS may exceed the default 64 KB opts in to SAMPLER_LDS_MAX
template <class Kernel>
void allow_large_lds(Kernel* kernel) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)cpmppi_k::SAMPLER_LDS_MAX);
}

// GRU predictor (BASELINE configs[4]): 256 threads = 4 waves x 32 rollouts
constexpr int GRU_ROLLOUTS_PER_BLOCK = 32 * cpmppi_k::WAVES;

// The one-workgroup-per-env control steps (cpmppi_rpgd_step, cpmppi_cem_step, cpmppi_cem_step_gru; not cpmppi_rpgd_step_gru, whose rows
// are the staged adjoint's): the row width of their
// workspaces - N rounded up to whole waves, a lane per plan / sample - and the floats of the CEM steps' workspace for E envs: the
// samples; refining, also check-points (6), gradient, and Adam's two moments.
inline uint32_t rpgd_block(const cpmppi_handle* h) { return (h->cfg.N + 63u) & ~63u; }
inline size_t cem_floats(const cpmppi_handle* h, uint32_t E, bool refine) {
  return (size_t)h->cfg.H * (refine ? 10 : 1) * E * rpgd_block(h);
}

// ---- host functions one unit calls in another -------------------------------------------------------------------------
// cpmppi.hip.  check_step: every check of a step's argument block that needs no launch (cpmppi_groups_run_gather runs them for
// all groups before its first launch).  step_impl: cpmppi_step, with the pinned ticket of cpmppi_step_host and / or the
// step-gather whose finalize it takes part in (cpmppi_step_gather; cpmppi_groups_run_gather, where the ticket is shared by the
// launches of every group).  plan_launch: the launch plan (cpmppi_launch_plan.hpp: which build of rollout_cost_kernel, its grid,
// block split and LDS) of E envs of this handle.  launch_rollout: launches what the plan names and records it for
// cpmppi_last_launch; `prm` is the kernel-argument block of THIS launch (the handle's, or a modified copy: cost-only launches), and
// the caller has filled nb, W and stash of the pointer block from the same plan.
int check_step(cpmppi_handle* h, const cpmppi_step_args* a);
int step_impl(cpmppi_handle* h, const cpmppi_step_args* a, void* stream, uint32_t* host_ticket,
              const cpmppi_comm::GatherTicket* gather = nullptr);
cpmppi_plan::RolloutPlan plan_launch(const cpmppi_handle* h, uint32_t E, uint32_t noise_kind);
int launch_rollout(cpmppi_handle* h, const cpmppi::Params& prm, const cpmppi_plan::RolloutPlan& plan, hipStream_t s,
                   const cpmppi_k::StepPtrs& a_in);
// cpmppi_plant.hip: every check of a plant step's argument block that needs no launch (see check_step)
int check_plant(cpmppi_handle* h, const cpmppi_plant_args* a);
// cpmppi_gru.hip: the fused GRU rollout kernel of a step (p.nb counted in GRU blocks); the caller checks the launch
void launch_gru_rollout(cpmppi_handle* h, const cpmppi_step_args* a, const cpmppi_k::StepPtrs& p, hipStream_t s);
// cpmppi_gru_adjoint.hip: the reverse sweep of cpmppi_rollout_cost_grad_gru behind its forward sweep (cpmppi_gru.hip), whose
// arguments these are and whose check-points, in the handle's workspace, it reads; and the LDS opt-in of its kernels (cpmppi_set_gru)
void launch_gru_grad_reverse(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* x_t, const float* te,
                             const float* h0, float* grad, hipStream_t s);
void allow_large_lds_gru_adjoint();
// cpmppi_gru_rpgd.hip: the LDS opt-in of the fused rpgd / gradient step over the network (cpmppi_set_gru)
void allow_large_lds_gru_rpgd();
// cpmppi_gru_model.hip: where every float of the exact-f32 image and, behind it, of the transposed image comes from, read off
// pack_f32_image / pack_transposed_image themselves: src[2 * i], src[2 * i + 1] = indices into the flat parameter vector whose sum
// the float is (-1: none; both -1: zero) - the table of the on-device rebuild (cpmppi_gru_train.hip)
void gru_image_sources(std::vector<int32_t>& src);
// cpmppi_gru_train.hip: frees what training allocated (cpmppi_destroy); ends a training run, whose master copy, moments and step
// counter belong to the model before this one - the step and get entry points refuse until cpmppi_gru_train_begin (cpmppi_set_gru)
void gru_train_destroy(cpmppi_handle* h);
void gru_train_end(cpmppi_handle* h);
// cpmppi_ode_fit.hip: frees what a fit of the physical parameters allocated (cpmppi_destroy)
void ode_fit_destroy(cpmppi_handle* h);
// cpmppi_dense.hip: frees what the neural imitator allocated (cpmppi_destroy)
void dense_destroy(cpmppi_handle* h);
// cpmppi_gru_seam.hip: the Brunton test's GRU kernel (one partial row per wave of 32 starts: brunton_gru_rows of them); the caller
// has checked the arguments, checks the launch and reduces the partial rows
inline size_t brunton_gru_rows(size_t starts) { return (starts + 31) / 32; }
void launch_gru_brunton(cpmppi_handle* h, const cpmppi::BruntonArgs& a, hipStream_t s);
// cpmppi_optim.hip: *count_dev += 1 behind a fused control step, stream-ordered (one launch of one lane); the caller checks the launch
void launch_step_count(unsigned long long* count_dev, hipStream_t s);
// called by cpmppi_create: the LDS opt-ins of the kernels of cpmppi_seams.hip and cpmppi_optim.hip
void allow_large_lds_seams();
void allow_large_lds_optim();
