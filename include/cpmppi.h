/*
 * cpmppi.h — C ABI of libcpmppi.so: the MI355X-native (gfx950) MPPI rollout hot path for CartPoleSimulation.
 *
 * One fused HIP path replaces three nested Python plugin seams of the reference (paths relative to the
 * reference checkout):
 *
 *   predictor seam   PredictorWrapper.predict_core(s[N,6], Q[N,H,1]) -> [N,H+1,6]
 *                    call sites: Control_Toolkit_ASF/Controllers/controller_mppi_cartpole.py:191,
 *                    SI_Toolkit_ASF/ToolkitCustomization/Modules/ODE_module.py:46-50; per-step hook
 *                    SI_Toolkit_ASF/ToolkitCustomization/predictors_customization_v0.py:41-55
 *                    -> cpmppi_predict()
 *   cost seam        cost_function.get_stage_cost / get_terminal_cost / get_trajectory_cost
 *                    Control_Toolkit_ASF/Cost_Functions/CartPole/quadratic_boundary_grad_minimal.py:95-126,
 *                    .../default.py:41-88, Cost_Functions/GymlikeCartPole/cost_function_gym.py:12-21
 *                    -> cpmppi_trajectory_cost()
 *   optimizer seam   optimizer_mppi.step(s, time) (Control_Toolkit submodule, absent from the reference mount;
 *                    in-tree statement of the same algorithm: controller_mppi_cartpole.py:454-569 with
 *                    trajectory_rollouts :164-224, q :227-275, phi :278-303, reward_weighted_average :306-321,
 *                    initialize_perturbations :392-452)
 *                    -> cpmppi_sample() + cpmppi_step()
 *                    optimizer_rpgd.step / optimizer_gradient.step (config_optimizers.yml:49-86), the whole control step
 *                    -> cpmppi_rpgd_step()
 *                    optimizer_cem.step and its two gradient hybrids (config_optimizers.yml:1-11, 21-48), the whole control step
 *                    -> cpmppi_cem_step()
 *
 * Conventions
 *   - every array argument is a caller-owned DEVICE pointer to contiguous float32 (e.g. torch.Tensor.data_ptr() of a
 *     ROCm tensor); the library owns only the handle and its small reduction workspace;
 *   - all work is enqueued on the hipStream_t passed as `stream` (NULL = default stream); no hidden synchronisation,
 *     no allocation inside the launch functions (they are hipGraph-capturable);
 *   - return value 0 = success, negative = cpmppi_status; the message of the last failure of a handle is
 *     available from cpmppi_last_error();
 *   - a handle is not thread-safe: one handle per (device, stream);
 *   - there is NO CPU fallback: without a gfx950 device cpmppi_create() fails with CPMPPI_ERR_NO_DEVICE.
 *
 * State layout (CartPole/state_utilities.py:5-23): [angle, angleD, angle_cos, angle_sin, position, positionD].
 */
#ifndef CPMPPI_H
#define CPMPPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPMPPI_ABI_VERSION 5u   /* 2: cpmppi_step_args.u_nom_out, cpmppi_plant_advance_record(log_rows), cpmppi_comm_*;
                                   3: cpmppi_config.ode_predictor (+ cost ids 4 / 5, cpmppi_last_launch, cpmppi_comm_set_timeout);
                                   4: cpmppi_plant_step / cpmppi_plant_args (the experiment schedule), cpmppi_write_recordings takes
                                      per-row columns (cpmppi_recording), cpmppi_launch_info.cost_plugin, CPMPPI_ERR_IO,
                                      cpmppi_comm_info, cpmppi_groups_*.  cpmppi_abi_version() reports what a loaded library was built as;
                                   5: cpmppi_comm_set_stamped (+ cpmppi_comm_info.stamped), cpmppi_groups_comm_init / cpmppi_groups_run_gather;
                                      a caller-given rccl_path now wins over an RCCL the process has already loaded;
                                      cpmppi_set_pole_mass_rows (a new entry point: no layout and no existing semantics change);
                                      cpmppi_rpgd_step / cpmppi_rpgd_reserve / cpmppi_rpgd_args (new entry points, likewise);
                                      cpmppi_cem_step / cpmppi_cem_reserve / cpmppi_cem_args (new entry points, likewise);
                                      cpmppi_cem_step_gru / cpmppi_cem_gru_args (a new entry point, likewise);
                                      cpmppi_rpgd_step_gru / cpmppi_rpgd_gru_reserve / cpmppi_rpgd_gru_args (new entry points, likewise);
                                      cpmppi_gru_advance (a new entry point, likewise);
                                      cpmppi_brunton / cpmppi_brunton_args, cpmppi_gru_washout (new entry points, likewise);
                                      cpmppi_score_runs / cpmppi_score_args, cpmppi_set_tuning_rows (new entry points, likewise);
                                      cpmppi_rpgd_step_rows (a new entry point, likewise);
                                      cpmppi_gru_loss_grad / cpmppi_gru_loss_args, cpmppi_gru_train_reserve / _begin / _step / _get
                                      (new entry points, likewise);
                                      cpmppi_gru_rollout_loss_grad / cpmppi_gru_rollout_train_step (new entry points, likewise);
                                      cpmppi_ode_fit_loss_grad / cpmppi_ode_fit_args, cpmppi_ode_fit_reserve / _begin / _set_theta /
                                      _step / _get (new entry points, likewise);
                                      cpmppi_set_dense / cpmppi_dense_model, cpmppi_dense_control / cpmppi_dense_control_args,
                                      cpmppi_dense_loss_grad / cpmppi_dense_loss_args, cpmppi_dense_train_reserve / _begin / _step /
                                      _get (new entry points, likewise);
                                      cpmppi_dagger_step / cpmppi_dagger_args (a new entry point, likewise);
                                      cpmppi_dense_policy_reserve / _loss_grad / _train_step, cpmppi_dense_policy_args,
                                      cpmppi_dense_policy_ckpt_floats / _ckpt_copy (new entry points, likewise). */
#define CPMPPI_STATE_DIM 6u
#define CPMPPI_MAX_HORIZON 1024u

typedef enum {
  CPMPPI_OK = 0,
  CPMPPI_ERR_BAD_ARG = -1,      /* null pointer, bad shape, unknown enum value */
  CPMPPI_ERR_ABI = -2,          /* abi_version mismatch */
  CPMPPI_ERR_NO_DEVICE = -3,    /* no HIP device / not a gfx950 part */
  CPMPPI_ERR_HIP = -4,          /* a HIP runtime call failed (text in cpmppi_last_error) */
  CPMPPI_ERR_ALIGN = -5,        /* pointer not 4-byte aligned */
  CPMPPI_ERR_COMM = -6,         /* RCCL missing or an RCCL call failed (text in cpmppi_last_error) */
  CPMPPI_ERR_IO = -7,           /* a file could not be created or written (cpmppi_write_recordings; errno text in cpmppi_last_error) */
  CPMPPI_ERR_NOMEM = -8         /* host memory exhausted (no C++ exception ever leaves the library) */
} cpmppi_status;

/* cost_id: which in-tree cost formulation the rollout kernel evaluates. */
enum {
  CPMPPI_COST_QBGM = 0,    /* quadratic_boundary_grad_minimal.py:64-126 ; cost_w = {dd_quadratic_weight, db_weight,
                              ep_weight, ekp_weight, cc_weight, R, permissible_track_fraction} */
  CPMPPI_COST_DEFAULT = 1, /* default.py:23-88 ; cost_w = {dd_weight, ep_weight, cc_weight, R} */
  CPMPPI_COST_LEGACY = 2,  /* controller_mppi_cartpole.py:119-161,227-303 (q + phi); cost_w = {dd_weight, ep_weight,
                              ekp_weight, ekc_weight, cc_weight, ccrc_weight}; the MPPI correction term is part of q */
  CPMPPI_COST_QBG = 3,     /* quadratic_boundary_grad.py:64-232; cost_w = {up: dd_quadratic, dd_linear, db, ep, ekp, cc,
                              ccrc | down: the same seven | target_angular_speed_sqr_max_correction up, down |
                              permissible_track_fraction | cos(admissible_angle) | R}; the set is chosen per env by
                              target_equilibrium == 1 */
  CPMPPI_COST_QB = 4,      /* quadratic_boundary.py:26-87 ; cost_w = {dd_weight, ep_weight, cc_weight, R, ccrc_weight}: default.py
                              with a quadratic track-edge term beyond 0.95 THL and a control-change-rate term against
                              previous_input (added only when a previous input is given, :83-85); default.py's terminal
                              cost.  Runs on default.py's kernels (one more wave-uniform switch); no adjoint, no GRU */
  CPMPPI_COST_QB_NONCONVEX = 5 /* quadratic_boundary_nonconvex.py:27-105: the same plus the cosine ripple on the position term.
                              The reference cannot import this module as shipped (it reads `cem_ccrc_weight`, absent from
                              config_cost_function.yml:47-52); pinned to the outputs of its own class with that one key supplied
                              (:= the section's ccrc_weight; tests/golden/qb_costs.npz "nc/...") */
};

enum { CPMPPI_REDUCE_SUM = 0, CPMPPI_REDUCE_MEAN = 1 };            /* horizon aggregation of the plugin costs */
enum { CPMPPI_CONTROL_CLIP = 0, CPMPPI_CONTROL_PENALISE = 1 };     /* clip u_run & u_nom | legacy 1e5 penalty */
enum { CPMPPI_SHIFT_REPEAT_LAST = 0, CPMPPI_SHIFT_APPEND_ZERO = 1, CPMPPI_SHIFT_NONE = 2 };
enum { CPMPPI_CORRECTION_U_RUN = 0, CPMPPI_CORRECTION_U_NOM = 1 }; /* which u enters the MPPI correction term */
enum { CPMPPI_MATH_PRECISE = 0,  /* IEEE divide, libm-grade sincos, no FMA contraction: closest to numpy float32 */
       CPMPPI_MATH_FAST = 1 };   /* same float32 formulas with folded constants and FMA, v_rcp_f32 divide (<=1.5 ulp),
                                    polynomial sincos on the wrapped angle; inside a control step (cos,sin) advance
                                    by rotation through w*t and are re-synchronised by the exact wrap + sincos at the
                                    step's last substep, so states at control-step granularity carry rounding noise
                                    only (tools/deviation.py: median 1e-6, p99 1e-5 of the reference's own mode A) */
enum { CPMPPI_ODE_V0 = 0,        /* predictor_ODE_v0 (predictors_customization_v0.py:22-57 -> cartpole_numba.py:55-78):
                                    simultaneous forward Euler, elastic edge bounce, fmod angle wrap - the default */
       CPMPPI_ODE_CROMER = 1 };  /* predictor_ODE, predictor_specification "ODE" - what the shipped config_controllers.yml:3,14
                                    names (predictors_customization.py:25-69 -> cartpole_equations.py:181-259,293-308):
                                    Euler-Cromer, NO edge bounce, angle = atan2(sin, cos).  Serves every entry point
                                    that integrates the ODE: cpmppi_step*, cpmppi_predict, cpmppi_rollout_cost (the CEM
                                    family) and cpmppi_rollout_cost_grad (the adjoint of this substep) */
enum { CPMPPI_NOISE_DELTA_U = 0, /* noise = delta_u[E,N,H]  (reference layout, rollout-major)              */
       CPMPPI_NOISE_KNOTS = 1,   /* noise = knots[E,N,P], P = ceil(H/period)+1; interpolated in-kernel       */
       CPMPPI_NOISE_PHILOX = 2,  /* knots generated in-kernel from (seed, offset): no perturbation buffer   */
       CPMPPI_NOISE_DELTA_U_TILED = 3 }; /* noise = delta_u in the library's tiled layout (cpmppi_sample_tiled /
                                    cpmppi_tile_delta_u): [E][ceil(N/64)][ceil(H/4)][64][4], 16-byte aligned          */

typedef struct {
  uint32_t abi_version;          /* CPMPPI_ABI_VERSION */
  uint32_t E;                    /* capacity: independent MPPI problem instances (envs) per call */
  uint32_t N;                    /* rollouts (samples) per env          config_optimizers.yml:91 num_rollouts */
  uint32_t H;                    /* horizon in control steps            config_optimizers.yml:89 mpc_horizon  */
  uint32_t S;                    /* Euler substeps per control step     config_predictors.yml:21 intermediate_steps */
  float dt;                      /* control period; t_step = dt / S     config_optimizers.yml:90 mpc_timestep */
  /* physics — cartpole_physical_parameters.yml:6-17,34,42 rounded to float32 (cartpole_parameters.py:27-31) */
  float k, m_cart, m_pole, g, J_fric, M_fric, u_max, track_half_length;
  float L_default;               /* used where the per-env L pointer is NULL */
  /* cost */
  uint32_t cost_id;
  float cost_w[24];
  /* MPPI — config_optimizers.yml:92-97 */
  float R, LBD, NU, cc_weight;
  float sigma;                   /* knot std-dev = SQRTRHOINV / sqrt(dt) */
  uint32_t period;               /* period_interpolation_inducing_points */
  float action_low, action_high; /* control_limits */
  uint32_t horizon_reduce;       /* CPMPPI_REDUCE_*      (unpinned upstream choice) */
  uint32_t control_mode;         /* CPMPPI_CONTROL_*     (u3) */
  uint32_t shift_mode;           /* CPMPPI_SHIFT_*       (u2) */
  uint32_t correction_u;         /* CPMPPI_CORRECTION_*  */
  uint32_t math_mode;            /* CPMPPI_MATH_* */
  uint32_t rollouts_per_lane;    /* lane mapping of the FAST rollout kernel: 0 = automatic (2 for launches of
                                    >= 131072 rollouts = one packed wave on every SIMD, else 1; measured crossover),
                                    1 = one rollout per lane (lowest latency), 2 = two rollouts per lane as packed
                                    float2 (highest throughput) */
  uint32_t ode_predictor;        /* CPMPPI_ODE_*: which in-tree ODE predictor integrates the rollouts (predictor_type of
                                    SI_Toolkit_ASF/config_predictors.yml:18-26) */
} cpmppi_config;

typedef struct cpmppi_handle cpmppi_handle;

enum { CPMPPI_PREDICTOR_ODE_V0 = 0,   /* the handle's ODE predictor (cpmppi_config.ode_predictor; the name is ABI 1's) */
       CPMPPI_PREDICTOR_GRU = 1 };

/* Neural predictor of BASELINE configs[4] (model naming SI_Toolkit_ASF/config_predictors.yml:8-13): two GRU layers of
 * 32 units and a dense head, torch.nn.GRU convention (gate rows r, z, n; b_ih and b_hh).  HOST pointers; inputs are
 * ordered (Q, angleD, angle_cos, angle_sin, position, positionD), outputs (angleD, angle_cos, angle_sin, position,
 * positionD) — SI_Toolkit's alphabetical feature order; normalised = x*scale + shift (NULL = identity). */
typedef struct {
  uint32_t inputs, hidden, layers, outputs;   /* 6, 32, 2, 5 */
  const float* w_ih[2];                       /* [96,6], [96,32] */
  const float* w_hh[2];                       /* [96,32] */
  const float* b_ih[2];                       /* [96] */
  const float* b_hh[2];                       /* [96] */
  const float* w_out;                         /* [5,32] */
  const float* b_out;                         /* [5] */
  const float* in_scale;  const float* in_shift;    /* [6] */
  const float* out_scale; const float* out_shift;   /* [5] */
} cpmppi_gru_model;

/* One optimizer step for `E` envs (E <= config.E).  All pointers are device pointers. */
typedef struct {
  uint32_t E;                       /* active envs in this call */
  const float* s0;                  /* [E,6]  current state of each env */
  float* u_nom;                     /* [E,H]  in: nominal sequence as left by the previous step (the kernel applies
                                              config.shift_mode itself); out: updated nominal sequence */
  const float* u_prev;              /* [E,H]  legacy control-change-rate term only; NULL = use u_nom as found on entry
                                              (controller_mppi_cartpole.py:558) */
  const float* target_position;     /* [E] */
  const float* target_equilibrium;  /* [E] */
  const float* L;                   /* [E] pole length per env, or NULL = config.L_default */
  uint32_t noise_kind;              /* CPMPPI_NOISE_* */
  const float* noise;               /* delta_u[E,N,H], knots[E,N,P] or the tiled delta_u; ignored for CPMPPI_NOISE_PHILOX */
  uint64_t seed;                    /* CPMPPI_NOISE_PHILOX: key */
  uint64_t offset;                  /* CPMPPI_NOISE_PHILOX: step counter (fresh noise per step) */
  uint32_t env_offset;              /* CPMPPI_NOISE_PHILOX: global index of env 0 (rank * E_local when sharded) */
  float* Q_out;                     /* [E]    first element of the updated nominal sequence */
  float* S_out;                     /* [E,N]  per-rollout total cost, or NULL */
  uint32_t predictor;               /* CPMPPI_PREDICTOR_ODE_V0 (default, 0) or CPMPPI_PREDICTOR_GRU */
  const float* h0;                  /* GRU only: hidden state per env [E,2,32] shared by the env's rollouts, or NULL=0 */
  const float* previous_input;      /* [E] control applied before this step (Q_ccrc of CartPole/__init__.py:517): the
                                       control-change-rate term of quadratic_boundary_grad at stage 0; NULL = 0 */
  uint64_t* offset_dev;             /* CPMPPI_NOISE_PHILOX, optional: the step counter in DEVICE memory — read by the kernel
                                       instead of `offset` and incremented by one after the step, stream-ordered.  With it a
                                       captured HIP graph of (step, plant, ...) can be replayed: no launch argument changes
                                       between control steps.  NULL = use `offset`. */
  float* u_nom_out;                 /* [E,H] optional (ODE predictor): where the updated nominal sequence is written; `u_nom`
                                       is then only read.  Two buffers used alternately let a consumer of step i's result
                                       (the all-gather of cpmppi_comm_gather) overlap step i+1 without a snapshot copy.
                                       NULL = in place (u_nom). */
} cpmppi_step_args;

int cpmppi_create(const cpmppi_config* cfg, int device, cpmppi_handle** out);
void cpmppi_destroy(cpmppi_handle* h);
const char* cpmppi_last_error(const cpmppi_handle* h);  /* h may be NULL: error of the last failed cpmppi_create */
int cpmppi_get_config(const cpmppi_handle* h, cpmppi_config* out);

/* Which instantiation of the rollout kernel the handle's most recent cpmppi_step / cpmppi_step_host / cpmppi_step_gather /
 * cpmppi_rollout_cost launch used (all zero before the first one) - so that a caller that verifies or times a launch can
 * name the kernel it ran: rollout_cost_kernel<cost_id, math_mode == FAST, noise_kind, rollouts_per_lane, build_variant>.
 * build_variant: 0 = latency build (one rollout per lane, at most one wave per SIMD), 1 = throughput build, 2 = mid-size
 * build (phased horizon loop), 3 = its form for launches of at most one wave per SIMD. */
typedef struct {
  uint32_t cost_id, math_mode, noise_kind, rollouts_per_lane, build_variant, ode_predictor, blocks;
  uint32_t cost_plugin;   /* the PUBLIC cost id of the handle (CPMPPI_COST_*): quadratic_boundary (4) and _nonconvex (5) run on
                             default.py's kernels, so `cost_id` - the kernel's template argument - reads 1 for both */
} cpmppi_launch_info;
int cpmppi_last_launch(const cpmppi_handle* h, cpmppi_launch_info* out);

/* Mutable per-call knobs (GUI sliders / attribute updates in the reference mutate these between steps). */
int cpmppi_set_cost_weights(cpmppi_handle* h, uint32_t cost_id, const float* cost_w, uint32_t n);
/* The pole mass every later call of this handle computes with (config.m_pole until then): predictor_ODE takes it from
 * variable_parameters.m_pole at every step (predictors_customization.py:55-58; the simulator sends 'm_pole' with every
 * controller.step, CartPole/__init__.py:509-520).  Handle-wide (one value for all envs; a mass per row: cpmppi_set_pole_mass_rows
 * below); launches already enqueued - and captured graphs - keep the value they were enqueued with.  This is the
 * CONTROLLER's belief (the simulator sends m_pole_for_controller): the plant of cpmppi_plant_advance* keeps config.m_pole. */
int cpmppi_set_pole_mass(cpmppi_handle* h, float m_pole);
/* Per-row pole mass the ODE predictor computes with: m_pole[n], DEVICE pointer, caller-owned, read by every later launch
 * of this handle where that call's L would be indexed (env for step / step_gather / groups / rollout_cost / rollout_cost_grad /
 * step_host, row for predict).  NULL (n ignored) returns to the handle's scalar (cpmppi_set_pole_mass).  A call with more
 * rows than n fails with CPMPPI_ERR_BAD_ARG and launches nothing.  Refused (BAD_ARG) on a handle whose ode_predictor is
 * ODE_v0: predictor_ODE_v0 never reads the attribute.  GRU steps ignore it.  The plant keeps its own mass.
 * next_state_predictor_ODE broadcasts variable_parameters.m_pole per row exactly as it does L (predictors_customization.py:51-64);
 * a row computes bit for bit what a handle whose scalar is that row's mass computes.  A misaligned pointer is refused (BAD_ARG).
 * Only the POINTER is taken: launches already enqueued, and captured graphs, keep the pointer they were enqueued with and read the
 * VALUES when they run - a caller may rewrite the array between launches (stream-ordered) without calling this again.  Each handle
 * of an env group is given the array offset by the group's first env. */
int cpmppi_set_pole_mass_rows(cpmppi_handle* h, const float* m_pole, uint32_t n);
/* Per-env controller tuning of the fused MPPI step: rows[n][CPMPPI_TUNING_ROW_FLOATS], DEVICE pointer, caller-owned, 64-byte
 * aligned, read by every later cpmppi_step / cpmppi_step_gather / cpmppi_step_host of this handle at the env index where that
 * call indexes L.  A row holds the seven entries of quadratic_boundary_grad_minimal's cost vector in cpmppi_set_cost_weights
 * order (dd_weight, db_weight, ep_weight, ekp_weight, cc_weight, R, permissible_track_fraction - the sliders of the reference's
 * GUI/_ControllerGUI_MPPIOptionsWindow.py), then LBD ([CPMPPI_TUNING_LBD]) and sigma = SQRTRHOINV / sqrt(dt)
 * ([CPMPPI_TUNING_SIGMA]); the other floats pad the row to 64 bytes and are not read.  The optimizer's own R, NU, cc_weight and
 * the control limits stay the handle's.  NULL (n ignored) returns to the handle's scalars.  An env computes bit for bit what a
 * handle whose scalars are its row computes (the same build of the rollout kernel, compiled a second time with the nine values
 * read per env through wave-uniform loads; the throughput build's per-env fold reads the row).  Only the POINTER is taken:
 * launches already enqueued, and captured graphs, keep the pointer they were enqueued with and read the VALUES when they run - a
 * caller may rewrite the array between launches and between replays (stream-ordered) without calling this again.
 * Refused (CPMPPI_ERR_BAD_ARG, "cpmppi_set_tuning_rows: ...", nothing changes): n == 0 with a non-null pointer, a misaligned
 * pointer, a handle whose cost plugin is not quadratic_boundary_grad_minimal, a handle with pole-mass rows registered
 * (cpmppi_set_pole_mass_rows refuses the reverse).  While rows are registered a step with more envs than n, with a noise_kind other
 * than CPMPPI_NOISE_PHILOX or with the GRU predictor is refused (nothing launched, outputs untouched), and so are, by name,
 * cpmppi_rollout_cost, cpmppi_rollout_cost_grad, cpmppi_rpgd_step, cpmppi_cem_step, cpmppi_predict, cpmppi_trajectory_cost,
 * cpmppi_groups_run / _run_gather, cpmppi_rollout_cost_gru, cpmppi_rollout_cost_grad_gru, the samplers that draw with the
 * handle's sigma (cpmppi_sample, and cpmppi_sample_tiled without knots_in), cpmppi_reward_weighted_average, and cpmppi_set_cost_weights with another cost plugin.
 * A handle without the fused finalize (CPMPPI_FUSE_FINALIZE=0) merges an env's block partials with the row's LBD as well. */
#define CPMPPI_TUNING_ROW_FLOATS 16u
enum { CPMPPI_TUNING_LBD = 7, CPMPPI_TUNING_SIGMA = 8 };
int cpmppi_set_tuning_rows(cpmppi_handle* h, const float* rows, uint32_t n);

/* a17 — device sampler: knots ~ sigma * N(0,1) from Philox4x32-10 keyed by (seed), counter (rollout, env, knot pair,
 * offset); writes knots[E,N,P] and/or the interpolated delta_u[E,N,H] (either pointer may be NULL).
 * Interpolation follows controller_mppi_cartpole.py:434-446. */
int cpmppi_sample(cpmppi_handle* h, uint32_t E, uint64_t seed, uint64_t offset, uint32_t env_offset,
                  float* knots_out, float* delta_u_out, void* stream);

/* Interpolate caller-provided knots[E,N,P] (e.g. drawn with numpy SFC64 for bit-identical parity runs) to
 * delta_u[E,N,H]. */
int cpmppi_interpolate(cpmppi_handle* h, uint32_t E, const float* knots, float* delta_u_out, void* stream);

/* The TILED perturbation layout — delta_u[E,N,H] (controller_mppi_cartpole.py:434-446 produces it rollout-major) stored as
 * [E][G = ceil(N/64)][Hq = ceil(H/4)][64 rows][4 steps]: element (env, n, k) at
 * ((((env*G + n/64)*Hq + k/4)*64 + n%64)*4 + k%4, padding zero.  The rollout kernel reads it with fully used, contiguous
 * 1 KB wave accesses (the rollout-major layout costs 5.9x the algorithmic traffic at H = 50).
 *   cpmppi_tiled_floats   number of floats of the tiled buffer for E envs (allocate 16-byte aligned)
 *   cpmppi_sample_tiled   a17 straight into it: Philox knots (knots_in NULL) or caller knots[E,N,P], interpolated
 *   cpmppi_tile_delta_u   re-tile a reference-layout delta_u[E,N,H] (one coalesced pass: worth it when the buffer is
 *                         reused over several steps — for a single step the extra pass costs more than the rollout-major
 *                         kernel's over-fetch: 0.7 ms vs 0.36 ms at 8192 envs x 1024 x 50) */
size_t cpmppi_tiled_floats(const cpmppi_handle* h, uint32_t E);
int cpmppi_sample_tiled(cpmppi_handle* h, uint32_t E, uint64_t seed, uint64_t offset, uint32_t env_offset,
                        const float* knots_in, float* tiled_out, void* stream);
int cpmppi_tile_delta_u(cpmppi_handle* h, uint32_t E, const float* delta_u, float* tiled_out, void* stream);

/* Predictor seam (a9-a11): B independent rollouts.  s0[B,6], Q[B,H] (dimensionless control in [-1,1]),
 * L[B] or NULL -> traj[B,H+1,6] with traj[:,0]=s0.  horizon may be < config.H (0 = config.H). */
int cpmppi_predict(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* s0, const float* Q, const float* L,
                   float* traj_out, void* stream);

/* Cost seam (a12-a14): trajectories traj[B,H+1,6], inputs[B,H] -> stage_out[B,H] (may be NULL), terminal_out[B]
 * (may be NULL), total_out[B] (may be NULL; sum or mean per config.horizon_reduce, plugin costs only).
 * target_position / target_equilibrium are host scalars here (the plugin reads them from variable_parameters).
 * Legacy cost additionally needs u_nom[H], u_prev[H] (device) and interprets `inputs` as delta_u;
 * quadratic_boundary_grad reads its previous_input from u_prev[0] (NULL = 0). */
int cpmppi_trajectory_cost(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* traj, const float* inputs,
                           float target_position, float target_equilibrium, const float* u_nom, const float* u_prev,
                           float* stage_out, float* terminal_out, float* total_out, void* stream);

/* Fused hot path: rollout (a3-a11) + cost (a12-a15) + importance-weighted update (a16) + shift/clip (a18). */
int cpmppi_step(cpmppi_handle* h, const cpmppi_step_args* args, void* stream);

/* The fused step for a caller whose state lives on the HOST - the simulator's own call, controller.step(s, time,
 * updated_attributes) -> Q (CartPole/__init__.py:509-520): s0[E,6], target_position[E], target_equilibrium[E], L[E] (or
 * NULL) and Q[E] are HOST pointers, u_nom[E,H] stays a device buffer (the plan persists between control steps); in-kernel
 * Philox noise (seed, offset, env_offset as in cpmppi_step_args).  Synchronous by nature.
 *   up to 64 envs (CPMPPI_HOST_ZERO_COPY_MAX; the simulator's call is one): NO copy and NO stream wait - the inputs are
 *     staged into the handle's pinned, device-mapped block, which the kernel reads directly; the env's finalizing block
 *     stores Q into the same block and bumps a system-scope ticket the calling thread spins on (the stream is polled
 *     every few thousand spins, so a failed launch returns CPMPPI_ERR_HIP instead of hanging);
 *   more envs: one asynchronous copy up, the launch, one copy down, a wait on the stream. */
int cpmppi_step_host(cpmppi_handle* h, uint32_t E, const float* s0, const float* target_position,
                     const float* target_equilibrium, const float* L, float* u_nom, uint64_t seed, uint64_t offset,
                     uint32_t env_offset, float* Q, void* stream);

/* Kernel timing with HIP events recorded on the launch stream (off by default; enable = 0 switches it off).
 * enable = 1: every cpmppi_step is bracketed by an event before the rollout kernel, one after it and - only when a
 *   separate finalize or counter kernel follows - a third after those; rollout_ms / finalize_ms are per step.
 * enable = n > 1: ONE bracket around every n consecutive steps (an event costs ~5 us on the stream - two per launch
 *   are 10 % of a 100 us launch and would show in any wall-clock figure taken at the same time); rollout_ms then holds,
 *   per completed group, the bracket divided by n: the average duration of a step's kernels back to back, inter-launch
 *   gaps included; finalize_ms is 0.
 * cpmppi_get_profile synchronises on the events, returns the entries recorded since the last call (at most max_steps
 * are written; *n_steps receives their number) and resets the recorder. */
int cpmppi_set_profiling(cpmppi_handle* h, int enable);
int cpmppi_get_profile(cpmppi_handle* h, float* rollout_ms, float* finalize_ms, uint32_t max_steps, uint32_t* n_steps);

/* Attach / replace the GRU model of a handle (synchronous upload; not for the launch path).  The model is packed into three weight
 * images: the exact-f32 fragments with their plain vectors, the transposed fragments of the reverse sweeps, and the f16 split image
 * of the FAST kernels (every weight as hi = f16(w), lo = f16(w - hi)).
 * Refused with CPMPPI_ERR_BAD_ARG ("cpmppi_set_gru: ..."):
 *   "non-finite value in <tensor>": a NaN or an infinity in any of the ten weight tensors or of the four normalisation vectors;
 *   "weights beyond the f16 range": a value v STORED in the f16 image with !(|v| < 60000).  Gate rows are stored pre-scaled - r and
 *     z by -log2(e), n by 2 log2(e) - so the largest accepted float32 magnitude of a weight of w_ih / w_hh differs per gate:
 *     41588.83 (r, z), 20794.414 (n); of the head w_out, stored as it is, 59999.996.  Biases are kept in float32: finite is all
 *     they need be.  (Measured on the MI355X with one entry per matrix and gate at 0.9 of its limit in a model of scale 0.3: FAST
 *     and PRECISE both conform to the float32 / float64 oracle under the cost and control rules of the tests: DESIGN 8, N5.)
 * A refusal changes nothing: the handle keeps the three images, the normalisation and the flat parameters of the model it held
 * (none, if none was set: the GRU entry points go on refusing with "no model set"), and a training run goes on.  Everything that
 * can refuse is checked on host copies before the handle or the device is touched.
 * The f16 split carries an OPERAND only within +-65504: a normalised input x * in_scale + in_shift, a fed-back head output or a
 * memory entry beyond that splits into hi = inf, lo = -inf and the FAST products are NaN, where the exact-f32 kernels stay finite.
 * The memory lies in [-1, 1]; inputs and outputs are the caller's to keep inside (a normalised control of 6.0e4 is confirmed to
 * agree with the oracle in both modes).  Nothing checks it at run time. */
int cpmppi_set_gru(cpmppi_handle* h, const cpmppi_gru_model* model);

/* Predictor seam with the neural predictor (predictor_autoregressive_neural; augmentation angle = atan2(sin, cos),
 * SI_Toolkit_ASF/ToolkitCustomization/predictors_customization.py:121-127): s0[B,6], Q[B,H], h0[2,B,32] or NULL ->
 * traj[B,H+1,6], h_out[2,B,32] or NULL (device pointers). */
int cpmppi_gru_predict(cpmppi_handle* h, uint32_t B, uint32_t horizon, const float* s0, const float* Q, const float* h0,
                       float* traj_out, float* h_out, void* stream);

/* Advance each env's GRU memory by one control step, in place: h_io[E,2,32] (the layout of cpmppi_step_args.h0)
 * <- hidden states after one cell step on (s[E,6], Q[E]) - update_internal_state of the reference
 * (Control_Toolkit_ASF/Controllers/controller_mppi_cartpole.py:566-567) for every env at once.  Exact-f32 chain in both math
 * modes: the value cpmppi_gru_predict(B = E, horizon = 1, h0 = transpose(h_io)) writes to h_out, bit for bit.
 * ONE launch on `stream`, no allocation, no host synchronisation: can be captured.  With it a neural control period of the device
 * loop is cpmppi_step(predictor = CPMPPI_PREDICTOR_GRU, h0 = h_io), cpmppi_gru_advance, cpmppi_plant_step.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned (cpmppi_last_error: "cpmppi_gru_advance: ...") when no model is set,
 * E == 0 or E > cfg.E, or a pointer is NULL. */
int cpmppi_gru_advance(cpmppi_handle* h, uint32_t E, const float* s, const float* Q, float* h_io, void* stream);

/* The GRU memory along R recordings of T rows each (update_before_predicting of the reference's Brunton test):
 * h_rows_out[R,T,2,32] with h_rows_out[r,0] = h0[r] (h0[R,2,32], NULL = zeros) and h_rows_out[r,t+1] = the memory after one
 * exact cell step on (states[r,t], Q[r,t]) from h_rows_out[r,t] - bit for bit what T-1 successive cpmppi_gru_advance calls
 * leave in h_io.  states[R,T,6], Q[R,T]; device pointers.  ONE launch on `stream`, no allocation: can be captured.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_gru_washout: ...") when no model is set, R == 0, T == 0 or a
 * required pointer is NULL. */
int cpmppi_gru_washout(cpmppi_handle* h, uint32_t R, uint32_t T, const float* states, const float* Q, const float* h0,
                       float* h_rows_out, void* stream);

/* Brunton test (SI_Toolkit_ASF/Run/A3_Run_Brunton_Test.py, config_testing.yml): the open-loop error of a predictor over
 * recordings.  From every start row t = start .. start+count-1 of each of R recordings of T rows the predictor is rolled forward
 * `horizon` control steps on the RECORDED controls Q[r,t+k], beginning at states[r,t]; the state after step k is compared with
 * states[r,t+k+1].  Error per feature, in state order, in float32: e = predicted - recorded, the angle's wrapped afterwards,
 * e - 2 pi rint(e / 2 pi).  stats_out[horizon,6,3] (DEVICE doubles): (sum |e|, sum e^2, max |e|) over all R*count starts, horizon
 * step k+1 at index k - reduced in a fixed order without atomics: the same bits from run to run.  pred_out (optional)
 * [R*count,horizon+1,6]: the predictions, [b,0] the start state, b = r*count + (t-start): what cpmppi_predict /
 * cpmppi_gru_predict return for the materialised windows, bit for bit.
 * predictor CPMPPI_PREDICTOR_ODE_V0: the handle's ODE predictor in the handle's math mode, pole length L[r,t] of the start row or
 * config.L_default, pole mass the handle's (cpmppi_set_pole_mass_rows is not read).  CPMPPI_PREDICTOR_GRU: the network of
 * cpmppi_set_gru (exact-f32 cell) with the memory h_rows[r,t] of the start row (cpmppi_gru_washout; NULL = zeros everywhere).
 * Two launches on `stream`; the workspace of partial sums is allocated on first use and grown on demand - a capture that
 * would have to allocate is refused (run the call once before capturing).
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_brunton: ...") for a NULL required pointer; R, count or
 * horizon == 0; horizon > config.H; start + count + horizon > T; an unknown predictor; the GRU without a model; L with the GRU;
 * h_rows without it. */
typedef struct {
  uint32_t R, T;                 /* recordings, rows of each */
  uint32_t start, count;         /* start rows start .. start+count-1 of every recording */
  uint32_t horizon;              /* control steps predicted from each start (test_max_horizon) */
  uint32_t predictor;            /* CPMPPI_PREDICTOR_ODE_V0 or CPMPPI_PREDICTOR_GRU */
  const float* states;           /* [R,T,6] */
  const float* Q;                /* [R,T] */
  const float* L;                /* [R,T] or NULL (ODE only) */
  const float* h_rows;           /* [R,T,2,32] or NULL (GRU only) */
  double* stats_out;             /* [horizon,6,3] */
  float* pred_out;               /* [R*count,horizon+1,6] or NULL */
} cpmppi_brunton_args;
int cpmppi_brunton(cpmppi_handle* h, const cpmppi_brunton_args* args, void* stream);

/* Score of a recording, per env, reduced on the device: the two numbers the reference's simulator prints after every experiment
 * (CartPole/__init__.py:727-729) and three more, from the device loop's logs where they lie (cpmppi_plant_step /
 * cpmppi_plant_advance_record: states_log, the target-position table, Q_log).  Over the saved rows r of the window
 * first_row <= r < last_row (last_row = 0: rows) it writes score_out[env][CPMPPI_SCORE_FLOATS]:
 *   [CPMPPI_SCORE_MEAN_ABS_DISTANCE]   mean |position - target_position|                                  (:727)
 *   [CPMPPI_SCORE_MEAN_ABS_ANGLE_DEG]  mean |angle| * 180 / pi                                            (:728)
 *   [CPMPPI_SCORE_MEAN_Q_SQUARED]      mean Q^2 over the controller calls q_first <= c < q_last (q_last = 0: q_rows); 0 without Q
 *   [CPMPPI_SCORE_STABLE_SHARE]        the share of the window's rows with |angle| < pi / 5, compared in float32 as the reference
 *                                      compares (TARGET_ANGLE_UP, CartPole/CheckStabilized.py:7,24)
 *   [CPMPPI_SCORE_FIRST_STABLE_ROW]    the first saved row of the window from which |angle| < pi / 5 holds to the window's end,
 *                                      `rows` if the window's last row is outside that angle (a NaN angle is outside it)
 * The target of saved row r: row min(r * save_every / sched_stride, sched_rows - 1) of target_position_table (the rule of
 * cpmppi_plant_step; save_every, sched_stride 0 = 1), else target_position[env], else the scalar target_position_value.
 * Every term is formed and summed in float64 - rows r = first_row + w, + w + W, ... by wave w of the W waves of a workgroup, the
 * waves' sums added in wave order through LDS - and rounded to float32 once: no atomics, the same bits from run to run.  Lanes
 * run along envs (the logs are env-contiguous).  ONE launch on `stream` for any E and rows, no allocation, no host synchronisation:
 * can be captured.  Reads no configuration of the handle (its device and error text only).
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_score_runs: ...") for a NULL states or score_out; E or rows == 0;
 * row_envs != 0 and < E; an empty or reversed window, or one that ends beyond rows (likewise Q's against q_rows); a table without
 * sched_rows; more than 2^24 rows.  A misaligned pointer is CPMPPI_ERR_ALIGN. */
#define CPMPPI_SCORE_FLOATS 5u
enum { CPMPPI_SCORE_MEAN_ABS_DISTANCE = 0, CPMPPI_SCORE_MEAN_ABS_ANGLE_DEG = 1, CPMPPI_SCORE_MEAN_Q_SQUARED = 2,
       CPMPPI_SCORE_STABLE_SHARE = 3, CPMPPI_SCORE_FIRST_STABLE_ROW = 4 };
typedef struct {
  uint32_t E;                           /* envs scored */
  uint32_t row_envs;                    /* envs per ROW of the logs and the table (0 = E), as in cpmppi_plant_args */
  uint32_t rows;                        /* saved rows of states */
  uint32_t first_row, last_row;         /* the window of saved rows; last_row 0 = rows */
  uint32_t q_rows;                      /* rows of Q (controller calls) */
  uint32_t q_first, q_last;             /* the window of controller calls; q_last 0 = q_rows */
  uint32_t save_every, sched_stride;    /* simulation steps per saved row / per table row */
  uint64_t sched_rows;                  /* rows of target_position_table */
  const float* states;                  /* [rows][row_envs][6] */
  const float* target_position_table;   /* [sched_rows][row_envs], or NULL */
  const float* target_position;         /* [E] without a table, or NULL */
  float target_position_value;          /* the target without either */
  const float* Q;                       /* [q_rows][row_envs], or NULL */
  float* score_out;                     /* [E][CPMPPI_SCORE_FLOATS] */
} cpmppi_score_args;
int cpmppi_score_runs(cpmppi_handle* h, const cpmppi_score_args* args, void* stream);

/* Control along recorded trajectories (SI_Toolkit_ASF/Run/PreprocessData_Add_Control_Along_Trajectories.py; fanned out over 120
 * single-CPU jobs by others/EulerClusterScripts/ControllerAlongTrajectories.sh): a controller's output along recordings that exist
 * already.  This call stands where cpmppi_plant_step stands in the device loop: it hands the controller the RECORDED row where the
 * plant would hand it the simulated one, and reduces the evaluations of a row to one number.  The upstream transformation
 * (SI_Toolkit.data_preprocessing.transform_dataset) is not part of the reference checkout, so the semantics here are this
 * library's own.
 * R recordings padded to T rows, rows[r] their true lengths; K evaluations (independent controller instances) per recording:
 * env e = r*K + k, E = R*K, the copies of a recording contiguous.  Inputs in the layout of cpmppi_brunton.
 * One call = one control period c, ONE kernel:
 *   collect  for every recording with c < rows[r]: Q_mean_out[r*T + c] = mean over k of Q[r*K + k]; Q_std_out[r*T + c] = the sample
 *            standard deviation (divisor K - 1; 0 for K == 1); Q_all_out[c][E] = Q as found.  Rows at or past rows[r] are not
 *            written.  Mean and deviation are formed in float64 by ONE wave per recording, in a fixed order without atomics -
 *            lane l adds Q[r*K + l], Q[r*K + l + 64], ... in ascending k; the 64 lane sums are added by a butterfly (each lane adds
 *            lane l^32's sum, then l^16's, l^8's, l^4's, l^2's, l^1's); mean = sum / K; the deviation is a second pass in the same
 *            order over (Q - mean)^2, sqrt(sum / (K - 1)) - and each is rounded to float32 once: the same bits from run to run,
 *            for any K.
 *   publish  for all K copies of r, from row p = min(c + 1, rows[r] - 1) of the recording: s_out[e][6], target_position_out[e],
 *            target_equilibrium_out[e], L_out[e], previous_input_out[e] (the recorded Q_ccrc / "Q_applied_-1": point the step's
 *            previous_input there) - what controller call c + 1 reads.  A period past the longest recording keeps publishing
 *            last rows and collects nothing: a graph replayed beyond the end reads and writes nothing outside the buffers.
 *   prime    (prime != 0) publishes row 0 and collects nothing: called once before controller call 0.
 *   reset    u_nom_reset[E,H] given: zero-filled, so that every row is solved from a cold plan (any H).
 * period_dev: c = *period_dev - 1 under the rule of cpmppi_plant_step (the step's counter, already advanced); a counter that is
 * still 0 names no controller call made: the call then behaves as a prime call (row 0 published, nothing collected).
 * No allocation, no host synchronisation: can be captured.  Reads no configuration of the handle but config.E.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_replay_step: ...") for a NULL states, Q, rows or rows_host; R, T
 * or K == 0; R*K > config.E; a rows_host[r] of 0 or above T; no output at all; an output without its input column; u_nom_reset
 * without H.  A misaligned pointer is CPMPPI_ERR_ALIGN. */
typedef struct {
  uint32_t R, T, K;                     /* recordings, rows of each (padded), evaluations per recording */
  uint32_t H;                           /* columns of u_nom_reset */
  uint32_t prime;                       /* != 0: publish row 0, collect nothing */
  uint64_t period;                      /* c */
  const void* period_dev;               /* or NULL */
  const uint32_t* rows;                 /* [R] DEVICE: the true lengths, 1..T (the kernel clamps what it reads to that range) */
  const uint32_t* rows_host;            /* [R] HOST: the same lengths, checked by every call */
  const float* states;                  /* [R,T,6] */
  const float* target_position;         /* [R,T] or NULL */
  const float* target_equilibrium;      /* [R,T] or NULL */
  const float* L;                       /* [R,T] or NULL */
  const float* previous_input;          /* [R,T] or NULL */
  const float* Q;                       /* [E] the controls of controller call c */
  float* Q_mean_out;                    /* [R,T] or NULL */
  float* Q_std_out;                     /* [R,T] or NULL */
  float* Q_all_out;                     /* [T][E] or NULL */
  float* s_out;                         /* [E,6] or NULL */
  float* target_position_out;           /* [E] or NULL */
  float* target_equilibrium_out;        /* [E] or NULL */
  float* L_out;                         /* [E] or NULL */
  float* previous_input_out;            /* [E] or NULL */
  float* u_nom_reset;                   /* [E,H] or NULL */
} cpmppi_replay_args;
int cpmppi_replay_step(cpmppi_handle* h, const cpmppi_replay_args* args, void* stream);

/* Training the GRU predictor on recordings (SI_Toolkit_ASF/Run/A2_Train_Network.py with config_training.yml; the training code
 * itself is not part of the reference checkout, so the semantics here are this library's own): the teacher-forced loss of the
 * handle's model over windows of recordings, its gradient by back-propagation through time, and Adam on the device.
 * The parameters are ONE flat float32 vector of CPMPPI_GRU_PARAMS floats in the torch.nn.GRU order of cpmppi_gru_model:
 *   w_ih0[96,6] w_hh0[96,32] b_ih0[96] b_hh0[96] w_ih1[96,32] w_hh1[96,32] b_ih1[96] b_hh1[96] w_out[5,32] b_out[5].
 *
 * cpmppi_gru_loss_grad: B windows (r, t0) of W + P rows each, W = wash_out, P = post_wash_out, over recordings in the layout of
 * cpmppi_brunton.  Per window the memory starts at zero and rows t0 .. t0+W+P-1 are fed AS RECORDED - the normalised
 * (Q, angleD, angle_cos, angle_sin, position, positionD); nothing is fed back.  The loss is the mean over B x P x 5 of the squared
 * difference between the head's normalised output at window row j >= W and the label (x - out_shift) / out_scale of the features
 * x of recorded row t0 + j + shift_labels.  loss_out: one DEVICE double.  grad_out[CPMPPI_GRU_PARAMS] (DEVICE): d loss / d
 * parameters in the flat order, or NULL for the loss alone (validation), which equals the loss of a gradient call bit for bit.
 * Exact-f32 cell and exact-f32 MFMA throughout; every reduction runs in a fixed order without atomics: the same bits from run to
 * run.  Launches on `stream`: forward sweep, loss; with a gradient also the reverse sweep, the weight-gradient contraction and its
 * reduction.  The workspace (check-points and adjoints of every (row, window)) is reserved by cpmppi_gru_train_reserve(h, B, rows)
 * for windows of up to `rows` = W + P rows, or on first use - a capture that would have to allocate is refused.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_gru_loss_grad: ...") when no model is set; states, Q, windows,
 * windows_host or loss_out is NULL; B, R, T or post_wash_out is 0; a host window lies outside r < R,
 * t0 + W + P - 1 + shift_labels <= T - 1.  A misaligned pointer is CPMPPI_ERR_ALIGN.
 *
 * cpmppi_gru_train_begin: a device master copy of the handle's model (the weights of the last cpmppi_set_gru) in the flat order,
 * both Adam moments zero, the device step counter 0; the two float32 images below are rebuilt from it.  Synchronous.
 * cpmppi_gru_train_step: (1) cpmppi_gru_loss_grad into the handle's own gradient buffer (loss_args->grad_out is not read),
 * (2) one bias-corrected Adam update of the master copy, t = the device counter + 1, formed in float64 and stored as float32:
 *     m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2, p -= lr (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + eps),
 * (3) the rebuild ON THE DEVICE of the two float32 weight images the training kernels read - the fragment image and the
 * transposed image of the exact-f32 cell - bit for bit what cpmppi_set_gru builds on the host for the same weights, the plain
 * vectors (gate biases, head) of the PRECISE fused kernels included.  The f16 image of the FAST kernels keeps the model of the last
 * cpmppi_set_gru: a trained model reaches them through cpmppi_gru_train_get and cpmppi_set_gru.  So during a run a PRECISE handle
 * rolls out, costs and differentiates the TRAINED model, a FAST handle's fused steps and cpmppi_rollout_cost_gru the model of the
 * last cpmppi_set_gru - and a FAST cpmppi_rollout_cost_grad_gru mixes the two (its forward sweep reads the f16 image, its reverse
 * sweep the float32 images): do not use it between cpmppi_gru_train_begin and the next cpmppi_set_gru.
 * No host synchronisation: capturable after a reserving call.
 * CPMPPI_ERR_BAD_ARG ("cpmppi_gru_train_step: ...") without cpmppi_gru_train_begin, and what cpmppi_gru_loss_grad refuses.
 * cpmppi_gru_train_get: the master copy -> params_host[CPMPPI_GRU_PARAMS], synchronously.
 * A successful cpmppi_set_gru ENDS a training run (a refused one leaves it alone): the master copy, the moments and the counter belong to the model before it.  Until the next
 * cpmppi_gru_train_begin - which starts a run from the model just set - cpmppi_gru_train_step, cpmppi_gru_rollout_train_step and
 * cpmppi_gru_train_get return CPMPPI_ERR_BAD_ARG ("...: call cpmppi_gru_train_begin first"), launch nothing and leave the images
 * of the model just set as they are.  cpmppi_gru_loss_grad and its rollout sibling need no run and read the model just set.
 * (A step captured into a graph before cpmppi_set_gru is not the library's to refuse at replay: capture it again after the new
 * cpmppi_gru_train_begin.)
 *
 * cpmppi_gru_rollout_loss_grad: the same loss THROUGH THE OPEN-LOOP ROLLOUT, which is how every consumer of a trained model runs it
 * (cpmppi_gru_predict, cpmppi_brunton, the control steps).  The same argument block, windows (r, t0) of W + P rows, zero start
 * memory and recording layout.  Rows j <= W are fed as recorded: the wash-out is teacher-forced and row W, the first scored row, is
 * the recorded start row, as in the Brunton test.  Rows j > W take input rows 0..4 (angleD .. positionD) from the head's NORMALISED
 * OUTPUT of row j - 1, unchanged - the rule of cpmppi_gru_predict, not a de-normalise / re-normalise round trip - and row 5 from the
 * recorded Q[t0 + j] normalised with in_scale[0], in_shift[0].  The loss is the teacher-forced one: the mean over B x P x 5 of
 * (y_j - (features of row t0 + j + 1 - out_shift) / out_scale)^2 for j >= W.  shift_labels must be 1: the output of row j is the
 * input of row j + 1.  grad_out: d loss / d all CPMPPI_GRU_PARAMS parameters through the feedback - the head adjoint of row j,
 * W <= j < W + P - 1, is its own 2 (y - label) / (B P 5) plus rows 0..4 of the input adjoint of row j + 1; the input adjoints of
 * rows <= W and of the Q row are dropped.  With P = 1 nothing is fed back and the loss is cpmppi_gru_loss_grad's bit for bit.
 * The same launches, workspace (cpmppi_gru_train_reserve, unchanged in size), determinism and capture rule as cpmppi_gru_loss_grad.
 * Refused ("cpmppi_gru_rollout_loss_grad: ..."), nothing launched: what cpmppi_gru_loss_grad refuses, and shift_labels != 1.
 * cpmppi_gru_rollout_train_step: cpmppi_gru_train_step with that loss and gradient ("cpmppi_gru_rollout_train_step: ...").  Steps of
 * both kinds may alternate on one master copy and one Adam state; cpmppi_gru_train_begin / _get serve both. */
#define CPMPPI_GRU_PARAMS 10341u
typedef struct {
  uint32_t B;                           /* windows */
  uint32_t R, T;                        /* recordings, rows of each */
  uint32_t wash_out, post_wash_out;     /* W rows that only build the memory, then P >= 1 rows that are scored */
  uint32_t shift_labels;                /* the label of a row lies this many rows on (1 for a dynamics model) */
  const float* states;                  /* [R,T,6] */
  const float* Q;                       /* [R,T] */
  const uint32_t* windows;              /* [B][2] DEVICE: (r, t0) */
  const uint32_t* windows_host;         /* [B][2] HOST: the same, checked by every call */
  double* loss_out;                     /* DEVICE, one double */
  float* grad_out;                      /* [CPMPPI_GRU_PARAMS] DEVICE, or NULL */
} cpmppi_gru_loss_args;
int cpmppi_gru_train_reserve(cpmppi_handle* h, uint32_t B, uint32_t rows);
int cpmppi_gru_loss_grad(cpmppi_handle* h, const cpmppi_gru_loss_args* args, void* stream);
int cpmppi_gru_train_begin(cpmppi_handle* h);
int cpmppi_gru_train_step(cpmppi_handle* h, const cpmppi_gru_loss_args* args, float lr, float beta1, float beta2, float eps,
                          void* stream);
int cpmppi_gru_train_get(cpmppi_handle* h, float* params_host);
int cpmppi_gru_rollout_loss_grad(cpmppi_handle* h, const cpmppi_gru_loss_args* args, void* stream);
int cpmppi_gru_rollout_train_step(cpmppi_handle* h, const cpmppi_gru_loss_args* args, float lr, float beta1, float beta2, float eps,
                                  void* stream);

/* Fitting the ODE predictor's PHYSICAL PARAMETERS to recordings (SI_Toolkit_ASF/ToolkitCustomization/Modules/ODE_module.py, the
 * "fake network" Custom-ODE_module-ODEModel of config_training.yml whose weights are the cartpole's parameters; the training code
 * itself is not part of the reference checkout, so windows, loss, parametrisation and schedule are this library's own).
 * The parameters are CPMPPI_ODE_FIT_PARAMS = 8 floats in the order  k, m_cart, m_pole, g, J_fric, M_fric, u_max, L ; bit i of
 * `trainable` selects parameter i.  TrackHalfLength is not offered: only the edge-bounce test reads it, and the derivative of the
 * open-loop error with respect to it is zero almost everywhere.
 *
 * cpmppi_ode_fit_loss_grad: B windows (r, t0) over recordings in the layout of cpmppi_brunton.  A window starts at states[r,t0]
 * and integrates `horizon` control steps on the RECORDED controls Q[r,t0+j] with the plain substep of the handle's math mode and ODE
 * predictor (wrap + sin / cos on every substep: what cpmppi_rollout_cost_grad differentiates); step j predicts row t0+j+1.  The loss
 * is the mean over B x horizon x 5 of ((predicted - recorded) * feature_scale[f])^2, f = angleD, angle_cos, angle_sin, position,
 * positionD (the angle itself is not scored: a wrap taken differently costs nothing).  The derivative is carried FORWARD with the
 * state (tangents of angle, angleD, position, positionD per trained parameter); the branch taken decides it through the edge
 * bounce, which reads L directly, and it is 1 through fmod, the wrap and atan2(sin, cos).  The parameters are the running ones of a
 * fit (below) or, before cpmppi_ode_fit_begin, the handle's own with its scalar pole mass; L[R,T], when given, is the pole length
 * per start row as in cpmppi_brunton and replaces parameter 7.
 * loss_out: one DEVICE double.  grad_out[8] DEVICE doubles: d loss / d theta_i = p_i d loss / d p_i (see cpmppi_ode_fit_begin;
 * exactly 0 for a parameter that is not trainable), or NULL for the loss alone, which equals the loss of a gradient call with the
 * same `trainable` bit for bit.  per_window_out[B][1+8] DEVICE floats, or NULL: per window the sum over its steps and features of
 * the squared scaled error and that sum's derivative d / d p_i - neither divided by B x horizon x 5 nor multiplied by p_i.
 * No atomics: a workgroup writes its own row of partial sums, a second kernel walks the rows in a fixed order in float64 - the same
 * bits from run to run.  The workspace is reserved by cpmppi_ode_fit_reserve(h, B) for up to B windows, or on first use - a capture
 * that would have to allocate is refused.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned ("cpmppi_ode_fit_loss_grad: ...") for a NULL states, Q, windows,
 * windows_host or loss_out; B, R, T or horizon equal to 0; horizon > config.H; a host window outside r < R, t0 + horizon <= T - 1;
 * an empty or unknown `trainable` mask; a trainable parameter whose base value is <= 0; trainable L together with L rows; per-row
 * pole masses registered on the handle (cpmppi_set_pole_mass_rows).  A misaligned pointer is CPMPPI_ERR_ALIGN.
 *
 * cpmppi_ode_fit_begin: a fit starts.  base_i = the handle's configuration with its scalar pole mass (L: L_default);
 * p_i = base_i * exp(theta_i) with theta = 0 - the parameters span five decades, must stay positive, and one learning rate has to
 * serve them all -; both Adam moments and the device step counter are zero.  Synchronous.
 * cpmppi_ode_fit_set_theta: theta <- theta_host[8] and p = (float)(base * exp((double)theta)) on the device; the moments and the
 * counter stay.  Synchronous.
 * cpmppi_ode_fit_step: (1) the loss and d loss / d theta of cpmppi_ode_fit_loss_grad into the handle's own buffer (grad_out is
 * not read), (2) per trainable parameter the bias-corrected Adam update of theta stated at cpmppi_gru_train_step, t = the device
 * counter + 1, formed in float64 and stored as float32, (3) p = (float)(base * exp((double)theta)) rewritten for the next step's
 * kernel.  A parameter that is not trainable keeps theta and p bit for bit.  No host synchronisation: capturable after a reserving
 * call.  cpmppi_ode_fit_get: p -> params_host[8], theta -> theta_host[8] (either may be NULL), synchronously.
 * cpmppi_ode_fit_step, _get and _set_theta before cpmppi_ode_fit_begin: CPMPPI_ERR_BAD_ARG ("...: call cpmppi_ode_fit_begin
 * first").  The handle's own physics is never changed: a fitted model reaches the other kernels through a new handle. */
#define CPMPPI_ODE_FIT_PARAMS 8u
typedef struct {
  uint32_t B;                           /* windows */
  uint32_t R, T;                        /* recordings, rows of each */
  uint32_t horizon;                     /* control steps per window, 1..config.H */
  uint32_t trainable;                   /* bit i: parameter i of k, m_cart, m_pole, g, J_fric, M_fric, u_max, L */
  const float* states;                  /* [R,T,6] */
  const float* Q;                       /* [R,T] */
  const float* L;                       /* [R,T] pole length per start row, or NULL = parameter 7 */
  const uint32_t* windows;              /* [B][2] DEVICE: (r, t0) */
  const uint32_t* windows_host;         /* [B][2] HOST: the same, checked by every call */
  float feature_scale[5];               /* angleD, angle_cos, angle_sin, position, positionD */
  double* loss_out;                     /* DEVICE, one double */
  double* grad_out;                     /* [8] DEVICE: d loss / d theta, or NULL */
  float* per_window_out;                /* [B][1+8] DEVICE, or NULL */
} cpmppi_ode_fit_args;
int cpmppi_ode_fit_reserve(cpmppi_handle* h, uint32_t B);
int cpmppi_ode_fit_loss_grad(cpmppi_handle* h, const cpmppi_ode_fit_args* args, void* stream);
int cpmppi_ode_fit_begin(cpmppi_handle* h);
int cpmppi_ode_fit_set_theta(cpmppi_handle* h, const float* theta_host);
int cpmppi_ode_fit_step(cpmppi_handle* h, const cpmppi_ode_fit_args* args, float lr, float beta1, float beta2, float eps,
                        void* stream);
int cpmppi_ode_fit_get(cpmppi_handle* h, float* params_host, float* theta_host);

/* The NEURAL IMITATOR of the MPC: the one Dense network the reference ships (GymlikeCartPole/Dense-7IN-32H1-32H2-1OUT-0/, forward
 * pass C_implementation/network.c; config_training.yml configures its training as shipped) as a controller and its training on
 * recordings.  7 inputs -> 32 tanh -> 32 tanh -> 1 linear output.  The reference's controller_neural_imitator lives in a submodule
 * that is absent from the reference checkout, and so does the training code: the semantics below - the feature order, the clip of
 * the control, windows, loss and schedule - are THIS LIBRARY'S OWN.  Other layer sizes, activations, several models per launch and a
 * Dense dynamics model inside an optimizer are not built.
 * The parameters are ONE flat float32 DEVICE vector of CPMPPI_DENSE_PARAMS = 1345 floats in torch.nn.Linear order ([out,in]):
 *   w1[32,7] b1[32] w2[32,32] b2[32] w3[1,32] b3[1].
 * The 7 inputs in the shipped folder's (alphabetical) order: angleD, angle_cos, angle_sin, position, positionD,
 * target_equilibrium, target_position.  Normalisation: x_n = in_scale x + in_shift per input; Q = out_scale y + out_shift for the
 * head's output y.  That vector is the only image: the control kernel and the training kernels read it as it stands and Adam
 * updates it in place - nothing is repacked.  tanh is the one of the exact-f32 GRU cell: 1 - 2 / (exp(2x) + 1).
 *
 * cpmppi_set_dense: HOST pointers; in_scale / in_shift [7] and out_scale / out_shift [1] may be NULL (identity).  Everything that
 * can refuse runs on host copies before the handle changes - a NULL weight array, a non-finite value in any of the eight arrays
 * (CPMPPI_ERR_BAD_ARG, "cpmppi_set_dense: ...") -: a refused call leaves the model held, the bits of cpmppi_dense_control and a
 * live training run as they were.  A successful call ENDS a training run (as cpmppi_set_gru does).  Synchronous.
 *
 * cpmppi_dense_control: one control per env, Q_out[e] = clamp(out_scale y + out_shift, -1, 1), from the state s[E,6] in this
 * library's layout (angle, angleD, angle_cos, angle_sin, position, positionD; the angle itself is not an input) and the env's
 * targets.  y_out[E], optional: the head's normalised output y before de-normalisation and clip.  A NaN in an env's inputs gives
 * a NaN control in that env (the clamp passes it on) and touches no other env.  With count_dev: *count_dev += 1 after the step,
 * stream-ordered, exactly as cpmppi_rpgd_step documents it - a captured graph of (control, plant step with period_dev) replays.
 * One launch (a lane per env; the weights arrive wave-uniform through the constant address space), no host synchronisation, no
 * allocation.  Refused ("cpmppi_dense_control: ..."), nothing launched: no model set; E == 0; a NULL s, target_position,
 * target_equilibrium or Q_out; a misaligned pointer (CPMPPI_ERR_ALIGN; count_dev: 8 bytes).
 *
 * cpmppi_dense_loss_grad: B windows (r, t0) of P = post_wash_out rows over recordings states[R,T,6], target_position[R,T],
 * target_equilibrium[R,T], labels[R,T].  The network has no memory, so a window is P independent samples: sample (b, j) reads the
 * inputs of row t0 + j and the label of row t0 + j + shift_labels.  loss = the mean over the B P samples of
 * (y - (label - out_shift) / out_scale)^2.  loss_out: one DEVICE double.  grad_out[CPMPPI_DENSE_PARAMS] DEVICE floats: d loss / d
 * parameters in the flat order, or NULL for the loss alone (validation), which equals the loss of a gradient call bit for bit.
 * Two launches: (1) forward, backward and, per workgroup of 128 samples, its own row of partial sums written with plain stores - the
 * contraction over the samples (d w2 = sum dz2 (x) h1, likewise d w1, d w3 and the bias sums against ones) on
 * v_mfma_f32_32x32x2_f32 in exact f32 with the sample as the contraction index; (2) one workgroup walks the rows first to last in
 * float64 and scales by 2 / (B P).  No atomics, every sum in a fixed order: the same bits from run to run, whatever ran before.
 * The rows are reserved by cpmppi_dense_train_reserve(h, samples) for calls of up to `samples` = B P, or on first use - a capture
 * that would have to allocate is refused.
 * Refused ("cpmppi_dense_loss_grad: ..."), nothing launched: no model set; a NULL states, target_position, target_equilibrium,
 * labels, windows, windows_host or loss_out; B, R, T or post_wash_out equal to 0; more than 2^31 samples; a host window outside
 * r < R, t0 + P - 1 + shift_labels <= T - 1.  A misaligned pointer is CPMPPI_ERR_ALIGN.
 *
 * cpmppi_dense_train_begin: a run starts from the model held: both Adam moments and the device step counter zero.  Synchronous.
 * cpmppi_dense_train_step: launch (1) of cpmppi_dense_loss_grad (grad_out is not read), then launch (2) which also applies the
 * bias-corrected Adam update stated at cpmppi_gru_train_step to the parameter vector IN PLACE, t = the device counter + 1, the
 * gradient and the update formed in float64, moments and parameters stored as float32.  A parameter whose gradient is exactly 0 and
 * whose moments are 0 keeps its bits.  From the next launch on cpmppi_dense_control runs the trained model.  No host
 * synchronisation: capturable after a reserving call.  loss_out: the batch's loss BEFORE the update.
 * cpmppi_dense_train_get: the parameter vector -> params_host[CPMPPI_DENSE_PARAMS], synchronously.
 * cpmppi_dense_train_step and _get before cpmppi_dense_train_begin, or after a successful cpmppi_set_dense:
 * CPMPPI_ERR_BAD_ARG ("...: call cpmppi_dense_train_begin first"), nothing launched. */
#define CPMPPI_DENSE_PARAMS 1345u
typedef struct {
  const float* w1;                      /* [32,7]  HOST, rows = units, columns in the input order above */
  const float* b1;                      /* [32] */
  const float* w2;                      /* [32,32] */
  const float* b2;                      /* [32] */
  const float* w3;                      /* [1,32] */
  const float* b3;                      /* [1] */
  const float* in_scale;                /* [7] or NULL (1) */
  const float* in_shift;                /* [7] or NULL (0) */
  const float* out_scale;               /* [1] or NULL (1) */
  const float* out_shift;               /* [1] or NULL (0) */
} cpmppi_dense_model;
typedef struct {
  uint32_t E;                           /* envs */
  const float* s;                       /* [E,6] */
  const float* target_position;         /* [E] */
  const float* target_equilibrium;      /* [E] */
  float* Q_out;                         /* [E] */
  float* y_out;                         /* [E] or NULL */
  unsigned long long* count_dev;        /* DEVICE counter advanced by one behind the step, or NULL */
} cpmppi_dense_control_args;
typedef struct {
  uint32_t B;                           /* windows */
  uint32_t R, T;                        /* recordings, rows of each */
  uint32_t post_wash_out;               /* P >= 1 rows per window, each one sample */
  uint32_t shift_labels;                /* the label of a row lies this many rows on (0 for an imitator) */
  const float* states;                  /* [R,T,6] */
  const float* target_position;         /* [R,T] */
  const float* target_equilibrium;      /* [R,T] */
  const float* labels;                  /* [R,T] the control to imitate */
  const uint32_t* windows;              /* [B][2] DEVICE: (r, t0) */
  const uint32_t* windows_host;         /* [B][2] HOST: the same, checked by every call */
  double* loss_out;                     /* DEVICE, one double */
  float* grad_out;                      /* [CPMPPI_DENSE_PARAMS] DEVICE, or NULL */
} cpmppi_dense_loss_args;
int cpmppi_set_dense(cpmppi_handle* h, const cpmppi_dense_model* model);
int cpmppi_dense_control(cpmppi_handle* h, const cpmppi_dense_control_args* args, void* stream);
int cpmppi_dense_train_reserve(cpmppi_handle* h, uint32_t samples);
int cpmppi_dense_loss_grad(cpmppi_handle* h, const cpmppi_dense_loss_args* args, void* stream);
int cpmppi_dense_train_begin(cpmppi_handle* h);
int cpmppi_dense_train_step(cpmppi_handle* h, const cpmppi_dense_loss_args* args, float lr, float beta1, float beta2, float eps,
                            void* stream);
int cpmppi_dense_train_get(cpmppi_handle* h, float* params_host);

/* FINE-TUNING the neural imitator ON THE TASK COST through the ODE plant: the exact derivative of the closed-loop trajectory cost
 * - the net drives the handle's ODE predictor, the handle's plugin cost scores the trajectory - with respect to the 1345
 * parameters.  The reference trains its controller net with PPO from stable-baselines3 (GymlikeCartPole/Train_RL_Cartpole.py, a
 * score-function estimator over 500 000 CPU steps); this library holds the reverse sweep of both ODE predictors and of the plugin
 * costs (cpmppi_rollout_cost_grad) and the net's backward pass (cpmppi_dense_loss_grad), and composes them.  The semantics are
 * THIS LIBRARY'S OWN.
 * The handle's predictor is ODE_v0 or ODE, its cost quadratic_boundary_grad_minimal or default; dt, the substep count S,
 * horizon_reduce and the physical parameters are the handle's.  Recordings states[R,T,6], target_position[R,T],
 * target_equilibrium[R,T]; a batch is B windows (r, t0), each needing ONE row.  For window b, with s_0 = states[r,t0] and the two
 * targets of that row held over the horizon, for k = 0 .. horizon-1:
 *   x_k = the 7 normalised inputs of (s_k, target_equilibrium, target_position); y_k = the net's output; q_k = out_scale y_k +
 *   out_shift; u_k = clamp(q_k, -1, 1) - the bits cpmppi_dense_control gives for that state; the stage cost is that of (s_k, u_k);
 *   s_{k+1} = S substeps of the predictor in the plain form cpmppi_rollout_cost_grad integrates (stage 0 takes cos(angle) of the
 *   given state, as there).
 * J_b = scale (sum of the stage costs + the terminal cost), scale = 1 or 1 / (horizon + 1) by horizon_reduce, exactly what
 * cpmppi_rollout_cost_grad returns for the plan u_0 .. u_{horizon-1} from s_0 on a handle whose H is `horizon`.
 * loss = (1 / B) sum_b J_b.  grad_out: d loss / d parameters in the flat order.  Non-smooth pieces as cpmppi_rollout_cost_grad
 * differentiates them: the branch taken at the bounce, derivative 1 through the wrap, 0 through indicators and through a clipped
 * control - a step whose q_k lies outside [-1, 1] passes nothing back through the net at that step.  L[R], optional: the pole
 * length per recording (NULL: the handle's); the pole mass is the handle's.  cost_out[B], optional: J_b.  Q_out[B,horizon],
 * optional: the u_k.  The sensitivity of the closed loop grows fast with the horizon (an unstable plant under a net that does not
 * stabilise it yet): float32 gradients are meaningful for short horizons, and the train step guards itself (below).
 * Two launches: (1) a lane per start state, ONE wave per workgroup: forward with s_k check-pointed per control step, then for
 * k = horizon-1 .. 0 the substeps' reverse sweep, the stage gradient and the net's backward pass with d J / d y_k in the place of
 * the MSE residual, contracted over the wave's 64 samples on v_mfma_f32_32x32x2_f32 into accumulators that live across all steps;
 * one partial row per workgroup, plain stores.  (2) cpmppi_dense_loss_grad's finalize launch with the scale 1 / B.  No atomics, no
 * host synchronisation, every sum in a fixed order: the same bits from run to run, whatever ran before.  grad_out == NULL: the
 * loss alone, bit for bit the loss of a gradient call.
 * cpmppi_dense_policy_reserve(h, B, horizon): check-points and partial rows for calls of up to B windows and that horizon; they
 * are otherwise allocated on first use, and a capture that would have to allocate is refused.
 * cpmppi_dense_policy_train_step: launch (1), then a finalize launch that walks the partial rows in float64 in fixed order, forms
 * the gradient's global 2-norm over the 1345 entries in a fixed order, scales the gradient by min(1, clip_norm / norm)
 * (clip_norm <= 0: off) and applies the Adam update of cpmppi_dense_train_step to the live parameter vector in place.  The run is
 * the one cpmppi_dense_train_begin starts: moments and counter are shared with cpmppi_dense_train_step, so MSE steps and cost
 * steps may alternate.  If the loss or the norm is not finite, parameters, moments and the step counter keep their bits;
 * loss_out still carries the non-finite value.  loss_out: the loss BEFORE the update.  grad_out is not read.
 * Refused ("cpmppi_dense_policy_...: ..."), nothing launched, CPMPPI_ERR_BAD_ARG: no model set; _train_step before
 * cpmppi_dense_train_begin; a NULL states, target_position, target_equilibrium, windows, windows_host or loss_out; B, R, T or
 * horizon equal to 0 (horizon > CPMPPI_MAX_HORIZON); a host window outside r < R, t0 <= T - 1; a handle that holds a GRU model
 * (cpmppi_set_gru: the GRU as the differentiated plant is not built); a cost other than the two above; a math mode other than
 * FAST; per-env tuning rows or pole-mass rows registered; S beyond the LDS sub-state buffer.  A misaligned pointer is
 * CPMPPI_ERR_ALIGN (loss_out: 8 bytes).  Not built: measurement noise, latency or control disturbance inside the differentiated
 * rollout, stochastic policies, other net sizes. */
typedef struct {
  uint32_t B;                           /* windows = start states */
  uint32_t R, T;                        /* recordings, rows of each */
  uint32_t horizon;                     /* control steps of the closed loop */
  const float* states;                  /* [R,T,6] */
  const float* target_position;         /* [R,T] */
  const float* target_equilibrium;      /* [R,T] */
  const float* L;                       /* [R] pole length per recording, or NULL (the handle's) */
  const uint32_t* windows;              /* [B][2] DEVICE: (r, t0) */
  const uint32_t* windows_host;         /* [B][2] HOST: the same, checked by every call */
  double* loss_out;                     /* DEVICE, one double */
  float* grad_out;                      /* [CPMPPI_DENSE_PARAMS] DEVICE, or NULL */
  float* cost_out;                      /* [B] DEVICE, or NULL: J_b */
  float* Q_out;                         /* [B,horizon] DEVICE, or NULL: the controls u_k */
} cpmppi_dense_policy_args;
int cpmppi_dense_policy_reserve(cpmppi_handle* h, uint32_t B, uint32_t horizon);
int cpmppi_dense_policy_loss_grad(cpmppi_handle* h, const cpmppi_dense_policy_args* args, void* stream);
int cpmppi_dense_policy_train_step(cpmppi_handle* h, const cpmppi_dense_policy_args* args, float lr, float beta1, float beta2,
                                   float eps, float clip_norm, void* stream);
/* Test aid: the check-point workspace of the calls above is the handle's own, so a test cannot fence it from outside.
 * cpmppi_dense_policy_ckpt_floats: how many floats are reserved (0 before the first reserving call).
 * cpmppi_dense_policy_ckpt_copy: the first `floats` of them <- host[floats] (to_device != 0) or -> host[floats], synchronously (the
 * device is synchronised before and after).  A launch of `rows` = ceil(B / 64) workgroups and `horizon` steps writes and reads
 * exactly the first horizon * 6 * rows * 64 floats.  Refused (CPMPPI_ERR_BAD_ARG): a NULL host, more floats than are reserved. */
uint64_t cpmppi_dense_policy_ckpt_floats(cpmppi_handle* h);
int cpmppi_dense_policy_ckpt_copy(cpmppi_handle* h, float* host, uint64_t floats, int to_device);

/* DAgger (Ross, Gordon, Bagnell 2011) for the neural imitator: one control period in which the EXPERT labels the state and the
 * imitator - or, per env and period, a coin that favours the expert with probability beta - drives.  cpmppi_dagger_step is ONE
 * launch, a lane per env, enqueued after the expert's step of the period (the fused cpmppi_step, cpmppi_rpgd_step, ... writing
 * Q_expert) and before the plant launch (reading Q_out).  Per env e, in this order:
 *  1. Q_imi = what cpmppi_dense_control gives for s[e], target_position[e], target_equilibrium[e], bit for bit (one forward body,
 *     on the live parameter vector: a cpmppi_dense_train_step enqueued before this call is seen by it).
 *  2. The gate: one Philox4x32-10 block with the counter (0xFFFFFFFF, env_offset + e, 0, low word of c) - no rollout has that
 *     index, so the block is none of the sampler's - and the sampler's key (low word of seed ^ 0x51ed270b, high word of seed ^ high
 *     word of c).  ub = (word 1 >> 8) 2^-24 in [0, 1); the expert drives iff ub < beta[e]: always for beta = 1, never for
 *     beta <= 0 or a NaN.
 *  3. Q_out[e] = the expert drives ? Q_expert[e] : Q_imi.  No arithmetic on the chosen value: a NaN passes, in its env only.
 *  4. Only if c < T, row (r0 + e, c) of the dataset - exactly the tensors cpmppi_dense_loss_args reads - is written:
 *     states <- s[e], rec_target_position / rec_target_equilibrium <- the two targets, labels <- Q_expert[e]; and, where given,
 *     imitator_out <- Q_imi, gate_out <- 0 / 1.  For c >= T the control is still computed and nothing else is written: a captured
 *     graph replayed past the end touches nothing outside the buffers.
 *  5. With sq_err, for a sample that was recorded (c < T): d = (double)Q_imi - (double)Q_expert; sq_err[e] = sq_err[e] + d * d (two
 *     roundings, a plain load and store by the env's own lane, no atomics): the on-policy disagreement over the env's recording,
 *     summed by the caller.  Past the end nothing changes anywhere but Q_out.
 * c is `period`, or with period_dev *period_dev - 1: the expert's step has already advanced the counter (the rule of
 * cpmppi_replay_step / cpmppi_plant_step).  The host cannot see that counter, so one still at 0 is not refused here: on the device
 * the call is then treated as c = 0.  The kernel does not advance the counter.  No allocation, no host synchronisation: capturable.
 * Refused ("cpmppi_dagger_step: ..."), nothing launched, CPMPPI_ERR_BAD_ARG: no model set (cpmppi_set_dense); E == 0 or
 * E > config.E; a NULL s, target_position, target_equilibrium, Q_expert, beta, Q_out, states, rec_target_position,
 * rec_target_equilibrium or labels; R or T equal to 0; r0 + E > R; Q_out overlapping Q_expert.  A misaligned pointer is
 * CPMPPI_ERR_ALIGN (sq_err and period_dev: 8 bytes). */
typedef struct {
  uint32_t E;                           /* envs */
  const float* s;                       /* [E,6] the state the controllers are shown */
  const float* target_position;         /* [E] */
  const float* target_equilibrium;      /* [E] */
  const float* Q_expert;                /* [E] the expert's control of this period */
  const float* beta;                    /* [E] DEVICE: the probability that the expert drives */
  uint64_t seed;                        /* the gate's Philox key */
  uint32_t env_offset;                  /* global index of env 0 */
  uint64_t period;                      /* c, unless period_dev is given */
  const unsigned long long* period_dev; /* DEVICE counter already advanced by the expert's step (c = *period_dev - 1), or NULL */
  float* Q_out;                         /* [E] the applied control */
  uint32_t R, T, r0;                    /* the dataset: recordings, rows of each - env e writes recording r0 + e */
  float* states;                        /* [R,T,6] */
  float* rec_target_position;           /* [R,T] */
  float* rec_target_equilibrium;        /* [R,T] */
  float* labels;                        /* [R,T] */
  float* imitator_out;                  /* [R,T] or NULL */
  uint8_t* gate_out;                    /* [R,T] or NULL: 1 where the expert drove */
  double* sq_err;                       /* [E] DEVICE, accumulated, or NULL */
} cpmppi_dagger_args;
int cpmppi_dagger_step(cpmppi_handle* h, const cpmppi_dagger_args* args, void* stream);

/* Rollout + cost only (no update): per-rollout trajectory cost S[E,N] of GIVEN input sequences inputs[E,N,H] under the
 * handle's plugin cost — cost_function.get_trajectory_cost(predictor.predict_core(s, Q), Q) fused; the building block of
 * the sampling optimizers that are not MPPI. */
int cpmppi_rollout_cost(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs, const float* target_position,
                        const float* target_equilibrium, const float* L, float* S_out, void* stream);

/* The same with the neural predictor in the rollout loop (cpmppi_set_gru): S[E,N] = get_trajectory_cost(predict_core_GRU(s,
 * Q), Q) of GIVEN input sequences inputs[E,N,H] - what a cpmppi_step with predictor = CPMPPI_PREDICTOR_GRU writes into S_out
 * when inputs are its delta_u, the nominal sequence is zero, cc_weight is 0 and nothing is shifted, without the MPPI update
 * (no weights, no weighted sums, no finalize).  The building block of cem, cem-gmm and random-action over the GRU.
 * h0[E,2,32] (the layout of cpmppi_step_args.h0: one memory per env, shared by its rollouts) or NULL = zeros.  The handle's
 * control_mode applies to the inputs (clip: to [action_low, action_high]); FAST math runs the split-f16 cell, PRECISE the
 * exact-f32 chains, as the fused step chooses them.  Reads no pole mass and no L.  ONE launch on `stream`, no allocation and
 * no host synchronisation: the call can be captured into a graph.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned (cpmppi_last_error: "cpmppi_rollout_cost_gru: ...") when no model is
 * set, E == 0 or E > cfg.E, a pointer other than h0 is NULL, or the handle's cost is neither quadratic_boundary_grad_minimal
 * nor default. */
int cpmppi_rollout_cost_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs,
                            const float* target_position, const float* target_equilibrium, const float* h0, float* S_out,
                            void* stream);

/* cpmppi_rollout_cost_gru and the gradient of its costs with respect to the inputs: S[E,N] (may be NULL) and
 * grad[E,N,H] = d get_trajectory_cost(predict_core_GRU(s, Q), Q) / d Q - what the gradient optimizers (gradient-tf, rpgd, the
 * CEM + gradient hybrids) need of the neural predictor.  The function differentiated is exactly the one
 * cpmppi_rollout_cost_gru evaluates (same h0[E,2,32] or NULL, the same two costs, horizon_reduce and clamp); non-smooth pieces
 * follow cpmppi_rollout_cost_grad: 0 through a clipped control and through the indicator terms of `default` (its terminal cost
 * and therefore atan2 included); cos(angle) = c / sqrt(c^2 + s^2) is differentiated through both network outputs; the stage-0
 * cos(angle) comes from s0 and carries no gradient.
 * Two launches on `stream`.  (1) Forward sweep: the cost-only rollout in the handle's math mode (FAST: split f16, PRECISE:
 * exact f32) - S_out is bit-identical to cpmppi_rollout_cost_gru's - which parks, after every control step but the last, both
 * hidden tiles and the five fed-back outputs of every rollout: 69 floats per rollout and step, padded to 72 (16-byte accesses);
 * the gates are not stored.  (2) Reverse sweep, exact-f32
 * MFMA in BOTH math modes over a transposed weights image that cpmppi_set_gru builds beside the other two: per step, from the
 * last to the first, head adjoint, then each layer's gates recomputed from the check-points right before its cell adjoint: layer-2 cell,
 * layer-1 cell; the Q row of the input adjoint is the gradient, its five feature rows are the feedback into the step before.
 * Workspace: H * 72 * cfg.E * cfg.N floats ([H][E N][72]), allocated on first use; under stream capture a call that would have to allocate is
 * refused - call once before the capture, after that the call can be captured.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned (cpmppi_last_error: "cpmppi_rollout_cost_grad_gru: ...") when no model
 * is set, E == 0 or E > cfg.E, a pointer other than h0 and S_out is NULL, or the handle's cost is neither
 * quadratic_boundary_grad_minimal nor default. */
int cpmppi_rollout_cost_grad_gru(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs,
                                 const float* target_position, const float* target_equilibrium, const float* h0,
                                 float* S_out, float* grad_out, void* stream);

/* Rollout + plugin cost + its gradient with respect to the inputs: S[E,N] (may be NULL) and
 * grad[E,N,H] = d get_trajectory_cost(predict_core(s, Q), Q, previous_input) / d Q — what TensorFlow's GradientTape
 * hands to the gradient-based optimizers of the absent Control_Toolkit (Control_Toolkit_ASF/config_optimizers.yml:49-86,
 * sections gradient-tf and rpgd; :21-48 the CEM+gradient hybrids).  FAST arithmetic, plugin costs only; the edge bounce
 * is differentiated along the branch taken, indicators and a clipped control contribute zero.  previous_input[E] may be
 * NULL (0).  Allocates H*6*E*N floats of check-points on first use. */
int cpmppi_rollout_cost_grad(cpmppi_handle* h, uint32_t E, const float* s0, const float* inputs,
                             const float* target_position, const float* target_equilibrium, const float* L,
                             const float* previous_input, float* S_out, float* grad_out, void* stream);

/* One Adam iteration on the input sequences Q[E,N,H] (in place; m, v are the caller-owned moment buffers, zero before
 * iteration 1): per-rollout gradient-norm clipping to gradmax_clip (<= 0: off), Keras-style bias correction, then the
 * clip to [action_low, action_high] (config_optimizers.yml:52-58,69-73). */
int cpmppi_adam_step(cpmppi_handle* h, uint32_t E, float* Q, const float* grad, float* m, float* v, uint32_t iteration,
                     float learning_rate, float beta1, float beta2, float epsilon, float gradmax_clip, void* stream);

/* The whole rpgd / gradient-tf control step of E envs in ONE call: no host synchronisation, no allocation, and - with
 * count_dev - no launch argument that changes between control steps, so a captured graph of (step, plant) replays.
 * It is cpmppi_rollout_cost_grad + cpmppi_adam_step `iterations` times, the final cost, the choice of the best plan, the
 * resampling of rpgd and the shift, written out below.  `c` = control steps taken before this call: *count_dev if given,
 * else count.
 *   1. for i = 1..iterations: cost and gradient of every plan (cpmppi_rollout_cost_grad's arithmetic, previous_input and
 *      per-env pole masses included), then cpmppi_adam_step's update with t = a + i, a = adam_iteration (host mode) or
 *      c * iterations (device mode); lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) is formed in double IN THE KERNEL in both modes.
 *   2. final cost S of every plan: the adjoint kernel's forward sweep (sin / cos evaluated on every substep).
 *   3. best = first plan in the stable order by (cost, index) of cpmppi_cem_update: torch.argmin's choice for finite costs;
 *      where a cost is NaN it is ranked LAST, so a finite plan is chosen (torch.argmin would pick the NaN).
 *      Q_out[env] = Q[env, best, 0]; plan_out, S_out and order_out are filled as found BEFORE steps 4 and 5.
 *   4. if resamp_per > 0, keep_k < N and (c + 1) % resamp_per == 0: rows 0..keep_k-1 become the keep_k best plans in rank
 *      order with their moments; rows keep_k..N-1 are redrawn with zero moments - row n gets what cpmppi_sample(seed, o,
 *      env_offset) interpolates for rollout n (the handle's sigma and period), + sample_mean (CPMPPI_RPGD_NORMAL) or mapped
 *      through the normal CDF to U(uniform_lo, uniform_hi) (CPMPPI_RPGD_UNIFORM), clipped to the action limits;
 *      o = draw_offset (host mode) or draw_offset + c / resamp_per (device mode).
 *   5. Q, m, v are shifted left by `shift`; Q repeats its last element, m and v are filled with 0.
 *   6. with count_dev: *count_dev += 1 after the step, stream-ordered (as cpmppi_step treats offset_dev).
 * Refused with CPMPPI_ERR_BAD_ARG: everything cpmppi_rollout_cost_grad refuses, N > 256 (one workgroup per env, one lane per
 * plan), keep_k == 0 or > N, iterations == 0, shift > H, a NULL or misaligned required pointer, and a stream under capture
 * while the workspace of cpmppi_rpgd_reserve is missing or too small (outside a capture the step allocates it itself).
 * cpmppi_rpgd_reserve(h, E): allocates the workspace for steps of up to E envs (H * 7 * E * ceil64(N) floats). */
typedef enum { CPMPPI_RPGD_NORMAL = 0, CPMPPI_RPGD_UNIFORM = 1 } cpmppi_rpgd_distribution;
typedef struct {
  uint32_t E;                       /* active envs in this call */
  const float* s0;                  /* [E,6] */
  const float* target_position;     /* [E] */
  const float* target_equilibrium;  /* [E] */
  const float* L;                   /* [E] pole length per env, or NULL = config.L_default */
  const float* previous_input;      /* [E] control applied before this step, or NULL = 0 */
  float* Q;                         /* [E,N,H] the plans, updated in place */
  float* m;                         /* [E,N,H] Adam first moments, updated in place */
  float* v;                         /* [E,N,H] Adam second moments, updated in place */
  uint32_t iterations;              /* Adam iterations in this step */
  uint32_t adam_iteration;          /* Adam iterations taken before this call (host mode) */
  float learning_rate;
  float beta1;
  float beta2;
  float epsilon;
  float gradmax_clip;               /* <= 0: off */
  uint32_t keep_k;                  /* keep_k == N or resamp_per == 0: never resample */
  uint32_t resamp_per;
  uint32_t shift;                   /* 0 .. H */
  uint32_t distribution;            /* cpmppi_rpgd_distribution */
  float sample_mean;
  float uniform_lo;
  float uniform_hi;
  uint64_t seed;                    /* Philox key of the redraw */
  uint64_t draw_offset;             /* Philox offset of the redraw (host mode), or of the first redraw (device mode) */
  uint32_t env_offset;              /* global index of env 0 */
  uint64_t count;                   /* control steps taken before this call (host mode) */
  uint64_t* count_dev;              /* the same counter in DEVICE memory (8-byte aligned), or NULL = host mode */
  float* Q_out;                     /* [E]   the chosen control */
  float* S_out;                     /* [E,N] final costs, indexed by the plan rows as they are BEFORE step 4, or NULL */
  float* plan_out;                  /* [E,H] the best plan before the shift, or NULL */
  uint32_t* order_out;              /* [E,N] the ranking (plan rows, cheapest first), or NULL */
} cpmppi_rpgd_args;
int cpmppi_rpgd_reserve(cpmppi_handle* h, uint32_t E);
int cpmppi_rpgd_step(cpmppi_handle* h, const cpmppi_rpgd_args* args, void* stream);

/* cpmppi_rpgd_step with the controller's tuning PER ENV: rows[n_rows][CPMPPI_TUNING_ROW_FLOATS], DEVICE pointer, caller-owned,
 * 64-byte aligned, indexed by the env index with which the call indexes L.  Entries 0-6 of a row are
 * quadratic_boundary_grad_minimal's cost vector in cpmppi_set_cost_weights order (as a row of cpmppi_set_tuning_rows), entry
 * CPMPPI_RPGD_ROW_LR Adam's learning rate and entry CPMPPI_RPGD_ROW_GRADMAX_CLIP the gradient-norm clip (<= 0: off); the other
 * floats pad the row to 64 bytes and are not read.  args->learning_rate and args->gradmax_clip are not read.
 * An env computes bit for bit what cpmppi_rpgd_step computes on a handle whose cost weights are its row, with that row's learning
 * rate and clip in the argument block (rpgd_step_kernel compiled a second time, the nine values read per env through wave-uniform
 * loads; with cpmppi_set_pole_mass_rows registered the env's pole mass is read as well).  The redraw of step 4 keeps the handle's
 * sigma, as cpmppi_sample does, which draws the first plans.
 * The call is stateless: nothing is registered on the handle.  Only the POINTER is fixed by a launch or a capture - the VALUES
 * are read when the kernel runs, so a caller may rewrite the array between launches and between replays (stream-ordered).
 * Otherwise the contract is cpmppi_rpgd_step's: count_dev, the workspace of cpmppi_rpgd_reserve under capture, the step counter.
 * Refused (CPMPPI_ERR_BAD_ARG, "cpmppi_rpgd_step_rows: ...", nothing launched, outputs untouched): everything cpmppi_rpgd_step
 * refuses, rows == NULL, a misaligned rows, n_rows < args->E, a handle whose cost plugin is not quadratic_boundary_grad_minimal,
 * and a handle with rows of cpmppi_set_tuning_rows registered (those are the MPPI step's). */
#define CPMPPI_RPGD_ROW_LR 7
#define CPMPPI_RPGD_ROW_GRADMAX_CLIP 8
int cpmppi_rpgd_step_rows(cpmppi_handle* h, const cpmppi_rpgd_args* args, const float* rows, uint32_t n_rows, void* stream);

/* Plain gradient step Q <- clip(Q - learning_rate * clip_by_norm(grad, gradmax_clip)) on Q[E,N,H] in place
 * (cem-naive-grad-tf, config_optimizers.yml:21-31). */
int cpmppi_sgd_step(cpmppi_handle* h, uint32_t E, float* Q, const float* grad, float learning_rate, float gradmax_clip,
                    void* stream);

/* CEM (hyper-parameters: Control_Toolkit_ASF/config_optimizers.yml:1-11, section cem-tf).
 * cpmppi_cem_sample: Q[E,N,H] = clip(mean[E,H] + stdev[E,H] * z), z ~ N(0,1) from Philox(seed, offset, env, rollout).
 * cpmppi_cem_update: per env, the best_k sequences by cost (stable ascending order) -> their mean and population
 * standard deviation per time-step, the latter floored at stdev_min; elite_idx_out[E,best_k] (may be NULL).  The order is
 * numpy's argsort(kind="stable"): -inf < finite < +inf < NaN, -0.0 equal to +0.0, equal costs (all NaNs among them) by
 * index; every elite index is < N whatever S holds - a NaN cost is taken only once best_k exceeds the number of others. */
int cpmppi_cem_sample(cpmppi_handle* h, uint32_t E, const float* mean, const float* stdev, uint64_t seed, uint64_t offset,
                      uint32_t env_offset, float* Q_out, void* stream);
int cpmppi_cem_update(cpmppi_handle* h, uint32_t E, const float* S, const float* Q, uint32_t best_k, float stdev_min,
                      float* mean_out, float* stdev_out, uint32_t* elite_idx_out, void* stream);
/* cem-gmm (config_optimizers.yml:12-20): Q[E,N,H] = clip(centres[E, c, :] + stdev[E,H] * z) with the component c of every
 * rollout uniform over the K centres (the elite sequences of the previous iteration); component_out[E,N] may be NULL. */
int cpmppi_cem_gmm_sample(cpmppi_handle* h, uint32_t E, const float* centres, uint32_t K, const float* stdev, uint64_t seed,
                          uint64_t offset, uint32_t env_offset, float* Q_out, uint32_t* component_out, void* stream);

/* The whole control step of cem-tf, cem-naive-grad-tf and cem-grad-bharadhwaj-tf for E envs in ONE call: no host
 * synchronisation, no allocation, and - with count_dev - no launch argument that changes between control steps, so a captured
 * graph of (step, plant) replays.  It is cpmppi_cem_sample, (the hybrids: cpmppi_rollout_cost_grad + cpmppi_sgd_step /
 * cpmppi_adam_step,) the cost and cpmppi_cem_update `iterations` times, then the shift, written out below.
 * `c` = control steps taken before this call: *count_dev if given, else 0.
 *   for i = 0 .. iterations-1, with the Philox offset o = offset + c * iterations + i:
 *   1. samples[env, n, :] = what cpmppi_cem_sample(mean, stdev, seed, o, env_offset) draws for rollout n.
 *   2. refine != NONE: cost gradient of every sample (cpmppi_rollout_cost_grad's arithmetic, previous_input and per-env pole
 *      masses included), then cpmppi_sgd_step's update (SGD) or cpmppi_adam_step's (ADAM: moments zero at the start of the call,
 *      t = i + 1, lr_t formed in double in the kernel).
 *   3. cost S of every (refined) sample: the adjoint kernel's forward sweep (sin / cos evaluated on every substep), i.e.
 *      cpmppi_rollout_cost_grad's S_out.
 *   4. mean, stdev = cpmppi_cem_update(S, samples, best_k, stdev_min): the same stable order (NaN last, ties by index), the
 *      same sums in the same order - bit for bit.
 *   then Q_out[env] = mean[env, 0], plan_out = mean; S_out, samples_out and order_out (the whole ranking, cheapest first; its
 *   first best_k entries are the elite) are the LAST iteration's; mean and stdev are shifted left by `shift`, the tail
 *   filled with mean_fill and stdev_fill; with count_dev: *count_dev += 1 after the step, stream-ordered.
 * Refused with CPMPPI_ERR_BAD_ARG: a legacy cost, quadratic_boundary / _nonconvex, PRECISE arithmetic, N > 256 (one workgroup per
 * env, one lane per sample), refining with S beyond the LDS sub-state buffer, best_k == 0 or > N, iterations == 0, shift > H,
 * an unknown refine kind, a NULL or misaligned required pointer, fewer registered pole-mass rows than E, and a stream under
 * capture while the workspace of cpmppi_cem_reserve is missing or too small (outside a capture the step allocates it itself).
 * cpmppi_cem_reserve(h, E, refine): the workspace for steps of up to E envs - H * E * ceil64(N) floats, ten times that when
 * refining (check-points, gradient, moments). */
typedef enum { CPMPPI_CEM_REFINE_NONE = 0, CPMPPI_CEM_REFINE_SGD = 1, CPMPPI_CEM_REFINE_ADAM = 2 } cpmppi_cem_refine;
typedef struct {
  uint32_t E;                       /* active envs in this call (cpmppi_cem_args) */
  const float* s0;                  /* [E,6] */
  const float* target_position;     /* [E] */
  const float* target_equilibrium;  /* [E] */
  const float* L;                   /* [E] pole length per env, or NULL = config.L_default */
  const float* previous_input;      /* [E] control applied before this step, or NULL = 0 */
  float* mean;                      /* [E,H] the sampling mean, updated in place */
  float* stdev;                     /* [E,H] the sampling stdev, updated in place */
  uint32_t iterations;              /* outer iterations in this step */
  uint32_t best_k;                  /* elite size, 0 < best_k <= N */
  float stdev_min;
  uint32_t refine;                  /* cpmppi_cem_refine */
  float learning_rate;
  float beta1;
  float beta2;
  float epsilon;
  float gradmax_clip;               /* <= 0: off */
  uint32_t shift;                   /* 0 .. H */
  float mean_fill;
  float stdev_fill;
  uint64_t seed;                    /* Philox key of the sampler */
  uint64_t offset;                  /* Philox offset of the first iteration (host mode), or of the first step's (device mode) */
  uint32_t env_offset;              /* global index of env 0 */
  uint64_t* count_dev;              /* control steps taken, in DEVICE memory (8-byte aligned), or NULL = host mode */
  float* Q_out;                     /* [E]   the control: mean[:, 0] before the shift */
  float* S_out;                     /* [E,N] costs of the last iteration, or NULL */
  float* plan_out;                  /* [E,H] the mean before the shift, or NULL */
  float* samples_out;               /* [E,N,H] the (refined) samples of the last iteration, or NULL */
  uint32_t* order_out;              /* [E,N] the last iteration's ranking (sample rows, cheapest first), or NULL */
} cpmppi_cem_args;
int cpmppi_cem_reserve(cpmppi_handle* h, uint32_t E, uint32_t refine);
int cpmppi_cem_step(cpmppi_handle* h, const cpmppi_cem_args* args, void* stream);

/* The whole control step of cem-tf over the NEURAL predictor (cpmppi_set_gru) for E envs in ONE call: cpmppi_cem_step with
 * cpmppi_rollout_cost_gru in the place of the ODE sweep, without the hybrids' refinement - no host synchronisation, no
 * allocation, and - with count_dev - no launch argument that changes between control steps.  It is cpmppi_cem_sample,
 * cpmppi_rollout_cost_gru and cpmppi_cem_update `iterations` times, then the shift, bit for bit:
 * `c` = control steps taken before this call: *count_dev if given, else 0.
 *   for i = 0 .. iterations-1, with the Philox offset o = offset + c * iterations + i:
 *   1. samples[env, n, :] = what cpmppi_cem_sample(mean, stdev, seed, o, env_offset) draws for rollout n.
 *   2. S = cpmppi_rollout_cost_gru(s0, samples, target_position, target_equilibrium, h0): every rollout of an env from the
 *      env's memory h0[env] (NULL: zeros), in the handle's math mode (FAST: split f16, PRECISE: exact f32), control_mode applied.
 *   3. mean, stdev = cpmppi_cem_update(S, samples, best_k, stdev_min): the same stable order (NaN last, ties by index), the
 *      same sums in the same order.
 *   then Q_out[env] = mean[env, 0], plan_out = mean; S_out, samples_out and order_out (the whole ranking, cheapest first; its
 *   first best_k entries are the elite) are the LAST iteration's; mean and stdev are shifted left by `shift`, the tail
 *   filled with mean_fill and stdev_fill; with count_dev: *count_dev += 1 after the step, stream-ordered.
 * h0 is read, not written: the memory is handed on by cpmppi_gru_advance, so the closed loop is cpmppi_cem_step_gru,
 * cpmppi_gru_advance(s0, Q_out, h0), cpmppi_plant_step - three calls whose arguments never change.  Reads no pole mass and no L.
 * One workgroup per env, a pair of lanes per sample (at most 8 waves); the workspace is cpmppi_cem_reserve(h, E,
 * CPMPPI_CEM_REFINE_NONE)'s - on a handle with a model that call accepts both math modes.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned (cpmppi_last_error: "cpmppi_cem_step_gru: ...") for: per-env tuning
 * rows registered, no model set, E == 0 or E > config.E, a NULL s0, target_position, target_equilibrium, mean, stdev or Q_out, a
 * cost other than quadratic_boundary_grad_minimal and default, a misaligned pointer, iterations == 0, best_k == 0 or > N,
 * shift > H, N > 256, and a stream under capture while the workspace of cpmppi_cem_reserve is missing or too small (outside a
 * capture the step allocates it itself). */
typedef struct {
  uint32_t E;                       /* active envs in this call (cpmppi_cem_gru_args) */
  const float* s0;                  /* [E,6] */
  const float* target_position;     /* [E] */
  const float* target_equilibrium;  /* [E] */
  const float* h0;                  /* [E,2,32] the network's memory per env, or NULL = zeros; read, not written */
  float* mean;                      /* [E,H] the sampling mean, updated in place */
  float* stdev;                     /* [E,H] the sampling stdev, updated in place */
  uint32_t iterations;              /* outer iterations in this step */
  uint32_t best_k;                  /* elite size, 0 < best_k <= N */
  float stdev_min;
  uint32_t shift;                   /* 0 .. H */
  float mean_fill;
  float stdev_fill;
  uint64_t seed;                    /* Philox key of the sampler */
  uint64_t offset;                  /* Philox offset of the first iteration (host mode), or of the first step's (device mode) */
  uint32_t env_offset;              /* global index of env 0 */
  uint64_t* count_dev;              /* control steps taken, in DEVICE memory (8-byte aligned), or NULL = host mode */
  float* Q_out;                     /* [E]   the control: mean[:, 0] before the shift */
  float* S_out;                     /* [E,N] costs of the last iteration, or NULL */
  float* plan_out;                  /* [E,H] the mean before the shift, or NULL */
  float* samples_out;               /* [E,N,H] the samples of the last iteration, or NULL */
  uint32_t* order_out;              /* [E,N] the last iteration's ranking (sample rows, cheapest first), or NULL */
} cpmppi_cem_gru_args;
int cpmppi_cem_step_gru(cpmppi_handle* h, const cpmppi_cem_gru_args* args, void* stream);

/* The whole rpgd / gradient-tf control step over the NEURAL predictor (cpmppi_set_gru) for E envs in ONE call: cpmppi_rpgd_step
 * with the network in the place of the ODE - no host synchronisation, no allocation, and - with count_dev - no launch argument
 * that changes between control steps, so a captured graph of (step, cpmppi_gru_advance, plant) replays.  It is
 * cpmppi_rollout_cost_grad_gru + cpmppi_adam_step `iterations` times, cpmppi_rollout_cost_gru, the choice of the best plan, the
 * resampling of rpgd and the shift.  `c` = control steps taken before this call: *count_dev if given, else count.
 *   1. for i = 1..iterations: cost gradient of every plan - the forward sweep in the handle's math mode (FAST: split f16,
 *      PRECISE: exact f32) from the env's memory h0[env] (NULL: zeros), the check-points parked as cpmppi_rollout_cost_grad_gru parks
 *      them, then its exact-f32 reverse sweep - and cpmppi_adam_step's update with t = a + i, a = adam_iteration (host mode) or
 *      c * iterations (device mode); lr_t is formed in double in the kernel, as cpmppi_rpgd_step forms it.
 *   2. final cost S of every plan: cpmppi_rollout_cost_gru's rollout.
 *   3. - 6. the ranking, Q_out / plan_out / S_out / order_out, the resampling, the shift and the step counter: steps 3 to 6 of
 *      cpmppi_rpgd_step, word for word.
 * Every quantity equals the composition of those entry points bit for bit, except that lr_t carries the powers of beta from
 * iteration to iteration where cpmppi_adam_step calls pow() (the statement cpmppi_rpgd_step has as well).
 * h0 is read, not written: the memory is handed on by cpmppi_gru_advance, so the closed loop is cpmppi_rpgd_step_gru,
 * cpmppi_gru_advance(s0, Q_out, h0), cpmppi_plant_step - three calls whose arguments never change.  Reads no pole mass, no L and no
 * previous input (neither cost of the GRU kernels has a term in it).
 * One workgroup per env (gru_rpgd_step_kernel), plan n on a pair of lanes of wave n / 32, one wave per 32 plans; the reverse sweep
 * needs one wave per SIMD, so N <= 128.  Workspace: cpmppi_rpgd_gru_reserve(h, E) - the check-points of
 * cpmppi_rollout_cost_grad_gru (the same buffer: H * 72 * cfg.E * cfg.N floats) and behind them the gradient, H * cfg.E * cfg.N
 * floats; E is checked, the size is that of the handle's largest launch.
 * Nothing is launched and CPMPPI_ERR_BAD_ARG is returned (cpmppi_last_error: "cpmppi_rpgd_step_gru: ...") for: per-env tuning
 * rows registered, no model set, E == 0 or E > config.E, a NULL s0, target_position, target_equilibrium, Q, m, v or Q_out, a cost
 * other than quadratic_boundary_grad_minimal and default, a misaligned pointer (count_dev: 8 bytes), iterations == 0, keep_k == 0
 * or > N, shift > H, an unknown distribution, N > 128, and a stream under capture while the workspace of cpmppi_rpgd_gru_reserve
 * is missing or too small (outside a capture the step allocates it itself).  cpmppi_rpgd_gru_reserve refuses a handle without a
 * model, E out of range, such a cost and N > 128 in the same words under its own name.
 * The block is cpmppi_rpgd_args without L and previous_input, with h0 in their place. */
typedef struct {
  uint32_t E;                       /* active envs in this call (cpmppi_rpgd_gru_args) */
  const float* s0;                  /* [E,6] */
  const float* target_position;     /* [E] */
  const float* target_equilibrium;  /* [E] */
  const float* h0;                  /* [E,2,32] the network's memory per env, or NULL = zeros; read, not written */
  float* Q;                         /* [E,N,H] the plans, updated in place */
  float* m;                         /* [E,N,H] Adam first moments, updated in place */
  float* v;                         /* [E,N,H] Adam second moments, updated in place */
  uint32_t iterations;              /* Adam iterations in this step */
  uint32_t adam_iteration;          /* Adam iterations taken before this call (host mode) */
  float learning_rate;
  float beta1;
  float beta2;
  float epsilon;
  float gradmax_clip;               /* <= 0: off */
  uint32_t keep_k;                  /* keep_k == N or resamp_per == 0: never resample */
  uint32_t resamp_per;
  uint32_t shift;                   /* 0 .. H */
  uint32_t distribution;            /* cpmppi_rpgd_distribution */
  float sample_mean;
  float uniform_lo;
  float uniform_hi;
  uint64_t seed;                    /* Philox key of the redraw */
  uint64_t draw_offset;             /* Philox offset of the redraw (host mode), or of the first redraw (device mode) */
  uint32_t env_offset;              /* global index of env 0 */
  uint64_t count;                   /* control steps taken before this call (host mode) */
  uint64_t* count_dev;              /* the same counter in DEVICE memory (8-byte aligned), or NULL = host mode */
  float* Q_out;                     /* [E]   the chosen control */
  float* S_out;                     /* [E,N] final costs, indexed by the plan rows as they are BEFORE the resampling, or NULL */
  float* plan_out;                  /* [E,H] the best plan before the shift, or NULL */
  uint32_t* order_out;              /* [E,N] the ranking (plan rows, cheapest first), or NULL */
} cpmppi_rpgd_gru_args;
int cpmppi_rpgd_gru_reserve(cpmppi_handle* h, uint32_t E);
int cpmppi_rpgd_step_gru(cpmppi_handle* h, const cpmppi_rpgd_gru_args* args, void* stream);

/* a16 alone: S[E,N], delta_u[E,N,H] -> weighted average [E,H] (controller_mppi_cartpole.py:306-321). */
int cpmppi_reward_weighted_average(cpmppi_handle* h, uint32_t E, const float* S, const float* delta_u, float* out,
                                   void* stream);

/* Plant (the CALLER of the hot path; SURVEY.md §8b harness row / §8f N1): advance E simulated cartpoles by
 * n_substeps simulation steps of dt_sim under the held controls Q[E] — Euler-Cromer + edge bounce + cos/sin + wrap as
 * CartPole/__init__.py:283-324 (cartpole_equations.py:367-378, :341-347).  s[E,6] is updated in place. */
int cpmppi_plant_advance(cpmppi_handle* h, uint32_t E, float* s, const float* Q, const float* L, uint32_t n_substeps,
                         float dt_sim, void* stream);

/* The same advance with the closed loop's recording in the same launch (the experiment loop of
 * CartPole/__init__.py:659-735 appends one row per control period): Q_log[row][E] = Q and states_log[row + 1][E][6] =
 * the advanced state; either log may be NULL.  row = the control-step index, or, when row_dev is given, *row_dev - 1:
 * the device step counter of cpmppi_step_args.offset_dev, which the preceding cpmppi_step has already advanced (a
 * captured graph of control steps then replays without any changing launch argument).  log_rows = the number of
 * control periods the logs hold (Q_log[log_rows][E], states_log[log_rows + 1][E][6]): a host `row` >= log_rows is
 * CPMPPI_ERR_BAD_ARG; a device counter that is still 0 or points past the logs advances the plant WITHOUT recording
 * (a graph replayed beyond the recording's end never writes outside the buffers). */
int cpmppi_plant_advance_record(cpmppi_handle* h, uint32_t E, float* s, const float* Q, const float* L, uint32_t n_substeps,
                                float dt_sim, float* states_log, float* Q_log, uint64_t log_rows, uint64_t row,
                                const void* row_dev, void* stream);

/* The plant with the reference's EXPERIMENT SCHEDULE: what CartPole.update_state does around the controller on
 * every SIMULATION step (CartPole/__init__.py:283-324) - update_parameters (:529-537: the pole length may change in time),
 * update_target_position (:360-378: target_position = random_track_f(time)), update_target_equilibrium (:380-388: flips after
 * keep_target_equilibrium_x_seconds_up / _down), integration + bounce + wrap, the controller every dt_control (Update_Q :475-527),
 * the second derivatives, save_csv_routine every dt_save (:403-433).  The schedule is a function of TIME only, so the host
 * tabulates it once per experiment (cartpolesimulation_amd/schedule.py) and the device loop indexes the tables with its own step
 * counter: a captured graph of control periods still replays without a changing launch argument.
 *   simulation step g = 0 is the initial state; control period c advances steps c*period_steps + 1 .. (c + 1)*period_steps;
 *   table row of step g = min(g / sched_stride, sched_rows - 1): the value the simulator holds AFTER step g's updates.
 * One call = one control period, ONE kernel:
 *   1. held control q = Q[env]; Q_log[c][E] = q (c < ctrl_rows); with a Q_disturbance_table the plant is driven by
 *      q_applied = (q + Q_disturbance_table[c][env]) + Q_bias instead (add_control_noise after Update_Q, :523-524)
 *   2. second derivatives of (s, q) with the pole length of step c*period_steps; dd_log[r][E][2] = (angleDD, positionDD) if that
 *      step is a saved one (r = step / save_every < save_rows) - the row whose state the PREVIOUS period stored, completed with
 *      the control computed from it (save_csv_routine runs after Update_Q, :316-324)
 *   3. n_substeps x { pole length and pole mass of the step (L_table, else L / config.L_default; m_pole_table, else m_pole /
 *      config.m_pole: update_parameters, :529-537); Euler-Cromer + edge bounce + cos / sin + wrap;
 *      second derivatives; if step % save_every == 0: states_log[step / save_every][E][6] = state, and dd_log unless the step ends
 *      the period }
 *   4. *_out[E] = row ((c + 1)*period_steps) of the tables: what the NEXT controller call is handed (updated_attributes
 *      target_position / target_equilibrium / L, :509-520) - point cpmppi_step_args.target_position / target_equilibrium / L there.
 * n_substeps = 0 records only (1. and 2.: the run's last controller call is followed by no plant step, :690-716).
 * period_dev: c = *period_dev - 1, the device step counter of cpmppi_step_args.offset_dev (already advanced by the step); a
 * counter that is still 0 advances the plant from table row 0 WITHOUT recording or publishing: the state is that of a host-named
 * period 0 without a disturbance row, and Q_log, states_log, dd_log, state_history, the three *_out and s_measured are left as they
 * are.  Q_applied_out is written all the same (= Q): it is no schedule value but the control this launch drove the plant by, which
 * is what the next controller call is to be handed whatever the counter said (Q_ccrc = Q_applied, CartPole/__init__.py:493).
 * A counter past the recording (c >= ctrl_rows, saved rows >= save_rows) advances the plant with the tables' LAST row and adds no
 * disturbance or noise row; it writes no log, and still keeps the ring, publishes the *_out (the last row) and s_measured, and
 * writes Q_applied_out = Q: a graph replayed beyond the recording's end never reads or writes outside the buffers.  Any log /
 * table / out pointer may be NULL.  The pole MASS the controller computes with is
 * the handle's (config.m_pole / cpmppi_set_pole_mass, or per env cpmppi_set_pole_mass_rows), whatever the plant's: this call neither
 * reads nor publishes it (the caller copies the row of its own controller-mass table into the registered array between periods). */
typedef struct {
  uint32_t E;
  float* s;                             /* [E,6] in / out */
  const float* Q;                       /* [E] held controls */
  const float* L;                       /* [E] pole length when there is no L_table; NULL = config.L_default */
  uint32_t n_substeps;                  /* simulation steps to advance now: period_steps (fewer: a run's trailing partial period), or 0 (record only) */
  uint32_t period_steps;                /* simulation steps per control period (dt_control / dt_sim); 0 = n_substeps */
  float dt_sim;
  uint64_t period;                      /* c */
  const void* period_dev;               /* or NULL */
  float* states_log;                    /* [save_rows][E][6]; row 0 is the caller's (the initial state) */
  float* dd_log;                        /* [save_rows][E][2] */
  uint64_t save_rows;
  uint32_t save_every;                  /* simulation steps per saved row (dt_save / dt_sim); 0 = period_steps */
  float* Q_log;                         /* [ctrl_rows][E] */
  uint64_t ctrl_rows;
  const float* target_position_table;   /* [sched_rows][E] */
  const float* target_equilibrium_table;/* [sched_rows][E] */
  const float* L_table;                 /* [sched_rows][E] */
  uint64_t sched_rows;
  uint32_t sched_stride;                /* simulation steps per table row; 0 = 1 */
  float* target_position_out;           /* [E] */
  float* target_equilibrium_out;        /* [E] */
  float* L_out;                         /* [E] */
  uint32_t row_envs;                    /* envs per ROW of the logs and tables (0 = E): an env group that works on a slice of a larger
                                           batch's buffers passes the batch's env count and pointers to its first env (cpmppi_groups_run) */
  const float* m_pole;                  /* [E] the PLANT's pole mass when there is no m_pole_table; NULL = config.m_pole */
  const float* m_pole_table;            /* [sched_rows][E] a pole mass that changes in time, like L_table (the `m_pole:` updater) */
  const float* L_controller_table;      /* [sched_rows][E] what L_out publishes instead of L_table: the pole length the CONTROLLER is
                                           told (inform_controller_about_parameters_change, CartPole/controller_informer.py: the true
                                           value or the initial one); NULL = L_table */
  const float* Q_disturbance_table;     /* [ctrl_rows][E] the simulator's additive control disturbance (CartPole/noise_control_signal.py:
                                           14-16): the plant of period c is driven by Q_applied = (Q + table[c]) + Q_bias in float32,
                                           table = controlDisturbance * N(0,1) drawn on the host; Q_log keeps the CALCULATED control.
                                           NULL = none.  Needs ctrl_rows > 0 */
  float Q_bias;                         /* controlBias */
  float* Q_applied_out;                 /* [E] the control the plant was driven by this period: what the simulator hands the NEXT controller
                                           call as Q_ccrc / "Q_applied_-1" (CartPole/__init__.py:489, 517-518) - point
                                           cpmppi_step_args.previous_input there for the costs that read it; NULL = not needed */
  /* The measurement chain between plant and controller (CartPole.add_noise_and_latency, CartPole/__init__.py:336-356; latency 0,
   * noise OFF, offset 0 as shipped): with s_measured given, a period that is followed by a controller call ends with
   *   delayed  = state(g - latency_steps) + latency_frac * (state(g - latency_steps - 1) - state(g - latency_steps))   (float64;
   *              before the first step: zeros with cos = 1, CartPole/latency_adder.py:24-26, 63-67)
   *   noise      (measurement_noise_table row c + 1: angle += n0, wrap, cos / sin, position += n1, angleD += n2, positionD += n3)
   *   offset     angle = wrap(angle + angle_offset), cos / sin (:348-356); informed (informed_table, NULL = yes): taken out again
   *              with another wrap + cos / sin (:501-505)
   * and s_measured[E][6] = that state in float32 - point cpmppi_step_args.s0 there (the caller puts the initial state in before
   * the t = 0 call, which sees the true state, :869-870). */
  float* s_measured;                    /* [E][6] out; NULL = no measurement chain */
  float* state_history;                 /* [history_len][row_envs][6] ring: the state after simulation step g at slot g % history_len; the
                                           caller fills it with zeros and cos = 1 before the run.  Needed when latency > 0 */
  uint32_t history_len;                 /* >= latency_steps + 2 */
  uint32_t latency_steps;               /* int(latency / dt_sim) */
  double latency_frac;                  /* latency / dt_sim - latency_steps */
  const float* measurement_noise_table; /* [ctrl_rows][row_envs][4] sigma * N(0,1) for angle, position, angleD, positionD, or NULL */
  const double* angle_offset_table;     /* [sched_rows][row_envs] the vertical angle offset after the table row's step, or NULL = 0 */
  const uint8_t* informed_table;        /* [sched_rows][row_envs] 1 = the controller is informed (the offset is taken out), NULL = 1 */
} cpmppi_plant_args;
int cpmppi_plant_step(cpmppi_handle* h, const cpmppi_plant_args* args, void* stream);

/* Multi-GPU (no reference counterpart - its only fan-out is share-nothing SLURM job arrays,
 * others/EulerClusterScripts/ParallelDataGeneration.sh:2-17): one process per GPU, each owning a contiguous block of
 * envs, and ONE all-gather of the chosen control sequences per step over RCCL / xGMI, enqueued from C on a high-priority
 * side stream so that it runs under the NEXT step's rollout kernel:
 *   cpmppi_comm_unique_id  rank 0: the 128-byte RCCL id every rank needs (distribute it by any means - a
 *                          torch.distributed store, MPI, a file); rccl_path may be NULL (the RCCL already in the process,
 *                          else librccl.so by name)
 *   cpmppi_comm_init       collective over all ranks: creates the handle's communicator, side stream and events
 *   cpmppi_comm_gather     after step i on `stream`: recv_all[world][count] <- all-gather of send[count] on the side stream,
 *                          ordered after everything enqueued on `stream` so far; `stream` itself does not wait.  slot <
 *                          CPMPPI_COMM_SLOTS names the completion event of this gather
 *   cpmppi_comm_wait       `stream` waits (on the device) for the gather of `slot` - call it before the step that overwrites
 *                          that gather's send buffer (with the two u_nom buffers of cpmppi_step_args.u_nom_out: two steps later)
 *                          or before reading recv_all on `stream`
 *   cpmppi_comm_sync       host wait for every gather enqueued so far; reports (once) and clears a device-side timeout
 *   cpmppi_comm_set_timeout  how long a device-side wait of cpmppi_step_gather may last, in seconds (default 10; <= 0: for
 *                          ever): the finalize of a step that is about to overwrite a buffer an all-gather still reads
 *                          waits for that gather, which completes only when EVERY rank has joined it
 *   cpmppi_comm_get_info   what the communicator IS, as RCCL itself reports it (ncclCommCount / ncclCommUserRank), next to what
 *                          cpmppi_comm_init was told: a bench line can then state how many ranks the collective really spanned
 * The side stream's wait for a published step is a one-lane kernel of the library's with the same timeout (the default form); the
 * stream-memory-operation form of rounds 4-5 (environment: CPMPPI_COMM_WAITER=stream-ops; hipStreamWaitValue32 has no timeout of its
 * own) is covered by cpmppi_comm_sync and cpmppi_comm_destroy, which poll the side stream for at most the timeout and then release
 * the wait from the host, raise the error and return CPMPPI_ERR_COMM.  Either way a rollout launch that never published - failed,
 * aborted - cannot wedge them.  cpmppi_step_gather refuses a stream that is being captured.
 * PEERS: a rank whose device-side wait timed out keeps its buffers intact and its already-enqueued all-gathers still run, so the
 * other ranks receive a well-formed but STALE block from it and no error of their own.  Two ways to know:
 *   - cpmppi_comm_set_stamped(h, 1) (before the first cpmppi_step_gather, the same on every rank): every gathered block carries
 *     CPMPPI_GATHER_STAMP_FLOATS trailing words - the u_nom / u_nom_out buffers handed to cpmppi_step_gather are then
 *     [E*H + CPMPPI_GATHER_STAMP_FLOATS] floats (the caller zeroes the trailing words once), recv_all is
 *     [world][E*H + CPMPPI_GATHER_STAMP_FLOATS].  Word 0 of the trailer (read as uint32_t) is the STAMP: the number of the
 *     cpmppi_step_gather call (1, 2, ... per communicator; the same on every rank, collectives being called in the same order) that
 *     produced the block, written on the side stream between the step's publication and its all-gather - unless a device-side
 *     wait of the communicator has given up: a rank that dropped a step (timeout) leaves buffer AND stamp as they were, and stamps
 *     nothing until cpmppi_comm_sync has cleared the condition.  A receiver accepts block r of the n-th gather iff its stamp == n
 *     and otherwise keeps what it had for rank r (it may so discard a good block that was gathered while the error was up - never
 *     accept a stale one).  No extra collective, nothing on the launch stream; words 1.. of the trailer are reserved (0).
 *   - or treat gathered blocks as unverified until cpmppi_comm_sync has returned CPMPPI_OK on EVERY rank (exchange the return
 *     codes with the collective of your choice).
 * Errors: CPMPPI_ERR_COMM.  RCCL is bound at run time: the library loads without it.  rccl_path, when given, is loaded as given
 * and wins over an RCCL the process already holds (a site-specific build; the two-process test double of tests/fake_rccl). */
typedef struct {
  uint32_t world, rank;            /* as given to cpmppi_comm_init */
  int32_t rccl_ranks, rccl_rank;   /* ncclCommCount / ncclCommUserRank of the communicator; -1 = this RCCL does not export them */
  int32_t rccl_version;            /* ncclGetVersion (e.g. 22606), 0 = unknown */
  uint32_t stream_memory_ops;      /* 0 = the one-lane waiter kernel orders the side stream (default), 1 = hipStreamWaitValue32 / WriteValue32 */
  uint32_t gathers_enqueued;       /* cpmppi_step_gather calls so far (= the stamp of the most recent one) */
  uint32_t stamped;                /* cpmppi_comm_set_stamped */
} cpmppi_comm_info;
#define CPMPPI_COMM_ID_BYTES 128
#define CPMPPI_COMM_SLOTS 4
#define CPMPPI_GATHER_STAMP_FLOATS 4   /* 16 bytes: every rank's block in recv_all stays 16-byte aligned */
int cpmppi_comm_unique_id(void* id_out, const char* rccl_path);
int cpmppi_comm_init(cpmppi_handle* h, const void* id, int world, int rank, const char* rccl_path);
int cpmppi_comm_gather(cpmppi_handle* h, uint32_t slot, const float* send, float* recv_all, size_t count, void* stream);
int cpmppi_comm_wait(cpmppi_handle* h, uint32_t slot, void* stream);
int cpmppi_comm_sync(cpmppi_handle* h);
int cpmppi_comm_set_timeout(cpmppi_handle* h, double seconds);
int cpmppi_comm_destroy(cpmppi_handle* h);
int cpmppi_comm_get_info(cpmppi_handle* h, cpmppi_comm_info* out);
int cpmppi_comm_set_stamped(cpmppi_handle* h, int on);

/* cpmppi_step + the all-gather of its result in ONE call - the production form of the per-step collective:
 * recv_all[world][E*H] <- all-gather of the nominal sequences this step writes (args->u_nom_out, or args->u_nom when the
 * step runs in place).  The launch stream receives the rollout kernel and nothing else; step and gather are ordered
 * through device memory (the kernel's finalizing blocks publish the step number, a one-lane kernel on the side stream waits
 * for it - hipStreamWaitValue32 on signal memory with CPMPPI_COMM_WAITER=stream-ops; the finalize of a
 * later step that overwrites a buffer still being gathered waits for that gather).  Use two
 * u_nom buffers alternately (step i: u_nom = B[i & 1], u_nom_out = B[(i + 1) & 1]) so that the gather of step i runs
 * under step i + 1; in place is correct too, but then step i + 1's finalize waits for gather i.  recv_all must stay
 * untouched until cpmppi_comm_sync (host) returns or a later cpmppi_comm_gather/wait pair orders the reader.
 * A launch of more than 512 envs performs that wait once, with one lane, in FRONT of the kernel too (a one-lane kernel on `stream`,
 * ~5 us): thousands of finalizing blocks spinning for a late gather would hold every workgroup slot of the device (two ranks sharing
 * one device deadlocked on that until the timeout) - so with many envs and in place the step no longer overlaps the previous gather:
 * alternate two buffers.
 * A device-side wait that outlasts cpmppi_comm_set_timeout does NOT proceed: the step drops its result (the buffer being
 * gathered is not overwritten), so does every later step of the handle, and the next cpmppi_step_gather - or
 * cpmppi_comm_sync, which also clears the condition - returns CPMPPI_ERR_COMM. */
int cpmppi_step_gather(cpmppi_handle* h, const cpmppi_step_args* args, float* recv_all, void* stream);

/* Recording writer (HOST pointers, no GPU involved): E experiment recordings in the reference's CSV layout
 * (CartPole/csv_logger.py:10-58,125-159; column set and order CartPole/__init__.py:221-259), byte for byte what the reference's
 * csv.writer produces from the values its simulator logs - pinned to a recording written by the reference itself
 * (tests/golden/schedule.npz "csv_rows"): every column in the representation of the TYPE the reference holds it in -
 *   time, Q_calculated, target_position, L, m_pole, the vertical-angle-offset columns: Python floats -> repr(float) of the double
 *   the state, angleDD / positionDD, Q_applied, Q_ccrc, u: numpy float32 scalars -> str(numpy.float32), shortest float32 digits
 *   target_equilibrium: an int; L_for_controller / m_pole_for_controller: the controller informer's 'true' / 'default'
 *   Q_update_time: empty until the first controller update inside the loop, then `q_update_time` (the reference logs the wall
 *   clock of its controller call there: not reproducible by construction)
 * rows end with "\r\n".  One thread per file.
 *   paths[E]      one file per experiment; a path that already exists is an error (CPMPPI_ERR_IO) - the caller makes the names
 *                 unique (csv_logger.py:61-91) and nothing is ever appended to or overwritten.  Files are written under a
 *                 temporary name and renamed when complete; on any failure the files of THIS call are removed again.
 *   preamble      the comment block and the column-name row as ready-made bytes, the same for every file
 *   n_threads     0 = one per hardware thread (at most 32) */
typedef struct {
  uint32_t E, rows;
  const double* time;                   /* [rows] */
  const float* states;                  /* [rows][E][6] */
  const float* dd;                      /* [rows][E][2] angleDD, positionDD */
  const float* Q;                       /* [rows][E] the control in force when the row was saved (Q_calculated = Q_applied) */
  const float* Q_ccrc;                  /* [rows][E] the control before it */
  const double* target_position;        /* [rows][E] */
  const int32_t* target_equilibrium;    /* [rows][E] */
  const float* L;                       /* [rows][E] */
  double m_pole;
  float u_max;                          /* u = u_max * Q in float32 (CartPole/cartpole_equations.py:119-127) */
  uint32_t first_update_row;            /* rows before it have an empty Q_update_time */
  double q_update_time;
  const float* m_pole_rows;             /* [rows][E] a pole mass that changed during the run (the float32 values the simulator held), or
                                           NULL: `m_pole` in every row */
  const uint8_t* informed;              /* [rows][E] L_for_controller / m_pole_for_controller: 1 = 'true', 0 = 'default' (the controller
                                           informer's state when the row was saved); NULL = 'true' in every row (mode ON, as shipped) */
  const float* Q_applied;               /* [rows][E] the control the plant was driven by when it differs from the calculated one (control
                                           disturbance): the Q_applied and u columns; NULL = Q */
  const double* angle_offset;           /* [rows][E][3] the vertical angle offset, its cos and its sin when the row was saved, or NULL:
                                           0.0, 1.0, 0.0 in every row */
} cpmppi_recording;
int cpmppi_write_recordings(const char* const* paths, const char* preamble, size_t preamble_len, const cpmppi_recording* rec,
                            int n_threads);

/* A HIP stream with a hardware queue OF ITS OWN (hipExtStreamCreateWithCUMask with every CU enabled): the runtime multiplexes
 * ordinary streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and two streams that land on the same
 * queue run their kernels one after the other - which defeats env groups that are meant to run side by side
 * (cartpolesimulation_amd/pipeline.py; measured: two groups of C3 on pooled streams 327 us per step, serialised, against 175 us).
 * The returned hipStream_t is an ordinary stream for every other purpose; destroy it with cpmppi_stream_destroy. */
int cpmppi_stream_create(int device, void** stream_out);
int cpmppi_stream_destroy(void* stream);

/* ENV GROUPS: the E envs of one device as `groups` contiguous groups, each with a handle and a dedicated-queue stream of its own,
 * every group running its OWN chain of launches - independent MPPI problem instances need not march in step (a launch of a few
 * dozen envs ends with its slowest wave, waves differ by 20-40 %; measured on MI355X: 64 envs x 2048 x 50 74.5 -> 63.8 us per
 * step of all envs with two groups, 64 x 4096 x 100 224.6 -> 177.1 us).  No reference counterpart beyond its share-nothing job arrays
 * (others/EulerClusterScripts/ParallelDataGeneration.sh:2-17).  Philox keys are GLOBAL env indices (env_offset + env): a result
 * does not depend on the split (bit-identical to the unsplit launch whenever both pick the same lane mapping).
 *   cpmppi_groups_create   cfg->E = all envs of the device; env_offset = global index of env 0 (rank * E when sharded over GPUs)
 *   cpmppi_groups_slice / _handle / _stream   a group's envs [first, first + n), its handle (cost weights, GRU model, ... are set
 *                          per handle) and its hipStream_t
 *   cpmppi_groups_fork     every group stream waits for what `stream` has enqueued so far (uploads, allocations)
 *   cpmppi_groups_join     `stream` waits for every group
 *   cpmppi_groups_run      `periods` control periods of EVERY group enqueued from C, round robin (period k, group g: cpmppi_step
 *                          with the Philox step counter step->offset + k, then - if `plant` is given - cpmppi_plant_step with period
 *                          plant->period + k).  `step` and `plant` describe the FULL [E, ...] arrays exactly as for one handle over
 *                          all envs; every group works on its slice of them in place (plant->row_envs is filled in).  No group waits
 *                          for another.  step->offset_dev / plant->period_dev (one shared device counter) are refused.
 *   cpmppi_groups_comm_init   the env groups of a device under ONE communicator and ONE side stream (collective over all ranks, as
 *                          cpmppi_comm_init).  The communicator lives in group 0's handle: cpmppi_comm_set_timeout / _set_stamped /
 *                          _sync / _get_info / _destroy take cpmppi_groups_handle(g, 0)
 *   cpmppi_groups_run_gather  cpmppi_groups_run + the per-step all-gather of cpmppi_step_gather: per period ONE all-gather of the
 *                          device's whole u_nom[E, H] (recv_all[world][E*H], + the stamp words when stamped) on the side stream.  The
 *                          finalizing blocks of ALL groups count themselves on the communicator's shared arrival counter
 *                          (alternating with the step's parity: the groups drift by at most one step), the last env of the last
 *                          group publishes the step, and a group's finalize that is about to overwrite sequences a gather still
 *                          reads waits for it - exactly the single-handle protocol, with `envs` = all envs of the device.  With
 *                          step->u_nom_out given, the two buffers alternate per period of the call (period 0 reads u_nom and writes
 *                          u_nom_out, period 1 the other way round, ...); NULL = in place.  recv_all holds the LAST period's gather
 *                          once cpmppi_comm_sync(cpmppi_groups_handle(g, 0)) has returned.
 *                          Failures: (a) what the argument blocks can be checked for without a launch - every group's step and plant
 *                          arguments, the plant period of the call's LAST period against ctrl_rows - is checked before the first
 *                          launch: CPMPPI_ERR_BAD_ARG / _ALIGN with nothing enqueued and the communicator untouched.  (b) A failure in
 *                          period k before any step launch of that period is out (group 0's guard or step call) returns its code;
 *                          periods 0..k-1 are enqueued complete and gathered, the communicator stays usable.  (c) A failure once a step
 *                          launch of period k is out (any later call of that period) returns its code and POISONS the communicator:
 *                          periods 0..k-1 still run, stamp and gather as usual, period k is not gathered, the next
 *                          cpmppi_groups_run_gather returns CPMPPI_ERR_COMM, and cpmppi_comm_sync returns CPMPPI_ERR_COMM once,
 *                          after resetting the arrival counters and published step numbers that period left behind.  Some groups
 *                          may have run period k: prepare the buffers again before going on.  (d) A device-side wait that times out
 *                          drops the store of its step and of every later step of either parity, as for cpmppi_step_gather.
 * Errors as for the single-handle calls; text in cpmppi_groups_last_error. */
typedef struct cpmppi_groups cpmppi_groups;
int cpmppi_groups_create(const cpmppi_config* cfg, int device, uint32_t groups, uint32_t env_offset, cpmppi_groups** out);
void cpmppi_groups_destroy(cpmppi_groups* g);
uint32_t cpmppi_groups_count(const cpmppi_groups* g);
int cpmppi_groups_slice(const cpmppi_groups* g, uint32_t group, uint32_t* first_env, uint32_t* n_envs);
cpmppi_handle* cpmppi_groups_handle(cpmppi_groups* g, uint32_t group);
void* cpmppi_groups_stream(cpmppi_groups* g, uint32_t group);
int cpmppi_groups_fork(cpmppi_groups* g, void* stream);
int cpmppi_groups_join(cpmppi_groups* g, void* stream);
int cpmppi_groups_run(cpmppi_groups* g, const cpmppi_step_args* step, const cpmppi_plant_args* plant, uint32_t periods);
int cpmppi_groups_comm_init(cpmppi_groups* g, const void* id, int world, int rank, const char* rccl_path);
int cpmppi_groups_run_gather(cpmppi_groups* g, const cpmppi_step_args* step, const cpmppi_plant_args* plant, uint32_t periods,
                             float* recv_all);
const char* cpmppi_groups_last_error(const cpmppi_groups* g);

/* The ABI version this library was BUILT as (CPMPPI_ABI_VERSION of its header): lets a client that was compiled against another
 * header notice before it passes a struct of the wrong layout (cpmppi_create refuses a mismatching cpmppi_config.abi_version). */
uint32_t cpmppi_abi_version(void);

/* Build info, e.g. "cpmppi 1 gfx950 hip-7.2". */
const char* cpmppi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CPMPPI_H */
