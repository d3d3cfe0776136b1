// cpmppi_plant.hip — the simulated plant.   Contract: include/cpmppi.h, cpmppi_plant_args.
//
// Kernel inventory
//   plant_kernel                          one control period of every simulated cartpole, with the experiment schedule, the
//                                         rows saved in the period and the measurement chain (one env per lane).
// Entry points: cpmppi_plant_step, cpmppi_plant_advance, cpmppi_plant_advance_record; check_plant (also cpmppi_groups_run).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>

#include "cpmppi.h"
#include "cpmppi_internal.hpp"
#include "cpmppi_ode.hpp"

using namespace cpmppi_k;

namespace {

// Plant (caller side): one control period of E simulated cartpoles under held controls, with the reference's
// experiment schedule and the recording in the same launch (include/cpmppi.h, cpmppi_plant_args, lists the order of events; one
// env per lane).  The pole length may change from one simulation step to the next (CartPole/__init__.py:529-537): its folded
// constants are re-formed only on a change.
struct PlantDev {
  uint32_t E, row_envs, n_sub, period_steps, save_every, sched_stride;
  float dt_sim;
  uint64_t period, save_rows, ctrl_rows, sched_rows;
  const unsigned long long* period_dev;
  float* s;
  const float* Q;
  const float* L;
  float *states_log, *dd_log, *Q_log;
  const float *tp_table, *te_table, *L_table;
  float *tp_out, *te_out, *L_out;
  const float *m_pole, *m_table, *Lc_table;
  const float* Qd_table;
  float Q_bias;
  float* Qa_out;
  // measurement chain
  float *s_meas, *hist;
  uint32_t hist_len, lat_steps;
  double lat_frac;
  const float* noise_table;
  const double* off_table;
  const uint8_t* informed_table;
};

// wrap_angle_rad on a float64 (CartPole/_CartPole_mathematical_helpers.py:13-21)
__device__ __forceinline__ double wrap_angle_f64(double a) {
  constexpr double PI = 3.141592653589793, TWO_PI = 6.283185307179586;
  const double m = fmod(a, TWO_PI);
  return m < -PI ? m + TWO_PI : (m > PI ? m - TWO_PI : m);
}

__global__ __launch_bounds__(BLOCK) void plant_kernel(const Params p0, const PlantDev a) {
  const uint32_t env = blockIdx.x * BLOCK + threadIdx.x;
  if (env >= a.E) return;
  const uint32_t E = a.row_envs;                                       // envs per ROW of the logs and tables (>= a.E: an env group's slice)
  // a period the device counter cannot name (still 0) is advanced from the schedule's first row and neither recorded nor published
  uint64_t c = a.period;
  bool known = true;
  if (a.period_dev) {
    const uint64_t cnt = (uint64_t)*a.period_dev;
    known = cnt != 0u;
    c = known ? cnt - 1u : 0u;
  }
  const uint64_t g0 = c * a.period_steps;                              // simulation step at which this period's control was computed
  auto sched_row = [&](uint64_t g) -> size_t {
    const uint64_t r = g / a.sched_stride;
    return (size_t)(r < a.sched_rows ? r : a.sched_rows - 1u) * E + env;
  };
  Params p = p0;                                                       // (this env's copy: its pole mass may differ and change)
  float Lcur = a.L_table ? a.L_table[sched_row(g0)] : (a.L ? a.L[env] : p.L_default);
  p.m_pole = a.m_table ? a.m_table[sched_row(g0)] : (a.m_pole ? a.m_pole[env] : p0.m_pole);
  EnvConst ec = make_env_const(p, Lcur);
  float* se = a.s + (size_t)env * 6;
  State<float> st{se[0], se[1], se[2], se[3], se[4], se[5]};
  float q = a.Q[env];
  if (a.Q_log && known && c < a.ctrl_rows) a.Q_log[(size_t)c * E + env] = q;
  if (a.Qd_table && known && c < a.ctrl_rows)                          // add_control_noise (:523-524): two float32 additions
    q = __fadd_rn(__fadd_rn(q, a.Qd_table[(size_t)c * E + env]), a.Q_bias);
  if (a.Qa_out) a.Qa_out[env] = q;                                     // the next call's Q_ccrc (:489)
  const float u = p.u_max * q;
  float aDD, xDD;
  ode_precise(st.c, st.s, st.w, st.v, u, p, ec, aDD, xDD);             // CartPole/__init__.py:316-320 (Update_Q, Q2u, cartpole_ode)
  auto log_dd = [&](uint64_t g) {
    if (!a.dd_log || !known || g % a.save_every) return;
    const uint64_t r = g / a.save_every;
    if (r < a.save_rows) { float* d = a.dd_log + ((size_t)r * E + env) * 2u; d[0] = aDD; d[1] = xDD; }
  };
  log_dd(g0);
  for (uint32_t i = 0; i < a.n_sub; ++i) {
    const uint64_t g = g0 + i + 1u;
    if (a.L_table || a.m_table) {                                      // update_parameters (:529-537) comes first in update_state
      const size_t r = sched_row(g);
      const float Ln = a.L_table ? a.L_table[r] : Lcur;
      const float mn = a.m_table ? a.m_table[r] : p.m_pole;
      if (Ln != Lcur || mn != p.m_pole) { Lcur = Ln; p.m_pole = mn; ec = make_env_const(p, Lcur); }
    }
    plant_substep(st, aDD, xDD, a.dt_sim, p, ec);
    if (a.hist && known) {                                             // the latency buffer (CartPole/latency_adder.py:36-47)
      float* hs = a.hist + ((size_t)(g % a.hist_len) * E + env) * 6u;
      hs[0] = st.th; hs[1] = st.w; hs[2] = st.c; hs[3] = st.s; hs[4] = st.x; hs[5] = st.v;
    }
    ode_precise(st.c, st.s, st.w, st.v, u, p, ec, aDD, xDD);
    if (known && g % a.save_every == 0u) {
      const uint64_t r = g / a.save_every;
      if (a.states_log && r < a.save_rows) {
        float* lg = a.states_log + ((size_t)r * E + env) * 6u;
        lg[0] = st.th; lg[1] = st.w; lg[2] = st.c; lg[3] = st.s; lg[4] = st.x; lg[5] = st.v;
      }
      // a FULL period's last step gets its control (hence its derivatives) from the next controller call; the steps of a
      // trailing partial period (n_sub < period_steps: the run ends inside a period) are followed by no call - their rows are
      // completed here under the held control, as the reference's save does (advisor, round 5)
      if (i + 1u < a.period_steps) log_dd(g);
    }
  }
  se[0] = st.th; se[1] = st.w; se[2] = st.c; se[3] = st.s; se[4] = st.x; se[5] = st.v;
  if (a.n_sub && known) {                                              // what the next controller call is handed (:509-520)
    const size_t r = sched_row(g0 + a.n_sub);
    if (a.tp_table && a.tp_out) a.tp_out[env] = a.tp_table[r];
    if (a.te_table && a.te_out) a.te_out[env] = a.te_table[r];
    if (a.L_table && a.L_out) a.L_out[env] = (a.Lc_table ? a.Lc_table : a.L_table)[r];
    if (a.s_meas && a.n_sub == a.period_steps) {                       // what the NEXT controller call sees (add_noise_and_latency, :336-356)
      const uint64_t g1 = g0 + a.n_sub;
      double m_th = st.th, m_w = st.w, m_c = st.c, m_s = st.s, m_x = st.x, m_v = st.v;
      if (a.hist) {
        // the state k steps back; before step 1: the buffer's initial content (zeros, cos = 1)
        const bool h1 = g1 >= (uint64_t)a.lat_steps + 1u, h2 = g1 >= (uint64_t)a.lat_steps + 2u;
        const float* p1 = a.hist + ((size_t)((g1 - (h1 ? a.lat_steps : 0u)) % a.hist_len) * E + env) * 6u;
        const float* p2 = a.hist + ((size_t)((g1 - (h2 ? a.lat_steps + 1u : 0u)) % a.hist_len) * E + env) * 6u;
        const double a_th = h1 ? (double)p1[0] : 0.0, a_w = h1 ? (double)p1[1] : 0.0, a_c = h1 ? (double)p1[2] : 1.0,
                     a_s = h1 ? (double)p1[3] : 0.0, a_x = h1 ? (double)p1[4] : 0.0, a_v = h1 ? (double)p1[5] : 0.0;
        const double b_th = h2 ? (double)p2[0] : 0.0, b_w = h2 ? (double)p2[1] : 0.0, b_c = h2 ? (double)p2[2] : 1.0,
                     b_s = h2 ? (double)p2[3] : 0.0, b_x = h2 ? (double)p2[4] : 0.0, b_v = h2 ? (double)p2[5] : 0.0;
        const double f = a.lat_frac;
        m_th = a_th + f * (b_th - a_th); m_w = a_w + f * (b_w - a_w); m_c = a_c + f * (b_c - a_c);
        m_s = a_s + f * (b_s - a_s); m_x = a_x + f * (b_x - a_x); m_v = a_v + f * (b_v - a_v);
      }
      if (a.noise_table && c + 1u < a.ctrl_rows) {                     // noise_adder.py:71-82
        const float* nz = a.noise_table + ((size_t)(c + 1u) * E + env) * 4u;
        m_th = wrap_angle_f64(m_th + (double)nz[0]);
        m_c = cos(m_th); m_s = sin(m_th);
        m_x += (double)nz[1]; m_w += (double)nz[2]; m_v += (double)nz[3];
      }
      const double off = a.off_table ? a.off_table[r] : 0.0;          // :348-356 (always re-forms cos / sin from the float64 angle)
      m_th = wrap_angle_f64(m_th + off);
      if (!a.informed_table || a.informed_table[r]) m_th = wrap_angle_f64(m_th - off);   // :501-505 (cos / sin formed again: only the last pair survives)
      m_c = cos(m_th); m_s = sin(m_th);
      float* sm = a.s_meas + (size_t)env * 6u;
      sm[0] = (float)m_th; sm[1] = (float)m_w; sm[2] = (float)m_c; sm[3] = (float)m_s; sm[4] = (float)m_x; sm[5] = (float)m_v;
    }
  }
}

}  // namespace

int check_plant(cpmppi_handle* h, const cpmppi_plant_args* a) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (!a || a->E == 0 || !a->s || !a->Q || !(a->dt_sim > 0.0f)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: bad argument");
  const uint32_t period_steps = a->period_steps ? a->period_steps : a->n_substeps;
  if (a->n_substeps > period_steps)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: n_substeps must not exceed period_steps");
  const uint32_t save_every = a->save_every ? a->save_every : period_steps;
  if ((a->states_log || a->dd_log) && save_every == 0)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: save_every / period_steps missing");
  const bool tables = a->target_position_table || a->target_equilibrium_table || a->L_table || a->m_pole_table || a->L_controller_table;
  if (a->Q_disturbance_table && a->ctrl_rows == 0)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: Q_disturbance_table needs ctrl_rows > 0");
  // (the kernel writes the ring whenever it is given, measurement chain or not: advisor, round 5)
  if (a->state_history && a->history_len == 0u)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: state_history needs history_len > 0");
  if (misaligned(a->state_history)) return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_plant_step: misaligned");
  if (a->s_measured) {
    const bool delayed = a->latency_steps != 0u || a->latency_frac != 0.0;
    if (delayed && (!a->state_history || a->history_len < a->latency_steps + 2u))
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: a latency needs state_history with history_len >= latency_steps + 2");
    if (!(a->latency_frac >= 0.0 && a->latency_frac < 1.0))
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: latency_frac must lie in [0, 1)");
    if ((a->angle_offset_table || a->informed_table) && a->sched_rows == 0)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: schedule tables need sched_rows > 0");
    if (a->measurement_noise_table && a->ctrl_rows == 0)
      return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: measurement_noise_table needs ctrl_rows > 0");
    if (misaligned(a->s_measured) || misaligned(a->state_history) || misaligned(a->measurement_noise_table) ||
        ((uintptr_t)a->angle_offset_table & 7u))
      return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_plant_step: misaligned");
  }
  if (a->L_controller_table && !a->L_table)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: L_controller_table stands in for L_table in L_out: give both");
  if (tables && a->sched_rows == 0) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: schedule tables need sched_rows > 0");
  if (a->row_envs != 0 && a->row_envs < a->E) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: row_envs < E");
  // a host-named period must lie inside the control log it is to be written to (rows of the state logs that fall outside are
  // skipped by the kernel, as for a device counter)
  if (!a->period_dev && a->Q_log && a->period >= a->ctrl_rows)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_step: period outside Q_log (period >= ctrl_rows)");
  if (misaligned(a->s) || misaligned(a->Q) || misaligned(a->L) || misaligned(a->states_log) || misaligned(a->dd_log) ||
      misaligned(a->Q_log) || misaligned(a->target_position_table) || misaligned(a->target_equilibrium_table) ||
      misaligned(a->L_table) || misaligned(a->target_position_out) || misaligned(a->target_equilibrium_out) || misaligned(a->L_out) ||
      misaligned(a->m_pole) || misaligned(a->m_pole_table) || misaligned(a->L_controller_table) || misaligned(a->Q_disturbance_table) ||
      misaligned(a->Q_applied_out) ||
      (a->period_dev && ((uintptr_t)a->period_dev & 7u)))
    return fail(h, CPMPPI_ERR_ALIGN, "cpmppi_plant_step: misaligned");
  return CPMPPI_OK;
}

extern "C" {

int cpmppi_plant_step(cpmppi_handle* h, const cpmppi_plant_args* a, void* stream) {
  if (const int rc = check_plant(h, a); rc != CPMPPI_OK) return rc;
  const uint32_t period_steps = a->period_steps ? a->period_steps : a->n_substeps;
  const uint32_t save_every = a->save_every ? a->save_every : period_steps;
  CPMPPI_ON_DEVICE(h);
  Params plant = h->prm;                  // the simulated system's own pole mass (see cpmppi_set_pole_mass)
  plant.m_pole = h->plant_m_pole;
  PlantDev d{};
  d.E = a->E; d.row_envs = a->row_envs ? a->row_envs : a->E; d.n_sub = a->n_substeps; d.period_steps = period_steps; d.save_every = save_every ? save_every : 1u;
  d.sched_stride = a->sched_stride ? a->sched_stride : 1u;
  d.dt_sim = a->dt_sim;
  d.period = a->period; d.save_rows = a->save_rows; d.ctrl_rows = a->ctrl_rows; d.sched_rows = a->sched_rows ? a->sched_rows : 1u;
  d.period_dev = (const unsigned long long*)a->period_dev;
  d.s = a->s; d.Q = a->Q; d.L = a->L;
  d.states_log = a->states_log; d.dd_log = a->dd_log; d.Q_log = a->Q_log;
  d.tp_table = a->target_position_table; d.te_table = a->target_equilibrium_table; d.L_table = a->L_table;
  d.tp_out = a->target_position_out; d.te_out = a->target_equilibrium_out; d.L_out = a->L_out;
  d.m_pole = a->m_pole; d.m_table = a->m_pole_table; d.Lc_table = a->L_controller_table;
  d.Qd_table = a->Q_disturbance_table; d.Q_bias = a->Q_bias; d.Qa_out = a->Q_applied_out;
  d.s_meas = a->s_measured; d.hist = a->state_history; d.hist_len = a->history_len; d.lat_steps = a->latency_steps;
  d.lat_frac = a->latency_frac; d.noise_table = a->measurement_noise_table; d.off_table = a->angle_offset_table;
  d.informed_table = a->informed_table;
  hipLaunchKernelGGL(plant_kernel, dim3((a->E + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, plant, d);
  return launched(h);
}

int cpmppi_plant_advance(cpmppi_handle* h, uint32_t E, float* s, const float* Q, const float* L, uint32_t n_substeps,
                         float dt_sim, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || !s || !Q || !(dt_sim > 0.0f)) return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_advance: bad argument");
  cpmppi_plant_args a{};
  a.E = E; a.s = s; a.Q = Q; a.L = L; a.n_substeps = n_substeps; a.period_steps = n_substeps; a.dt_sim = dt_sim;
  return cpmppi_plant_step(h, &a, stream);
}

// (ABI 2's form of the recording plant: states_log[row + 1] = the advanced state, Q_log[row] = Q - cpmppi_plant_step with one saved
// row per control period)
int cpmppi_plant_advance_record(cpmppi_handle* h, uint32_t E, float* s, const float* Q, const float* L, uint32_t n_substeps,
                                float dt_sim, float* states_log, float* Q_log, uint64_t log_rows, uint64_t row,
                                const void* row_dev, void* stream) {
  if (!h) return CPMPPI_ERR_BAD_ARG;
  if (E == 0 || !s || !Q || !(dt_sim > 0.0f) || n_substeps == 0)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_advance_record: bad argument");
  if ((states_log || Q_log) && !row_dev && row >= log_rows)
    return fail(h, CPMPPI_ERR_BAD_ARG, "cpmppi_plant_advance_record: row outside the logs (row >= log_rows)");
  cpmppi_plant_args a{};
  a.E = E; a.s = s; a.Q = Q; a.L = L; a.n_substeps = n_substeps; a.period_steps = n_substeps; a.dt_sim = dt_sim;
  a.period = row; a.period_dev = row_dev;
  a.states_log = states_log; a.save_rows = log_rows + 1u; a.save_every = n_substeps;
  a.Q_log = Q_log; a.ctrl_rows = log_rows;
  return cpmppi_plant_step(h, &a, stream);
}

}  // extern "C"
