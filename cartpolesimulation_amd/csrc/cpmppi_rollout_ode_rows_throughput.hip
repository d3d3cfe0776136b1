// Explicit instantiations of the rollout kernel for predictor_type "ODE" with the pole mass read PER ENV (PREDICTOR_ODE_ROWS:
// cpmppi_set_pole_mass_rows), throughput build: the instances of cpmppi_rollout_ode_throughput.hip over again, compiled with that unit's
// flags (see __graft_entry__.build) and launched only while an array of masses is registered with the handle.
#include "cpmppi_rollout.hpp"

namespace cpmppi_k {
CPMPPI_ODE_THROUGHPUT_INSTANCES(CPMPPI_DEFINE_ROLLOUT_ODE_ROWS)
}  // namespace cpmppi_k
