// cpmppi_rollout_tuned_latency.hip - rollout_cost_tuned_kernel (the cost weights, LBD and sigma read per env: cpmppi_set_tuning_rows):
// the latency builds of both ODE predictors (the flags of cpmppi_rollout_latency.hip / cpmppi_rollout_ode_latency.hip).
#include "cpmppi_rollout.hpp"

namespace cpmppi_k {
CPMPPI_TUNED_LATENCY_INSTANCES(CPMPPI_DEFINE_ROLLOUT_TUNED)
}  // namespace cpmppi_k
