// cpmppi_rollout_tuned_throughput.hip - rollout_cost_tuned_kernel (the cost weights, LBD and sigma read per env: cpmppi_set_tuning_rows):
// the throughput builds of both ODE predictors and predictor_ODE's lone-wave form (the flags of
// cpmppi_rollout_throughput.hip / cpmppi_rollout_ode_throughput.hip / cpmppi_rollout_ode_lone.hip).
#include "cpmppi_rollout.hpp"

namespace cpmppi_k {
CPMPPI_TUNED_THROUGHPUT_INSTANCES(CPMPPI_DEFINE_ROLLOUT_TUNED)
}  // namespace cpmppi_k
