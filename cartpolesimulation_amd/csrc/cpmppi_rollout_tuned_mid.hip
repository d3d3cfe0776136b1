// cpmppi_rollout_tuned_mid.hip - rollout_cost_tuned_kernel (the cost weights, LBD and sigma read per env: cpmppi_set_tuning_rows):
// the mid-size build and its lone-wave form (the flags of cpmppi_rollout_mid.hip).
#include "cpmppi_rollout.hpp"

namespace cpmppi_k {
CPMPPI_TUNED_MID_INSTANCES(CPMPPI_DEFINE_ROLLOUT_TUNED)
}  // namespace cpmppi_k
