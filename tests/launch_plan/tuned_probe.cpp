// TEST INFRASTRUCTURE (tests/test_tuning_rows_host.py): plan_rollout of csrc/cpmppi_launch_plan.hpp with its input "tuning rows
// registered".  Reads launches from standard input, one per line - ode_predictor math_mode rollouts_per_lane N H P E noise_kind
// tuning_rows - and prints each one's plan: fast rpl variant integ noise nb blocks W lds_bytes stash fold_first tuned.
#include <stdio.h>
#include "cpmppi_launch_plan.hpp"

int main() {
  unsigned ode, math, rpl, N, H, P, E, noise, tuned;
  while (scanf("%u %u %u %u %u %u %u %u %u", &ode, &math, &rpl, &N, &H, &P, &E, &noise, &tuned) == 9) {
    cpmppi_config cfg{};
    cfg.ode_predictor = ode; cfg.math_mode = math; cfg.rollouts_per_lane = rpl; cfg.N = N; cfg.H = H; cfg.E = E;
    const cpmppi_plan::RolloutPlan p =
        cpmppi_plan::plan_rollout(cfg, P, E, noise, false, cpmppi_plan::RolloutLimits{}, tuned != 0);
    printf("%u %u %u %u %u %u %u %u %u %u %d %d\n", p.fast, p.rpl, p.variant, p.integ, p.noise, p.nb, p.blocks, p.W, p.lds_bytes,
           p.stash, p.fold_first ? 1 : 0, p.tuned ? 1 : 0);
  }
  return 0;
}
