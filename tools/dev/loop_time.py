"""Development tool (GPU): wall time per control step of harness.run, launched and as a replayed graph, at three sizes.
python tools/dev/loop_time.py"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cartpolesimulation_amd.configs import MPPIConfig  # noqa: E402
from cartpolesimulation_amd.engine import MPPIEngine  # noqa: E402
from cartpolesimulation_amd.harness import BatchedCartPoleExperiment, generate_random_initial_states  # noqa: E402

for E, N, H in ((1, 1024, 50), (1, 256, 20), (64, 2048, 50)):
    eng = MPPIEngine(E, MPPIConfig(num_rollouts=N, mpc_horizon=H))
    s0 = generate_random_initial_states(E, np.random.Generator(np.random.SFC64(1)))
    exp = BatchedCartPoleExperiment(eng, seed=1)
    for graph in (False, True):
        exp.run(s0, 50, graph=graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp.run(s0, 1000, graph=graph, steps_per_graph=10)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"E={E} N={N} H={H} graph={graph}: {dt/1000*1e6:.1f} us per control step", flush=True)
    eng.close()
