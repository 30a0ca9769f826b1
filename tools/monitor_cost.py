"""The workload behind DESIGN 2.7's sample-cost figures: a 4096 x 4096 fp32 lattice that alternates one 8-step launch unit, one
lbm_mean_u (k_reduce_u) and one lbm_monitor (k_monitor + k_monitor_final), REPS times, so that one kernel trace holds all of them:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o monitor -- python3 tools/monitor_cost.py

The per-kernel times are in <dir>/.../monitor_kernel_stats.csv; profiles/monitor_cost_kernel_stats.csv keeps the rows of these kernels.
Also prints the wall-clock cost of a series: 2048 steps with the monitor off, every 8, 64 and 512 steps."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latticeboltzmannsimulations_amd import CavitySolver  # noqa: E402

REPS = 20

if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32) as s:
        print(s.describe())
        s.step(64)
        off, win = n // 40, (n // 40, n - 1 - n // 40, n // 40, n - 1 - n // 40)
        for _ in range(REPS):
            s.step(8)
            m = s.mean_u()
            r = s.monitor(window=win, probes=((n // 2, n // 2),))
        print("mean_u", m, "monitor", (r["sum_ux"] + r["sum_uy"]) / (2.0 * n * n), r["min_x"], r["min_y"])
        for every in (0, 8, 64, 512):
            if every:
                s.begin_monitor(every=every, capacity=2048 // every, window=win)
            ms = [s.time_steps(2048) for _ in range(2)]
            print(f"2048 steps, monitor every {every}: {ms[0]:.1f} / {ms[1]:.1f} ms")
            if every:
                s.end_monitor()
