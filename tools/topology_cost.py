"""The workload behind DESIGN 2.8's cost figures: a 4096 x 4096 fp32 MRT lattice (arith = fast) that, after 128 steps, alternates one
lbm_monitor and one lbm_topology of four windows (the vortex table's), REPS times, then times lbm_get_stream_function:

    python3 tools/topology_cost.py                                        # wall-clock times of the calls (host clock; each call synchronises)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o topology -- python3 tools/topology_cost.py

The per-kernel times are in <dir>/.../topology_kernel_stats.csv; profiles/topology_cost_kernel_stats.csv keeps the rows of these
kernels.  The yardstick is the monitor pass, which reads the nine planes once; the topology's record path reads them twice."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latticeboltzmannsimulations_amd import CavitySolver  # noqa: E402
from latticeboltzmannsimulations_amd import topology as T  # noqa: E402

REPS = 20


def _ms(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t)), max(t)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32, arith="fast") as s:
        print(s.describe())
        s.step(128)
        wins = T.vortex_windows(n, n)
        win = (n // 40, n - 1 - n // 40, n // 40, n - 1 - n // 40)
        s.monitor(window=win); s.topology(wins)                      # warm-up: code objects, the buffers of the first call
        for _ in range(3):                                             # alternated, so that neither sees a warmer cache than the other
            mon = _ms(lambda: s.monitor(window=win), REPS)
            top = _ms(lambda: s.topology(wins), REPS)
            print("lbm_monitor  min / median / max ms: %.3f %.3f %.3f" % mon)
            print("lbm_topology min / median / max ms: %.3f %.3f %.3f   ratio of the medians %.2f" % (top + (top[1] / mon[1],)))
        s.stream_function()
        print("lbm_get_stream_function (psi and omega, 2 x %d MiB to the host) min / median / max ms: %.1f %.1f %.1f"
              % ((n * n * 8 >> 20,) + _ms(lambda: s.stream_function(), 5)))
        print("vortex table", s.vortex_table())
