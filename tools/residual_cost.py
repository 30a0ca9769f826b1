"""The measurements behind DESIGN 2.9 (field residual), one run on the GPU box:

    python3 tools/residual_cost.py cost [N]      wall clock of one residual sample, one lbm_monitor call and the host route
                                                 (get_fields + NumPy) on an N x N fp32 MRT lattice (default 4096)
    python3 tools/residual_cost.py cases         the three cases of the issue's table on the device: the residual per step at every
                                                 check, where it reaches its floor, and where the mean-u rule fires
    python3 tools/residual_cost.py sweep [tol]   datagen at 384 x 384, Re 100 .. 400 step 100, under both criteria: iterations per Re
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latticeboltzmannsimulations_amd import CavitySolver, datagen, residual  # noqa: E402

ULB = 0.08


def _timed(f, sync, reps):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), min(out), max(out)


def cost(n):
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32) as s:
        print(s.describe())
        s.step(64)
        s.begin_residual(capacity=4096)
        s.sample_residual()
        win = (n // 40, n - 1 - n // 40, n // 40, n - 1 - n // 40)
        prev = list(s.get_fields(out_dtype=np.float32))

        def host_route():
            u, rho = s.get_fields(out_dtype=np.float32)
            residual.host_residual(prev[0], prev[1], u, rho)
            prev[0], prev[1] = u, rho
        for name, f, reps in (("residual sample (k_residual + k_residual_final)", s.sample_residual, 50),
                              ("lbm_monitor (k_monitor + k_monitor_final + 272 B to the host)", lambda: s.monitor(window=win), 50),
                              ("one 8-step launch unit", lambda: s.step(8), 50),
                              ("host route: get_fields + residual.host_residual", host_route, 3)):
            med, lo, hi = _timed(f, s.sync, reps)
            print(f"{name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} repetitions)")
        for every in (0, 8, 64, 512):
            if every:
                s.begin_residual(every=every, capacity=2048 // every + 1)
            ms = [s.time_steps(2048) for _ in range(2)]
            print(f"2048 steps, residual every {every}: {ms[0]:.1f} / {ms[1]:.1f} ms")
        s.end_residual()


def cases():
    for nx, Re, RT, P, maxIt in ((64, 100.0, "MRT", 250, 40000), (96, 400.0, "SRT", 500, 100000), (64, 1000.0, "MRT", 250, 40000)):
        with CavitySolver(nx, nx, Re, RT=RT, dtype=np.float32, turb=0) as s:
            s.begin_residual(capacity=maxIt // P + 2, out_dtype=np.float32)
            past, count, fired = 0.0, 0, None
            for It in range(0, maxIt, P):
                s.step(It + 1 - s.steps_done)
                s.sample_residual()
                m = s.mean_u()
                if abs(m - past) / ULB < 1e-8:
                    count += 1
                    if count > 5 and fired is None:
                        fired = s.steps_done
                past = m
            ser = s.residual_series()
        v = residual.norms(ser, ULB)["rel_l2_per_step"]
        floor = float(np.median(v[-10:]))
        reach = next((int(ser["step"][i]) for i in range(len(v)) if v[i] < 2.0 * floor), None)
        print(f"{nx}^2 Re {Re:g} {RT}, check every {P}: first {v[0]:.2e}, last {v[-1]:.2e}, median of the last ten {floor:.2e}, "
              f"within 2x of it from step {reach}; still falling: {bool(v[-1] < 0.8 * v[-11])}; mean-u rule (lbm_mean_u) fires at step {fired}")
        print("   every 8th check:", ", ".join(f"{int(a)}: {b:.2e}" for a, b in zip(ser["step"][::8], v[::8])))


def sweep(tol):
    Res = np.arange(100, 500, 100)
    kw = dict(Re_range=Res, xsize=384, ysize=384, Pinterval=10000, maxIt=600001, save=False, quiet=True, convergence="device")
    t0 = time.perf_counter()
    its_mean = datagen.generate(**kw)[4]
    t1 = time.perf_counter()
    out = datagen.generate(criterion="residual", residual_tol=tol, **kw)
    t2 = time.perf_counter()
    print(f"384^2, SRT + closure, Re {list(Res)}, Pinterval 10000, maxIt 600001")
    print(f"  mean-u rule (tolerance 1e-7, six hits): iterations {list(its_mean)}, {t1 - t0:.1f} s")
    print(f"  residual rule (residual_tol {tol:g}): iterations {list(out[4])}, residual_final {['%.2e' % v for v in out[5]]}, {t2 - t1:.1f} s")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    if what == "cost":
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif what == "cases":
        cases()
    else:
        sweep(float(sys.argv[2]) if len(sys.argv) > 2 else 1e-6)
