#!/usr/bin/env python3
"""A/B timing of launch plans and kernel variants on one MI355X (run through gpurun).

    python tools/perf_ab.py [--steps 600] [--reps 3] case [case ...]

A case is  size:dtype:arith[:key=value,...]  e.g.  4096:f32:fast   4096:f32:strict:tb_steps=4   8192x1024:f64:fast:coll=SRT,turb=1
(keys: coll, turb, kernel, layout, sem (semantics: mrt_gpu, mrt_py, bounce_back), solid (with sem=bounce_back: fluid -- the all-fluid mask --,
block -- one block of an eighth of the width squared in the middle --, disc -- one disc of an eighth of the width across in the middle --,
random -- 20 % of the cells, seeded --, interior -- the same, one cell clear of the perimeter), motion (with solid: rest -- set_body_motion of
zeros, the kernels of obstacles at rest -- or rotate -- the solid cells turn as one body about their centroid, 0.05 at three quarters of the
width from it; not with route=tiles), shape (with solid: disc -- set_shape with the exact fractions of the circle of solid=disc --, random -- q uniform in (0, 1], seeded, for any
mask -- or half -- 1/2 on every link: the kernels of a shaped lattice; set before the motion; not with route=tiles), periodic (with solid: x, y
or xy -- set_periodic, the k_wrap launch behind every step; the mask is wrapped first), drive (with solid: 1 -- set_driving_force(1e-6, 0)),
scalar (with solid: D -- begin_scalar(D, 1.0), every wall adiabatic: the scalar step behind every flow step),
buoyancy (with scalar: A -- set_buoyancy(0, A, 1.0): the buoyant twins of the flow and scalar kernels),
subgrid (with solid: CS2 -- set_subgrid(CS2): the kernels with the sub-grid closure; 0 sets nothing),
relax (with solid: 1 -- set_relaxation_field with one plane, the lattice's omega jittered by 5 %, seeded: the kernels that read a rate per cell --
or 2 -- with TRT's second plane as well (coll=TRT); 0 sets nothing),
rheo (with solid: 1 -- set_rheology with the table of a power-law fluid, n = 0.7, whose viscosity at the shear rate uLB / ny is ten times the lattice's and never below twice it,
4096 entries, g_max 0.1: the kernels that look a rate up per cell; 0 sets nothing),
route (with solid: single --
one step per launch, the default -- or tiles -- the multi-step tile kernel, tuning solid_tiles), force (with solid: series.E -- the run
with begin_force(every=E) --, loop.E -- the host loop step(E); solid_force() --, plain.E -- step(E); sync() without any force --, or call -- no stepping: microseconds per call of
body_force() and of solid_force(); these three are timed with the host clock around work that ends in a synchronisation), batch (that
many lattices, GLUPS in aggregate) and every CavitySolver tuning switch).  Prints GLUPS (best of --reps timings of --steps steps
after a device wake-up and a warm-up), microseconds per step and the GLUPS of every repeat, one line per case.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, solid  # noqa: E402


def solid_mask(kind, nx, ny):
    m = np.zeros((nx, ny), dtype=bool)
    if kind == "block":
        w = max(1, nx // 8)
        m[(nx - w) // 2:(nx + w) // 2, (ny - w) // 2:(ny + w) // 2] = True
    elif kind == "disc":
        x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        m = np.hypot(x - (nx - 1) / 2, y - (ny - 1) / 2) < nx / 16
    elif kind in ("random", "interior"):
        m = np.random.default_rng(1).random((nx, ny)) < 0.2
        if kind == "interior":
            m[0] = m[-1] = m[:, 0] = m[:, -1] = False
    elif kind != "fluid":
        raise ValueError("solid must be fluid, block, disc, random or interior")
    return m


def parse(case):
    parts = case.split(":")
    size, dt, arith = parts[0], parts[1], parts[2]
    nx, ny = (int(v) for v in size.split("x")) if "x" in size else (int(size), int(size))
    kw = dict(RT="MRT", turb=0, kernel="auto", layout="auto")
    tune = {}
    if len(parts) > 3 and parts[3]:
        for kv in parts[3].split(","):
            k, v = kv.split("=")
            if k == "coll":
                kw["RT"] = v
            elif k in ("kernel", "layout"):
                kw[k] = v
            elif k == "sem":
                kw["semantics"] = v
            elif k == "turb":
                kw["turb"] = int(v)
            elif k == "solid":
                kw["solid"] = solid_mask(v, nx, ny)
            elif k == "route":
                if v not in ("single", "tiles"):
                    raise ValueError("route must be single or tiles")
                tune["solid_tiles"] = v == "tiles"
            elif k == "force":
                kw["force"] = v
            elif k == "motion":
                if v not in ("rest", "rotate"):
                    raise ValueError("motion must be rest or rotate")
                kw["motion"] = v
            elif k == "shape":
                if v not in ("disc", "half", "random"):
                    raise ValueError("shape must be disc, half or random")
                kw["shape"] = v
            elif k == "periodic":
                if v not in ("x", "y", "xy"):
                    raise ValueError("periodic must be x, y or xy")
                kw["periodic"] = v
            elif k == "drive":
                kw["drive"] = int(v)
            elif k == "scalar":
                kw["scalar"] = float(v)
            elif k == "buoyancy":
                kw["buoyancy"] = float(v)
            elif k == "subgrid":
                kw["subgrid"] = float(v)
            elif k == "relax":
                if v not in ("0", "1", "2"):
                    raise ValueError("relax must be 0, 1 or 2")
                kw["relax"] = int(v)
            elif k == "rheo":
                if v not in ("0", "1"):
                    raise ValueError("rheo must be 0 or 1")
                kw["rheo"] = int(v)
            elif k == "batch":
                kw["batch"] = int(v)
            elif k in ("tb_steps", "frame_seg"):
                tune[k] = int(v)
            else:
                tune[k] = v not in ("0", "false", "False")
    return nx, ny, np.float32 if dt == "f32" else np.float64, arith, kw, tune


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("cases", nargs="+")
    a = ap.parse_args()
    for case in a.cases:
        nx, ny, dtype, arith, kw, tune = parse(case)
        B = kw.pop("batch", 1)
        force = kw.pop("force", None)
        motion = kw.pop("motion", None)
        shape = kw.pop("shape", None)
        per = kw.pop("periodic", None)
        drive = kw.pop("drive", 0)
        scalar_D = kw.pop("scalar", None)
        buoy = kw.pop("buoyancy", None)
        cs2 = kw.pop("subgrid", 0.0)
        relax = kw.pop("relax", 0)
        rheo = kw.pop("rheo", 0)
        if per is not None:
            from latticeboltzmannsimulations_amd import periodic
            kw["solid"] = periodic.wrap(kw["solid"], "x" in per, "y" in per)
        make = (lambda *a_, **k_: CavityBatch(a_[0], a_[1], [a_[2]] * B, **k_)) if B > 1 else CavitySolver
        with make(nx, ny, 1000.0, dtype=dtype, arith=arith, tuning=tune, **kw) as s:
            if per is not None:
                s.set_periodic("x" in per, "y" in per)
            if drive:
                s.set_driving_force(1e-6, 0.0)
            if shape is not None:
                q = {"half": lambda: np.full((8, nx, ny), 0.5), "random": lambda: 1.0 - np.random.default_rng(2).random((8, nx, ny)),
                     "disc": lambda: solid.disc_fractions(kw["solid"], (nx - 1) / 2, (ny - 1) / 2, nx / 16)}[shape]()
                s.set_shape(q)
            if motion is not None:
                s.set_body_motion(np.broadcast_to([0.0, 0.0, 0.05 / (0.75 * nx) if motion == "rotate" else 0.0], (B, 1, 3)[B == 1:]))
            if scalar_D is not None:
                s.begin_scalar(scalar_D, 1.0)
            if buoy is not None:
                s.set_buoyancy(0.0, buoy, 1.0)
            if cs2:
                s.set_subgrid(cs2)
            if relax:
                r = np.random.default_rng(3)
                planes = [np.clip(s.relax[k] * (1.0 + 0.05 * r.standard_normal((nx, ny))), 0.05, 1.95) for k in ("omega", "omegam")[:relax]]
                s.set_relaxation_field(*planes)
            if rheo:
                from latticeboltzmannsimulations_amd import rheology
                nu0, gd0 = (1.0 / s.relax["omega"] - 0.5) / 3.0, s.uLB / ny
                s.set_rheology(*rheology.table(rheology.power_law(10.0 * nu0 / gd0 ** (0.7 - 1.0), 0.7, 2.0 * nu0, 2.0), 4096, 0.1), 0.1)
            s.copy_bandwidth(1 << 30, 60)
            s.step(max(60, a.steps // 10)); s.sync()
            if force == "call":
                for name, call in (("body_force", s.body_force), ("solid_force", s.solid_force)):
                    call()
                    reps = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        for _ in range(50):
                            call()
                        reps.append((time.perf_counter() - t0) / 50)
                    print(f"{case:48s} {name:12s} {min(reps) * 1e6:9.2f} us/call  repeats {' '.join('%.2f' % (r * 1e6) for r in reps)}", flush=True)
                continue
            if force is not None:
                mode, every = force.split(".")
                every = int(every)

                def timed():
                    if mode == "series":
                        s.begin_force(every=every, capacity=a.steps // every + 1)
                    s.sync()
                    t0 = time.perf_counter()
                    if mode == "series":
                        s.step(a.steps)
                        s.sync()
                    else:
                        for _ in range(a.steps // every):
                            s.step(every)
                            s.solid_force() if mode == "loop" else s.sync()
                    return (time.perf_counter() - t0) * 1e3 / a.steps
                timed()
                reps = [timed() for _ in range(a.reps)]
            else:
                reps = [s.time_steps(a.steps) / a.steps for _ in range(a.reps)]
            ms = min(reps)
            print(f"{case:48s} S={s.next_unit(1000)}{' move' if s.describe().get('wall_motion') else ''}{' shape' if s.describe().get('wall_shape') else ''}{' periodic=' + s.describe()['periodic'] if 'periodic' in s.describe() else ''}{' drive' if s.describe().get('driving_force') else ''}{' buoyant' if s.describe().get('buoyancy') else ''}{' subgrid' if s.describe().get('subgrid') else ''}{' relax_field' if s.describe().get('relax_field') else ''}{' relax_field+m' if s.describe().get('relax_field+m') else ''}{' rheology' if s.describe().get('rheology') else ''}  {B * nx * ny / ms / 1e6:8.1f} GLUPS  {ms * 1e3:9.2f} us/step  "
                  f"repeats {' '.join('%.1f' % (B * nx * ny / r / 1e6) for r in reps)}"
                  + (f"  us/step {' '.join('%.2f' % (r * 1e3) for r in reps)}" if force else ""), flush=True)


if __name__ == "__main__":
    main()
