"""Batched Reynolds-number sweep -- the reference's MRT_GPU_datagen.py: many independent cavity
solves (default Re = 100, 110, ... 5090 at 384 x 384, SRT + Smagorinsky), each run to the reference's convergence
criterion, producing the four arrays its CNN scripts consume:

    feq_initial.npy [9, X, Y]   the common initial equilibrium      (MRT_GPU_datagen.py:899)
    f_final.npy     [n, 9, X, Y] converged populations per Re        (MRT_GPU_datagen.py:879-900)
    u_final.npy     [n, 2, X, Y] converged velocity per Re           (MRT_GPU_datagen.py:879-901)
    Re_range.npy    [n]                                              (MRT_GPU_datagen.py:902)

The reference solves them one after another (MRT_GPU_datagen.py:57); a 384^2 lattice keeps an MI355X busy for a few
microseconds per step, so here `concurrent` lattices form ONE batch (`CavityBatch`, lbm_params.batch): the same launches
advance all of them, each with its own relaxation rates (measured: 7.8 us per step for one 384^2 lattice, 1.6 us per
lattice and step in a batch of 64).  Consecutive Reynolds numbers share a batch (similar convergence times); a lattice that
meets the criterion is recorded at that iteration and merely keeps stepping until the rest of its batch is done.  With
`devices` the batches are dealt to several GPUs of the node, one host thread per device.  Every solve is bit-identical to
running it alone.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from timeit import default_timer as timer

import numpy as np

from . import residual as RS
from .solid import mask_from
from .solver import CavityBatch
from .stopping import MeanUStop, ResidualStop, by_residual, subgrid_constant, wall_model


def _solve_batch(idx, Re_range, xsize, ysize, RT, turb, uLB, maxIt, Pinterval, tolerance, device, dtype, say, out, arith, convergence="host",
                 semantics="mrt_gpu", residual_tol=None, residual_final=None, batch_factory=None, solid=None, solid_tiles=False, subgrid=None):
    """Runs the lattices Re_range[idx] in lock step; fills out = (f_final, u_final, its) rows idx.  The per-lattice logic is
    the reference's loop body (MRT_GPU_datagen.py:707-731,862-871): a check after iteration It = 0, Pinterval, 2 Pinterval, ...
    (i.e. after It + 1 steps), and a lattice stops where its stop rule says so (stopping.MeanUStop with `tolerance`).
    residual_final (criterion='residual'): every check takes a sample of the field residual on the device instead (one record per
    lattice crosses PCIe), and a lattice stops at the first check below residual_tol (stopping.ResidualStop) -- the rule of
    run_cavity(criterion='residual'); residual_final rows idx receive the value each lattice stopped at."""
    by_res = residual_final is not None
    f_final, u_final, its = out
    sem = {} if semantics == "mrt_gpu" else {"semantics": semantics}
    if solid is not None:      # [n, X, Y]: every lattice of the batch its own mask
        sem["solid"] = np.ascontiguousarray(solid[idx])
    elif subgrid is not None:  # (the closure lives on the obstacle lattices: an empty mask is the plain bounce-back cavity)
        sem["solid"] = np.zeros((len(idx), xsize, ysize), dtype=bool)
    if solid_tiles:
        sem["tuning"] = dict(solid_tiles=True)
    make = CavityBatch if batch_factory is None else batch_factory
    with make(xsize, ysize, [float(Re_range[i]) for i in idx], RT=RT, uLB=uLB, dtype=dtype, turb=turb, device=device, arith=arith, **sem) as b:
        if subgrid is not None:
            b.set_subgrid(subgrid)
        feq_initial = b.get_fields(want_fin=True, out_dtype=np.float32)[2][0]      # fin = equ(1, InitVel) = feq_initial
        stops = [ResidualStop(uLB, residual_tol) if by_res else MeanUStop(uLB, tolerance) for _ in idx]
        open_ = set(range(len(idx)))
        It = 0
        if by_res:
            b.begin_residual(every=0, capacity=min(maxIt // int(Pinterval) + 2, 1 << 18), out_dtype=np.float32)
        seen = 0
        while open_:
            b.step(It + 1 - b.steps_done)
            # the check value: NumPy's float32 mean of the downloaded field (the reference's own definition), or the mean reduced on
            # the device in double -- B doubles cross PCIe instead of B fields; the fields are then fetched only when a lattice stops
            means = u = ser = None
            if by_res:
                ser = b.sample_residual().residual_series()
            elif convergence == "device":
                means = b.mean_u()
            else:
                u = b.get_fields(out_dtype=np.float32)[0]
            finished = []
            for j in sorted(open_):
                say("current Re is " + str(Re_range[idx[j]]) + " and iteration is " + str(It))
                if by_res:
                    rec = RS.latest(ser, seen, j)
                    done = False
                    if rec is not None:
                        residual_final[idx[j]], done = stops[j].update(rec)
                        say("current residual is " + str(residual_final[idx[j]]))
                else:
                    mean_u = float(np.mean(u[j]) if means is None else means[j])
                    say("current mean u is " + str(mean_u / uLB))
                    done = stops[j].update(mean_u)
                if done:
                    say("breaking out of loop because of convergence")
                    finished.append(j)
            if by_res:
                seen = ser["count"]
            last = It + Pinterval > maxIt - 1          # no further check: the rest finishes the loop like the reference
            if finished:
                if u is None:
                    u = b.get_fields(out_dtype=np.float32)[0]
                fin = b.get_fields(want_fin=True, out_dtype=np.float32)[2]
                for j in finished:
                    f_final[idx[j]], u_final[idx[j]], its[idx[j]] = fin[j], u[j], b.steps_done
                    open_.discard(j)
            if last and open_:
                say("max iterations reached. More needed for convergence.")
                if maxIt > b.steps_done:
                    b.step(maxIt - b.steps_done)
                u, _, fin = b.get_fields(want_fin=True, out_dtype=np.float32)
                for j in open_:
                    f_final[idx[j]], u_final[idx[j]], its[idx[j]] = fin[j], u[j], b.steps_done
                open_ = set()
            It += Pinterval
    return feq_initial


def generate(Re_range=None, xsize=32 * 12, ysize=32 * 12, RT="SRT", turb=1, uLB=0.08, maxIt=3000000, Pinterval=10000,
             tolerance=0.0000001, OutputFolder="./output", save=True, concurrent=64, devices=(0,), dtype=np.float32,
             quiet=False, arith="strict", convergence="host", BC="EB-NEBB ", criterion="mean_u", residual_tol=None, batch_factory=None,
             solid=None, solid_tiles=False, subgrid=None):
    """Returns (feq_initial, f_final, u_final, Re_range, iterations_per_Re); writes the four .npy files when `save`.
    criterion: 'mean_u' (default, the reference's rule) or 'residual' -- each lattice stops at the first check whose field residual (the
    relative L2 change of u per step since the previous check, reduced on the device) is below residual_tol, which must be given; the
    function then returns a sixth item, residual_final [n], the value each lattice stopped at (the last one seen for a lattice that
    ran out of iterations, NaN if it saw none), and saves it as residual_final.npy beside the four files, which do not change.
    BC: 'EB-NEBB ' (default, the wet-node walls of MRT_GPU.py) or 'BB' (half-way bounce-back, semantics='bounce_back': the
    cavity's mass is conserved to rounding; needs turb=0).
    solid: solid obstacles at rest inside every cavity (CavitySolver(solid=...); BC='BB' only) -- one mask [X, Y] for all lattices or
    [n, X, Y], one per Reynolds number; saved as solid.npy [n, X, Y] beside u_final.npy.  None (default): nothing changes.
    solid_tiles=True (with solid=...): the batches step three to five steps per launch on the tile kernel
    (CavityBatch(tuning=dict(solid_tiles=True))) instead of one; the same bits.
    subgrid (BC='BB'): the constant Cs^2 of the local Smagorinsky closure (CavityBatch.set_subgrid; the reference's is 0.025) in every
    lattice, each with its own tau0 -- a sweep to Reynolds numbers a coarse lattice cannot resolve; without solid=... the cavities run
    as obstacle lattices with an empty mask.  None (default) and 0: no closure, nothing changes.
    batch_factory (default: CavityBatch, i.e. liblbm_hip.so) exists so that the sweep's loop can be unit-tested with a stand-in, like
    run_cavity's solver_factory; it is not a fallback."""
    semantics = wall_model(BC, "mrt_gpu", turb, solid is not None, solid_tiles)
    by_res = by_residual(criterion, residual_tol)
    cs2 = subgrid_constant(subgrid, BC, solid_tiles)
    say = (lambda *a: None) if quiet else print
    Re_range = np.arange(100, 5100, 10) if Re_range is None else np.asarray(Re_range)   # MRT_GPU_datagen.py:55
    n = len(Re_range)
    if solid is not None:
        solid = np.asarray(solid) != 0
        if solid.shape == (xsize, ysize):
            solid = np.broadcast_to(solid, (n, xsize, ysize))
        if solid.shape != (n, xsize, ysize):
            raise ValueError(f"solid must have shape {(xsize, ysize)} or {(n, xsize, ysize)}")
    tstart = timer()
    out = (np.zeros((n, 9, xsize, ysize), dtype=np.float32), np.zeros((n, 2, xsize, ysize), dtype=np.float32),
           np.zeros(n, dtype=np.int64))
    residual_final = np.full(n, np.nan) if by_res else None
    chunks = [list(range(i, min(n, i + concurrent))) for i in range(0, n, concurrent)]

    def work(k):
        return _solve_batch(chunks[k], Re_range, xsize, ysize, RT, turb, uLB, maxIt, Pinterval, tolerance,
                            devices[k % len(devices)], dtype, say, out, arith, convergence, semantics,
                            float(residual_tol) if by_res else None, residual_final, batch_factory, solid, solid_tiles, cs2)
    if len(devices) > 1 and len(chunks) > 1:
        with ThreadPoolExecutor(max_workers=len(devices)) as pool:      # lbm_step runs in C with the GIL released
            feq = list(pool.map(work, range(len(chunks))))
    else:
        feq = [work(k) for k in range(len(chunks))]
    feq_initial = feq[0] if feq else None
    f_final, u_final, its = out
    if save:
        if not os.path.isdir(OutputFolder):
            os.makedirs(OutputFolder, exist_ok=True)
        np.save(os.path.join(OutputFolder, "feq_initial.npy"), feq_initial)
        np.save(os.path.join(OutputFolder, "f_final.npy"), f_final)
        np.save(os.path.join(OutputFolder, "u_final.npy"), u_final)
        np.save(os.path.join(OutputFolder, "Re_range.npy"), Re_range)
        if by_res:
            np.save(os.path.join(OutputFolder, "residual_final.npy"), residual_final)
        if solid is not None:
            np.save(os.path.join(OutputFolder, "solid.npy"), np.ascontiguousarray(solid))
    say("TOTAL time elapsed is ", timer() - tstart, "seconds")
    if by_res:
        return feq_initial, f_final, u_final, Re_range, its, residual_final
    return feq_initial, f_final, u_final, Re_range, its


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Reynolds-number sweep (drop-in for MRT_GPU_datagen.py)")
    ap.add_argument("--Re", type=float, nargs=3, default=[100, 5100, 10], metavar=("START", "STOP", "STEP"))
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--concurrent", type=int, default=64, help="lattices per batch")
    ap.add_argument("--Pinterval", type=int, default=10000)
    ap.add_argument("--maxIt", type=int, default=3000000)
    ap.add_argument("--OutputFolder", default="./output")
    ap.add_argument("--arith", choices=["strict", "fast", "promoted"], default="strict",
                    help="fast: agrees with strict to rounding, ~1.3x faster; promoted: MRT_GPU.py's CUDA text arithmetic (fp32)")
    ap.add_argument("--convergence", choices=["host", "device"], default="host",
                    help="device: the convergence test on lbm_mean_u (reduced on the GPU) instead of the downloaded field")
    ap.add_argument("--BC", choices=["EB-NEBB", "BB"], default="EB-NEBB",
                    help="wall model: EB-NEBB wet-node walls (with the Smagorinsky closure), or BB half-way bounce-back (without it)")
    ap.add_argument("--criterion", choices=["mean_u", "residual"], default="mean_u",
                    help="stop rule per lattice: the reference's test on mean(u), or the field residual reduced on the GPU")
    ap.add_argument("--residual-tol", type=float, default=None, help="with --criterion residual: stop below this value (required, no default)")
    ap.add_argument("--solid-box", type=int, nargs=4, action="append", default=[], metavar=("X0", "X1", "Y0", "Y1"),
                    help="a solid obstacle in every cavity: the cells [X0, X1) x [Y0, Y1), y = 0 the lid (repeatable; needs --BC BB)")
    ap.add_argument("--solid-tiles", action="store_true",
                    help="with --solid-box: three to five steps per launch on the tile kernel instead of one (the same bits)")
    ap.add_argument("--subgrid", type=float, default=None, metavar="CS2",
                    help="the local Smagorinsky closure in every cavity with this constant (the reference's is 0.025; needs --BC BB)")
    a = ap.parse_args(argv)
    bb = dict(BC="BB", turb=0) if a.BC == "BB" else {}
    if a.subgrid is not None:
        try:
            subgrid_constant(a.subgrid, a.BC, a.solid_tiles)
        except ValueError as e:
            ap.error(str(e))
        bb["subgrid"] = a.subgrid
    if a.solid_box or a.solid_tiles:
        try:
            mask = mask_from(a.size, a.size, a.solid_box)
            wall_model(a.BC, "mrt_gpu", bb.get("turb", 1), mask is not None, a.solid_tiles)
        except ValueError as e:
            ap.error(str(e))
        bb["solid"] = mask
        if a.solid_tiles:
            bb["solid_tiles"] = True
    generate(np.arange(*a.Re), xsize=a.size, ysize=a.size, concurrent=a.concurrent, Pinterval=a.Pinterval, maxIt=a.maxIt,
             OutputFolder=a.OutputFolder, arith=a.arith, convergence=a.convergence, criterion=a.criterion, residual_tol=a.residual_tol,
             **bb)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
