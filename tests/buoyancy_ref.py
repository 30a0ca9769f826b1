"""CPU reference of Boussinesq buoyancy on obstacle lattices (lbm_set_buoyancy; TEST HELPER).

BuoyantOracle is PeriodicOracle (tests/periodic_ref.py, imported, never edited) with the one piece: with buoyancy (ax, ay, c_ref) set, in
Python floats (double, every operation rounded once, none fused) B_k = (3 w_k) (cx_k ax + cy_k ay) -- drive_terms of (ax, ay) -- each B_k
and c_ref rounded once to the lattice type; every collision of a cell that is neither solid nor held is followed by

    t = Cp - c_ref;   d_k = F_k + B_k t;   fpost_k = fpost_k + d_k        (k = 1 .. 8, every operation in the lattice type)

F_k the constants of the driving force, zeros without one.  Cp is the plane the caller sets before each flow step.

Coupled is the loop of lbm_step with a scalar (tests/scalar_ref.py): Cp = sc.conc() before each flow step, sc.step(*macros(fin)[1:])
after it -- flow step n + 1 reads the C that scalar step n summed, scalar step n the velocity of the state flow step n produced.

RollBuoyant is the second, independent restatement on WrapOracle's plan: no image cells, the real cells alone, np.roll; solid cells at
rest and Dirichlet values.  tests/test_buoyancy_cpu.py checks the first against it bit for bit on the real cells.
"""
import numpy as np

from bounce_back_ref import BOUNCE
from oracle import lbm_numpy as on
from periodic_ref import PeriodicOracle, WrapOracle, drive_terms
from scalar_ref import OPP, WEIGHT, ScalarOracle, collide as scalar_collide, rates


class BuoyantOracle(PeriodicOracle):
    def __init__(self, nx, ny, Re, buoyancy=None, **kw):
        self.buoy = None
        self.Cp = None
        super().__init__(nx, ny, Re, **kw)
        if buoyancy is not None:
            self.set_buoyancy(*buoyancy)

    def set_buoyancy(self, ax=0.0, ay=0.0, c_ref=0.0):
        """No geometry: the state and the step count stay.  (0, 0): none."""
        assert np.isfinite(ax) and np.isfinite(ay) and np.isfinite(c_ref)
        on_ = ax != 0.0 or ay != 0.0
        self.buoy = (float(ax), float(ay), float(c_ref)) if on_ else None
        self.B = [self.par(v) for v in drive_terms(ax, ay)] if on_ else None
        self.c_ref = self.par(c_ref) if on_ else None
        return self

    def collide(self, f, rho, feq, w_nu=None):
        if self.buoy is None:
            return super().collide(f, rho, feq, w_nu)
        out = super(PeriodicOracle, self).collide(f, rho, feq, w_nu)      # (the collision alone: the force enters through d_k, one add)
        assert self.Cp is not None and self.Cp.dtype == np.dtype(self.R), "the plane comes in the lattice type"
        F = self.drive if self.drive is not None else [self.R(0.0)] * 9
        fl = self.fluid()
        t = self.Cp[fl] - self.c_ref
        for k in range(1, 9):
            out[k][fl] = out[k][fl] + (F[k] + self.B[k] * t)
        return out


class Coupled:
    """A flow reference and a scalar reference stepped as lbm_step steps them."""

    def __init__(self, flow, sc):
        self.flow, self.sc = flow, sc

    def step(self, n=1):
        for _ in range(n):
            self.flow.Cp = self.sc.conc()
            self.flow.step(1)
            _, ux, uy = self.flow.macros(self.flow.fin)
            self.sc.step(ux, uy)
        return self


class RollBuoyant:
    """mask[X', Y'] of the periodic domain (no image cells); wall_value NaN on adiabatic solid cells.  The flow part is WrapOracle's plan
    restated with the buoyant add, the scalar part the contract of include/lbm.h on np.roll."""

    def __init__(self, mask, Re, periodic, ny_global, D, c0, wall_value=None, force=(0.0, 0.0), buoyancy=(0.0, 0.0, 0.0), magic=0.25, **kw):
        self.w = WrapOracle(mask, Re, periodic, ny_global, force=force, **kw)
        w = self.w
        R = self.R = w.R
        self.mask = w.mask
        X, Y = self.mask.shape
        self.B = [w.op.par(v) for v in drive_terms(buoyancy[0], buoyancy[1])]
        self.c_ref = w.op.par(buoyancy[2])
        self.on = buoyancy[0] != 0.0 or buoyancy[1] != 0.0
        wp, wm = rates(D, magic)
        self.wp, self.wm = R(wp), R(wm)
        wv = np.full((X, Y), np.nan) if wall_value is None else np.asarray(wall_value, dtype=np.float64)
        self.dl, self.tv = [None] * 9, [None] * 9
        for k in range(1, 9):
            src_solid = w._pull(self.mask, k)
            src_val = w._pull(np.where(self.mask, wv, np.nan), k)
            inside = w.bounce[k] & src_solid
            # (a source outside a side that is not periodic bounces adiabatically: bounce[k] without a solid source inside the lattice)
            out = np.zeros((X, Y), bool)
            xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
            sx, sy = xs - int(on.CX[k]), ys + int(on.CY[k])
            if not w.px:
                out |= (sx < 0) | (sx >= X)
            if not w.py:
                out |= (sy < 0) | (sy >= Y)
            self.dl[k] = inside & ~out & ~np.isnan(src_val) & ~self.mask
            self.tv[k] = ((2.0 * WEIGHT[k]) * np.where(self.dl[k], src_val, 0.0)).astype(R)
        c0 = np.broadcast_to(np.asarray(c0, dtype=np.float64), (X, Y)).astype(R)
        self.g = np.stack([R(WEIGHT[k]) * c0 for k in range(9)])      # arriving populations
        self.g[:, self.mask] = R(0)
        self.gpost = None
        self.C = ((((((((self.g[0] + self.g[1]) + self.g[2]) + self.g[3]) + self.g[4]) + self.g[5]) + self.g[6]) + self.g[7]) + self.g[8])

    def step(self, n=1):
        w = self.w
        for _ in range(n):
            # the flow step, with the C the last scalar step summed
            rho, ux, uy = w.op.macros(w.fin)
            fpost = w.op.collide(w.fin, rho, on.equ(rho, ux, uy, w.t))
            fl = ~self.mask
            if self.on:
                t = self.C[fl] - self.c_ref
                F = w.drive if w.drive is not None else [self.R(0.0)] * 9
                for k in range(1, 9):
                    fpost[k][fl] = fpost[k][fl] + (F[k] + self.B[k] * t)
            elif w.drive is not None:
                for k in range(1, 9):
                    fpost[k][fl] = fpost[k][fl] + w.drive[k]
            fin = np.empty_like(fpost)
            for k in range(9):
                fin[k] = np.where(w.bounce[k], fpost[BOUNCE[k]], w._pull(fpost[k], k))
            if not w.py:
                from bounce_back_ref import lid_term
                tl = lid_term(rho[:, 0], w.op.par(w.op.uLB), self.R)
                fin[8, :, 0] = fin[8, :, 0] + tl
                fin[7, :, 0] = fin[7, :, 0] - tl
            fin[:, self.mask] = w.t[:, None]
            w.fin, w.rho, w.u = fin, rho, np.stack([ux, uy])
            w.nsteps += 1
            # the scalar step, with the velocity of the state the flow step produced
            _, vx, vy = w.op.macros(w.fin)
            with np.errstate(all="ignore"):
                gpost, C = scalar_collide(self.g, vx, vy, self.wp, self.wm, self.R)
            gpost[:, self.mask] = self.R(0)
            g = np.empty_like(gpost)
            g[0] = gpost[0]
            for k in range(1, 9):
                own = gpost[OPP[k]]
                a = np.where(w.bounce[k], own, w._pull(gpost[k], k))
                g[k] = np.where(self.dl[k], self.tv[k] - own, a)
            g[:, self.mask] = self.R(0)
            self.g, self.gpost, self.C = g, gpost, np.where(self.mask, self.R(0), C)
        return self
