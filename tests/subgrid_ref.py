"""CPU reference of the sub-grid closure of the obstacle lattices (lbm_set_subgrid; TEST HELPER).

The references of the obstacle toolkit (tests/solid_ref.py ... tests/periodic_ref.py, imported, never edited), constructed with turb = 0,
with one more piece: a constant cs2.  While it is positive every collision takes, per cell, the rate 1 / tau of

    Sxx = ((((f1 + f3) + f5) + f6) + f7) + f8      Syy = ((((f2 + f4) + f5) + f6) + f7) + f8      Sxy = ((f5 - f6) + f7) - f8
    Pxx = Sxx - (rho (1/3) + (rho ux) ux)          Pyy = Syy - (rho (1/3) + (rho uy) uy)          Pxy = Sxy - (rho ux) uy
    N   = sqrt((Pxx Pxx + 2 (Pxy Pxy)) + Pyy Pyy)
    tau = 0.5 (tau0 + sqrt(tau0 tau0 + (k N) / rho)),    tau0 = 1 / omega,    k = (18 sqrt(2)) cs2 in double, rounded once

f the populations the step starts from, rho, ux, uy the moments its collision takes -- every operation in the lattice type, rounded once,
in the order written: subgrid_tau of csrc/lbm_device.hpp, restated.  The rate goes into collide(..., w_nu) of the oracle, where its own
closure's rate goes: SRT's omega, TRT's omega+, MRT's omega_nu.  No history.  `tau` is the field of the last step; peek_tau() the one the
next step would use, which is what lbm_get_tau returns (solid cells and hold cells, which no step updates: tau0).
"""
import math

import numpy as np

from periodic_ref import PeriodicOracle
from solid_ref import SolidOracle


def subgrid_k(cs2):
    """k in double, in the order of the operations the library states."""
    return (18.0 * math.sqrt(2.0)) * float(cs2)


class SubgridMixin:
    cs2 = 0.0

    def set_subgrid(self, cs2=0.025):
        """No geometry and no history: the state and the step count stay."""
        assert np.isfinite(cs2) and cs2 >= 0.0
        self.cs2 = float(cs2)
        return self

    def tau0(self):
        return self.R(1.0) / self.par(self.relax["omega"])

    def subgrid_tau(self, f, rho, ux, uy):
        R = self.R
        tau0, k = self.tau0(), self.par(subgrid_k(self.cs2))
        sxx = ((((f[1] + f[3]) + f[5]) + f[6]) + f[7]) + f[8]
        syy = ((((f[2] + f[4]) + f[5]) + f[6]) + f[7]) + f[8]
        sxy = ((f[5] - f[6]) + f[7]) - f[8]
        r3, jx = rho * R(1.0 / 3), rho * ux
        pxx = sxx - (r3 + jx * ux)
        pyy = syy - (r3 + (rho * uy) * uy)
        pxy = sxy - jx * uy
        n = np.sqrt((pxx * pxx + R(2) * (pxy * pxy)) + pyy * pyy)
        return R(0.5) * (tau0 + np.sqrt(tau0 * tau0 + (k * n) / rho))

    def _tau_of(self, f):
        rho, ux, uy = self.macros(f)
        with np.errstate(all="ignore"):      # (a hold cell may hold anything; its tau is never used)
            tau = self.subgrid_tau(f, rho, ux, uy)
        tau[self.mask] = self.tau0()
        if getattr(self, "hold", None) is not None:
            tau[self.hold] = self.tau0()
        return tau

    def peek_tau(self):
        """tau of the step that starts from the current state; the constant without the closure."""
        if not self.cs2 > 0.0:
            return np.full((self.nx, self.ny), self.tau0(), dtype=self.dtype)
        return self._tau_of(self.fin)

    def collide(self, f, rho, feq, w_nu=None):
        if self.cs2 > 0.0 and w_nu is None:
            self.tau = self._tau_of(f)
            w_nu = self.R(1.0) / self.tau
        return super().collide(f, rho, feq, w_nu)


class SubgridSolidOracle(SubgridMixin, SolidOracle):
    """SolidOracle with the closure: a mask at rest."""

    def __init__(self, nx, ny, Re, cs2=0.0, **kw):
        super().__init__(nx, ny, Re, turb=0, **kw)
        self.set_subgrid(cs2)


class SubgridOracle(SubgridMixin, PeriodicOracle):
    """PeriodicOracle -- bodies, motions, shapes, wall velocities, hold cells, periodic sides, the driving force -- with the closure."""

    def __init__(self, nx, ny, Re, cs2=0.0, **kw):
        super().__init__(nx, ny, Re, turb=0, **kw)
        self.set_subgrid(cs2)
