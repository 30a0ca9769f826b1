"""CPU reference of the relaxation field of the obstacle lattices (lbm_set_relaxation_field; TEST HELPER).

The references of the obstacle toolkit (tests/solid_ref.py ... tests/periodic_ref.py, tests/subgrid_ref.py, imported, never edited) with
one more piece: omega[X, Y], the viscous rate of each cell, and optionally omegam[X, Y], TRT's odd rate of each cell, each rounded once
to the lattice type.  While a field is set every collision takes, per cell,

    w_nu = omega of the cell                 (SRT's omega, TRT's omega+, MRT's omega_nu; MRT's other rates stay the lattice's)
    w_m  = omegam of the cell                (TRT; without that plane the lattice's)

the same operations of the oracle's collide() on an array per rate where it has a scalar.  With the closure (SubgridMixin) tau0 of
subgrid_tau is 1 / omega of the cell, one division in the lattice type.  peek_tau() is what lbm_get_tau returns: the tau of the step that
starts from the current state -- 1 / omega of the cell, or the closure's value on it -- and the lattice's tau0 on solid and hold cells.
"""
import numpy as np

from periodic_ref import PeriodicOracle
from solid_ref import SolidOracle
from subgrid_ref import SubgridMixin


class ViscosityMixin:
    """Goes in front of SubgridMixin (or of the oracle itself) in the bases."""
    w_field = None
    wm_field = None

    def set_relaxation_field(self, omega=None, omegam=None):
        """No geometry and no history: the state and the step count stay.  None clears the field."""
        if omega is None:
            assert omegam is None
            self.w_field = self.wm_field = None
            return self
        for a in (omega, omegam):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                assert a.shape == (self.nx, self.ny) and np.isfinite(a).all() and (a > 0.0).all() and (a < 2.0).all()
        assert omegam is None or self.coll == "TRT"
        self.w_field = self._rounded(omega)
        self.wm_field = None if omegam is None else self._rounded(omegam)
        return self

    def _rounded(self, a):
        """A parameter array as the device holds it (par of the oracle, element by element)."""
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=self.dtype)
        flat, src = out.reshape(-1), a.reshape(-1)
        for i in range(src.size):
            flat[i] = self.par(float(src[i]))
        return out

    def lattice_tau0(self):
        return self.R(1.0) / self.par(self.relax["omega"])

    def tau0(self):
        """The closure's tau0: per cell with a field."""
        return self.lattice_tau0() if self.w_field is None else self.R(1.0) / self.w_field

    def _pinned(self):
        p = self.mask.copy()
        if getattr(self, "hold", None) is not None:
            p |= self.hold
        return p

    def _tau_of(self, f):
        rho, ux, uy = self.macros(f)
        with np.errstate(all="ignore"):      # (a hold cell may hold anything; its tau is never used)
            tau = self.subgrid_tau(f, rho, ux, uy)
        tau[self._pinned()] = self.lattice_tau0()
        return tau

    def peek_tau(self):
        if getattr(self, "cs2", 0.0) > 0.0:
            return self._tau_of(self.fin)
        tau = np.full((self.nx, self.ny), self.lattice_tau0(), dtype=self.dtype)
        if self.w_field is not None:
            tau = (self.R(1.0) / self.w_field).astype(self.dtype)
            tau[self._pinned()] = self.lattice_tau0()
        return tau

    def collide(self, f, rho, feq, w_nu=None):
        if self.w_field is None:
            return super().collide(f, rho, feq, w_nu)
        if w_nu is None:
            if getattr(self, "cs2", 0.0) > 0.0:
                self.tau = self._tau_of(f)
                w_nu = self.R(1.0) / self.tau
            else:
                w_nu = self.w_field
        if self.wm_field is None:
            return super().collide(f, rho, feq, w_nu)
        # the oracle's TRT reads its odd rate as par(relax["omegam"]): hand it the plane (already rounded) for this one call
        keep_rate, keep_par = self.relax["omegam"], self.par
        self.relax["omegam"] = self.wm_field
        self.par = lambda v: v if isinstance(v, np.ndarray) else keep_par(v)
        try:
            return super().collide(f, rho, feq, w_nu)
        finally:
            self.relax["omegam"], self.par = keep_rate, keep_par


class ViscositySolidOracle(ViscosityMixin, SubgridMixin, SolidOracle):
    """SolidOracle with a relaxation field and, cs2 > 0, the closure: a mask at rest."""

    def __init__(self, nx, ny, Re, omega_field=None, omegam_field=None, cs2=0.0, **kw):      # (omegam=...: the lattice's uniform odd rate, the oracle's own)
        super().__init__(nx, ny, Re, turb=0, **kw)
        self.set_subgrid(cs2)
        self.set_relaxation_field(omega_field, omegam_field)


class ViscosityOracle(ViscosityMixin, SubgridMixin, PeriodicOracle):
    """PeriodicOracle -- bodies, motions, shapes, wall velocities, hold cells, periodic sides, the driving force -- with a field and,
    cs2 > 0, the closure."""

    def __init__(self, nx, ny, Re, omega_field=None, omegam_field=None, cs2=0.0, **kw):      # (omegam=...: the lattice's uniform odd rate, the oracle's own)
        super().__init__(nx, ny, Re, turb=0, **kw)
        self.set_subgrid(cs2)
        self.set_relaxation_field(omega_field, omegam_field)
