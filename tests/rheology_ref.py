"""CPU reference of the rheology table of the obstacle lattices (lbm_set_rheology; TEST HELPER).

The references of the obstacle toolkit (tests/solid_ref.py ... tests/periodic_ref.py, imported, never edited), constructed with turb = 0,
with one more piece: a table omega[n] (and optionally omegam[n], TRT's odd rate) over the shear g, and g_max.  While a table is set every
collision takes, per cell, from the populations f the step starts from and the moments rho, ux, uy its collision takes,

    jx = rho ux                      jy = rho uy
    a  = ((f1 + f3) - (f2 + f4)) - (jx ux - jy uy)
    b  = (((f5 - f6) + f7) - f8) - jx uy
    N  = sqrt(0.5 (a a) + 2 (b b))
    g  = N / rho
    s  = g * inv_dg                  inv_dg = (n - 1) / g_max in double, rounded once
    sc = fmax(fmin(s, n - 1), 0)
    i  = min((int) sc, n - 2)        fr = sc - i
    w_nu = t[i] + fr * d[i]          w_m = tm[i] + fr * dm[i]

every operation in the lattice type, rounded once, in the order written: rheology_rates of csrc/lbm_device.hpp, restated.  t[i] is omega[i]
rounded once to the lattice type, d[i] = t[i + 1] - t[i] formed in the lattice type, d[n - 1] = 0.  w_nu goes into collide(..., w_nu) of the
oracle, where its closure's rate goes; w_m reaches TRT's odd rate the way tests/viscosity_ref.py hands its plane over.  No history.
peek_tau() is what lbm_get_tau returns -- 1 / w_nu of the step that starts from the current state, the lattice's tau0 on solid and hold
cells -- and peek_shear() what lbm_get_shear returns, 0 on those cells.
"""
import numpy as np

from periodic_ref import PeriodicOracle
from solid_ref import SolidOracle


class RheologyMixin:
    rheo = None      # (t, d, tm or None, dm or None, n, inv_dg, g_max)
    last_index = None      # the interval of every cell in the most recent evaluation, and the clamped place sc
    last_sc = None

    def set_rheology(self, omega=None, omegam=None, g_max=None):
        """No geometry and no history: the state and the step count stay.  None clears the table."""
        if omega is None:
            assert omegam is None
            self.rheo = None
            return self
        omega = np.asarray(omega, dtype=np.float64)
        n = omega.size
        assert omega.ndim == 1 and 2 <= n <= 65536 and np.isfinite(g_max) and g_max > 0.0
        assert omegam is None or self.coll == "TRT"
        parts = []
        for a in (omega, omegam):
            if a is None:
                parts += [None, None]
                continue
            a = np.asarray(a, dtype=np.float64)
            assert a.shape == (n,) and np.isfinite(a).all() and (a > 0.0).all() and (a < 2.0).all()
            t = np.array([self.par(float(v)) for v in a], dtype=self.dtype)
            d = np.zeros(n, dtype=self.dtype)
            d[:-1] = t[1:] - t[:-1]
            parts += [t, d]
        self.rheo = (*parts, n, self.par((n - 1) / float(g_max)), float(g_max))
        return self

    def lattice_tau0(self):
        return self.R(1.0) / self.par(self.relax["omega"])

    def _pinned(self):
        p = self.mask.copy()
        if getattr(self, "hold", None) is not None:
            p |= self.hold
        return p

    def shear_of(self, f, rho, ux, uy):
        R = self.R
        jx, jy = rho * ux, rho * uy
        a = ((f[1] + f[3]) - (f[2] + f[4])) - (jx * ux - jy * uy)
        b = (((f[5] - f[6]) + f[7]) - f[8]) - jx * uy
        n = np.sqrt(R(0.5) * (a * a) + R(2) * (b * b))
        return n / rho

    def rates_of(self, f):
        """(g, w_nu, w_m or None) of every cell, whatever it holds; the index is asserted to lie in the table for every input."""
        R = self.R
        t, d, tm, dm, n, inv_dg, _ = self.rheo
        rho, ux, uy = self.macros(f)
        with np.errstate(all="ignore"):      # (a hold cell, or a lost lattice, may hold anything)
            g = self.shear_of(f, rho, ux, uy)
            s = g * inv_dg
            sc = np.fmax(np.fmin(s, R(n - 1)), R(0))
        assert np.isfinite(sc).all() and (sc >= 0).all() and (sc <= n - 1).all()
        i = np.minimum(sc.astype(np.int64), n - 2)
        assert (i >= 0).all() and (i <= n - 2).all()
        fr = sc - i.astype(self.dtype)
        assert (fr >= 0).all() and (fr <= 1).all()
        self.last_index, self.last_sc = i, sc
        w_nu = t[i] + fr * d[i]
        w_m = None if tm is None else tm[i] + fr * dm[i]
        return g, w_nu, w_m

    def peek_shear(self):
        rho, ux, uy = self.macros(self.fin)
        with np.errstate(all="ignore"):
            g = self.shear_of(self.fin, rho, ux, uy)
        g = np.array(g, dtype=self.dtype)
        g[self._pinned()] = 0
        return g

    def peek_tau(self):
        tau = np.full((self.nx, self.ny), self.lattice_tau0(), dtype=self.dtype)
        if self.rheo is not None:
            _, w_nu, _ = self.rates_of(self.fin)
            free = ~self._pinned()
            tau[free] = (self.R(1.0) / w_nu)[free]
        return tau

    def collide(self, f, rho, feq, w_nu=None):
        if self.rheo is None or w_nu is not None:
            return super().collide(f, rho, feq, w_nu)
        _, w_nu, w_m = self.rates_of(f)
        self.tau = self.R(1.0) / w_nu
        if w_m is None:
            return super().collide(f, rho, feq, w_nu)
        # the oracle's TRT reads its odd rate as par(relax["omegam"]): hand it the array (already in the lattice type) for this one call
        keep_rate, keep_par = self.relax["omegam"], self.par
        self.relax["omegam"] = w_m
        self.par = lambda v: v if isinstance(v, np.ndarray) else keep_par(v)
        try:
            return super().collide(f, rho, feq, w_nu)
        finally:
            self.relax["omegam"], self.par = keep_rate, keep_par


class RheologySolidOracle(RheologyMixin, SolidOracle):
    """SolidOracle with a rheology table: a mask at rest."""

    def __init__(self, nx, ny, Re, rheology=None, **kw):      # rheology: (omega, omegam or None, g_max)
        super().__init__(nx, ny, Re, turb=0, **kw)
        if rheology is not None:
            self.set_rheology(*rheology)


class RheologyOracle(RheologyMixin, PeriodicOracle):
    """PeriodicOracle -- bodies, motions, shapes, wall velocities, hold cells, periodic sides, the driving force -- with a rheology table."""

    def __init__(self, nx, ny, Re, rheology=None, **kw):
        super().__init__(nx, ny, Re, turb=0, **kw)
        if rheology is not None:
            self.set_rheology(*rheology)
