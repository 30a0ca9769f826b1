"""CPU stand-in for CavitySolver as far as the front ends use it with a rheology table (TEST DOUBLE; the product has no CPU stepper): the
stand-in of tests/subgrid_standin.py with the reference of tests/rheology_ref.py behind it -- set_rheology, rheology, get_shear on top of
get_tau, step, get_fields, mean_u, solid_force, and the set_relaxation, set_periodic and set_driving_force that the periodic channel
calls.  Every call is journalled on the class."""
import numpy as np

from rheology_ref import RheologyOracle
from subgrid_standin import SubgridSolver


class RheologySolver(SubgridSolver):
    journal = []

    def __init__(self, xsize, ysize, Re, RT="MRT", **kw):
        super().__init__(xsize, ysize, Re, RT=RT, **kw)
        self.o = RheologyOracle(xsize, ysize, Re, uLB=self.uLB, mask=self.o.mask, collision=RT, dtype=self.dtype.type)

    def set_relaxation(self, **kw):
        self._note("set_relaxation", kw)
        self.relax.update(kw)
        self.o.relax.update(kw)
        return self

    def set_periodic(self, x=False, y=False):
        self._note("set_periodic", bool(x), bool(y))
        self.o.set_periodic(x, y)
        return self

    def set_driving_force(self, fx, fy):
        self._note("set_driving_force", float(fx), float(fy))
        self.o.set_driving_force(fx, fy)
        return self

    def set_subgrid(self, cs2=0.025):
        raise RuntimeError("lbm_set_subgrid failed (-4): a rheology table is set")

    def set_rheology(self, omega, omegam=None, g_max=None):
        self._note("set_rheology", None if omega is None else np.array(omega), None if omegam is None else np.array(omegam), g_max)
        if omegam is not None and self.RT != "TRT":
            raise RuntimeError("lbm_set_rheology failed (-4): omegam is TRT's odd rate and this context's collision is not TRT")
        self.o.set_rheology(omega, omegam, g_max)
        return self

    @property
    def rheology(self):
        if self.o.rheo is None:
            return None
        t, _, tm, _, _, _, g_max = self.o.rheo
        return t.astype(np.float64), (None if tm is None else tm.astype(np.float64)), g_max

    def get_tau(self, out_dtype=None):
        self._note("get_tau")
        return self.o.peek_tau().astype(self.dtype if out_dtype is None else np.dtype(out_dtype))

    def get_shear(self, out_dtype=None):
        self._note("get_shear")
        return self.o.peek_shear().astype(self.dtype if out_dtype is None else np.dtype(out_dtype))
