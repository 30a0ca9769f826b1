"""CPU stand-in for CavitySolver as far as the front ends use it with a viscosity field (TEST DOUBLE; the product has no CPU stepper): the
stand-in of tests/subgrid_standin.py with the reference of tests/viscosity_ref.py behind it -- set_relaxation_field, set_viscosity,
relaxation_field on top of set_subgrid, get_tau, step, get_fields, mean_u, solid_force.  Every call is journalled on the class."""
import numpy as np

from latticeboltzmannsimulations_amd import viscosity
from subgrid_standin import SubgridSolver
from viscosity_ref import ViscositySolidOracle


class ViscositySolver(SubgridSolver):
    journal = []

    def __init__(self, xsize, ysize, Re, RT="MRT", **kw):
        super().__init__(xsize, ysize, Re, RT=RT, **kw)
        self.o = ViscositySolidOracle(xsize, ysize, Re, uLB=self.uLB, mask=self.o.mask, collision=RT, dtype=self.dtype.type)

    def set_relaxation_field(self, omega, omegam=None):
        self._note("set_relaxation_field", None if omega is None else np.array(omega), None if omegam is None else np.array(omegam))
        if omegam is not None and self.RT != "TRT":
            raise RuntimeError("lbm_set_relaxation_field failed (-4): omegam is TRT's odd rate and this context's collision is not TRT")
        self.o.set_relaxation_field(omega, omegam)
        return self

    def set_viscosity(self, nu, magic=None):
        self._note("set_viscosity", None if nu is None else np.array(nu), magic)
        if nu is None:
            self.o.set_relaxation_field(None)
            return self
        self.o.set_relaxation_field(*viscosity.rates(nu, magic))
        return self

    @property
    def relaxation_field(self):
        if self.o.w_field is None:
            return None
        return self.o.w_field.astype(np.float64), (None if self.o.wm_field is None else self.o.wm_field.astype(np.float64))
