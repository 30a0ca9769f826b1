"""A CPU stand-in for CavitySolver with obstacles and their bodies, as far as mrt_gpu.run_cavity uses them (A TEST DOUBLE; the product
has no CPU stepper): FrontEndStandIn of tests/front_end_standin.py stepping the reference of tests/solid_ref.py, plus solid=...,
bodies=..., solid_force and the force series, whose samples are solid.host_body_force of the reference's populations at the step
counts the library's schedule names (n0 + every, n0 + 2 every, ...: the lattice after that many steps)."""
import numpy as np

import front_end_standin as FS
from latticeboltzmannsimulations_amd import solid
from solid_ref import SolidOracle

KEYS = ("step", "body", "links", "fx", "fy", "tz")


class _ForceTap:
    """The reference, stepping in pieces that end where a force sample is due."""

    def __init__(self, oracle, owner):
        self._o, self._owner = oracle, owner

    def __getattr__(self, name):
        return getattr(self._o, name)

    def step(self, n=1):
        left = int(n)
        while left:
            f = self._owner._force
            k = left if not (f and f["every"]) else min(left, f["every"] - (self._o.nsteps - f["n0"]) % f["every"])
            self._o.step(k)
            left -= k
            if f and f["every"] and (self._o.nsteps - f["n0"]) % f["every"] == 0:
                self._owner._sample(self._o.nsteps)
        return self


def make():
    """A fresh stand-in class with its own journal."""
    class BodyStandIn(FS.standin()):
        source = "solid"

        def __init__(self, xsize, ysize, Re, solid=None, bodies=None, **kw):
            self.mask, self._force = np.asarray(solid) != 0, None
            self.labels = np.where(self.mask, 0 if bodies is None else np.asarray(bodies), -1)
            self.nbodies = int(self.labels.max()) + 1
            FS.SOURCES["solid"] = lambda X, Y, R, k: SolidOracle(X, Y, R, mask=self.mask, uLB=k["uLB"], collision=k["RT"], dtype=np.float64)
            super().__init__(xsize, ysize, Re, **kw)
            self.o = _ForceTap(self.o, self)
            self._note("bodies", None if bodies is None else self.nbodies)

        def solid_force(self):
            self._note("solid_force", self.steps_done)
            F = self.o.force()
            return dict(step=self.steps_done, links=F["links"], fx=F["fx"], fy=F["fy"])

        def body_force_at(self, n):
            F = solid.host_body_force(self.o.fin, self.mask, self.labels, solid.centroids(self.mask, self.labels, self.nbodies))
            return dict(F, step=np.full(self.nbodies, n), body=np.arange(self.nbodies))

        def _sample(self, n):
            f = self._force
            if len(f["records"]) < f["capacity"]:
                f["records"].append(self.body_force_at(n))
            else:
                f["dropped"] += 1

        def begin_force(self, every=0, capacity=1024):
            assert self.o.nsteps > 0, "LBM_ERR_STATE before the first step"
            self._note("begin_force", self.o.nsteps, int(every), int(capacity))
            self._force = dict(n0=self.o.nsteps, every=int(every), capacity=int(capacity), records=[], dropped=0)
            return self

        def force_series(self):
            self._note("force_series")
            recs = self._force["records"]
            out = {k: np.array([r[k] for r in recs]).reshape(len(recs), self.nbodies) for k in KEYS}
            out["count"], out["dropped"] = len(recs), self._force["dropped"]
            return out
    return BodyStandIn
