"""What the two front ends (mrt_gpu.run_cavity, datagen.generate) share: the two stop rules, each as an object that is asked once per
check, and the checks of the arguments that select the wall model and the stop rule."""
from . import residual as RS


class MeanUStop:
    """The reference's rule (MRT_GPU.py:883-889, MRT_GPU_datagen.py:862-871): |mean(u) - mean(u) at the previous check| / uLB < tolerance
    is a hit, consecutive or not, and the `hits`-th hit ends the run.  The arithmetic is done on the values as they are handed in --
    NumPy float32 scalars keep float32's rounding, Python floats double's --, so which check stops a run depends on the caller's type."""

    def __init__(self, uLB, tolerance, hits=6):
        self.uLB, self.tolerance, self.hits = uLB, tolerance, hits
        self.past, self.count = 0, 0

    def update(self, mean):
        """True when this check completes the run."""
        hit = abs(mean - self.past) / self.uLB < self.tolerance
        self.past = mean
        self.count += bool(hit)
        return bool(hit) and self.count >= self.hits


class ResidualStop:
    """The field-residual rule: the relative L2 change of u per step (residual.norms) below `tol` at `hits` consecutive checks."""

    def __init__(self, uLB, tol, hits=1):
        self.uLB, self.tol, self.hits, self.count = uLB, float(tol), int(hits), 0

    def update(self, record):
        """(value, done) for the residual record of this check."""
        value = RS.norms(record, self.uLB)["rel_l2_per_step"]
        self.count = self.count + 1 if RS.below(value, self.tol) else 0
        return value, self.count >= self.hits


def wall_model(BC, semantics, turb, solid=False, solid_tiles=False):
    """The semantics the wall model BC selects: 'EB-NEBB ' keeps `semantics`, 'BB' is 'bounce_back' (without the closure).  solid: the
    run has solid obstacles, which exist with the bounce-back walls only.  solid_tiles: it asks for the multi-step tile kernel of a
    lattice with obstacles (tuning=dict(solid_tiles=True)), which needs some."""
    bc = BC.strip()
    if bc not in ("EB-NEBB", "BB"):
        raise ValueError("BC must be 'EB-NEBB ' or 'BB'")
    if solid_tiles and not solid:
        raise ValueError("solid_tiles selects the multi-step tile kernel for a lattice with solid obstacles: it needs solid=... (a mask)")
    if solid and bc != "BB":
        raise ValueError("solid obstacles need the bounce-back walls: pass BC='BB' (and turb=0)")
    if bc == "BB":
        if semantics not in ("mrt_gpu", "bounce_back"):
            raise ValueError(f"BC='BB' selects semantics='bounce_back', not {semantics!r}")
        if turb:
            raise ValueError("BC='BB' runs without the Smagorinsky closure: pass turb=0")
        return "bounce_back"
    if semantics == "bounce_back":
        raise ValueError("semantics='bounce_back' is BC='BB'")
    return semantics


def subgrid_constant(subgrid, BC, solid_tiles=False):
    """The sub-grid constant of a run (CavitySolver.set_subgrid), or None: a finite number > 0 (None and 0: no closure), with the
    bounce-back walls, one step per launch."""
    if subgrid is None:
        return None
    cs2 = float(subgrid)
    if not (cs2 >= 0.0 and cs2 != float("inf")):
        raise ValueError("subgrid must be a finite constant >= 0 (Cs^2 of the local Smagorinsky closure; the reference's is 0.025)")
    if cs2 == 0.0:
        return None
    if BC.strip() != "BB":
        raise ValueError("subgrid is the closure of the bounce-back and obstacle lattices: pass BC='BB' (the wet-node walls have turb=1)")
    if solid_tiles:
        raise ValueError("subgrid needs one step per launch: the tile kernel (solid_tiles) has no closure")
    return cs2


def by_residual(criterion, residual_tol, residual_hits=1):
    """True for criterion='residual' (False for 'mean_u'), with its arguments checked."""
    if criterion not in ("mean_u", "residual"):
        raise ValueError("criterion must be 'mean_u' or 'residual'")
    if criterion == "mean_u":
        return False
    if residual_tol is None or not float(residual_tol) > 0.0:
        raise ValueError("criterion='residual' needs an explicit residual_tol > 0 (the noise floor depends on dtype and lattice size)")
    if int(residual_hits) < 1:
        raise ValueError("residual_hits must be >= 1")
    return True
