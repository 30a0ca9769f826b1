"""CPU reference of periodic sides and the uniform driving force in the bounce-back cavity (lbm_set_periodic, lbm_set_driving_force; TEST
HELPER).

PeriodicOracle is OpenFlowOracle (tests/open_flow_ref.py, imported, never edited) with the two pieces:

  * IMAGE CELLS.  With x, columns 0 and X - 1 are images of columns X - 2 and 1 (likewise y; both: the corners are images of the
    diagonally opposite real cells).  The mask and the labels must equal their own wrap.  An image cell whose partner is not solid is a
    hold cell: never updated, pulled from by the plain pull, no link starts at it, no fluid cell for the `near` test of a shape.  What it
    holds is refreshed after every step and after every state upload: the nine values the lattice STORES at its partner -- the partner's
    post-collision populations, with the driving force and (a motion without a shape) the delta the partner adds to its stored slot
    opp(k); after a state upload the partner's plain populations.  The image's neighbours then pull what they would pull across the seam.
  * THE DRIVING FORCE.  In Python floats (double, every operation rounded once, none fused) F_k = (3 w_k) (cx_k fx + cy_k fy), 3 w_k =
    1/3 (k <= 4) or 1/12, rounded once to the lattice type; every collision of a cell that is neither solid nor held is followed by
    fpost_k = fpost_k + F_k, one add in the lattice type, before everything a wall adds.

WrapOracle is the second, independent restatement: no image cells at all, the real cells alone, streamed with true wrap-around (np.roll
of the populations and of the mask).  It knows solid cells at rest and the force, which is what the image-cell reference is checked
against, bit for bit on the interior.
"""
import numpy as np

from bounce_back_ref import BOUNCE, BounceBackOracle, lid_term
from open_flow_ref import OpenFlowOracle
from oracle import lbm_numpy as on
from solid_ref import SolidOracle

W3 = [0.0] + [1.0 / 3.0] * 4 + [1.0 / 12.0] * 4


def drive_terms(fx, fy):
    """[F_0 .. F_8] in double, in the order of the operations the library states."""
    return [W3[k] * (float(on.CX[k]) * float(fx) + float(on.CY[k]) * float(fy)) for k in range(9)]


def partner(i, n, periodic):
    return i if not periodic else (n - 2 if i == 0 else (1 if i == n - 1 else i))


def wrap_own(a, px, py):
    """a[..., X, Y] with its image cells filled from their partners, on this file's own loops."""
    a = np.array(a)
    X, Y = a.shape[-2:]
    for x in range(X):
        for y in range(Y):
            sx, sy = partner(x, X, px), partner(y, Y, py)
            if (sx, sy) != (x, y):
                a[..., x, y] = a[..., sx, sy]
    return a


class PeriodicOracle(OpenFlowOracle):
    def __init__(self, nx, ny, Re, periodic=(False, False), force=(0.0, 0.0), q=None, wall_velocity=None, motion=None, **kw):
        self.img = None
        self.drive = None
        super().__init__(nx, ny, Re, **kw)
        self.set_periodic(*periodic)
        self.set_shape(q)
        self.set_wall_velocity(wall_velocity)
        self.set_motion(motion)
        self.set_driving_force(*force)

    # -- the driving force ----------------------------------------------------------------------------------------------------------------
    def set_driving_force(self, fx=0.0, fy=0.0):
        """No geometry: the state and the step count stay."""
        assert np.isfinite(fx) and np.isfinite(fy)
        self.force_xy = (float(fx), float(fy))
        self.drive = [self.par(v) for v in drive_terms(fx, fy)] if (fx != 0.0 or fy != 0.0) else None
        return self

    def collide(self, f, rho, feq, w_nu=None):
        out = super().collide(f, rho, feq, w_nu)
        if getattr(self, "drive", None) is not None:
            fl = self.fluid()
            for k in range(1, 9):
                out[k][fl] = out[k][fl] + self.drive[k]
        return out

    # -- the image cells --------------------------------------------------------------------------------------------------------------------
    def set_periodic(self, px=False, py=False):
        """Geometry comes first: no shape, no motion, no wall velocity.  The state restarts from the initial equilibrium."""
        assert self.q is None and not np.any(self.motion) and self.uw is None
        px, py = bool(px), bool(py)
        X, Y = self.nx, self.ny
        assert (not px or X >= 4) and (not py or Y >= 4)
        uh = getattr(self, "_uhold", None)
        self.per = (px, py)
        if not (px or py):
            self.img = None
            self.hold, self.held = uh, (None if uh is None else self._uheld)
        else:
            xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
            img = (px & ((xs == 0) | (xs == X - 1))) | (py & ((ys == 0) | (ys == Y - 1)))
            self.ix, self.iy = np.nonzero(img)
            self.ipx = np.array([partner(int(x), X, px) for x in self.ix])
            self.ipy = np.array([partner(int(y), Y, py) for y in self.iy])
            assert np.array_equal(self.mask[self.ix, self.iy], self.mask[self.ipx, self.ipy]), "the mask differs from its own wrap"
            lab = np.where(self.mask, self.labels, -1)
            assert np.array_equal(lab[self.ix, self.iy], lab[self.ipx, self.ipy]), "the labels differ from their own wrap"
            assert uh is None or not (uh & img).any(), "a user hold cell on an image cell"
            self.img = img
            self.hold = (img & ~self.mask) | (uh if uh is not None else False)
            assert (~self.hold & ~self.mask).any()
            self.held = np.zeros((9, int(self.hold.sum())), dtype=self.R)      # (filled by set_state below)
        self._drop_hold_links()
        self.set_motion(None)
        self.set_state(self._fin0)
        self.rho = np.ones((X, Y), dtype=self.dtype)
        self.u = np.zeros((2, X, Y), dtype=self.dtype)
        self.nsteps = 0
        return self

    def set_open_cells(self, hold=None, f=None):
        """The user's hold cells; the periodic sides stay."""
        per = getattr(self, "per", (False, False))
        self.img = None
        super().set_open_cells(hold, f)
        self._uhold, self._uheld = self.hold, self.held
        if any(per):
            self.set_periodic(*per)
        return self

    def set_solid(self, mask):
        self.img, self._uhold, self._uheld, self.per = None, None, None, (False, False)
        return super().set_solid(mask)

    def _stored(self, fpost):
        """What the lattice stores after a step: fpost, and on the links of a motion without a shape the delta on slot opp(k)."""
        if not (getattr(self, "moving", False) and self.q is None) or not self.links:
            return fpost
        st = fpost.copy()
        L = np.array(self.links, dtype=np.int64).reshape(-1, 4)
        x, y, k = L[:, 0], L[:, 1], L[:, 2]
        o = np.array(BOUNCE)[k]
        st[o, x, y] = st[o, x, y] + self.delta[k, x, y]      # (a link is one (cell, slot): no index repeats)
        return st

    def _refresh(self, f, stored):
        """The image cells of f from their partners in `stored`; then what the hold cells hold, from f."""
        if getattr(self, "img", None) is None:
            return
        if self._uhold is not None:
            f[:, self._uhold] = self._uheld
            if stored is not f:
                stored[:, self._uhold] = self._uheld
        f[:, self.ix, self.iy] = stored[:, self.ipx, self.ipy]
        self.held = f[:, self.hold].copy()

    def set_state(self, fin):
        super().set_state(fin)          # (pins the solid cells and whatever the hold cells held before)
        if getattr(self, "img", None) is not None:
            SolidOracle._pin(self, self.fin)
            self._refresh(self.fin, self.fin)

    def stream_bb(self, fpost, rho):
        if getattr(self, "img", None) is not None:
            self._refresh(fpost, self._stored(fpost))
        return super().stream_bb(fpost, rho)

    def real(self):
        """(slice x, slice y) of the real cells."""
        return (slice(1, -1) if self.per[0] else slice(None), slice(1, -1) if self.per[1] else slice(None))


class WrapOracle:
    """True wrap-around on the real cells alone: mask[X', Y'] of the periodic domain (no image cells), solid cells at rest, the force.
    ny_global: the row count the relaxation rates derive from (the full lattice's, images included)."""

    def __init__(self, mask, Re, periodic, ny_global, force=(0.0, 0.0), fin=None, **kw):
        self.mask = np.asarray(mask) != 0
        X, Y = self.mask.shape
        self.px, self.py = bool(periodic[0]), bool(periodic[1])
        self.op = BounceBackOracle(X, Y, Re, ny_global=ny_global, **kw)      # (the operators and the rates; its walls are never used)
        self.R, self.t = self.op.R, self.op.t
        self.drive = [self.op.par(v) for v in drive_terms(*force)] if any(v != 0.0 for v in force) else None
        self.fin = (self.op.fin if fin is None else np.asarray(fin, dtype=self.op.dtype)).copy()
        self.fin[:, self.mask] = self.t[:, None]
        self.bounce = []
        xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
        for k in range(9):
            sx, sy = xs - int(on.CX[k]), ys + int(on.CY[k])
            out = np.zeros((X, Y), dtype=bool)
            if not self.px:
                out |= (sx < 0) | (sx >= X)
            if not self.py:
                out |= (sy < 0) | (sy >= Y)
            self.bounce.append(out | self._pull(self.mask, k))
        self.bounce[0][:] = False
        self.nsteps = 0

    @staticmethod
    def _pull(a, k):
        """a(x - cx_k, y + cy_k) with wrap-around."""
        return np.roll(a, (int(on.CX[k]), -int(on.CY[k])), axis=(0, 1))

    def step(self, n=1):
        for _ in range(n):
            rho, ux, uy = self.op.macros(self.fin)
            fpost = self.op.collide(self.fin, rho, on.equ(rho, ux, uy, self.t))
            if self.drive is not None:
                fl = ~self.mask
                for k in range(1, 9):
                    fpost[k][fl] = fpost[k][fl] + self.drive[k]
            fin = np.empty_like(fpost)
            for k in range(9):
                fin[k] = np.where(self.bounce[k], fpost[BOUNCE[k]], self._pull(fpost[k], k))
            if not self.py:
                t = lid_term(rho[:, 0], self.op.par(self.op.uLB), self.R)
                fin[8, :, 0] = fin[8, :, 0] + t
                fin[7, :, 0] = fin[7, :, 0] - t
            fin[:, self.mask] = self.t[:, None]
            self.fin, self.rho, self.u = fin, rho, np.stack([ux, uy])
            self.nsteps += 1
        return self
