"""CPU reference of curved obstacle surfaces in the bounce-back cavity (lbm_set_solid_shape; TEST HELPER).

MovingWallOracle (tests/moving_wall_ref.py, imported, never edited) whose links carry a wall distance: q[8, X, Y], plane k - 1 for slot
k, on every link the fraction of the link from the fluid cell P = (x, y) to the wall, towards the source (x - cx_k, y + cy_k).  Per link,
in Python floats (double, every operation rounded once, none fused), with N = (x + cx_k, y - cy_k):

    near = q < 1/2 and N is a fluid cell inside the lattice;  q < 1/2 without such a cell: q = 1/2
    a = 2 q if near else 1 / (2 q)
    rx = (x - q cx_k) - x0;   ry = (y + q cy_k) - y0
    uwx = Ux + Om ry;  uwy = Uy + Om rx;  delta = (6 w_k) (cx_k uwx + cy_k uwy)
    d = delta if near else a delta

a and d rounded once to the lattice type.  One step: SolidOracle's (the stores carry no term), then on every link, in the lattice type,

    own = fpost_opp(k)(P);  other = fpost_opp(k)(N) if near else fpost_k(P)
    fin_k(P) = own + d                       where a == 1
             = (a own + (1 - a) other) + d   elsewhere.

The rule sits on the read side: a motion set after n steps shows in the populations arriving for step n + 1, so set_motion streams the
last post-collision state again.  The force on a link is c_opp(k) (f_out + f_in), f_out = fpost_opp(k)(P), f_in = fin_k(P), both
converted to double; the arm of the torque is (rx, ry).  Without a shape (set_shape(None)) it is MovingWallOracle, operation for operation.

It restates the rule on its own loops over the link list; the links of a step are applied as arrays, so that 6000 steps at 48 x 48 stay
near ten seconds.
"""
import math

import numpy as np

from bounce_back_ref import BOUNCE
from moving_wall_ref import W6, MovingWallOracle
from oracle import lbm_numpy as on
from solid_ref import SolidOracle


def link_figures(x, y, k, q, next_fluid, centre, motion):
    """dict(q, near, a, d, rx, ry) of one link in double."""
    cx, cy = float(on.CX[k]), float(on.CY[k])
    q = float(q)
    near = q < 0.5 and next_fluid
    if q < 0.5 and not next_fluid:
        q = 0.5
    a = 2.0 * q if near else 1.0 / (2.0 * q)
    rx = (float(x) - q * cx) - float(centre[0])
    ry = (float(y) + q * cy) - float(centre[1])
    uwx = float(motion[0]) + float(motion[2]) * ry
    uwy = float(motion[1]) + float(motion[2]) * rx
    delta = W6[k] * (cx * uwx + cy * uwy)
    return dict(q=q, near=near, a=a, d=delta if near else a * delta, rx=rx, ry=ry)


class CurvedWallOracle(MovingWallOracle):
    def __init__(self, nx, ny, Re, mask=None, labels=None, centres=None, motion=None, q=None, **kw):
        self.q = None
        self._streamed = False
        super().__init__(nx, ny, Re, mask=mask, labels=labels, centres=centres, motion=None, **kw)
        self.set_shape(q)
        self.set_motion(motion)

    # -- state ------------------------------------------------------------------------------------------------------------------------
    def set_state(self, fin):
        super().set_state(fin)
        self._streamed = False          # (plain populations: nothing to stream again)

    def step(self, n=1):
        super().step(n)
        self._streamed = n > 0 or self._streamed
        return self

    def set_solid(self, mask):
        self.q = None
        return super().set_solid(mask)

    def set_shape(self, q=None):
        """q[8, X, Y] or None.  Only with every body at rest, as the library; neither the state nor the step count changes."""
        assert not np.any(self.motion), "the shape first, then the motion"
        self.q = None if q is None else np.array(q, dtype=np.float64)
        self._build()
        return self

    def set_motion(self, motion=None):
        super().set_motion(motion)
        if getattr(self, "q", None) is not None:
            self._build()
            if self._streamed:          # the read side: the arriving populations carry the new term at once
                self.fin = self.stream_bb(self.fpost, self.rho)
        return self

    def _build(self):
        if self.q is None:
            return
        X, Y = self.nx, self.ny
        figs = []
        for x, y, k, b in self.links:
            fx, fy = x + int(on.CX[k]), y - int(on.CY[k])
            nf = 0 <= fx < X and 0 <= fy < Y and not self.mask[fx, fy]
            v = float(self.q[k - 1, x, y])
            assert math.isfinite(v) and 0.0 < v <= 1.0, (x, y, k, v)
            figs.append(link_figures(x, y, k, v, nf, self.centres[b], self.motion[b]))
        self.figs = figs
        L = np.array(self.links, dtype=np.int64).reshape(-1, 4)
        self.lx, self.ly, self.lk, self.lb = L[:, 0], L[:, 1], L[:, 2], L[:, 3]
        self.lo = np.array(BOUNCE)[self.lk]
        self.lnx, self.lny = self.lx + on.CX[self.lk].astype(np.int64), self.ly - on.CY[self.lk].astype(np.int64)
        self.l_near = np.array([f["near"] for f in figs], dtype=bool)
        # (the fallback keeps N out of reach where it is no cell; clip for the gather of the unused branch)
        self.lnx, self.lny = np.clip(self.lnx, 0, X - 1), np.clip(self.lny, 0, Y - 1)
        self.l_a = np.array([self.par(f["a"]) for f in figs], dtype=self.R)
        self.l_d = np.array([self.par(f["d"]) for f in figs], dtype=self.R)
        self.l_q = np.array([f["q"] for f in figs])
        self.q_eff = np.zeros((8, X, Y))
        self.q_eff[self.lk - 1, self.lx, self.ly] = self.l_q

    # -- the rule -----------------------------------------------------------------------------------------------------------------------
    def stream_bb(self, fpost, rho):
        if self.q is None:
            return super().stream_bb(fpost, rho)
        fin = SolidOracle.stream_bb(self, fpost, rho)
        if len(self.links):
            own = fpost[self.lo, self.lx, self.ly]
            other = np.where(self.l_near, fpost[self.lo, self.lnx, self.lny], fpost[self.lk, self.lx, self.ly])
            a, d = self.l_a, self.l_d
            t1 = a * own
            b = self.R(1.0) - a
            t2 = b * other
            fin[self.lk, self.lx, self.ly] = np.where(a == self.R(1.0), own + d, (t1 + t2) + d)
        return fin

    # -- the force ----------------------------------------------------------------------------------------------------------------------
    def _terms(self):
        """per link (tx, ty, tz) in double, of the state after the last step."""
        assert self._streamed
        out = []
        for i, (x, y, k, b) in enumerate(self.links):
            o = BOUNCE[k]
            t = float(self.fpost[o, x, y]) + float(self.fin[k, x, y])
            tx, ty = float(on.CX[o]) * t, float(on.CY[o]) * t
            out.append((tx, ty, self.figs[i]["rx"] * ty + self.figs[i]["ry"] * tx))
        return out

    def body_force(self):
        if self.q is None:
            return super().body_force()
        n = self.nbodies
        T = [dict(tx=[], ty=[], tz=[]) for _ in range(n)]
        for (x, y, k, b), (tx, ty, tz) in zip(self.links, self._terms()):
            T[b]["tx"].append(tx); T[b]["ty"].append(ty); T[b]["tz"].append(tz)
        out = dict(links=np.array([len(t["tx"]) for t in T]))
        for key, name in (("tx", "fx"), ("ty", "fy"), ("tz", "tz")):
            out[name] = np.array([math.fsum(t[key]) for t in T])
            out["abs_" + name[-1]] = np.array([math.fsum(abs(v) for v in t[key]) for t in T])
        return out

    def force(self):
        if self.q is None:
            return super().force()
        T = self._terms()
        tx, ty = [t[0] for t in T], [t[1] for t in T]
        return dict(links=len(tx), fx=math.fsum(tx), fy=math.fsum(ty), abs_x=math.fsum(abs(v) for v in tx), abs_y=math.fsum(abs(v) for v in ty))


# ---- Taylor-Couette at any resolution: body_cases.tc_case scaled --------------------------------------------------------
TC_UW = 0.05


def tc_scaled(scale=1):
    """The Taylor-Couette case of body_cases at `scale` times its resolution: N = 48 scale, radii 6.2 scale and 20.6 scale about
    (N - 1) / 2, wall speed Om R1 = 0.05, nu = 1/6 (Re = 0.08 N 6).  scale = 1 is body_cases.tc_case(), value for value.  q: the exact
    fractions of both circles."""
    N, R1, R2 = 48 * scale, 6.2 * scale, 20.6 * scale
    C = (N - 1) / 2.0
    xs, ys = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    r = np.hypot(xs - C, ys - C)
    mask = (r < R1) | (r > R2)
    Om = TC_UW / R1
    return dict(N=N, C=C, R1=R1, R2=R2, Re=0.08 * N * 6, mask=mask, labels=np.where(r < R1, 0, 1).astype(np.int32), centres=[[C, C], [C, C]],
                motion=[[0.0, 0.0, Om], [0.0, 0.0, 0.0]], r=r, xs=xs, ys=ys, Om=Om)


def circle_fractions(mask, C, radii):
    """q[8, X, Y] on its own loops: for every link the fraction t in (0, 1] at which P + t (S - P) meets one of the circles about (C, C)
    -- the one the link's two ends lie on different sides of; 1/2 where there is none."""
    X, Y = mask.shape
    q = np.full((8, X, Y), 0.5)
    for x in range(X):
        for y in range(Y):
            if mask[x, y]:
                continue
            for k in range(1, 9):
                sx, sy = x - int(on.CX[k]), y + int(on.CY[k])
                if not (0 <= sx < X and 0 <= sy < Y and mask[sx, sy]):
                    continue
                px, py, ex, ey = x - C, y - C, float(sx - x), float(sy - y)
                for R in radii:
                    ip, isrc = math.hypot(px, py) < R, math.hypot(sx - C, sy - C) < R
                    if ip == isrc:
                        continue
                    A, B, Cq = ex * ex + ey * ey, px * ex + py * ey, px * px + py * py - R * R
                    root = math.sqrt(max(B * B - A * Cq, 0.0))
                    t = (-B + root) / A if ip else (-B - root) / A
                    q[k - 1, x, y] = min(max(t, 2.0 ** -20), 1.0)
    return q


def tc_errors_scaled(u, tz, case):
    """body_cases.tc_errors for a case of tc_scaled: (torque errors of both bodies, profile error as a fraction of the wall speed), the
    profile over R1 + 1.5 < r < R2 - 1.5 (a band of cells, as body_cases.tc_errors: it reaches closer to the walls as the lattice is
    refined)."""
    R1, R2, Om, r, C = case["R1"], case["R2"], case["Om"], case["r"], case["C"]
    band = 1.5
    T = 4.0 * math.pi * (1.0 / 6.0) * Om * R1 ** 2 * R2 ** 2 / (R2 ** 2 - R1 ** 2)
    A, B = -Om * R1 ** 2 / (R2 ** 2 - R1 ** 2), Om * R1 ** 2 * R2 ** 2 / (R2 ** 2 - R1 ** 2)
    sel = (r > R1 + band) & (r < R2 - band)
    ut = ((case["ys"] - C) * u[0] + (case["xs"] - C) * u[1]) / r
    return (abs(tz[0] / -T - 1.0), abs(tz[1] / T - 1.0)), float(np.abs(ut - (A * r + B / r))[sel].max() / TC_UW)


# What this reference measured once on tc_scaled(1) with the exact fractions of both circles, fp64, TRT, 6000 steps:
# |tz / closed form - 1| of the two bodies (1.721349e-2 and 1.721342e-2), the profile error as a fraction of the wall speed, and the
# relative change of the fluid mass -- the interpolated rule does not conserve it.  At rest the annulus, which the ring closes off from
# the lid, never leaves the rest state and its mass stays to the last bit.  The tests assert TCQ_FACTOR times these and nothing wider.
TCQ_TORQUE_ERR, TCQ_PROFILE_ERR, TCQ_MASS_DRIFT, TCQ_MASS_DRIFT_AT_REST = 0.0172135, 0.0173845, 5.32613e-3, 0.0
TCQ_FACTOR = 2.0
