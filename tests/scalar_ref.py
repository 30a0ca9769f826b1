"""CPU reference of the passive scalar (lbm_scalar_*; TEST HELPER): an independent NumPy restatement of the rule include/lbm.h states, in
the lattice dtype, every operation elementwise and rounded once, in the spelled order.

ScalarOracle keeps what the device lattice keeps -- the STORED populations: post-collision values (plain ones while raw), zeros on solid
cells, the constants of the user's hold cells, and on the image cells of periodic sides the nine stored values of their partners,
refreshed after every step and upload.  step(ux, uy) takes the velocity the device reads for that step: the moments of the flow state
that the flow step of the same iteration has just produced -- what get_fields() exports after the NEXT step.  Arrays are [X, Y]; slot k
of cell (x, y) pulls from (x - CX[k], y + CY[k]), y = 0 is the lid row.

RollScalar (the second restatement: no image cells, the real cells alone, pushed with np.roll) lives in tests/test_scalar_cpu.py.
"""
import numpy as np

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
WEIGHT = (4.0 / 9.0,) + (1.0 / 9.0,) * 4 + (1.0 / 36.0,) * 4
OPP = (0, 3, 4, 1, 2, 7, 8, 5, 6)
PAIRS = ((1, 3), (2, 4), (5, 7), (6, 8))


def rates(D, magic):
    """(w+, w-) in double, the order of the contract."""
    tm = 3.0 * float(D) + 0.5
    tp = float(magic) / (tm - 0.5) + 0.5
    return 1.0 / tp, 1.0 / tm


def cu_of(k, ux, uy):
    """c_k . u as the flow spells it."""
    return {1: ux, 2: uy, 5: ux + uy, 6: -ux + uy}[k]


def collide(g, ux, uy, wp, wm, R):
    """The TRT collision of the contract on arrays g[9, ...] of dtype R; returns (out, C)."""
    w = [R(v) for v in WEIGHT]
    half, three = R(0.5), R(3.0)
    C = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8])
    out = np.empty_like(g)
    out[0] = g[0] - (g[0] - C * w[0]) * wp
    for a, b in PAIRS:
        cu = cu_of(a, ux, uy)
        gp = (g[a] + g[b]) * half
        gm = (g[a] - g[b]) * half
        e = C * w[a]
        dp = (gp - e) * wp
        dm = (gm - (e * three) * cu) * wm
        out[a] = (g[a] - dp) - dm
        out[b] = (g[b] - dp) + dm
    return out, C


def hold_values(f, Ch):
    """The nine doubles a user's hold cell keeps, from the flow populations f it holds (the contract's order)."""
    f = [float(v) for v in f]
    rho = ((((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8])
    ux = (((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]) / rho
    uy = (((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]) / rho
    return [(WEIGHT[k] * float(Ch)) * (1.0 + 3.0 * (float(CX[k]) * ux + float(CY[k]) * uy)) for k in range(9)]


def partner(i, n, periodic):
    return i if not periodic else (n - 2 if i == 0 else (1 if i == n - 1 else i))


class ScalarOracle:
    def __init__(self, mask, D, c0=0.0, dtype=np.float32, magic=0.25, wall_value=None, hold=None, hold_f=None, hold_value=None,
                 periodic=(False, False), param_dtype=None):
        """param_dtype (as CavityOracle's; default: dtype, or float64 when dtype is long double) is the lattice type the device runs
        in: the rates, the Dirichlet table, the held constants and the initial c0 are rounded once to it, then widened exactly."""
        self.R = np.dtype(dtype).type
        R = self.R
        P = np.dtype(param_dtype if param_dtype is not None else (np.float64 if np.dtype(dtype) == np.longdouble else dtype)).type
        self.par = lambda v: R(P(v))      # a parameter as the device holds it, in the arithmetic type
        self.mask = np.asarray(mask) != 0
        X, Y = self.X, self.Y = self.mask.shape
        self.per = (bool(periodic[0]), bool(periodic[1]))
        wp, wm = rates(D, magic)
        self.wp, self.wm = self.par(wp), self.par(wm)
        xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
        self.img = (self.per[0] & ((xs == 0) | (xs == X - 1))) | (self.per[1] & ((ys == 0) | (ys == Y - 1)))
        self.uhold = np.zeros((X, Y), bool) if hold is None else (np.asarray(hold) != 0)
        assert not (self.uhold & (self.mask | self.img)).any()
        self.hold = self.uhold | (self.img & ~self.mask)
        self.ix, self.iy = np.nonzero(self.img)
        self.ipx = np.array([partner(int(x), X, self.per[0]) for x in self.ix], dtype=np.int64)
        self.ipy = np.array([partner(int(y), Y, self.per[1]) for y in self.iy], dtype=np.int64)
        c0 = np.broadcast_to(np.asarray(c0, dtype=np.float64), (X, Y))
        # the wall values of the Dirichlet cells, NaN elsewhere
        wv = np.full((X, Y), np.nan) if wall_value is None else np.asarray(wall_value, dtype=np.float64)
        self.dirichlet = self.mask & ~np.isnan(wv)
        # per slot: the source lies outside; the source is a solid cell (the link bits of a cell that is neither solid nor held); the
        # link's table value t = 2 w_k Cw rounded once, where the source is a Dirichlet cell
        self.outside, self.link, self.dlink, self.t = [None] * 9, [None] * 9, [None] * 9, [None] * 9
        free = ~self.mask & ~self.hold
        for k in range(1, 9):
            sx, sy = xs - CX[k], ys + CY[k]
            out = (sx < 0) | (sx >= X) | (sy < 0) | (sy >= Y)
            sxc, syc = np.clip(sx, 0, X - 1), np.clip(sy, 0, Y - 1)
            self.outside[k] = out & free
            self.link[k] = ~out & self.mask[sxc, syc] & free
            self.dlink[k] = self.link[k] & self.dirichlet[sxc, syc]
            self.t[k] = ((2.0 * WEIGHT[k]) * np.where(self.dlink[k], wv[sxc, syc], 0.0)).astype(P).astype(R)
        # the constants of the user's hold cells, rounded once
        self.held = np.zeros((9, X, Y), dtype=R)
        hv = c0 if hold_value is None else np.broadcast_to(np.asarray(hold_value, dtype=np.float64), (X, Y))
        for x, y in zip(*np.nonzero(self.uhold)):
            self.held[:, x, y] = np.array(hold_values(np.asarray(hold_f, dtype=np.float64)[:, x, y], hv[x, y])).astype(P).astype(R)
        c0r = c0.astype(P).astype(R)
        self.set_state(np.stack([R(WEIGHT[k]) * c0r for k in range(9)]))

    # -- what the lattice stores -----------------------------------------------------------------------------------------------------
    def _pin(self, s):
        s[:, self.mask] = self.R(0)
        s[:, self.uhold] = self.held[:, self.uhold]
        s[:, self.ix, self.iy] = s[:, self.ipx, self.ipy]
        return s

    def set_state(self, g):
        """Plain populations; the next step is raw."""
        self.s = self._pin(np.array(g, dtype=self.R))
        self.raw = True
        self.prev = None
        self.nsteps = 0
        return self

    def _gather(self, s, raw):
        """The arriving populations of every cell from the stored lattice s."""
        if raw:
            return s.copy()
        g = np.empty_like(s)
        g[0] = s[0]
        for k in range(1, 9):
            pulled = np.roll(s[k], (CX[k], -CY[k]), axis=(0, 1))      # s_k(x - cx, y + cy); wrapped values only where `outside`
            own = s[OPP[k]]
            a = np.where(self.outside[k] | self.link[k], own, pulled)
            g[k] = np.where(self.dlink[k], self.t[k] - own, a)
        g[:, self.hold] = s[:, self.hold]
        g[:, self.mask] = self.R(0)
        return g

    def populations(self, stored=False):
        return self.s.copy() if stored else self._gather(self.s, self.raw)

    def conc(self):
        """C of the state the last step started from (before the first: of the state as set), as lbm_scalar_get returns it."""
        g = self._gather(*self.prev) if self.prev is not None else self._gather(self.s, self.raw)
        return ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8])

    def step(self, ux, uy):
        R = self.R
        ux, uy = np.asarray(ux), np.asarray(uy)
        assert ux.dtype == np.dtype(R) and uy.dtype == np.dtype(R), "the velocity comes in the lattice type"
        g = self._gather(self.s, self.raw)
        with np.errstate(all="ignore"):
            out, _ = collide(g, ux, uy, self.wp, self.wm, R)
        self.prev = (self.s, self.raw)
        self.s = self._pin(out)
        self.raw = False
        self.nsteps += 1
        return self

    def flux_terms(self):
        """(g_k - own) of every link in double, as lbm_scalar_flux forms them: dict k -> array [X, Y], zero off the links."""
        assert not self.raw
        out = {}
        for k in range(1, 9):
            own = self.s[OPP[k]]
            gk = np.where(self.dlink[k], self.t[k] - own, own)
            out[k] = np.where(self.link[k], gk.astype(np.float64) - own.astype(np.float64), 0.0)
        return out
