"""CPU reference of the half-way bounce-back walls (semantics='bounce_back', LBM_SEM_BOUNCE_BACK; TEST HELPER).

Built on the oracle's operators (oracle.lbm_numpy: equilibrium and the three collision operators, the relaxation rates of
semantics='mrt_gpu', omega_eps = 1.2), which it reuses unmodified; what it restates is the wall model, in the operation order of
lbm_device.hpp (gather_a, lid_term, macros):

  * every lattice cell is a fluid cell: the moments are the plain sums, rho = sum f, u = j / rho, on every cell (no override);
  * one step: moments -> equilibrium -> collision -> streaming.  Slot k of cell (x, y) pulls fpost_k(x - cx_k, y + cy_k); a source
    outside [0, X) x [0, Y) gives fpost_opp(k)(x, y) instead (bounce = [0, 3, 4, 1, 2, 7, 8, 5, 6]), and a source row above the lid
    (y + cy_k < 0, the corner ghosts included) adds Ladd's term 6 w_k rho_w (c_k . u_lid) = cx_k * t with
    t = (rho_w * uLB) * R(1/6) -- +t to slot 8, -t to slot 7, nothing to slot 4 -- where rho_w is the density of the cell's moments
    in this same step (the value the device parks for the next gather);
  * the first step after an initialisation or a set_state streams nothing that came before it (the device's `raw` lattice): it
    needs no parked density.

The state is `fin` (the populations a step starts from), as CavityOracle's; `rho`, `u` are the moments of the last step.
"""
import numpy as np

from oracle import lbm_numpy as on

BOUNCE = [0, 3, 4, 1, 2, 7, 8, 5, 6]


def lid_term(rho_w, uLB, R):
    """Ladd's moving-lid term of the diagonals that come from beyond the lid: cx_k * t, t as lbm_device.hpp:lid_term."""
    return (rho_w * uLB) * R(1.0 / 6.0)


class BounceBackOracle(on.CavityOracle):
    def __init__(self, nx, ny, Re, uLB=0.08, collision="MRT", dtype=np.float64, **kw):
        super().__init__(nx, ny, Re, uLB=uLB, semantics="mrt_gpu", collision=collision, dtype=dtype, **kw)
        assert not self.turb and not self.promote, "bounce-back walls run without the closure and without promotion"
        self.sem = "bounce_back"
        X, Y = nx, ny
        xs, ys = np.arange(X)[:, None], np.arange(Y)[None, :]
        # per slot: source indices clipped into the lattice, and where the source lies outside it
        self._src, self._out = [], []
        for k in range(9):
            sx, sy = xs - int(on.CX[k]) + 0 * ys, ys + int(on.CY[k]) + 0 * xs
            out = (sx < 0) | (sx >= X) | (sy < 0) | (sy >= Y)
            self._src.append((np.clip(sx, 0, X - 1), np.clip(sy, 0, Y - 1)))
            self._out.append(out)

    def macros(self, f):
        """The plain moments, every cell (lbm_device.hpp:macros, SEM_BB)."""
        rho = ((((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8])
        ux = (((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]) / rho
        uy = (((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]) / rho
        return rho, ux, uy

    def stream_bb(self, fpost, rho):
        """The populations of the next step from the post-collision ones (lbm_device.hpp:gather_a, SEM_BB)."""
        fin = np.empty_like(fpost)
        for k in range(9):
            sx, sy = self._src[k]
            fin[k] = np.where(self._out[k], fpost[BOUNCE[k]], fpost[k][sx, sy])
        t = lid_term(rho[:, 0], self.par(self.uLB), self.R)
        fin[8, :, 0] = fin[8, :, 0] + t
        fin[7, :, 0] = fin[7, :, 0] - t
        return fin

    def step(self, n=1):
        for _ in range(n):
            rho, ux, uy = self.macros(self.fin)
            feq = on.equ(rho, ux, uy, self.t)
            fpost = self.collide(self.fin, rho, feq)
            self.fin = self.stream_bb(fpost, rho)
            self.rho, self.u = rho, np.stack([ux, uy])
            self.feq, self.fpost = feq, fpost
            self.nsteps += 1
        return self

    def mass(self):
        return float(np.sum(self.fin, dtype=np.float64))

    def stream(self, fin, fpost):       # (the wet-node streaming and wall rules of the base class do not apply)
        raise NotImplementedError("bounce-back streams in stream_bb")

    wall_bc = stream
