"""Periodic, force-driven flows on the bounce-back cavity (CavitySolver.set_periodic, set_driving_force).

A periodic side is a pair of image columns (rows): with x, columns 0 and X - 1 of every [X, Y] array are images of columns X - 2 and 1,
and the periodic domain is columns 1 .. X - 2.  `wrap` fills the images of any array -- the mask, the labels, a wall velocity, each plane
of the wall distances, a state -- and `interior` cuts them off an export.  The driving force is the first-order one: the exported u is
the bare moment, and `velocity` adds the half-force shift.

    python -m latticeboltzmannsimulations_amd.periodic poiseuille --xsize 6 --ysize 18 --nu 0.1 --force 1e-6
    python -m latticeboltzmannsimulations_amd.periodic array --xsize 34 --ysize 34 --radius 6 --curved
"""
import argparse
import math
import sys

import numpy as np

from . import solid as S

MAGIC = 3.0 / 16.0      # the TRT product at which the half-way wall of a force-driven channel sits exactly half-way


def wrap(a, x=False, y=False):
    """A copy of a[..., X, Y] whose image columns (x) and rows (y) hold their partners' values: column 0 <- X - 2, X - 1 <- 1, then the
    rows likewise, so that with both the corners hold the diagonally opposite real cells."""
    a = np.array(a)
    if x:
        if a.shape[-2] < 4:
            raise ValueError("a periodic direction needs at least 4 cells")
        a[..., 0, :] = a[..., -2, :]
        a[..., -1, :] = a[..., 1, :]
    if y:
        if a.shape[-1] < 4:
            raise ValueError("a periodic direction needs at least 4 cells")
        a[..., :, 0] = a[..., :, -2]
        a[..., :, -1] = a[..., :, 1]
    return a


def interior(a, x=False, y=False):
    """a[..., X, Y] without its image columns (x) and rows (y): a view."""
    a = np.asarray(a)
    return a[..., slice(1, -1) if x else slice(None), slice(1, -1) if y else slice(None)]


def velocity(u, rho, force):
    """The physical velocity of the first-order forcing: (sum c f + F / 2) / rho = u + F / (2 rho), from the exported u[..., 2, X, Y] and
    rho[..., X, Y] and force = (fx, fy)."""
    u, rho = np.asarray(u, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    f = np.asarray(force, dtype=np.float64).reshape(2, 1, 1)
    return u + 0.5 * f / rho[..., None, :, :]


def trt_omegam(omega, magic=MAGIC):
    """The odd rate of TRT for the product `magic` = (1 / omega - 1/2) (1 / omegam - 1/2)."""
    return 1.0 / (0.5 + float(magic) / (1.0 / float(omega) - 0.5))


def solver_re(nu, ny, uLB=0.08):
    """The solver's Re for a viscosity: it derives nu = uLB ysize / Re."""
    return float(uLB) * float(ny) / float(nu)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def poiseuille(nx, ny):
    """A channel along x, periodic in x: dict(solid [X, Y] with the rows 0 and Y - 1 solid, periodic=(True, False), H = Y - 2, and y [Y],
    the distance of every row from the wall half-way between rows 0 and 1)."""
    nx, ny = int(nx), int(ny)
    if nx < 4 or ny < 3:
        raise ValueError("a periodic channel needs at least 4 x 3 cells")
    m = np.zeros((nx, ny), dtype=bool)
    m[:, 0] = m[:, ny - 1] = True
    return dict(solid=m, periodic=(True, False), H=ny - 2, y=np.arange(ny, dtype=np.float64) - 0.5)


def poiseuille_profile(ny, nu, force):
    """ux[Y] of the steady channel at rho = 1: F / (2 nu) s (H - s), s the distance from the wall; zero on the wall rows."""
    g = poiseuille(4, ny)
    u = float(force) / (2.0 * float(nu)) * g["y"] * (g["H"] - g["y"])
    u[0] = u[-1] = 0.0
    return u


def disc_array(nx, ny, r, curved=False):
    """One cell of a doubly periodic array of discs: dict(solid [X, Y], labels, nbodies = 1, periodic=(True, True), disc=(x0, y0, r)), the
    disc in the middle of the real cells 1 .. X - 2, 1 .. Y - 2, and with curved=True `shape` [8, X, Y], the exact wall distances of the
    disc's links (solid.disc_fractions), 1/2 elsewhere.  The disc must keep two cells from the seam."""
    nx, ny = int(nx), int(ny)
    x0, y0 = (nx - 1) / 2.0, (ny - 1) / 2.0
    if not 0 < r or x0 - r < 3 or y0 - r < 3:
        raise ValueError("the disc must keep two real cells between itself and the image cells")
    m, lab, n = S.discs_into(nx, ny, [(x0, y0, r)])
    m = wrap(m, True, True)
    out = dict(solid=m, labels=np.where(m, 0, -1).astype(np.int32), nbodies=n, periodic=(True, True), disc=(x0, y0, float(r)))
    if curved:
        out["shape"] = wrap(S.disc_fractions(m, x0, y0, float(r)), True, True)
    return out


def taylor_green(n, u0):
    """The Taylor-Green vortex on n x n real cells, doubly periodic: dict(solid [n + 2, n + 2] (all fluid), periodic=(True, True), k = 2 pi /
    n, u [2, X, Y], rho [X, Y], fin [9, X, Y] -- the equilibrium of ux = u0 cos(k i) sin(k j), uy = u0 sin(k i) cos(k j), rho = 1 - (3 u0^2 /
    4) (cos 2 k i + cos 2 k j), i, j the real cell's indices, images filled).  Its kinetic energy decays as exp(-4 nu k^2 t)."""
    n = int(n)
    N = n + 2
    k = 2.0 * math.pi / n
    i, j = np.meshgrid(np.arange(N) - 1.0, np.arange(N) - 1.0, indexing="ij")
    ux, uy = u0 * np.cos(k * i) * np.sin(k * j), u0 * np.sin(k * i) * np.cos(k * j)
    rho = 1.0 - 0.75 * u0 * u0 * (np.cos(2.0 * k * i) + np.cos(2.0 * k * j))
    u, rho = wrap(np.stack([ux, uy]), True, True), wrap(rho, True, True)
    return dict(solid=np.zeros((N, N), dtype=bool), periodic=(True, True), k=k, u0=float(u0), u=u, rho=rho, fin=S.equilibrium(rho, u[0], u[1]))


# ---- runs -------------------------------------------------------------------------------------------------------------------------------
def _factory(solver_factory):
    if solver_factory is None:
        from .solver import CavitySolver as solver_factory
    return solver_factory


def run_poiseuille(nx=6, ny=18, nu=0.1, force=1e-6, steps=20000, magic=MAGIC, dtype=np.float64, arith="strict", device=0, solver_factory=None,
                   quiet=False, rheology=None, output_every=None):
    """A force-driven channel, periodic in x, under TRT with the product `magic` (None: the solver's default).  Returns dict(error -- the
    largest deviation of the shifted velocity from F / (2 nu) s (H - s) over the fluid cells, as a fraction of its maximum --, umax,
    balance -- |wall force / (F fluid cells) - 1| --, u, rho, steps).
    rheology=(omega, omegam, g_max) or dict(law=..., g_max=..., entries=..., magic=...) (rheology.resolve): a generalised Newtonian fluid
    (CavitySolver.set_rheology) in the place of the one viscosity; nu then only sets the lattice's own rates, which solid cells report.
    The steps run in pieces of output_every (default: all at once), and after each piece one warning is printed if the largest shear
    exceeds g_max; the result gains g_top, the largest shear seen, and with rheology=dict(law=power_law(K, n), power=(K, n)) the error
    is against rheology.power_law_profile."""
    from . import rheology as RH
    g = poiseuille(nx, ny)
    Re = solver_re(nu, ny)
    with _factory(solver_factory)(nx, ny, Re, RT="TRT", semantics="bounce_back", dtype=dtype, arith=arith, device=device, solid=g["solid"]) as s:
        if magic is not None:
            s.set_relaxation(omegam=trt_omegam(s.relax["omega"], magic))
        s.set_periodic(*g["periodic"])
        s.set_driving_force(force, 0.0)
        g_max = RH.apply(s, rheology, "TRT") if rheology is not None else None
        g_top, left = 0.0, int(steps)
        while left > 0:
            n = left if not output_every else min(left, int(output_every))
            s.step(n)
            left -= n
            if g_max is not None:
                g_top = max(g_top, RH.over_range(s, g_max, (lambda *a: None) if quiet else print))
        u, rho = s.get_fields()[:2]
        wall = s.solid_force()
    out = poiseuille_figures(u, rho, wall["fx"], g, nu, force)
    out["steps"] = int(steps)
    if rheology is not None:
        out["g_top"] = g_top
        if isinstance(rheology, dict) and "power" in rheology:
            K, n = rheology["power"]
            exact = RH.power_law_profile(g["H"], K, n, force)
            ux = interior(velocity(u, rho, (force, 0.0))[0], True, False)[:, 1:-1]
            out.update(error=float(np.abs(ux - exact[None, :]).max() / exact.max()), umax=float(exact.max()))
    if not quiet:
        print(f"Poiseuille {nx} x {ny}, nu = {nu:g}, F = {force:g}, {steps} steps: profile error {out['error']:.3e} of umax = {out['umax']:.6e}, "
              f"force balance {out['balance']:.3e}")
    return out


def poiseuille_figures(u, rho, wall_fx, g, nu, force):
    """The figures of run_poiseuille from the exported u, rho and the x force on the walls."""
    px, py = g["periodic"]
    fluid = interior(~g["solid"], px, py)
    ux = interior(velocity(u, rho, (force, 0.0))[0], px, py)
    exact = poiseuille_profile(g["solid"].shape[1], nu, force)[None, :] * np.ones(ux.shape)
    umax = float(exact.max())
    return dict(error=float(np.abs(ux - exact)[fluid].max() / umax), umax=umax, u=u, rho=rho,
                balance=abs(float(wall_fx) / (float(force) * int(fluid.sum())) - 1.0))


def run_array(nx=34, ny=34, r=6.0, nu=0.1, force=1e-6, steps=20000, curved=False, RT="TRT", magic=MAGIC, dtype=np.float64, arith="strict", device=0,
              force_every=100, solver_factory=None, quiet=False):
    """Flow through a doubly periodic array of discs under a uniform force along x.  Returns dict(K -- the permeability nu ubar / F, ubar
    the mean of the shifted x velocity over all real cells, solid ones counting as zero --, drag -- the x force on the disc from the last
    sample of the force series --, balance -- |drag / (F fluid cells) - 1| --, ubar, series, steps)."""
    g = disc_array(nx, ny, r, curved)
    Re = solver_re(nu, ny)
    with _factory(solver_factory)(nx, ny, Re, RT=RT, semantics="bounce_back", dtype=dtype, arith=arith, device=device, solid=g["solid"],
                                  bodies=g["labels"]) as s:
        if RT == "TRT" and magic is not None:
            s.set_relaxation(omegam=trt_omegam(s.relax["omega"], magic))
        s.set_periodic(*g["periodic"])
        if curved:
            s.set_shape(g["shape"])
        s.set_driving_force(force, 0.0)
        every = max(1, int(force_every))
        s.step(1)
        s.begin_force(every=every, capacity=max(1, int(steps) // every + 1))
        s.step(int(steps) - 1)
        s.sample_force()
        series = s.force_series()
        s.end_force()
        u, rho = s.get_fields()[:2]
    fluid = interior(~g["solid"], True, True)
    ux = np.where(fluid, interior(velocity(u, rho, (force, 0.0))[0], True, True), 0.0)
    ubar = float(ux.mean())
    drag = float(series["fx"][-1][0])
    out = dict(K=float(nu) * ubar / float(force), drag=drag, balance=abs(drag / (float(force) * int(fluid.sum())) - 1.0), ubar=ubar, series=series,
               steps=int(steps))
    if not quiet:
        print(f"disc array {nx} x {ny}, r = {r:g}{' (curved)' if curved else ''}, nu = {nu:g}, F = {force:g}, {steps} steps: K = nu ubar / F = "
              f"{out['K']:.6g}, drag = {drag:.8g} (F x fluid cells: {force * int(fluid.sum()):.8g})")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m latticeboltzmannsimulations_amd.periodic", description=__doc__.split("\n\n")[0])
    ap.add_argument("run", choices=("poiseuille", "array"))
    ap.add_argument("--xsize", type=int, default=None)
    ap.add_argument("--ysize", type=int, default=None)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--force", type=float, default=1e-6)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--radius", type=float, default=6.0)
    ap.add_argument("--curved", action="store_true")
    ap.add_argument("--power-law", dest="power_law", type=float, nargs=2, metavar=("K", "N"), default=None,
                    help="poiseuille: a power-law fluid nu = K gdot^(N - 1) (clipped to [1e-3, 2]) through a rheology table")
    ap.add_argument("--g-max", dest="g_max", type=float, default=None, help="the shear of the table's last entry (default 0.1)")
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float64")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    dt = np.dtype(a.dtype).type
    if a.run == "poiseuille":
        rh = None
        if a.power_law is not None:
            from . import rheology as RH
            K, n = a.power_law
            rh = dict(law=RH.power_law(K, n), power=(K, n), g_max=RH.G_MAX_DEFAULT if a.g_max is None else a.g_max, magic=MAGIC)
        run_poiseuille(a.xsize or 6, a.ysize or 18, a.nu, a.force, a.steps, dtype=dt, device=a.device, rheology=rh)
    else:
        run_array(a.xsize or 34, a.ysize or 34, a.radius, a.nu, a.force, a.steps, a.curved, dtype=dt, device=a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
