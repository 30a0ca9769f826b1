"""Natural convection on the bounce-back cavity: the scalar acts on the flow (CavitySolver.set_buoyancy).

With buoyancy (ax, ay, c_ref) every fluid cell is pushed by a (C - c_ref) per unit mass, C the transported scalar (begin_scalar): the
Boussinesq approximation at rho0 = 1.  Rows count from the lid, y = 0, and uy > 0 points toward it, so "up" is ay > 0: gravity points at
row Y - 1.  The forcing is the first-order one of the driving force: the exported u is the bare moment, and `velocity` adds the half-force
shift -- the bare moment of a hydrostatic state is not zero, its shifted velocity is.

    python -m latticeboltzmannsimulations_amd.convection cavity --n 32 --Ra 1e4
    python -m latticeboltzmannsimulations_amd.convection benard --h 24
"""
import argparse
import math
import sys

import numpy as np

from . import periodic as P

C_REF = 0.5             # the reference value of the runs: the mean of the two wall values
RA_CRITICAL = 1707.76   # linear theory, rigid-rigid plates (k_c = 3.117; k = pi at aspect 2 differs in the fifth digit)


# ---- numbers ----------------------------------------------------------------------------------------------------------------------------
def rayleigh(a, dC, H, nu, D):
    """Ra = a dC H^3 / (nu D): a the acceleration per unit of C, dC the difference of the wall values, H the distance of the walls."""
    return float(a) * float(dC) * float(H) ** 3 / (float(nu) * float(D))


def acceleration(Ra, dC, H, nu, D):
    """The inverse of rayleigh: a = Ra nu D / (dC H^3)."""
    return float(Ra) * float(nu) * float(D) / (float(dC) * float(H) ** 3)


def velocity(u, rho, C, a, c_ref=0.0, force=(0.0, 0.0)):
    """The physical velocity of the first-order forcing, u + (F + a (C - c_ref)) / (2 rho), from the exported u[2, X, Y], rho[X, Y] and
    C[X, Y] (solver.scalar(): the C of the same iteration), a = (ax, ay) and the driving force, if any."""
    u, rho, C = (np.asarray(v, dtype=np.float64) for v in (u, rho, C))
    a = np.asarray(a, dtype=np.float64).reshape(2, 1, 1)
    f = np.asarray(force, dtype=np.float64).reshape(2, 1, 1)
    return u + 0.5 * (f + a * (C - float(c_ref))[None]) / rho[None]


def nusselt(flux, D, dC, length, H):
    """The Nusselt number of a flat wall from the scalar it gives off per step (scalar_flux()['flux']): the mean flux density flux / length
    against the conductive one D dC / H."""
    return (float(flux) / float(length)) * float(H) / (float(D) * float(dC))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def heated_cavity(n):
    """An n x n fluid box inside a solid frame, [n + 2, n + 2]: dict(solid, labels, nbodies = 3, wall_value, periodic, H = n).  Column 0 is
    Dirichlet at 1 (body 0), column X - 1 Dirichlet at 0 (body 1), both with their corner cells; rows 0 and Y - 1 between them are adiabatic
    (body 2).  The solid row 0 hides the lid.  The walls lie half a cell outside the fluid cells."""
    n = int(n)
    if n < 2:
        raise ValueError("the cavity needs at least 2 x 2 fluid cells")
    N = n + 2
    m = np.ones((N, N), dtype=bool)
    m[1:-1, 1:-1] = False
    lab = np.full((N, N), -1, dtype=np.int32)
    lab[m] = 2
    lab[0, :], lab[-1, :] = 0, 1
    wv = np.full((N, N), np.nan)
    wv[0, :], wv[-1, :] = 1.0, 0.0
    return dict(solid=m, labels=lab, nbodies=3, wall_value=wv, periodic=(False, False), H=n)


def benard(h, aspect=2):
    """A layer of h fluid rows between two plates, aspect * h real columns wide and periodic in x, [aspect h + 2, h + 2]: dict(solid, labels,
    nbodies = 2, wall_value, periodic, H = h, L = aspect h, s [Y]: the distance of every row from the upper plate as a fraction of H).  Row
    Y - 1 (body 1) is Dirichlet at 1, row 0 (body 0, which hides the lid) Dirichlet at 0: heated from below."""
    h, L = int(h), int(aspect) * int(h)
    if h < 2 or L < 2:
        raise ValueError("the layer needs at least 2 rows and 2 columns")
    X, Y = L + 2, h + 2
    m = np.zeros((X, Y), dtype=bool)
    m[:, 0] = m[:, -1] = True
    lab = np.full((X, Y), -1, dtype=np.int32)
    lab[:, 0], lab[:, -1] = 0, 1
    wv = np.full((X, Y), np.nan)
    wv[:, 0], wv[:, -1] = 0.0, 1.0
    return dict(solid=m, labels=lab, nbodies=2, wall_value=wv, periodic=(True, False), H=h, L=L, s=(np.arange(Y) - 0.5) / h)


def benard_start(g, amplitude=1e-2):
    """The conductive profile C = s of a layer with the perturbation amplitude sin(pi s) cos(2 pi x / L) on it, [X, Y], images filled."""
    X = g["solid"].shape[0]
    x = (np.arange(X) - 1.0)[:, None]
    s = g["s"][None, :]
    c0 = s + float(amplitude) * np.sin(math.pi * s) * np.cos(2.0 * math.pi * x / g["L"])
    return P.wrap(np.where(g["solid"], 0.0, c0), True, False)


# ---- runs -------------------------------------------------------------------------------------------------------------------------------
def _solver(g, nu, D, c0, a, solver_factory, dtype, arith, device, magic=0.25):
    """A TRT solver at its default rates on the geometry g, its scalar begun and the buoyancy set (up: ay = a)."""
    nx, ny = g["solid"].shape
    s = P._factory(solver_factory)(nx, ny, P.solver_re(nu, ny), RT="TRT", semantics="bounce_back", dtype=dtype, arith=arith, device=device,
                                   solid=g["solid"], bodies=g["labels"])
    try:
        s.set_periodic(*g["periodic"])
        s.begin_scalar(D, c0, magic, wall_value=g["wall_value"])
        s.set_buoyancy(0.0, a, C_REF)
    except Exception:
        s.__exit__(None, None, None)
        raise
    return s


def _fields(s, a):
    """(shifted velocity [2, X, Y], C [X, Y]) of a solver, in double."""
    u, rho = s.get_fields(out_dtype=np.float64)[:2]
    C = s.scalar(out_dtype=np.float64)
    return velocity(u, rho, C, (0.0, a), C_REF), C


def run_heated_cavity(n=32, Ra=1e4, Pr=0.71, nu=0.05, steps=10000, dtype=np.float64, arith="strict", device=0, solver_factory=None, quiet=False):
    """The differentially heated square cavity of de Vahl Davis: hot wall at x = 0, cold wall opposite, adiabatic floor and ceiling.  Returns
    dict(Nu_hot, Nu_cold -- the Nusselt numbers of the two walls from their scalar flux, the cold one negative --, umax -- the largest
    horizontal velocity on the vertical mid-line --, vmax -- the largest vertical velocity on the horizontal mid-line, both of the shifted
    velocity at the cells (no interpolation; the mid-line of an even n is the mean of the two columns or rows beside it) in units of
    D / H --, a, D, u, C, steps)."""
    g = heated_cavity(n)
    H, D = float(g["H"]), float(nu) / float(Pr)
    a = acceleration(Ra, 1.0, H, nu, D)
    with _solver(g, nu, D, C_REF, a, solver_factory, dtype, arith, device) as s:
        s.step(int(steps))
        flux = s.scalar_flux()["flux"]
        u, C = _fields(s, a)
    N = n + 2
    mid = (slice(N // 2 - 1, N // 2 + 1) if n % 2 == 0 else slice(N // 2, N // 2 + 1))
    ux_mid = u[0][mid, 1:-1].mean(axis=0)      # along the vertical mid-line
    uy_mid = u[1][1:-1, mid].mean(axis=1)      # along the horizontal mid-line
    out = dict(Nu_hot=nusselt(flux[0], D, 1.0, H, H), Nu_cold=nusselt(flux[1], D, 1.0, H, H), umax=float(np.abs(ux_mid).max()) * H / D,
               vmax=float(np.abs(uy_mid).max()) * H / D, a=a, D=D, u=u, C=C, steps=int(steps))
    if not quiet:
        print(f"heated cavity {n} x {n}, Ra = {Ra:g}, Pr = {Pr:g}, nu = {nu:g}, {steps} steps: Nu = {out['Nu_hot']:.6g} (hot wall), "
              f"{out['Nu_cold']:.6g} (cold wall); umax = {out['umax']:.6g}, vmax = {out['vmax']:.6g} D / H")
    return out


def mode_amplitude(uy, g):
    """The first Fourier mode in x of uy[X, Y] projected on sin(pi s) over the real fluid cells of a layer: a complex number."""
    X = g["solid"].shape[0]
    x = np.arange(X) - 1.0
    w = np.exp(-2j * math.pi * x / g["L"])[1:-1, None] * np.sin(math.pi * g["s"])[None, 1:-1]
    return complex((uy[1:-1, 1:-1] * w).sum() * 4.0 / (g["L"] * g["H"]))


def growth_rate(steps, amplitude):
    """The slope of log |amplitude| against the step count over the second half of the series, by least squares."""
    t, y = np.asarray(steps, dtype=np.float64), np.log(np.abs(np.asarray(amplitude)))
    half = len(t) // 2
    return float(np.polyfit(t[half:], y[half:], 1)[0])


def run_benard(h=16, Ra=1770.0, Pr=1.0, nu=0.05, steps=None, every=None, aspect=2, amplitude=1e-2, dtype=np.float64, arith="strict", device=0,
               solver_factory=None, quiet=False):
    """A layer heated from below, started from the conductive profile with the perturbation of benard_start (amplitude = 0: none).  Returns
    dict(rate -- the growth rate per step of the first Fourier mode in x of the shifted uy, fitted over the second half of the series --,
    step, amplitude -- the series, one sample per `every` steps --, umax -- the largest shifted velocity at the end as a fraction of
    sqrt(a dC H) --, a, D, steps).  steps: by default 1.5625 H^2 / D; every: steps / 200."""
    g = benard(h, aspect)
    H, D = float(g["H"]), float(nu) / float(Pr)
    a = acceleration(Ra, 1.0, H, nu, D)
    steps = int(round(1.5625 * H * H / D)) if steps is None else int(steps)
    every = max(1, steps // 200) if every is None else max(1, int(every))
    at, amp = [], []
    with _solver(g, nu, D, benard_start(g, amplitude), a, solver_factory, dtype, arith, device) as s:
        done = 0
        while done < steps:
            k = min(every, steps - done)
            s.step(k)
            done += k
            u, _ = _fields(s, a)
            at.append(done)
            amp.append(mode_amplitude(u[1], g))
    fluid = ~g["solid"][1:-1, :]
    umax = float(np.sqrt(u[0] ** 2 + u[1] ** 2)[1:-1, :][fluid].max() / math.sqrt(a * H))
    rate = growth_rate(at, amp) if amplitude != 0.0 and len(at) >= 4 else float("nan")
    out = dict(rate=rate, step=np.array(at), amplitude=np.array(amp), umax=umax, a=a, D=D, steps=steps)
    if not quiet:
        print(f"Rayleigh-Benard {g['L']} x {h}, Ra = {Ra:g}, Pr = {Pr:g}, nu = {nu:g}, {steps} steps: growth rate {rate:.6e} per step "
              f"({rate * H * H / D:.6g} D / H^2), |u|max = {umax:.3e} sqrt(a dC H)")
    return out


def critical_rayleigh(h=16, Ra_lo=1650.0, Ra_hi=1770.0, quiet=False, **kw):
    """The Rayleigh number of zero growth, on the line through the growth rates at Ra_lo and Ra_hi.  Returns dict(Ra_c, error -- Ra_c /
    1707.76 - 1 --, rate_lo, rate_hi, slope -- d rate / d Ra x Ra_c H^2 / D; linear theory gives 13.0 at Pr = 1)."""
    lo = run_benard(h, Ra_lo, quiet=quiet, **kw)
    hi = run_benard(h, Ra_hi, quiet=quiet, **kw)
    slope = (hi["rate"] - lo["rate"]) / (float(Ra_hi) - float(Ra_lo))
    Ra_c = float(Ra_lo) - lo["rate"] / slope
    out = dict(Ra_c=Ra_c, error=Ra_c / RA_CRITICAL - 1.0, rate_lo=lo["rate"], rate_hi=hi["rate"], slope=slope * Ra_c * float(h) ** 2 / lo["D"])
    if not quiet:
        print(f"critical Rayleigh number at H = {h}: {Ra_c:.6g} ({100.0 * out['error']:+.3g} % of {RA_CRITICAL}); d rate / d Ra x Ra_c H^2 / D = "
              f"{out['slope']:.4g}")
    return out


def main(argv=None, solver_factory=None):
    ap = argparse.ArgumentParser(prog="python -m latticeboltzmannsimulations_amd.convection", description=__doc__.split("\n\n")[0])
    ap.add_argument("run", choices=("cavity", "benard"))
    ap.add_argument("--n", type=int, default=32, help="cavity: fluid cells per side")
    ap.add_argument("--h", type=int, default=16, help="benard: fluid rows between the plates")
    ap.add_argument("--Ra", type=float, default=None, help="cavity: the Rayleigh number (1e4); benard: one run at it instead of the pair")
    ap.add_argument("--Ra-lo", dest="Ra_lo", type=float, default=1650.0)
    ap.add_argument("--Ra-hi", dest="Ra_hi", type=float, default=1770.0)
    ap.add_argument("--Pr", type=float, default=None)
    ap.add_argument("--nu", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float64")
    ap.add_argument("--arith", choices=("strict", "fast"), default="strict")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    kw = dict(nu=a.nu, dtype=np.dtype(a.dtype).type, arith=a.arith, device=a.device, solver_factory=solver_factory)
    if a.run == "cavity":
        run_heated_cavity(a.n, 1e4 if a.Ra is None else a.Ra, 0.71 if a.Pr is None else a.Pr, steps=10000 if a.steps is None else a.steps, **kw)
    elif a.Ra is not None:
        run_benard(a.h, a.Ra, 1.0 if a.Pr is None else a.Pr, steps=a.steps, **kw)
    else:
        critical_rayleigh(a.h, a.Ra_lo, a.Ra_hi, Pr=1.0 if a.Pr is None else a.Pr, steps=a.steps, **kw)
    return 0


if __name__ == "__main__":
    sys.exit(main())
