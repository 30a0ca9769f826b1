"""Shear-dependent viscosity on the obstacle lattices (CavitySolver.set_rheology): laws nu(gdot) of generalised Newtonian
fluids, the table of relaxation rates over the shear g that the device interpolates, and the closed form of the power-law channel.

The device knows g = |Pi| / rho of a cell, Pi the deviatoric non-equilibrium momentum flux (get_shear), without knowing tau.  The shear
rate is gdot = (3 / sqrt 2) g / tau, and tau = 1/2 + 3 nu(gdot) is what the law yields: so g = (sqrt 2 / 3) gdot (1/2 + 3 nu(gdot)), which
increases strictly in gdot wherever the stress nu(gdot) gdot does not fall.  table() inverts it once, on the host.

Everything is in lattice units, nu = (tau - 1/2) / 3.
"""
import numpy as np

MAGIC = 3.0 / 16.0      # the TRT product at which a half-way wall sits exactly half-way
_K = np.sqrt(2.0) / 3.0


def power_law(K, n, nu_min=1e-3, nu_max=2.0):
    """nu = K gdot^(n - 1), clipped to [nu_min, nu_max]: shear-thinning for n < 1, shear-thickening for n > 1."""
    K, n, nu_min, nu_max = float(K), float(n), float(nu_min), float(nu_max)
    if not (K > 0.0 and n > 0.0 and 0.0 < nu_min <= nu_max):
        raise ValueError("power_law needs K > 0, n > 0 and 0 < nu_min <= nu_max")

    def nu(gdot):
        gdot = np.asarray(gdot, dtype=np.float64)
        with np.errstate(divide="ignore", over="ignore"):
            v = K * np.power(gdot, n - 1.0)
        return np.clip(np.where(np.isnan(v), nu_max if n < 1.0 else nu_min, v), nu_min, nu_max)
    return nu


def carreau(nu0, nu_inf, lam, n, a=2.0):
    """Carreau-Yasuda: nu = nu_inf + (nu0 - nu_inf) (1 + (lam gdot)^a)^((n - 1) / a)."""
    nu0, nu_inf, lam, n, a = float(nu0), float(nu_inf), float(lam), float(n), float(a)
    if not (nu0 > 0.0 and nu_inf > 0.0 and lam > 0.0 and n > 0.0 and a > 0.0):
        raise ValueError("carreau needs positive nu0, nu_inf, lam, n and a")

    def nu(gdot):
        gdot = np.asarray(gdot, dtype=np.float64)
        return nu_inf + (nu0 - nu_inf) * np.power(1.0 + np.power(lam * gdot, a), (n - 1.0) / a)
    return nu


def bingham(nu_p, tau_y, m):
    """Papanastasiou's regularised Bingham fluid: nu = nu_p + tau_y (1 - exp(-m gdot)) / gdot (-> nu_p + tau_y m as gdot -> 0)."""
    nu_p, tau_y, m = float(nu_p), float(tau_y), float(m)
    if not (nu_p > 0.0 and tau_y >= 0.0 and m > 0.0):
        raise ValueError("bingham needs nu_p > 0, tau_y >= 0 and m > 0")

    def nu(gdot):
        gdot = np.asarray(gdot, dtype=np.float64)
        x = m * gdot
        small = x < 1e-8
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(small, m * (1.0 - 0.5 * x), -np.expm1(-x) / np.where(small, 1.0, gdot))
        return nu_p + tau_y * r
    return nu


def g_of(gdot, nu):
    """g = (sqrt 2 / 3) gdot (1/2 + 3 nu): the shear the device measures in a cell of shear rate gdot and viscosity nu."""
    return _K * np.asarray(gdot, dtype=np.float64) * (0.5 + 3.0 * np.asarray(nu, dtype=np.float64))


def shear_rate(g, tau):
    """gdot = (3 / sqrt 2) g / tau, from get_shear() and get_tau()."""
    return np.asarray(g, dtype=np.float64) / (_K * np.asarray(tau, dtype=np.float64))


def apparent_viscosity(tau):
    """nu = (tau - 1/2) / 3."""
    return (np.asarray(tau, dtype=np.float64) - 0.5) / 3.0


def table(law, entries=4096, g_max=None, magic=None, fine=200001):
    """(omega, omegam) for CavitySolver.set_rheology(omega, omegam, g_max): omega[i] = 1 / tau at g_i = i g_max / (entries - 1), tau = 1/2 +
    3 nu(gdot_i) with gdot_i the shear rate at which g_of(gdot, nu(gdot)) = g_i -- found by np.interp on a logarithmic grid of `fine` shear
    rates that reaches from far below the first interval to beyond g_max, then narrowed by bisection inside the grid's bracket on the law
    itself, so that every entry satisfies the implicit relation to rounding.  magic=L: omegam[i] = 1 / (L / (tau_i - 1/2) + 1/2), TRT's odd
    rate that keeps (tau+ - 1/2)(tau- - 1/2) = L in every entry; None without it.  ValueError: g(gdot) not strictly increasing on the grid
    (a law whose stress falls), or an omega outside (0, 2)."""
    entries = int(entries)
    if not 2 <= entries <= 65536:
        raise ValueError("a table has 2 to 65536 entries")
    if g_max is None or not (np.isfinite(g_max) and g_max > 0.0):
        raise ValueError("table needs g_max, finite and positive: the shear of the last entry")
    g_max = float(g_max)
    gs = np.linspace(0.0, g_max, entries)
    # every tau is > 1/2, so gdot < (3 / sqrt 2) g / (1/2): the grid's top; its bottom lies far below the first interval
    top = 2.0 * g_max / _K * 1.001
    gd = np.logspace(np.log10(top) - 14.0, np.log10(top), int(fine))
    nu = np.asarray(law(gd), dtype=np.float64)
    if nu.shape != gd.shape or not np.isfinite(nu).all() or not (nu > 0.0).all():
        raise ValueError("the law must give a finite viscosity > 0 for every shear rate")
    gg = g_of(gd, nu)
    if not (np.diff(gg) > 0.0).all():
        raise ValueError("g(gdot) = (sqrt 2 / 3) gdot (1/2 + 3 nu(gdot)) is not strictly increasing: the law's stress falls somewhere")
    if gg[-1] < g_max:
        raise ValueError("the shear-rate grid does not reach g_max (a viscosity below zero?)")
    gdot = np.interp(gs, gg, gd)
    gdot[0] = 0.0
    # polish: g(gdot) is monotone, so bisection inside the bracket the grid gives cannot leave it
    lo = np.interp(gs, gg, gd, left=0.0) * (1.0 - 1e-3)
    hi = gdot * (1.0 + 1e-3) + 1e-300

    def res(x):
        return g_of(x, law(np.maximum(x, 1e-300))) - gs
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        r = res(mid)
        lo = np.where(r <= 0.0, mid, lo)
        hi = np.where(r > 0.0, mid, hi)
    gdot = 0.5 * (lo + hi)
    gdot[0] = 0.0
    nu_i = np.asarray(law(np.maximum(gdot, 1e-300)), dtype=np.float64)
    nu_i[0] = float(np.asarray(law(np.array([gd[0]])))[0])      # (the zero-shear viscosity: the law's value at the bottom of the grid)
    tau = 0.5 + 3.0 * nu_i
    omega = 1.0 / tau
    if not (np.isfinite(omega).all() and (omega > 0.0).all() and (omega < 2.0).all()):
        raise ValueError("an omega of the table is not in (0, 2)")
    if magic is None:
        return omega, None
    if not (np.isfinite(magic) and magic > 0.0):
        raise ValueError("the magic parameter must be finite and > 0")
    omegam = 1.0 / (float(magic) / (tau - 0.5) + 0.5)
    if not (np.isfinite(omegam).all() and (omegam > 0.0).all() and (omegam < 2.0).all()):
        raise ValueError("an omegam of the table is not in (0, 2)")
    return omega, omegam


def power_law_channel(H, n, umax, nu_wall):
    """A force-driven channel of width H (walls half-way outside the first and last fluid row) of a power-law fluid with peak velocity umax
    whose viscosity at the wall is nu_wall: returns (K, force, g_wall).  With h = H / 2: u(s) = n / (n + 1) (F / K)^(1/n) (h^(1 + 1/n) -
    |s|^(1 + 1/n)), so the wall's shear rate is gdot_w = (F h / K)^(1/n) = umax (n + 1) / (n h), nu_wall = K gdot_w^(n - 1), and the stress
    there F h = nu_wall gdot_w; g_wall = g_of(gdot_w, nu_wall)."""
    H, n, umax, nu_wall = float(H), float(n), float(umax), float(nu_wall)
    h = 0.5 * H
    gdot_w = umax * (n + 1.0) / (n * h)
    K = nu_wall / gdot_w ** (n - 1.0)
    force = nu_wall * gdot_w / h
    return K, force, float(g_of(gdot_w, nu_wall))


def power_law_profile(H, K, n, force, s=None):
    """u(s) = n / (n + 1) (F / K)^(1/n) (h^(1 + 1/n) - |s|^(1 + 1/n)), h = H / 2, s the distance from the centre line (default: the H cell
    centres -h + 1/2, -h + 3/2, ...), at rho = 1."""
    H, K, n, F = float(H), float(K), float(n), float(force)
    h = 0.5 * H
    s = np.arange(int(round(H)), dtype=np.float64) + 0.5 - h if s is None else np.asarray(s, dtype=np.float64)
    e = 1.0 + 1.0 / n
    return n / (n + 1.0) * (F / K) ** (1.0 / n) * (h ** e - np.abs(s) ** e)


# ---- what the front ends share -------------------------------------------------------------------------------------------------------------
G_MAX_DEFAULT = 0.1      # the command lines' --g-max: g = (sqrt 2 / 3) gdot tau stays far below it at lattice velocities


def resolve(spec, RT="MRT"):
    """(omega, omegam, g_max) of a front end's rheology= argument: that tuple itself, or dict(law=nu(gdot), g_max=..., entries=4096,
    magic=None) for table() -- magic only reaches a TRT solver (None there: no second table, the lattice's omega-)."""
    if isinstance(spec, dict):
        g_max = float(spec.get("g_max", G_MAX_DEFAULT))
        omega, omegam = table(spec["law"], int(spec.get("entries", 4096)), g_max, spec.get("magic") if RT == "TRT" else None)
        return omega, omegam, g_max
    omega, omegam, g_max = spec
    return np.asarray(omega, dtype=np.float64), (None if omegam is None else np.asarray(omegam, dtype=np.float64)), float(g_max)


def apply(solver, spec, RT="MRT"):
    """set_rheology with the table of `spec` (resolve); returns g_max."""
    omega, omegam, g_max = resolve(spec, RT)
    solver.set_rheology(omega, omegam, g_max)
    return g_max


def over_range(solver, g_max, say=print):
    """One warning if the largest shear of the current state exceeds g_max (beyond it the table silently holds its last entry); returns
    that shear."""
    g = float(np.max(solver.get_shear()))
    if g > g_max:
        say(f"warning: the largest shear {g:.6g} exceeds the rheology table's g_max {g_max:.6g}: beyond it the table holds its last entry")
    return g
