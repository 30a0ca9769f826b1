"""Flow past a body in a stream or a channel, on the bounce-back cavity with open boundaries (CavitySolver.set_open_cells,
set_wall_velocity).

The lattice is [X, Y] with the stream along x.  Rows 0 and Y - 1 are solid side walls, so the walls sit half-way between rows 0 / 1 and
Y - 2 / Y - 1 and the channel is H = Y - 2 cells wide; column 0 is a solid inlet wall whose cells carry the inflow profile as their wall
velocity (a velocity bounce-back inlet); the cells of column X - 1 between the walls are hold cells at the equilibrium of rho = 1 and
the same profile (a pressure outlet with the far-field velocity).  The lid of the cavity lies behind the solid row 0 and drives nothing.

    python -m latticeboltzmannsimulations_amd.channel --xsize 440 --ysize 84 --Re-D 20 --umax 0.05 --disc 40 41.5 10 --curved --force-every 50
"""
import argparse
import sys

import numpy as np

from . import scalar as SC
from . import solid as S
from . import rheology as RH
from . import viscosity as V


def inflow_profile(ny, umax, kind="parabolic"):
    """ux[Y] of the inflow: 'parabolic' -- umax 4 (y - 1/2) (Y - 3/2 - y) / (Y - 2)^2, which vanishes on the walls, half a cell outside
    rows 1 and Y - 2 -- or 'plug', umax on every row; zero on the wall rows 0 and Y - 1 themselves."""
    if kind not in ("parabolic", "plug"):
        raise ValueError("profile must be 'parabolic' or 'plug'")
    y = np.arange(int(ny), dtype=np.float64)
    u = np.full(int(ny), float(umax)) if kind == "plug" else float(umax) * 4.0 * (y - 0.5) * (ny - 1.5 - y) / (ny - 2.0) ** 2
    u[0] = u[-1] = 0.0
    return u


def channel(nx, ny, umax, profile="parabolic", walls="rest", disc=None, curved=False):
    """The geometry of a channel (walls='rest': side walls at rest) or of a free stream (walls='stream': the side rows slide at umax) as a
    dict: solid [X, Y]; labels [X, Y] -- body 0 the side walls, body 1 the inlet column, each obstacle a body of its own after them --
    and nbodies; hold [X, Y] with f [9, X, Y]; wall_velocity [2, X, Y]; profile [Y], mean (the mean of the profile over the H = Y - 2
    rows between the walls) and H.  disc=(x0, y0, r), or a list of them: solid discs (solid.discs_into); curved=True: `shape`
    [8, X, Y], the exact wall distances of the discs' links (solid.disc_fractions), 1/2 on every other link."""
    nx, ny = int(nx), int(ny)
    if nx < 4 or ny < 4:
        raise ValueError("a channel needs at least 4 x 4 cells")
    if walls not in ("rest", "stream"):
        raise ValueError("walls must be 'rest' or 'stream'")
    prof = inflow_profile(ny, umax, profile)
    m = np.zeros((nx, ny), dtype=bool)
    m[:, 0] = m[:, ny - 1] = m[0, :] = True
    lab = np.full((nx, ny), -1, dtype=np.int32)
    lab[0, :] = 1
    lab[:, 0] = lab[:, ny - 1] = 0
    n = 2
    discs = [] if disc is None else ([tuple(disc)] if np.ndim(disc) == 1 else [tuple(d) for d in disc])
    if discs:
        m, lab, n = S.discs_into(nx, ny, discs, m, lab, n)
    hold = np.zeros((nx, ny), dtype=bool)
    hold[nx - 1, 1:ny - 1] = True
    if (hold & m).any():
        raise ValueError("an obstacle covers the outlet column")
    uw = np.zeros((2, nx, ny))
    uw[0, 0, :] = prof
    if walls == "stream":
        uw[0, :, 0] = uw[0, :, ny - 1] = float(umax)
    f = S.equilibrium(1.0, np.broadcast_to(prof[None, :], (nx, ny)), 0.0)
    out = dict(solid=m, labels=lab, nbodies=n, hold=hold, f=f, wall_velocity=uw, profile=prof, mean=float(prof[1:ny - 1].mean()), H=ny - 2,
               discs=discs)
    if curved:
        q = None
        for x0, y0, r in discs:
            q = S.disc_fractions(m, x0, y0, r, q)
        out["shape"] = np.full((8, nx, ny), 0.5) if q is None else q
    return out


def solver_re(Re_D, D, umax, mean, ny):
    """The solver's Re for a Reynolds number of the obstacle, Re_D = mean D / nu: the solver derives nu = uLB ysize / Re with
    uLB = umax, so Re = umax ysize Re_D / (mean D)."""
    return float(umax) * float(ny) * float(Re_D) / (float(mean) * float(D))


def run_channel(nx, ny, Re_D, umax=0.05, disc=None, curved=False, profile="parabolic", walls="rest", steps=20000, force_every=100, RT="MRT",
                dtype=np.float32, arith="strict", device=0, solver_factory=None, quiet=False, scalar=None, buoyancy=None, subgrid=None, sponge=None, rheology=None):
    """Step a channel and keep the force series of the (first) obstacle on the device.  Returns dict(Cd, Cl, fx, fy, steps, Re, nu,
    series): Cd = 2 Fx / (rho mean^2 D), Cl likewise from Fy, of the last sample (rho = 1); D = 2 r of the disc (without one: the
    channel's width and the force on the side walls).  Re_D = mean D / nu is converted to the solver's Re (solver_re).
    scalar=dict(D=..., disc_value=1.0, inlet_value=0.0, magic=0.25): a passive scalar (CavitySolver.begin_scalar) that starts at
    inlet_value, with the inlet column's solid cells Dirichlet at inlet_value, the obstacles Dirichlet at disc_value, the side walls
    adiabatic and the held outlet holding inlet_value; the result gains Nu, the Nusselt number of the (first) disc on its diameter
    (scalar.nusselt), its flux `scalar_flux` and the scalar diffusivity.  buoyancy=(ax, ay, c_ref): the scalar acts on the flow
    (CavitySolver.set_buoyancy; needs scalar=...).  subgrid=cs2: the local Smagorinsky closure (CavitySolver.set_subgrid) from the first
    step on, for a channel beyond the steady regime on a coarse lattice; the result gains tau_mean, the mean over the fluid cells of
    get_tau() after the last step.  The scalar keeps its molecular diffusivity; not with buoyancy.
    sponge=(length, factor): a zone of raised viscosity in front of the held outlet (CavitySolver.set_viscosity with nu times
    viscosity.sponge(nx, ny, length, factor), a quadratic ramp to factor nu at the outlet column; under TRT the magic parameter of the
    solver's rates is kept in every cell), which relaxes a wake towards the profile the outlet holds; the result gains outlet_drho, the
    largest |rho - 1| over the fluid cells of the last 20 columns in front of the outlet after the last step.  Not with buoyancy.
    rheology=(omega, omegam, g_max) or dict(law=..., g_max=..., entries=..., magic=...) (rheology.resolve): a generalised Newtonian fluid
    (CavitySolver.set_rheology) from the first step on; Re_D then only sets the lattice's own rates.  With the report after the last
    step one warning is printed if the largest shear exceeds g_max; the result gains g_top, that shear, and tau_mean.  Not with
    buoyancy, subgrid or sponge."""
    if rheology is not None and (buoyancy is not None or sponge is not None or (subgrid is not None and float(subgrid) > 0.0)):
        raise ValueError("rheology excludes buoyancy, subgrid and sponge: each pairing would be one more set of kernel twins")
    if sponge is not None and buoyancy is not None:
        raise ValueError("sponge and buoyancy exclude each other: the buoyant kernels read no viscosity field")
    if subgrid is not None and buoyancy is not None and float(subgrid) > 0.0:
        raise ValueError("subgrid and buoyancy exclude each other: a buoyant flow with the closure needs an eddy diffusivity for the scalar")
    g = channel(nx, ny, umax, profile, walls, disc, curved)
    D = 2.0 * g["discs"][0][2] if g["discs"] else float(g["H"])
    body = 2 if g["discs"] else 0
    Re = solver_re(Re_D, D, umax, g["mean"], ny)
    nu = float(umax) * ny / Re
    if solver_factory is None:
        from .solver import CavitySolver as solver_factory
    if not quiet:
        print(f"channel {nx} x {ny}: Re_D = {Re_D:g} on D = {D:g} with the mean velocity {g['mean']:.6g} -> nu = {nu:.6g}, "
              f"the solver's Re = umax ysize / nu = {Re:.6g}")
    with solver_factory(nx, ny, Re, RT=RT, uLB=umax, semantics="bounce_back", dtype=dtype, arith=arith, device=device, solid=g["solid"],
                        bodies=g["labels"]) as s:
        s.set_open_cells(g["hold"], g["f"])
        if curved:
            s.set_shape(g["shape"])
        s.set_wall_velocity(g["wall_velocity"])
        if subgrid is not None:
            s.set_subgrid(float(subgrid))
        g_max = RH.apply(s, rheology, RT) if rheology is not None else None
        if sponge is not None:
            length, factor = int(sponge[0]), float(sponge[1])
            rl = s.relax
            magic = (1.0 / rl["omega"] - 0.5) * (1.0 / rl["omegam"] - 0.5) if RT == "TRT" else None
            s.set_viscosity(nu * V.sponge(nx, ny, length, factor), magic)
        if scalar is not None:
            sc = dict(dict(disc_value=1.0, inlet_value=0.0, magic=0.25), **scalar)
            if not g["discs"]:
                raise ValueError("scalar=... reports the Nusselt number of a disc: it needs disc=...")
            wv = np.full((nx, ny), np.nan)
            wv[g["labels"] == 1] = float(sc["inlet_value"])
            wv[g["labels"] >= 2] = float(sc["disc_value"])
            s.begin_scalar(sc["D"], float(sc["inlet_value"]), sc["magic"], wall_value=wv, hold_value=float(sc["inlet_value"]))
        if buoyancy is not None:
            s.set_buoyancy(*buoyancy)
        every = max(1, int(force_every))
        s.step(1)
        s.begin_force(every=every, capacity=max(1, int(steps) // every + 1))
        s.step(int(steps) - 1)
        s.sample_force()
        series = s.force_series()
        s.end_force()
        flux = float(s.scalar_flux()["flux"][body]) if scalar is not None else None
        tau_mean = float(np.mean(s.get_tau()[~g["solid"] & ~g["hold"]], dtype=np.float64)) if subgrid is not None or rheology is not None else None
        g_top = RH.over_range(s, g_max, (lambda *a: None) if quiet else print) if rheology is not None else None
        if sponge is not None:
            rho = np.asarray(s.get_fields()[1], dtype=np.float64)
            tail = np.zeros((nx, ny), dtype=bool)
            tail[max(nx - 21, 1):nx - 1, :] = True
            outlet_drho = float(np.abs(rho - 1.0)[tail & ~g["solid"] & ~g["hold"]].max())
    fx, fy = float(series["fx"][-1][body]), float(series["fy"][-1][body])
    scale = 2.0 / (g["mean"] ** 2 * D)
    out = dict(Cd=scale * fx, Cl=scale * fy, fx=fx, fy=fy, steps=int(steps), Re=Re, nu=nu, series=series, body=body)
    if scalar is not None:
        out.update(scalar_flux=flux, scalar_D=float(sc["D"]), Nu=SC.nusselt(flux, sc["D"], float(sc["disc_value"]) - float(sc["inlet_value"]), D))
    if subgrid is not None:
        out.update(subgrid=float(subgrid), tau_mean=tau_mean)
    if rheology is not None:
        out.update(g_top=g_top, g_max=g_max, tau_mean=tau_mean)
    if sponge is not None:
        out.update(sponge=(length, factor), outlet_drho=outlet_drho)
    if not quiet:
        print(f"after {steps} steps: Fx = {fx:.8g}, Fy = {fy:.8g}, Cd = 2 Fx / (rho mean^2 D) = {out['Cd']:.6g}, Cl = {out['Cl']:.6g}" +
              (f", Nu = flux / (pi D_s dC) = {out['Nu']:.6g}" if scalar is not None else "") +
              (f", mean relaxation time {tau_mean:.6g}" if subgrid is not None or rheology is not None else "") +
              (f", max |rho - 1| in the last 20 columns {outlet_drho:.3e}" if sponge is not None else ""))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m latticeboltzmannsimulations_amd.channel", description=__doc__.split("\n\n")[0])
    ap.add_argument("--xsize", type=int, default=440)
    ap.add_argument("--ysize", type=int, default=84)
    ap.add_argument("--Re-D", dest="Re_D", type=float, default=20.0)
    ap.add_argument("--umax", type=float, default=0.05)
    ap.add_argument("--disc", type=float, nargs=3, metavar=("X0", "Y0", "R"), default=None)
    ap.add_argument("--curved", action="store_true")
    ap.add_argument("--profile", choices=("parabolic", "plug"), default="parabolic")
    ap.add_argument("--walls", choices=("rest", "stream"), default="rest")
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--force-every", dest="force_every", type=int, default=100)
    ap.add_argument("--RT", choices=("SRT", "TRT", "MRT"), default="MRT")
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scalar-D", dest="scalar_D", type=float, default=None, help="carry a passive scalar with this diffusivity; prints the disc's Nusselt number")
    ap.add_argument("--disc-value", dest="disc_value", type=float, default=1.0)
    ap.add_argument("--inlet-value", dest="inlet_value", type=float, default=0.0)
    ap.add_argument("--buoyancy", type=float, nargs=3, metavar=("AX", "AY", "CREF"), default=None, help="let the scalar act on the flow (needs --scalar-D)")
    ap.add_argument("--subgrid", type=float, default=None, metavar="CS2", help="the local Smagorinsky closure with this constant (the reference's is 0.025; not with --buoyancy)")
    ap.add_argument("--sponge", type=float, nargs=2, metavar=("LENGTH", "FACTOR"), default=None,
                    help="raise the viscosity over the last LENGTH columns in front of the held outlet, a quadratic ramp to FACTOR times nu (not with --buoyancy)")
    ap.add_argument("--power-law", dest="power_law", type=float, nargs=2, metavar=("K", "N"), default=None,
                    help="a power-law fluid nu = K gdot^(N - 1) (clipped to [1e-3, 2]) through a rheology table (not with --buoyancy, --subgrid, --sponge)")
    ap.add_argument("--carreau", type=float, nargs=4, metavar=("NU0", "NUINF", "LAMBDA", "N"), default=None,
                    help="a Carreau fluid nu = NUINF + (NU0 - NUINF) (1 + (LAMBDA gdot)^2)^((N - 1) / 2) through a rheology table")
    ap.add_argument("--g-max", dest="g_max", type=float, default=RH.G_MAX_DEFAULT, help="the shear of the table's last entry")
    a = ap.parse_args(argv)
    if a.power_law is not None and a.carreau is not None:
        ap.error("--power-law and --carreau exclude each other")
    law = RH.power_law(*a.power_law) if a.power_law is not None else RH.carreau(*a.carreau) if a.carreau is not None else None
    if law is not None and (a.buoyancy is not None or a.subgrid is not None or a.sponge is not None):
        ap.error("--power-law / --carreau exclude --buoyancy, --subgrid and --sponge")
    if a.subgrid is not None and a.buoyancy is not None:
        ap.error("--subgrid and --buoyancy exclude each other")
    if a.sponge is not None and a.buoyancy is not None:
        ap.error("--sponge and --buoyancy exclude each other")
    if a.curved and a.disc is None:
        ap.error("--curved gives the disc its exact wall distances: it needs --disc")
    if a.scalar_D is not None and a.disc is None:
        ap.error("--scalar-D reports the disc's Nusselt number: it needs --disc")
    run_channel(a.xsize, a.ysize, a.Re_D, a.umax, a.disc, a.curved, a.profile, a.walls, a.steps, a.force_every, a.RT, np.dtype(a.dtype).type,
                device=a.device, scalar=None if a.scalar_D is None else dict(D=a.scalar_D, disc_value=a.disc_value, inlet_value=a.inlet_value),
                buoyancy=a.buoyancy, subgrid=a.subgrid, sponge=a.sponge,
                rheology=None if law is None else dict(law=law, g_max=a.g_max, magic=V.MAGIC))
    return 0


if __name__ == "__main__":
    sys.exit(main())
