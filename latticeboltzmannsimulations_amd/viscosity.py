"""Viscosity fields of the obstacle lattices (CavitySolver.set_relaxation_field, set_viscosity): the rates of a field of
viscosities, layered fluids, a sponge zone in front of a held outlet, and the closed form of the two-layer Poiseuille flow.

Arrays are [X, Y] as everywhere, y = 0 the lid row; viscosities are in lattice units, nu = (1 / omega - 1/2) / 3.
"""
import numpy as np

MAGIC = 3.0 / 16.0      # the TRT product at which a half-way wall (and the link-midpoint interface of two layers) sits exactly half-way


def rates(nu, magic=None):
    """(omega, omegam) of a field of viscosities: omega = 1 / (3 nu + 1/2); with magic=L also TRT's omega- = 1 / (1/2 + L / (3 nu)), so
    that (1 / omega - 1/2)(1 / omegam - 1/2) = L in every cell; omegam is None without it."""
    nu = np.asarray(nu, dtype=np.float64)
    if not (np.isfinite(nu).all() and (nu > 0.0).all()):
        raise ValueError("every viscosity must be finite and > 0")
    omega = 1.0 / (3.0 * nu + 0.5)
    if magic is None:
        return omega, None
    if not (np.isfinite(magic) and magic > 0.0):
        raise ValueError("the magic parameter must be finite and > 0")
    return omega, 1.0 / (0.5 + float(magic) / (3.0 * nu))


def layers(nx, ny, edges, nus):
    """nu[X, Y] of layers along y: rows y < edges[0] take nus[0], edges[0] <= y < edges[1] take nus[1], ..., the rest nus[-1]
    (len(nus) == len(edges) + 1, edges ascending).  An edge e puts the interface on the link midpoint between rows e - 1 and e."""
    edges, nus = [int(e) for e in edges], [float(v) for v in nus]
    if len(nus) != len(edges) + 1 or sorted(edges) != edges:
        raise ValueError("layers needs ascending edges and one viscosity more than edges")
    row = np.full(int(ny), nus[0])
    for e, v in zip(edges, nus[1:]):
        row[max(e, 0):] = v
    return np.ascontiguousarray(np.broadcast_to(row[None, :], (int(nx), int(ny))))


def sponge(nx, ny, length, factor, side="east", power=2):
    """A multiplier field [X, Y] for a viscosity: 1 outside the zone, rising as (distance into the zone / length) ** power to `factor`
    at the cells of the side -- east: x = X - 1, west: x = 0, south: y = Y - 1, north: y = 0 (the lid row)."""
    nx, ny, length = int(nx), int(ny), int(length)
    if side not in ("east", "west", "north", "south"):
        raise ValueError("side must be east, west, north or south")
    n = nx if side in ("east", "west") else ny
    if not 0 <= length <= n or not factor > 0.0:
        raise ValueError("the sponge needs 0 <= length <= the lattice's extent and a factor > 0")
    i = np.arange(n, dtype=np.float64)
    depth = (i - (n - 1 - length)) if side in ("east", "south") else ((length - i))
    ramp = np.clip(depth / length, 0.0, 1.0) if length > 0 else np.zeros(n)
    line = 1.0 + (float(factor) - 1.0) * ramp ** power
    m = line[:, None] if side in ("east", "west") else line[None, :]
    return np.ascontiguousarray(np.broadcast_to(m, (nx, ny)))


def two_layer_profile(H, h, nu1, nu2, force, s=None):
    """The steady velocity of a force-driven channel of width H between two walls at rest with two fluids, nu1 for 0 < s < h and nu2 for
    h < s < H, at rho = 1, from stress continuity: tau(s) = F (s0 - s), du/ds = tau / nu(s), u(0) = u(H) = 0, so
    s0 = (h^2 / (2 nu1) + (H^2 - h^2) / (2 nu2)) / (h / nu1 + (H - h) / nu2).  s: the distances from the first wall (default: the H cell
    centres 1/2, 3/2, ...).  Returns u[len(s)]."""
    H, h, nu1, nu2, F = float(H), float(h), float(nu1), float(nu2), float(force)
    if not 0.0 < h < H:
        raise ValueError("the interface must lie inside the channel")
    s = np.arange(int(round(H)), dtype=np.float64) + 0.5 if s is None else np.asarray(s, dtype=np.float64)
    s0 = (h * h / (2.0 * nu1) + (H * H - h * h) / (2.0 * nu2)) / (h / nu1 + (H - h) / nu2)
    lower = F * (s0 * s - 0.5 * s * s) / nu1
    uh = F * (s0 * h - 0.5 * h * h) / nu1
    upper = uh + F * (s0 * (s - h) - 0.5 * (s * s - h * h)) / nu2
    return np.where(s <= h, lower, upper)
