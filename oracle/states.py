"""Off-equilibrium cavity states for the arithmetic error budgets.  TEST INFRASTRUCTURE ONLY.

  S0  the library's initial state (rest, the lid row at uLB)
  S1  the equilibrium of a smooth field: rho in [0.85, 1.15], |u| <= 0.12
  S2  S1 with seeded, independent multiplicative noise of 1e-2 on every population: every non-conserved moment is off
      equilibrium, and on the lid row f4 + f7 + f8 != f2 + f5 + f6
  S3  S2 with rho in [0.6, 1.6] (the reciprocals and the closure's square root away from rho = 1)

Built in fp64 and rounded once to the lattice type; populations are fin[9, X, Y] as everywhere in oracle/.
"""
import numpy as np

from .lbm_numpy import equ, weights

STATES = ("S0", "S1", "S2", "S3")


def smooth_equilibrium(nx, ny, rho_mid=1.0, rho_amp=0.15, u_amp=0.08):
    x = (np.arange(nx, dtype=np.float64)[:, None] + 0.5) / nx
    y = (np.arange(ny, dtype=np.float64)[None, :] + 0.5) / ny
    rho = rho_mid + rho_amp * np.sin(2 * np.pi * x + 0.3) * np.cos(np.pi * y + 0.2)
    ux = u_amp * np.sin(np.pi * x) * np.cos(2 * np.pi * y)          # |u| <= u_amp sqrt(2) = 0.113
    uy = -u_amp * np.cos(np.pi * x + 0.4) * np.sin(2 * np.pi * y)
    return equ(rho, ux, uy, weights(np.float64))


def state(name, nx, ny, dtype, uLB=0.08, seed=2026):
    """fin[9, nx, ny] of `dtype` for S0..S3."""
    if name == "S0":
        from .lbm_ref import CavityOracleC
        return CavityOracleC(nx, ny, 100.0, semantics="mrt_gpu", collision="SRT", dtype=dtype, uLB=uLB).fin.copy()
    f = smooth_equilibrium(nx, ny, *((1.1, 0.5) if name == "S3" else (1.0, 0.15)))
    if name in ("S2", "S3"):
        f = f * (1.0 + 1e-2 * np.random.default_rng(seed).uniform(-1.0, 1.0, f.shape))
    return np.ascontiguousarray(f.astype(dtype))
