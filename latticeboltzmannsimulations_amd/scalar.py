"""Host side of the passive scalar (CavitySolver.begin_scalar, lbm_scalar_* of include/lbm.h): the two relaxation rates, the NumPy twins
of the tables the library builds on the host (csrc/lbm_scalar.hpp: the wall values, the constants of the hold cells), the Nusselt number
of a body from its flux, and the helpers that cut the image cells of periodic sides off an exported field."""
import math

import numpy as np

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)          # slot k of cell (x, y) pulls from (x - CX[k], y + CY[k])
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
W = (4.0 / 9.0,) + (1.0 / 9.0,) * 4 + (1.0 / 36.0,) * 4
OPP = (0, 3, 4, 1, 2, 7, 8, 5, 6)


def rates(D, magic=0.25):
    """(w_plus, w_minus) of the scalar's TRT collision in double, in the library's order of operations: tm = 3 D + 1/2, w- = 1 / tm,
    w+ = 1 / (magic / (tm - 1/2) + 1/2).  magic = (1/w+ - 1/2)(1/w- - 1/2); BGK is magic = (3 D)**2.  The lattice rounds each once."""
    D, magic = float(D), float(magic)
    if not (math.isfinite(D) and D > 0.0 and math.isfinite(magic) and magic > 0.0):
        raise ValueError("D and magic must be finite and > 0")
    tm = 3.0 * D + 0.5
    tp = magic / (tm - 0.5) + 0.5
    return 1.0 / tp, 1.0 / tm


def host_wall_table(mask, wall_value, hold=None):
    """The wall values as the library's host builder lays them out: (cell_row[Y, X] int32, val[rows, 8] float64, bits[rows] uint8).
    mask [X, Y]: the solid cells; wall_value [X, Y]: the value of a Dirichlet solid cell, NaN on adiabatic cells (None: none); hold
    [X, Y]: the flow's hold cells, image cells of periodic sides included (None: none).  One row per fluid cell, in [y][x] order, that has
    a link to a Dirichlet cell; val[row, k - 1] = (2 w_k) Cw of link k, bits bit k - 1 marks it.  The lattice rounds val once."""
    mask = np.asarray(mask) != 0
    X, Y = mask.shape
    cell_row = np.full((Y, X), -1, dtype=np.int32)
    val, bits = [], []
    if wall_value is None:
        return cell_row, np.zeros((0, 8)), np.zeros(0, dtype=np.uint8)
    wv = np.asarray(wall_value, dtype=np.float64)
    dirichlet = mask & ~np.isnan(wv)
    held = np.zeros((X, Y), bool) if hold is None else np.asarray(hold) != 0
    for y in range(Y):
        for x in range(X):
            if mask[x, y] or held[x, y]:
                continue
            row = None
            for k in range(1, 9):
                sx, sy = x - CX[k], y + CY[k]
                if sx < 0 or sx >= X or sy < 0 or sy >= Y or not dirichlet[sx, sy]:
                    continue
                if row is None:
                    row = len(bits)
                    cell_row[y, x] = row
                    bits.append(0)
                    val.append([0.0] * 8)
                bits[row] |= 1 << (k - 1)
                val[row][k - 1] = (2.0 * W[k]) * float(wv[sx, sy])
    return cell_row, np.array(val, dtype=np.float64).reshape(-1, 8), np.array(bits, dtype=np.uint8)


def hold_values(f, Ch):
    """What a user's hold cell keeps, nine doubles: (w_k Ch) (1 + 3 (cx_k ux + cy_k uy)) with (ux, uy) the moments of the nine flow
    populations f it holds, in the library's order of operations.  The lattice rounds each once."""
    f = [float(v) for v in f]
    rho = ((((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8])
    ux = (((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]) / rho
    uy = (((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]) / rho
    return [(W[k] * float(Ch)) * (1.0 + 3.0 * (float(CX[k]) * ux + float(CY[k]) * uy)) for k in range(9)]


def nusselt(flux, D, dC, L, perimeter=None):
    """The Nusselt number of a body from the scalar it gives off per step (scalar_flux()['flux']): the mean flux density flux / perimeter
    against the conductive one D dC / L.  perimeter: the length of the body's surface, by default pi L, a disc of diameter L; a plate that
    spans nx columns has perimeter nx."""
    perimeter = math.pi * float(L) if perimeter is None else float(perimeter)
    return (float(flux) / perimeter) * float(L) / (float(D) * float(dC))


def interior(a, periodic):
    """a[..., X, Y] without the image cells of the periodic sides (x, y) -- what solver.periodic returns."""
    px, py = bool(periodic[0]), bool(periodic[1])
    return np.asarray(a)[..., (slice(1, -1) if px else slice(None)), (slice(1, -1) if py else slice(None))]


def real_cells(mask, periodic):
    """bool [X, Y]: the cells that are neither solid nor images -- the cells scalar_totals() counts."""
    mask = np.asarray(mask) != 0
    real = ~mask
    if periodic[0]:
        real[[0, -1], :] = False
    if periodic[1]:
        real[:, [0, -1]] = False
    return real
