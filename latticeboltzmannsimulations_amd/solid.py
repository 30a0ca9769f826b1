"""Host restatement of the solid obstacles of the bounce-back cavity (CavitySolver(..., semantics='bounce_back', solid=mask),
LBM_SEM_BOUNCE_BACK_SOLID): the links of a mask and the momentum-exchange force on the obstacles from public outputs alone.

A mask is [X, Y], nonzero = solid, y = 0 the lid.  Slot k of a cell pulls from (x - cx_k, y + cy_k); a LINK is a (fluid cell, slot k)
pair whose source is a solid cell inside the lattice.  There the cell receives its own post-collision population of the opposite
direction, which is what get_fields returns as fin_k of that cell, so the force the fluid exerts on the solid cells is

    F = sum over links of 2 c_opp(k) fin_k(x, y),        c_opp(k) = -c_k,

in the convention of u: F[1] > 0 points to the lid.  lbm_solid_force reduces the same terms on the device (CavitySolver.solid_force).
"""
import math

import numpy as np

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
OPP = (0, 3, 4, 1, 2, 7, 8, 5, 6)


def boxes_mask(nx, ny, boxes):
    """The mask of half-open boxes (x0, x1, y0, y1) in cells, as --solid-box gives them."""
    m = np.zeros((int(nx), int(ny)), dtype=bool)
    for x0, x1, y0, y1 in boxes:
        if not (0 <= x0 < x1 <= nx and 0 <= y0 < y1 <= ny):
            raise ValueError(f"solid box {(x0, x1, y0, y1)} is empty or not inside the {nx} x {ny} lattice")
        m[int(x0):int(x1), int(y0):int(y1)] = True
    return m


def mask_from(nx, ny, boxes=(), path=None):
    """The mask the command lines build: the union of --solid-box boxes and the nonzero cells of the --solid-file array ([X, Y], .npy);
    None when neither is given."""
    if not boxes and path is None:
        return None
    m = boxes_mask(nx, ny, boxes)
    if path is not None:
        f = np.load(path, allow_pickle=False)
        if f.shape != (nx, ny):
            raise ValueError(f"solid file {path} holds an array of shape {f.shape}, the lattice is {(nx, ny)}")
        m |= f != 0
    return m


def links(mask):
    """link[k] for k = 0 .. 8: bool [X, Y], True where the cell is fluid and the source of its slot k is a solid cell inside the lattice
    (link[0] is all False)."""
    m = np.asarray(mask) != 0
    X, Y = m.shape
    out = [np.zeros((X, Y), dtype=bool)]
    for k in range(1, 9):
        src = np.zeros((X, Y), dtype=bool)       # src[x, y] = m[x - cx, y + cy] where that cell exists
        xd = slice(max(0, CX[k]), X + min(0, CX[k]))
        xs = slice(max(0, -CX[k]), X + min(0, -CX[k]))
        yd = slice(max(0, -CY[k]), Y + min(0, -CY[k]))
        ys = slice(max(0, CY[k]), Y + min(0, CY[k]))
        src[xd, yd] = m[xs, ys]
        out.append(src & ~m)
    return out


def force_terms(fin, mask):
    """(tx, ty): the terms 2 cx_opp(k) fin_k and 2 cy_opp(k) fin_k of every link as float64 arrays [links], slots k = 1 .. 8 in order;
    the zero terms of the axis-aligned slots are kept, so both have one entry per link."""
    fin = np.asarray(fin)
    tx, ty = [], []
    for k, lk in enumerate(links(mask)):
        if k == 0:
            continue
        f = fin[k][lk].astype(np.float64)
        tx.append(2.0 * CX[OPP[k]] * f)
        ty.append(2.0 * CY[OPP[k]] * f)
    return np.concatenate(tx), np.concatenate(ty)


def host_force(fin, mask):
    """dict(links, fx, fy) from the populations fin[9, X, Y] that get_fields returns and the mask: the exactly rounded sums
    (math.fsum) of force_terms."""
    tx, ty = force_terms(fin, mask)
    return dict(links=int(tx.size), fx=math.fsum(tx.tolist()), fy=math.fsum(ty.tolist()))
