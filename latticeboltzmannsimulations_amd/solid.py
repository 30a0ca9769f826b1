"""Host restatement of the solid obstacles of the bounce-back cavity (CavitySolver(..., semantics='bounce_back', solid=mask),
LBM_SEM_BOUNCE_BACK_SOLID): the links of a mask and the momentum-exchange force on the obstacles from public outputs alone.

A mask is [X, Y], nonzero = solid, y = 0 the lid.  Slot k of a cell pulls from (x - cx_k, y + cy_k); a LINK is a (fluid cell, slot k)
pair whose source is a solid cell inside the lattice.  There the cell receives its own post-collision population of the opposite
direction, which is what get_fields returns as fin_k of that cell, so the force the fluid exerts on the solid cells is

    F = sum over links of 2 c_opp(k) fin_k(x, y),        c_opp(k) = -c_k,

in the convention of u: F[1] > 0 points to the lid.  lbm_solid_force reduces the same terms on the device (CavitySolver.solid_force).

BODIES.  Labels [X, Y] (integers in [0, nbodies) on the solid cells, ignored elsewhere) split the solid cells into bodies; a link
belongs to the body of its source cell.  With the centre (x0, y0) of a body in index coordinates and the link's midpoint relative to it,
(rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0), the torque on the body is

    tz = sum over its links of rx ty + ry tx,        (tx, ty) = 2 c_opp(k) fin_k(x, y):

y grows away from the lid while F[1] > 0 points to it, so this is the z-moment in the frame drawn with the lid on top, positive
counter-clockwise.  lbm_body_force reduces the same terms per body on the device (CavitySolver.body_force, force_series).
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


def force_terms(fin, mask, delta=None):
    """(tx, ty): the terms 2 cx_opp(k) fin_k and 2 cy_opp(k) fin_k of every link as float64 arrays [links], slots k = 1 .. 8 in order;
    the zero terms of the axis-aligned slots are kept, so both have one entry per link.  delta (wall_delta_field, bodies in motion):
    the terms are c_opp(k) (2 fin_k - delta_k) instead."""
    fin = np.asarray(fin)
    tx, ty = [], []
    for k, lk in enumerate(links(mask)):
        if k == 0:
            continue
        f = fin[k][lk].astype(np.float64)
        if delta is None:
            tx.append(2.0 * CX[OPP[k]] * f)
            ty.append(2.0 * CY[OPP[k]] * f)
        else:
            t = 2.0 * f - np.asarray(delta, dtype=np.float64)[k][lk]
            tx.append(float(CX[OPP[k]]) * t)
            ty.append(float(CY[OPP[k]]) * t)
    return np.concatenate(tx), np.concatenate(ty)


def host_force(fin, mask, delta=None):
    """dict(links, fx, fy) from the populations fin[9, X, Y] that get_fields returns and the mask: the exactly rounded sums
    (math.fsum) of force_terms.  delta: wall_delta_field(...) while the bodies move (CavitySolver.set_body_motion)."""
    tx, ty = force_terms(fin, mask, delta)
    return dict(links=int(tx.size), fx=math.fsum(tx.tolist()), fy=math.fsum(ty.tolist()))


def labels_from(nx, ny, boxes=(), path=None):
    """(mask, labels, nbodies) as the command lines build them: every --solid-box is a body of its own, in the order given, and a later
    box wins an overlap; the nonzero values of an integer --solid-file array are body ids, the distinct values in ascending order, and
    follow the boxes (the file wins an overlap).  A file of another type is one body.  (None, None, 0) when neither is given."""
    if not boxes and path is None:
        return None, None, 0
    lab = np.full((int(nx), int(ny)), -1, dtype=np.int32)
    n = 0
    for box in boxes:
        lab[boxes_mask(nx, ny, [box])] = n
        n += 1
    if path is not None:
        f = np.load(path, allow_pickle=False)
        if f.shape != (nx, ny):
            raise ValueError(f"solid file {path} holds an array of shape {f.shape}, the lattice is {(nx, ny)}")
        ids = np.unique(f[f != 0]) if np.issubdtype(f.dtype, np.integer) else []
        if len(ids) == 0 and np.any(f != 0):
            lab[f != 0] = n
            n += 1
        for v in ids:
            lab[f == v] = n
            n += 1
    return lab >= 0, lab, n


def centroids(mask, labels, nbodies):
    """[nbodies, 2]: the mean (x, y) of each body's cells, float64; (0, 0) for a body without cells (lbm_set_solid_bodies with
    centre = NULL)."""
    m = np.asarray(mask) != 0
    lab = np.asarray(labels)
    out = np.zeros((int(nbodies), 2))
    xs, ys = np.nonzero(m)
    for b in range(int(nbodies)):
        sel = lab[xs, ys] == b
        if sel.any():
            out[b] = float(xs[sel].sum()) / float(sel.sum()), float(ys[sel].sum()) / float(sel.sum())
    return out


def body_links(mask, labels):
    """The link list of a labelled mask as the library builds it: an int array [links, 4] of (x, y, k, body) -- the fluid cell, the slot
    and the body of the source cell (x - cx_k, y + cy_k) -- sorted by body, then by cell in [y][x] order, then by k."""
    lab = np.asarray(labels)
    rows = []
    for k, lk in enumerate(links(mask)):
        if k == 0:
            continue
        x, y = np.nonzero(lk)
        rows.append(np.stack([x, y, np.full(x.shape, k), lab[x - CX[k], y + CY[k]]], axis=1))
    out = np.concatenate(rows).astype(np.int64)
    return out[np.lexsort((out[:, 2], out[:, 0], out[:, 1], out[:, 3]))]


def wall_deltas(mask, labels, centres, motion, dtype=None):
    """(links, delta): body_links(mask, labels) and, per link, Ladd's moving-wall term of lbm_set_body_motion as a float64 array:
    with motion[nbodies, 3] = (Ux, Uy, Om) of the link's body and its midpoint relative to the body's centre,
        uwx = Ux + Om ry;  uwy = Uy + Om rx;  delta = (6 w_k) (cx_k uwx + cy_k uwy),        6 w_k = 2/3 (k <= 4) or 1/6,
    every product and sum rounded in this order.  dtype: the lattice type, to which the library rounds the term once (the value it adds,
    and the one the force subtracts); None leaves the double."""
    centres = np.asarray(centres, dtype=np.float64)
    motion = np.asarray(motion, dtype=np.float64)
    ln = body_links(mask, labels)
    x, y, k, b = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
    cx, cy = np.array(CX, dtype=np.float64), np.array(CY, dtype=np.float64)
    rx = (x.astype(np.float64) - 0.5 * cx[k]) - centres[b, 0]
    ry = (y.astype(np.float64) + 0.5 * cy[k]) - centres[b, 1]
    uwx = motion[b, 0] + motion[b, 2] * ry
    uwy = motion[b, 1] + motion[b, 2] * rx
    d = np.where(k < 5, 2.0 / 3.0, 1.0 / 6.0) * (cx[k] * uwx + cy[k] * uwy)
    return ln, (d if dtype is None else d.astype(dtype).astype(np.float64))


def wall_delta_field(mask, labels, centres, motion, dtype=None):
    """delta[9, X, Y], float64: wall_deltas at (k, x, y) of every link, zero elsewhere -- what host_force and host_body_force take."""
    ln, d = wall_deltas(mask, labels, centres, motion, dtype)
    out = np.zeros((9,) + np.asarray(mask).shape)
    out[ln[:, 2], ln[:, 0], ln[:, 1]] = d
    return out


def body_force_terms(fin, mask, labels, centres, delta=None):
    """(body, tx, ty, mx, my): per link of body_links(mask, labels) its body and, as float64, the force terms and the two products
    rx ty and ry tx of its torque, each product rounded once.  delta (wall_delta_field, bodies in motion): (tx, ty) =
    c_opp(k) (2 fin_k - delta_k)."""
    fin = np.asarray(fin)
    centres = np.asarray(centres, dtype=np.float64)
    ln = body_links(mask, labels)
    x, y, k, b = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
    cx, cy, opp = np.array(CX), np.array(CY), np.array(OPP)
    f = fin[k, x, y].astype(np.float64)
    if delta is None:
        tx, ty = 2.0 * cx[opp[k]] * f, 2.0 * cy[opp[k]] * f
    else:
        t = 2.0 * f - np.asarray(delta, dtype=np.float64)[k, x, y]
        tx, ty = cx[opp[k]].astype(np.float64) * t, cy[opp[k]].astype(np.float64) * t
    rx = (x.astype(np.float64) - 0.5 * cx[k]) - centres[b, 0]
    ry = (y.astype(np.float64) + 0.5 * cy[k]) - centres[b, 1]
    return b, tx, ty, rx * ty, ry * tx


def host_body_force(fin, mask, labels, centres, delta=None):
    """dict(links, fx, fy, tz) of arrays [nbodies] (nbodies = len(centres)) from the populations fin[9, X, Y] that
    get_fields(want_fin=True) returns: per body the exactly rounded sums (math.fsum) of body_force_terms.  delta:
    wall_delta_field(...) while the bodies move."""
    b, tx, ty, mx, my = body_force_terms(fin, mask, labels, centres, delta)
    n = len(centres)
    out = dict(links=np.zeros(n, dtype=np.int64), fx=np.zeros(n), fy=np.zeros(n), tz=np.zeros(n))
    for i in range(n):
        sel = b == i
        out["links"][i] = int(sel.sum())
        out["fx"][i] = math.fsum(tx[sel].tolist())
        out["fy"][i] = math.fsum(ty[sel].tolist())
        out["tz"][i] = math.fsum(mx[sel].tolist() + my[sel].tolist())
    return out
