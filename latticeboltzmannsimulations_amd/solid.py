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


def host_force(fin, mask, delta=None, shape=None):
    """dict(links, fx, fy) from the populations fin[9, X, Y] that get_fields returns and the mask: the exactly rounded sums
    (math.fsum) of force_terms.  delta: wall_delta_field(...) while the bodies move (CavitySolver.set_body_motion).  shape: on a
    solver with a shape (set_shape), the post-collision populations fpost[9, X, Y] of the last step: the terms are
    c_opp(k) (fpost_opp(k) + fin_k), see shaped_force_terms."""
    if shape is not None:
        _, tx, ty = shaped_force_terms(fin, shape, mask)
        return dict(links=int(tx.size), fx=math.fsum(tx.tolist()), fy=math.fsum(ty.tolist()))
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


def discs_into(nx, ny, discs, mask=None, labels=None, nbodies=0):
    """(mask, labels, nbodies) with the discs of --solid-disc added: (x0, y0, R) in index coordinates, the cells whose centre lies
    inside the circle, each disc a body of its own after the bodies already there (a later disc wins an overlap)."""
    m = np.zeros((int(nx), int(ny)), dtype=bool) if mask is None else np.array(mask) != 0
    lab = np.where(m, 0, -1).astype(np.int32) if labels is None else np.array(labels, dtype=np.int32)
    n = int(nbodies) if labels is not None else int(m.any())
    xs, ys = np.meshgrid(np.arange(int(nx)), np.arange(int(ny)), indexing="ij")
    for x0, y0, R in discs:
        inside = (xs - float(x0)) ** 2 + (ys - float(y0)) ** 2 < float(R) ** 2
        if not R > 0 or not inside.any():
            raise ValueError(f"solid disc {(x0, y0, R)} holds no cell of the {nx} x {ny} lattice")
        m |= inside
        lab[inside] = n
        n += 1
    return m, lab, n


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


def host_body_force(fin, mask, labels, centres, delta=None, shape=None, fpost=None):
    """dict(links, fx, fy, tz) of arrays [nbodies] (nbodies = len(centres)) from the populations fin[9, X, Y] that
    get_fields(want_fin=True) returns: per body the exactly rounded sums (math.fsum) of body_force_terms.  delta:
    wall_delta_field(...) while the bodies move.  shape: the q of a solver with a shape (CavitySolver.shape, the effective q), with
    fpost[9, X, Y], the post-collision populations of the last step: the terms are those of shaped_force_terms and the arm of the
    torque is the wall point."""
    if shape is None:
        b, tx, ty, mx, my = body_force_terms(fin, mask, labels, centres, delta)
    else:
        ln, tx, ty = shaped_force_terms(fin, fpost, mask, labels)
        x, y, k, b = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
        cen = np.asarray(centres, dtype=np.float64)
        qe = np.asarray(shape, dtype=np.float64)[k - 1, x, y]
        rx = (x.astype(np.float64) - qe * np.array(CX, dtype=np.float64)[k]) - cen[b, 0]
        ry = (y.astype(np.float64) + qe * np.array(CY, dtype=np.float64)[k]) - cen[b, 1]
        mx, my = rx * ty, ry * tx
    n = len(centres)
    out = dict(links=np.zeros(n, dtype=np.int64), fx=np.zeros(n), fy=np.zeros(n), tz=np.zeros(n))
    for i in range(n):
        sel = b == i
        out["links"][i] = int(sel.sum())
        out["fx"][i] = math.fsum(tx[sel].tolist())
        out["fy"][i] = math.fsum(ty[sel].tolist())
        out["tz"][i] = math.fsum(mx[sel].tolist() + my[sel].tolist())
    return out


# ---- curved surfaces: a wall distance per link (CavitySolver.set_shape, lbm_set_solid_shape) -------------------------------------------
def _link_arrays(mask):
    """(x, y, k) of every link, slots in order -- and the source cells (sx, sy)."""
    rows = []
    for k, lk in enumerate(links(mask)):
        if k:
            x, y = np.nonzero(lk)
            rows.append(np.stack([x, y, np.full(x.shape, k)], axis=1))
    ln = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 3), dtype=np.int64)
    cx, cy = np.array(CX), np.array(CY)
    return ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 0] - cx[ln[:, 2]], ln[:, 1] + cy[ln[:, 2]]


def disc_fractions(mask, x0, y0, R, q=None):
    """q[8, X, Y] for set_shape: on every link whose cell and source lie on different sides of the circle of radius R about (x0, y0)
    (index coordinates), the exact fraction of the link from the fluid cell to the circle, plane k - 1 for slot k; every other entry
    keeps the value of q (default: 1/2, the half-way wall).  Serves a solid disc (the cells inside) and a ring that is solid outside R
    alike; call it once per circle, passing the result on."""
    m = np.asarray(mask) != 0
    out = np.full((8,) + m.shape, 0.5) if q is None else np.array(q, dtype=np.float64)
    x, y, k, sx, sy = _link_arrays(m)
    px, py = x - float(x0), y - float(y0)
    ex, ey = (sx - x).astype(np.float64), (sy - y).astype(np.float64)
    inside_p = px * px + py * py < R * R
    inside_s = (sx - float(x0)) ** 2 + (sy - float(y0)) ** 2 < R * R
    cross = inside_p != inside_s
    A, B, C = ex * ex + ey * ey, px * ex + py * ey, px * px + py * py - R * R
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.maximum(B * B - A * C, 0.0))
        t = np.where(inside_p, (-B + root) / A, (-B - root) / A)       # leaving the disc: the far root; entering it: the near one
    t = np.clip(t, 2.0 ** -20, 1.0)
    out[k[cross] - 1, x[cross], y[cross]] = t[cross]
    return out


def fractions_from_distance(mask, phi):
    """q[8, X, Y] for set_shape from a signed distance phi[X, Y] at the cell centres (one sign in the fluid, the other in the solid):
    the linear estimate phi(P) / (phi(P) - phi(source)) on every link whose ends differ in sign, clipped into (0, 1]; 1/2 elsewhere."""
    m = np.asarray(mask) != 0
    phi = np.asarray(phi, dtype=np.float64)
    out = np.full((8,) + m.shape, 0.5)
    x, y, k, sx, sy = _link_arrays(m)
    a, b = phi[x, y], phi[sx, sy]
    ok = (a * b < 0.0) | ((a != 0.0) & (b == 0.0))
    with np.errstate(all="ignore"):
        t = np.clip(a / (a - b), 2.0 ** -20, 1.0)
    out[k[ok] - 1, x[ok], y[ok]] = t[ok]
    return out


def shape_table(mask, labels, centres, motion, q, dtype=None):
    """The public restatement of what lbm_set_solid_shape derives: dict of arrays [links] in the order of body_links(mask, labels) --
    links (x, y, k, body), q (the effective one: 1/2 where q < 1/2 and the next cell N = (x + cx_k, y - cy_k) is no fluid cell of the
    lattice), near, a = near ? 2 q : 1 / (2 q), the wall point (rx, ry) = ((x - q cx_k) - x0, (y + q cy_k) - y0), and
    d = near ? delta : a delta with delta = (6 w_k) (cx_k uwx + cy_k uwy) of the motion at the wall point -- float64, every operation
    rounded in this order.  dtype: the lattice type, to which a and d are rounded once."""
    m = np.asarray(mask) != 0
    X, Y = m.shape
    cen, mot, q = np.asarray(centres, dtype=np.float64), np.asarray(motion, dtype=np.float64), np.asarray(q, dtype=np.float64)
    ln = body_links(m, labels)
    x, y, k, b = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
    cx, cy = np.array(CX, dtype=np.float64), np.array(CY, dtype=np.float64)
    nx_, ny_ = x + np.array(CX)[k], y - np.array(CY)[k]
    inside = (nx_ >= 0) & (nx_ < X) & (ny_ >= 0) & (ny_ < Y)
    next_fluid = inside & ~m[np.clip(nx_, 0, X - 1), np.clip(ny_, 0, Y - 1)]
    qv = q[k - 1, x, y]
    near = (qv < 0.5) & next_fluid
    qe = np.where((qv < 0.5) & ~next_fluid, 0.5, qv)
    a = np.where(near, 2.0 * qe, 1.0 / (2.0 * qe))
    rx = (x.astype(np.float64) - qe * cx[k]) - cen[b, 0]
    ry = (y.astype(np.float64) + qe * cy[k]) - cen[b, 1]
    uwx = mot[b, 0] + mot[b, 2] * ry
    uwy = mot[b, 1] + mot[b, 2] * rx
    delta = np.where(k < 5, 2.0 / 3.0, 1.0 / 6.0) * (cx[k] * uwx + cy[k] * uwy)
    d = np.where(near, delta, a * delta)
    if dtype is not None:
        a, d = a.astype(dtype).astype(np.float64), d.astype(dtype).astype(np.float64)
    return dict(links=ln, q=qe, near=near, a=a, d=d, rx=rx, ry=ry)


def shaped_force_terms(fin, fpost, mask, labels=None):
    """(links, tx, ty) of a solver with a shape: per link f_in = fin_k(x, y), the arriving population with the rule applied, as
    get_fields returns it, and f_out = fpost_opp(k)(x, y), the population the cell sent towards the wall; (tx, ty) =
    c_opp(k) (f_out + f_in), both converted to float64 first.  f_out never arrives anywhere and is in no exported field -- only where
    the wall sits half-way does fin_k hold it -- so the post-collision populations fpost[9, X, Y] come from the caller (a reference, or
    a replay of the last step).  links: body_links order with labels, else slots in order."""
    m = np.asarray(mask) != 0
    fin, fpost = np.asarray(fin), np.asarray(fpost)
    if labels is None:
        x, y, k, _, _ = _link_arrays(m)
        ln = np.stack([x, y, k], axis=1)
    else:
        ln = body_links(m, labels)
        x, y, k = ln[:, 0], ln[:, 1], ln[:, 2]
    opp = np.array(OPP)
    t = fpost[opp[k], x, y].astype(np.float64) + fin[k, x, y].astype(np.float64)
    return ln, np.array(CX, dtype=np.float64)[opp[k]] * t, np.array(CY, dtype=np.float64)[opp[k]] * t


# ---- open boundaries: hold cells and a wall velocity per solid cell (CavitySolver.set_open_cells, set_wall_velocity) ---------------------
def equilibrium(rho, ux, uy):
    """feq[9, ...] in float64 of a density and a velocity (scalars or arrays that broadcast): w_k rho (1 + 3 cu + 4.5 cu^2 - 1.5 u^2),
    cu = cx_k ux + cy_k uy, uy > 0 towards the lid -- what a hold cell holds to stand for a stream of that state (set_open_cells)."""
    rho, ux, uy = (np.asarray(a, dtype=np.float64) for a in np.broadcast_arrays(rho, ux, uy))
    w = (4.0 / 9.0,) + (1.0 / 9.0,) * 4 + (1.0 / 36.0,) * 4
    usq = ux * ux + uy * uy
    out = np.empty((9,) + rho.shape)
    for k in range(9):
        cu = CX[k] * ux + CY[k] * uy
        out[k] = w[k] * rho * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * usq)
    return out


def host_open_tables(mask, labels, centres, motion, wall_velocity=None, hold=None, q=None, dtype=None):
    """The public restatement of the per-link deltas of a lattice with hold cells and a wall velocity per solid cell, as shape_table is
    for the shape: dict of arrays [links] in the order of the library's link list -- body_links(mask, labels) without the links that
    start at a hold cell, which bounces nothing.  links (x, y, k, body); delta, float64:

        delta = delta_body + (6 w_k) (cx_k uwx(S) + cy_k uwy(S)),        S = (x - cx_k, y + cy_k) the link's source cell,

    delta_body as wall_deltas forms it at the link's midpoint, then the cell term of wall_velocity[2, X, Y], each product and sum
    rounded in the order written, then the add.  S, A: the sums of delta and |delta| in the list's order; closed: what the flux check
    of set_body_motion / set_wall_velocity decides -- |S| <= links 2^-52 A, and always True on a lattice with a hold cell, which is
    open.  With q[8, X, Y] (set_shape) also q, near, a, d, rx, ry as shape_table gives them, the rigid-body part of delta at the wall
    point and a hold cell counting as no fluid cell behind a link; `delta` stays the midpoint's, which the flux check sums.
    dtype: the lattice type, to which delta (and a, d) are rounded once; S and A are formed before that."""
    m = np.asarray(mask) != 0
    X, Y = m.shape
    h = np.zeros_like(m) if hold is None else np.asarray(hold) != 0
    cen, mot = np.asarray(centres, dtype=np.float64), np.asarray(motion, dtype=np.float64)
    ln = body_links(m, labels)
    ln = ln[~h[ln[:, 0], ln[:, 1]]]
    x, y, k, b = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
    cx, cy = np.array(CX, dtype=np.float64), np.array(CY, dtype=np.float64)
    w6 = np.where(k < 5, 2.0 / 3.0, 1.0 / 6.0)

    def body_term(rx, ry):
        uwx = mot[b, 0] + mot[b, 2] * ry
        uwy = mot[b, 1] + mot[b, 2] * rx
        return w6 * (cx[k] * uwx + cy[k] * uwy)

    cell = None
    if wall_velocity is not None:
        uw = np.where(m[None], np.asarray(wall_velocity, dtype=np.float64), 0.0)
        sx, sy = x - np.array(CX)[k], y + np.array(CY)[k]
        cell = w6 * (cx[k] * uw[0, sx, sy] + cy[k] * uw[1, sx, sy])
    rnd = (lambda v: v) if dtype is None else (lambda v: v.astype(dtype).astype(np.float64))
    delta = body_term((x.astype(np.float64) - 0.5 * cx[k]) - cen[b, 0], (y.astype(np.float64) + 0.5 * cy[k]) - cen[b, 1])
    if cell is not None:
        delta = delta + cell
    S = A = 0.0
    for d in delta.tolist():
        S = S + d
        A = A + abs(d)
    out = dict(links=ln, delta=rnd(delta), S=S, A=A, closed=bool(h.any()) or not abs(S) > len(ln) * 2.0 ** -52 * A)
    if q is not None:
        q = np.asarray(q, dtype=np.float64)
        nx_, ny_ = x + np.array(CX)[k], y - np.array(CY)[k]
        inside = (nx_ >= 0) & (nx_ < X) & (ny_ >= 0) & (ny_ < Y)
        cxn, cyn = np.clip(nx_, 0, X - 1), np.clip(ny_, 0, Y - 1)
        next_fluid = inside & ~m[cxn, cyn] & ~h[cxn, cyn]
        qv = q[k - 1, x, y]
        near = (qv < 0.5) & next_fluid
        qe = np.where((qv < 0.5) & ~next_fluid, 0.5, qv)
        a = np.where(near, 2.0 * qe, 1.0 / (2.0 * qe))
        rx = (x.astype(np.float64) - qe * cx[k]) - cen[b, 0]
        ry = (y.astype(np.float64) + qe * cy[k]) - cen[b, 1]
        dw = body_term(rx, ry)
        if cell is not None:
            dw = dw + cell
        out.update(q=qe, near=near, a=rnd(a), d=rnd(np.where(near, dw, a * dw)), rx=rx, ry=ry)
    return out
