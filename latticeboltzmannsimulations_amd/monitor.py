"""The run monitor in NumPy, and the host side of its C ABI (include/lbm.h, `lbm_monitor*`).

An output iteration of the reference (MRT_GPU.py:752-889) downloads u and rho and computes from them two NaN-masked arg-mins of |u|^2
(the vortex search), np.mean(u) and the centre lines.  The library reduces the same fields on the device to a small record per
lattice; :func:`host_monitor` is that record stated in NumPy -- the documentation of the contract, the checker the tests compare the
device with, and the way to the same numbers for users without a GPU.  Everything in a record equals host_monitor(get_fields())
exactly, except the four sums, which depend on the order of summation (the device's is a fixed tree, NumPy's pairwise)."""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import lbm_monitor_record, lbm_monitor_spec  # noqa: F401  (the ctypes mirrors of the header's structs)

MAX_BOXES, MAX_PROBES = L.LBM_MONITOR_MAX_BOXES, L.LBM_MONITOR_MAX_PROBES
SCALARS = ("step", "nonfinite", "sum_ux", "sum_uy", "sum_rho", "sum_q", "max_q", "min_q", "min_x", "min_y")
RECORD_DOUBLES = len(SCALARS) + 3 * MAX_PROBES


def normalise(X, Y, window=None, exclude=(), probes=()):
    """(window, boxes, probes) as tuples of ints, checked against an X x Y lattice: window and boxes (x_lo, x_hi, y_lo, y_hi), half
    open, global rows, 0 <= lo <= hi <= size; probes (x, y), cells of the lattice.  window=None: the whole lattice."""
    X, Y = int(X), int(Y)

    def box(b, what):
        b = tuple(int(v) for v in b)
        if len(b) != 4 or not (0 <= b[0] <= b[1] <= X and 0 <= b[2] <= b[3] <= Y):
            raise ValueError(f"{what} {b} is not (x_lo, x_hi, y_lo, y_hi) inside the {X} x {Y} lattice")
        return b
    win = (0, X, 0, Y) if window is None else box(window, "window")
    boxes = tuple(box(b, "exclusion box") for b in exclude)
    if len(boxes) > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} exclusion boxes")
    pr = tuple(tuple(int(v) for v in p) for p in probes)
    if len(pr) > MAX_PROBES:
        raise ValueError(f"at most {MAX_PROBES} probes")
    for p in pr:
        if len(p) != 2 or not (0 <= p[0] < X and 0 <= p[1] < Y):
            raise ValueError(f"probe {p} is not a cell (x, y) of the {X} x {Y} lattice")
    return win, boxes, pr


def vortex_window(X, Y):
    """(off, window) of the reference's vortex search (MRT_GPU.py:764-772, ghia.locate_vortices): off = int(X / 40) cells along
    every wall are left out, and one more along the far walls."""
    off = int(X / 40)
    return off, (off, X - 1 - off, off, Y - 1 - off)


def vortex_box(loc, off):
    """The box ghia.locate_vortices blanks around the first minimum before it searches the second."""
    return (max(loc[0] - off, 0), loc[0] + off, max(loc[1] - off, 0), loc[1] + off)


def host_monitor(u, rho, uLB, window=None, exclude=(), probes=(), rows=None, step=None):
    """The monitor record of the fields u[2, X, Y], rho[X, Y] (what get_fields(out_dtype) returns), as a dict:

    nonfinite              cells where any of ux, uy, rho is not finite; they are left out of everything below but the probes
    sum_ux, sum_uy, sum_rho, sum_q   float64 sums over the finite cells; q = (ux * ux + uy * uy) / (uLB * uLB) in float64
    max_q                  the maximum of q over the finite cells (-inf when there is none)
    min_q, min_x, min_y    the minimum of q over the finite cells inside `window` and outside every box of `exclude`, and its cell:
                           np.nanargmin on the [X][Y] array, so ties go to the smaller x, then the smaller y.  No candidate:
                           (+inf, -1, -1)
    probe                  [len(probes), 3]: ux, uy, rho at the probe cells, float64

    rows=(y0, ny_local): the record of a slab that owns these rows only (probes in other rows are NaN)."""
    u, rho = np.asarray(u), np.asarray(rho)
    _, X, Y = u.shape
    win, boxes, pr = normalise(X, Y, window, exclude, probes)
    y0, nyl = (0, Y) if rows is None else (int(rows[0]), int(rows[1]))
    ux, uy, r = u[0].astype(np.float64), u[1].astype(np.float64), rho.astype(np.float64)
    own = np.zeros((X, Y), dtype=bool)
    own[:, y0:y0 + nyl] = True
    finite = np.isfinite(ux) & np.isfinite(uy) & np.isfinite(r)
    ok = own & finite
    with np.errstate(all="ignore"):
        q = (ux * ux + uy * uy) / (float(uLB) * float(uLB))
    region = np.zeros((X, Y), dtype=bool)
    region[win[0]:win[1], win[2]:win[3]] = True
    for b in boxes:
        region[b[0]:b[1], b[2]:b[3]] = False
    region &= ok
    out = dict(step=step, nonfinite=int(np.count_nonzero(own & ~finite)),
               sum_ux=float(np.sum(ux[ok])), sum_uy=float(np.sum(uy[ok])), sum_rho=float(np.sum(r[ok])), sum_q=float(np.sum(q[ok])),
               max_q=float(np.max(q[ok])) if ok.any() else -np.inf)
    if region.any():
        cand = np.where(region, q, np.nan)
        loc = np.unravel_index(np.nanargmin(cand), cand.shape)
        out.update(min_q=float(q[loc]), min_x=int(loc[0]), min_y=int(loc[1]))
    else:
        out.update(min_q=np.inf, min_x=-1, min_y=-1)
    probe = np.full((len(pr), 3), np.nan)
    for i, (x, y) in enumerate(pr):
        if y0 <= y < y0 + nyl:
            probe[i] = ux[x, y], uy[x, y], r[x, y]
    out["probe"] = probe
    return out


def host_locate_vortices(u, rho, uLB):
    """ghia.locate_vortices composed from two monitor records, the way CavitySolver.locate_vortices composes two device passes."""
    _, X, Y = np.asarray(u).shape
    off, win = vortex_window(X, Y)
    a = host_monitor(u, rho, uLB, window=win)
    loc1 = (a["min_x"], a["min_y"])
    b = host_monitor(u, rho, uLB, window=win, exclude=(vortex_box(loc1, off),))
    return loc1, (b["min_x"], b["min_y"])


# -- the C ABI's structs ---------------------------------------------------------------------
def make_spec(X, Y, host_dtype, window=None, exclude=(), probes=()):
    """lbm_monitor_spec for an X x Y lattice (host_dtype: LBM_F32 | LBM_F64); ValueError for anything outside the lattice."""
    win, boxes, pr = normalise(X, Y, window, exclude, probes)
    s = lbm_monitor_spec()
    s.struct_size = ctypes.sizeof(lbm_monitor_spec)
    s.host_dtype = int(host_dtype)
    s.x_lo, s.x_hi, s.y_lo, s.y_hi = win
    s.nboxes, s.nprobes = len(boxes), len(pr)
    for i, b in enumerate(boxes):
        for j in range(4):
            s.box[i][j] = b[j]
    for i, p in enumerate(pr):
        s.probe[i][0], s.probe[i][1] = p
    return s


def fields_to_dict(buf, shape, doubles, names, integers):
    """An array of records (ctypes) of `doubles` float64 each -> (a, out): the float64 array of shape + (doubles,) and the dict of
    its leading fields `names` as arrays of `shape`, those of `integers` as int64.  Shared with residual.records_to_dict."""
    full = tuple(shape) + (doubles,)
    a = np.frombuffer(buf, dtype=np.float64).reshape(full).copy() if ctypes.sizeof(buf) else np.zeros(full)
    out = {k: a[..., i] for i, k in enumerate(names)}
    for k in integers:
        out[k] = out[k].astype(np.int64)
    return a, out


def records_to_dict(buf, shape, nprobes):
    """An array of lbm_monitor_record (ctypes) -> dict of float64 arrays of `shape` (probe: shape + (nprobes, 3)); min_x, min_y and
    nonfinite as int64."""
    a, out = fields_to_dict(buf, shape, RECORD_DOUBLES, SCALARS, ("step", "nonfinite", "min_x", "min_y"))
    out["probe"] = a[..., len(SCALARS):].reshape(tuple(shape) + (MAX_PROBES, 3))[..., :nprobes, :]
    return out


def combine(records):
    """The record of the whole lattice from the records of its slabs, in rank order (dicts of scalars as CavitySolver.monitor()
    returns them): sums and nonfinite added in rank order, the maximum across the slabs, the minimum by (q, x, y), every probe from
    the slab that owns its row."""
    records = list(records)
    out = dict(step=records[0]["step"])
    for k in ("nonfinite", "sum_ux", "sum_uy", "sum_rho", "sum_q"):
        acc = records[0][k]
        for r in records[1:]:
            acc = acc + r[k]
        out[k] = acc
    out["max_q"] = max(float(r["max_q"]) for r in records)
    cands = [(float(r["min_q"]), int(r["min_x"]), int(r["min_y"])) for r in records if int(r["min_x"]) >= 0]
    out["min_q"], out["min_x"], out["min_y"] = min(cands) if cands else (np.inf, -1, -1)
    probe = np.array(records[0]["probe"], dtype=np.float64, copy=True)
    for r in records[1:]:
        p = np.asarray(r["probe"])
        take = ~np.isnan(p).all(axis=-1)
        probe[take] = p[take]
    out["probe"] = probe
    return out
