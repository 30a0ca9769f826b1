"""The field residual in NumPy, and the host side of its C ABI (include/lbm.h, `lbm_residual_*`).

A steady run is converged when its fields stop changing.  The library compares every sample of u and rho with the previous one, which
it keeps on the device, and reduces the differences to a small record per lattice; :func:`host_residual` is that record stated in
NumPy -- the documentation of the contract, the checker the tests compare the device with, and the way to the same numbers for users
without a GPU.  Everything in a record equals host_residual of two get_fields() results exactly, except the three sums, which depend on
the order of summation (the device's is a fixed tree, NumPy's pairwise)."""
import numpy as np

from ._lib import lbm_residual_record  # noqa: F401  (the ctypes mirror of the header's struct)
from .monitor import fields_to_dict

FIELDS = ("step", "step_prev", "cells", "nonfinite", "sum_du2", "sum_u2", "sum_drho2", "max_du2", "max_x", "max_y", "max_drho2")
INTEGERS = ("step", "step_prev", "cells", "nonfinite", "max_x", "max_y")
RECORD_DOUBLES = len(FIELDS)


def host_residual(u_prev, rho_prev, u, rho, rows=None, step=None, step_prev=None):
    """The residual record of two consecutive samples u_prev[2, X, Y], rho_prev[X, Y] and u, rho (what get_fields(out_dtype) returned
    at the two step counts), as a dict.  Every value is converted to float64; per cell

        d2 = (ux - pux) ** 2 + (uy - puy) ** 2,   u2 = ux ** 2 + uy ** 2,   dr2 = (rho - prho) ** 2

    and a cell takes part only if all six of its values are finite.

    cells, nonfinite             cells that take part / that do not
    sum_du2, sum_u2, sum_drho2   float64 sums over the cells that take part
    max_du2, max_x, max_y        the maximum of d2 over the same cells and its cell: np.argmax on the [X][Y] array, so ties go to the
                                 smaller x, then the smaller y.  No cell takes part: (-inf, -1, -1)
    max_drho2                    the maximum of dr2 (-inf when no cell takes part)

    rows=(y0, ny_local): the record of a slab that owns these rows only."""
    u_prev, rho_prev, u, rho = (np.asarray(a) for a in (u_prev, rho_prev, u, rho))
    _, X, Y = u.shape
    y0, nyl = (0, Y) if rows is None else (int(rows[0]), int(rows[1]))
    ux, uy, r = u[0].astype(np.float64), u[1].astype(np.float64), rho.astype(np.float64)
    pux, puy, pr = u_prev[0].astype(np.float64), u_prev[1].astype(np.float64), rho_prev.astype(np.float64)
    own = np.zeros((X, Y), dtype=bool)
    own[:, y0:y0 + nyl] = True
    finite = np.isfinite(ux) & np.isfinite(uy) & np.isfinite(r) & np.isfinite(pux) & np.isfinite(puy) & np.isfinite(pr)
    ok = own & finite
    with np.errstate(all="ignore"):
        dux, duy, dr = ux - pux, uy - puy, r - pr
        d2 = dux * dux + duy * duy
        u2 = ux * ux + uy * uy
        dr2 = dr * dr
    out = dict(step=step, step_prev=step_prev, cells=int(np.count_nonzero(ok)), nonfinite=int(np.count_nonzero(own & ~finite)),
               sum_du2=float(np.sum(d2[ok])), sum_u2=float(np.sum(u2[ok])), sum_drho2=float(np.sum(dr2[ok])))
    if ok.any():
        loc = np.unravel_index(np.argmax(np.where(ok, d2, -np.inf)), d2.shape)
        out.update(max_du2=float(d2[loc]), max_x=int(loc[0]), max_y=int(loc[1]), max_drho2=float(np.max(dr2[ok])))
    else:
        out.update(max_du2=-np.inf, max_x=-1, max_y=-1, max_drho2=-np.inf)
    return out


def combine(records):
    """The record of the whole lattice from the records of its slabs, in rank order (dicts of scalars as CavitySolver.residual_series()
    [i] / host_residual return them): cells, nonfinite and the sums added in rank order, the maximum of d2 by (d2, x, y) -- the larger
    d2, then the smaller x, then the smaller y --, the maximum of dr2 across the slabs."""
    records = list(records)
    out = dict(step=records[0]["step"], step_prev=records[0]["step_prev"])
    for k in ("cells", "nonfinite", "sum_du2", "sum_u2", "sum_drho2"):
        acc = records[0][k]
        for r in records[1:]:
            acc = acc + r[k]
        out[k] = acc
    cands = [(-float(r["max_du2"]), int(r["max_x"]), int(r["max_y"])) for r in records if int(r["max_x"]) >= 0]
    if cands:
        q, out["max_x"], out["max_y"] = min(cands)
        out["max_du2"] = -q
    else:
        out["max_du2"], out["max_x"], out["max_y"] = -np.inf, -1, -1
    out["max_drho2"] = max(float(r["max_drho2"]) for r in records)
    return out


def norms(record, uLB):
    """The usual residual norms of a record (scalars, or arrays of records as residual_series() returns them):

    rel_l2    sqrt(sum_du2 / sum_u2): the change of u relative to u, in the L2 norm
    rms_du    sqrt(sum_du2 / cells) / uLB
    max_du    sqrt(max_du2) / uLB
    rms_drho  sqrt(sum_drho2 / cells)

    and each of them per step (`<name>_per_step`), divided by step - step_prev."""
    with np.errstate(all="ignore"):
        cells = np.asarray(record["cells"], dtype=np.float64)
        out = dict(rel_l2=np.sqrt(np.asarray(record["sum_du2"], dtype=np.float64) / np.asarray(record["sum_u2"], dtype=np.float64)),
                   rms_du=np.sqrt(np.asarray(record["sum_du2"], dtype=np.float64) / cells) / float(uLB),
                   max_du=np.sqrt(np.asarray(record["max_du2"], dtype=np.float64)) / float(uLB),
                   rms_drho=np.sqrt(np.asarray(record["sum_drho2"], dtype=np.float64) / cells))
        dn = np.asarray(record["step"], dtype=np.float64) - np.asarray(record["step_prev"], dtype=np.float64)
        for k in list(out):
            out[k + "_per_step"] = out[k] / dn
    if np.ndim(cells) == 0:
        out = {k: float(v) for k, v in out.items()}
    return out


def below(value, tol):
    """The stop test of the front ends: a residual that is not a number (nothing took part, or a division 0 / 0) never passes."""
    return bool(np.isfinite(value) and value < tol)


# -- the C ABI's struct ---------------------------------------------------------------------
def records_to_dict(buf, shape):
    """An array of lbm_residual_record (ctypes) -> dict of float64 arrays of `shape`; the counts, steps and the cell as int64."""
    return fields_to_dict(buf, shape, RECORD_DOUBLES, FIELDS, INTEGERS)[1]


def record_at(series, i, b=None):
    """Record i of a residual_series() dict (lattice b of a batch) as a dict of scalars."""
    return {k: (series[k][i] if b is None else series[k][i, b]) for k in FIELDS}


def latest(series, seen, b=None):
    """The newest record of a residual_series() dict (lattice b of a batch) if the series holds more than the `seen` records the caller
    has had, else None: the first sample of a run only fills the snapshot and leaves no record."""
    return record_at(series, series["count"] - 1, b) if series["count"] > seen else None
