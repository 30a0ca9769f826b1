"""Stream function, vorticity and the vortex table in NumPy, and the host side of their C ABI (include/lbm.h, `lbm_topology`,
`lbm_get_stream_function`).

The quantity that names the vortices of the cavity is the stream function psi: the primary vortex is its extremum, the corner eddies
are the extrema of the opposite sign in their corners (Ghia, Ghia & Shin tabulate psi and the vorticity at exactly those points).
The library computes psi, the vorticity omega and the extrema of psi inside up to eight windows on the device;
:func:`host_stream_function` and :func:`host_topology` are the same quantities stated in NumPy operation for operation -- the
documentation of the contract, the checker the tests compare the device with (every bit), and the way to the same numbers without
a GPU.  :func:`vortex_table` composes Ghia's named vortices from one record of four windows.

Frame: the index y runs away from the lid and u[1] > 0 points towards the lid, so (x, Y = -y) with (ux, uy) is right-handed;
ux = d psi / dY, uy = -d psi / dx; omega = d uy / dx - d ux / dY is counter-clockwise positive (Ghia's table lists -omega)."""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import lbm_topology_record, lbm_topology_spec  # noqa: F401  (the ctypes mirrors of the header's structs)

MAX_WINDOWS = L.LBM_TOPOLOGY_MAX_WINDOWS
BLOCK = L.LBM_TOPOLOGY_BLOCK             # = LBM_TOPOLOGY_BLOCK of include/lbm.h: cells of x per block of the prefix sum
RECORD_DOUBLES = 2 + 8 * MAX_WINDOWS
VORTICES = ("Primary", "Top", "BL1", "BR1")   # the names vortex_table composes, = rows 0 .. 3 of ghia.VORTEX_GHIA


def normalise(X, Y, windows):
    """The windows as tuples of ints (x_lo, x_hi, y_lo, y_hi), half open, checked against an X x Y lattice: at most MAX_WINDOWS,
    0 <= lo <= hi <= size."""
    X, Y = int(X), int(Y)
    out = []
    for w in windows:
        w = tuple(int(v) for v in w)
        if len(w) != 4 or not (0 <= w[0] <= w[1] <= X and 0 <= w[2] <= w[3] <= Y):
            raise ValueError(f"window {w} is not (x_lo, x_hi, y_lo, y_hi) inside the {X} x {Y} lattice")
        out.append(w)
    if len(out) > MAX_WINDOWS:
        raise ValueError(f"at most {MAX_WINDOWS} windows")
    return tuple(out)


def _diff(v, axis):
    """d/di along `axis`: central inside (0.5 * (v[i + 1] - v[i - 1])), one-sided at either end (v[1] - v[0], v[n - 1] - v[n - 2])."""
    v = np.moveaxis(v, axis, 0)
    d = np.empty_like(v)
    d[1:-1] = 0.5 * (v[2:] - v[:-2])
    d[0] = v[1] - v[0]
    d[-1] = v[-1] - v[-2]
    return np.moveaxis(d, 0, axis)


def host_stream_function(u):
    """(psi, omega), float64 [X, Y], of the field u[2, X, Y] (what get_fields(out_dtype) returns; every value is converted to float64
    first).  psi is integrated along x from the left wall, row by row: t[0] = 0, t[x] = 0.5 * (uy[x - 1] + uy[x]), summed in blocks of
    BLOCK cells of x -- inside a block the running sum strictly left to right (np.cumsum), across blocks the offsets strictly in order
    -- psi = -(offset + running sum).  omega = dvdx + dudy with central differences inside and one-sided ones on the border."""
    u = np.asarray(u)
    ux, uy = u[0].astype(np.float64), u[1].astype(np.float64)
    X, Y = ux.shape
    with np.errstate(all="ignore"):
        t = np.zeros((X, Y))
        t[1:] = 0.5 * (uy[:-1] + uy[1:])
        psi = np.empty((X, Y))
        off = np.zeros(Y)
        for b in range(0, X, BLOCK):
            c = np.cumsum(t[b:b + BLOCK], axis=0)
            psi[b:b + BLOCK] = -(off + c)
            off = off + c[-1]
        omega = _diff(uy, 0) + _diff(ux, 1)
    return psi, omega


def _extremum(psi, omega, win, largest):
    """dict(psi, x, y, omega) of the minimum (largest: the maximum) of psi over the cells of `win` whose psi is finite; ties go to the
    smaller x, then the smaller y.  No candidate: psi = +inf (-inf), cell (-1, -1), omega = NaN."""
    sub = psi[win[0]:win[1], win[2]:win[3]]
    ok = np.isfinite(sub)
    if not ok.any():
        return dict(psi=-np.inf if largest else np.inf, x=-1, y=-1, omega=np.nan)
    best = sub[ok].max() if largest else sub[ok].min()
    i, j = np.unravel_index(np.argmax(ok & (sub == best)), sub.shape)     # the first hit in (x, y) order
    x, y = win[0] + int(i), win[2] + int(j)
    return dict(psi=float(psi[x, y]), x=x, y=y, omega=float(omega[x, y]))


def host_topology(u, uLB, windows, step=None):
    """The topology record of the field u[2, X, Y], as a dict: step; closure, the maximum of |psi[X - 1, y]| over the rows where it is
    finite (-inf if none) -- the net flux a row fails to close, a quality figure: the wet-node walls do not conserve mass, so it is
    not zero, and an extremum whose |psi| is not well above it is not resolved; window, a list with dict(min=..., max=...) per
    window, each extremum a dict(psi, x, y, omega) (see _extremum).  uLB is not used by the record (psi and omega are in lattice
    units); it is accepted so that the call reads like monitor.host_monitor."""
    u = np.asarray(u)
    _, X, Y = u.shape
    wins = normalise(X, Y, windows)
    psi, omega = host_stream_function(u)
    edge = np.abs(psi[X - 1])
    edge = edge[np.isfinite(edge)]
    return dict(step=step, closure=float(edge.max()) if edge.size else -np.inf,
                window=[dict(min=_extremum(psi, omega, w, False), max=_extremum(psi, omega, w, True)) for w in wins])


# -- Ghia's named vortices ---------------------------------------------------------------------
def vortex_windows(X, Y):
    """The four windows of vortex_table, in the order of VORTICES: the interior (1, X - 1, 1, Y - 1) for Primary, the quadrant at the
    lid's left end for Top, the bottom-left quadrant for BL1, the bottom-right one for BR1 (y = 0 is the lid)."""
    X, Y = int(X), int(Y)
    return ((1, X - 1, 1, Y - 1), (0, X // 2, 0, Y // 2), (0, X // 2, Y // 2, Y), (X // 2, X, Y // 2, Y))


def _inside(e, win):
    """The extremum is a cell of the window that is not on the window's border (one cut by the edge is a slope, not a centre)."""
    return e["x"] >= 0 and win[0] < e["x"] < win[1] - 1 and win[2] < e["y"] < win[3] - 1


def vortex_table(record, X, Y):
    """Ghia's named vortices from ONE topology record of the windows vortex_windows(X, Y): dict name -> dict(x, y, psi, omega) or None
    (absent).  Primary is the cell of the largest |psi| in the interior window -- the larger in magnitude of that window's minimum and
    maximum -- and s the sign of psi there.  Top, BL1 and BR1 are the extremum of -s * psi in their windows.  A vortex is absent unless
    -s * psi > 0 at that cell (Primary: psi != 0) and the cell is not on its window's border."""
    wins = vortex_windows(X, Y)
    w = record["window"]
    lo, hi = w[0]["min"], w[0]["max"]
    table = {name: None for name in VORTICES}
    if lo["x"] < 0:
        return table
    prim = lo if abs(lo["psi"]) >= abs(hi["psi"]) else hi
    s = np.sign(prim["psi"])
    if s == 0:
        return table
    pick = lambda e: dict(x=int(e["x"]), y=int(e["y"]), psi=float(e["psi"]), omega=float(e["omega"]))   # noqa: E731
    if _inside(prim, wins[0]):
        table["Primary"] = pick(prim)
    for i in (1, 2, 3):
        e = w[i]["max"] if s < 0 else w[i]["min"]
        if e["x"] >= 0 and -s * e["psi"] > 0 and _inside(e, wins[i]):
            table[VORTICES[i]] = pick(e)
    return table


def host_vortex_table(u, uLB):
    """vortex_table of the field u[2, X, Y] through host_topology: the numbers CavitySolver.vortex_table() gives, without a GPU."""
    _, X, Y = np.asarray(u).shape
    return vortex_table(host_topology(u, uLB, vortex_windows(X, Y)), X, Y)


# -- the C ABI's structs ---------------------------------------------------------------------
def make_spec(X, Y, host_dtype, windows=()):
    """lbm_topology_spec for an X x Y lattice (host_dtype: LBM_F32 | LBM_F64); ValueError for anything outside the lattice."""
    wins = normalise(X, Y, windows)
    s = lbm_topology_spec()
    s.struct_size = ctypes.sizeof(lbm_topology_spec)
    s.host_dtype = int(host_dtype)
    s.nwindows = len(wins)
    for i, w in enumerate(wins):
        for j in range(4):
            s.window[i][j] = w[j]
    return s


def records_to_dict(buf, nwindows):
    """An array of lbm_topology_record (ctypes) -> a list with one dict per record, in the form of host_topology (x, y and step as int)."""
    a = np.frombuffer(buf, dtype=np.float64).reshape(-1, RECORD_DOUBLES)
    out = []
    for r in a:
        e = r[2:].reshape(MAX_WINDOWS, 2, 4)
        ext = lambda v: dict(psi=float(v[0]), x=int(v[1]), y=int(v[2]), omega=float(v[3]))   # noqa: E731
        out.append(dict(step=int(r[0]), closure=float(r[1]), window=[dict(min=ext(e[i, 0]), max=ext(e[i, 1])) for i in range(nwindows)]))
    return out
