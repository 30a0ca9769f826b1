"""The states, comparisons and bounds the tests share; each has its one definition here.  tests/test_checks_cpu.py pins the
comparators themselves: one that wrongly passes would weaken every test that relies on it.  The case grids and the shared case
tables are in tests/cases.py."""
import ctypes
import warnings

import numpy as np

from cases import windows
from latticeboltzmannsimulations_amd import monitor, residual
from latticeboltzmannsimulations_amd import topology as T

W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)      # the D2Q9 weights

# fast arithmetic against strict fp64 under bounce-back walls (the GPU's strict fp64 = the reference, bit for bit,
# tests/test_bounce_back_gpu.py): max |f_fast - f_ref| / max |f_ref| over the populations after 2000 steps of a 128 x 96 lattice at
# Re 1000, every operator.  Measured (MI355X, FAST_MEASURED: the fp32 figures are mostly fp32's own distance from fp64); the bounds are
# the largest of each type with a factor of four of headroom, as tests/test_arith_error_budget_gpu.py sets its bounds.  The tighter
# check, against a long-double reference from off-equilibrium states after 1 .. 26 steps, is that file's
# test_fast_stays_within_the_budget_under_the_other_walls.  A solid mask selects populations and adds no arithmetic, and the moving-wall
# term is one more exact constant per link, so the obstacle and moving-body tests hold `fast` to the same bound.
FAST_MEASURED = {(np.float32, "SRT"): 2.940e-05, (np.float32, "TRT"): 2.956e-05, (np.float32, "MRT"): 1.616e-05,
                 (np.float64, "SRT"): 1.419e-14, (np.float64, "TRT"): 1.476e-14, (np.float64, "MRT"): 2.920e-15}
FAST_BOUND = {np.float32: 1.2e-4, np.float64: 6e-14}


# ---- states --------------------------------------------------------------------------------------------------------------------------
def perturbed(nx, ny, dtype, seed):
    """A non-trivial state for set_state: equilibrium-like populations with a seeded perturbation of a few per cent."""
    rng = np.random.default_rng(seed)
    return (W[:, None, None] * (1.0 + 0.03 * rng.standard_normal((9, nx, ny)))).astype(dtype)


def rest(nx, ny, dtype):
    """The rest state: every population is its weight."""
    return np.ascontiguousarray(np.broadcast_to(W[:, None, None], (9, nx, ny))).astype(dtype)


def smooth_state(nx, ny, dtype):
    """A smooth non-trivial state for slabs in loopback: such a slab never sees the lid, so from the rest state all its rows stay
    equal and a kernel that read a stale or not-yet-written row would go unnoticed."""
    x = np.arange(nx, dtype=np.float64)[:, None]
    y = np.arange(ny, dtype=np.float64)[None, :]
    base = 1.0 + 1e-3 * np.sin(0.01 * x) * np.cos(0.013 * y) + 5e-4 * np.cos(0.0037 * (x + 2 * y))
    fin = np.empty((9, nx, ny), dtype=dtype)
    for k in range(9):
        fin[k] = (base * (W[k] * (1.0 + 1e-4 * k))).astype(dtype)
    return fin


# ---- fields of a solver ----------------------------------------------------------------------------------------------------------------
def same_as_oracle(solver, oracle, what="state", finite=True):
    """fin, rho and u of a solver are the oracle's bits (and finite, unless finite=False); returns (u, rho, fin)."""
    u, rho, fin = solver.get_fields(want_fin=True)
    if finite:
        assert np.isfinite(fin).all() and np.isfinite(u).all() and np.isfinite(rho).all(), f"{what}: not finite"
    assert np.array_equal(fin, oracle.fin), f"{what}: fin differs in {np.count_nonzero(fin != oracle.fin)} values, max abs {np.abs(fin - oracle.fin).max()}"
    assert np.array_equal(rho, oracle.rho), f"{what}: rho differs"
    assert np.array_equal(u, oracle.u), f"{what}: u differs"
    return u, rho, fin


def same_fields(a, b, what):
    """u, rho and fin of a are finite and the bits of b's; a, b: two solvers, or two (u, rho, fin) tuples."""
    fa, fb = (x.get_fields(want_fin=True) if hasattr(x, "get_fields") else x for x in (a, b))
    for x, y, name in zip(fa, fb, ("u", "rho", "fin")):
        assert np.isfinite(x).all(), f"{what}: {name} not finite"
        assert np.array_equal(x, y), f"{what}: {name} differs in {np.count_nonzero(x != y)} values, max abs {np.abs(x - y).max()}"


# ---- records ---------------------------------------------------------------------------------------------------------------------------
def nan_equal(a, b):
    """Equal, or both NaN."""
    return a == b or (a != a and b != b)


def same_bits(a, b, keys, what):
    """Two records (dicts of scalars or arrays) hold the same values under `keys`, NaN equal to NaN."""
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), f"{what}: {k} differs: {a[k]} {b[k]}"


def reordered_sum_bound(terms):
    """2 gamma_n sum |x_i| over the finite terms: a sum of n doubles in any order is within gamma_n = n eps / (1 - n eps), eps = 2^-53,
    times sum |x_i| of the exact sum, so two orders differ by at most twice that."""
    x = np.asarray(terms, dtype=np.float64)
    x = x[np.isfinite(x)]
    n = x.size
    g = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    return 2.0 * g * float(np.abs(x).sum())


# ---- the samplers against their host statements (their own GPU tests, and the masked lattice of tests/test_solid_gpu.py) -------------
MON_EXACT = ("step", "nonfinite", "max_q", "min_q", "min_x", "min_y")
MON_SUMS = ("sum_ux", "sum_uy", "sum_rho", "sum_q")
RES_EXACT = ("step", "step_prev", "cells", "nonfinite", "max_du2", "max_x", "max_y", "max_drho2")
RES_SUMS = ("sum_du2", "sum_u2", "sum_drho2")


def monitor_sum_bounds(u, rho, uLB, rows=None):
    """reordered_sum_bound for the monitor's four sums, over the cells whose ux, uy and rho are all finite."""
    y0, n = (0, u.shape[2]) if rows is None else rows
    ux, uy, r = (a[:, y0:y0 + n].astype(np.float64) for a in (u[0], u[1], rho))
    ok = np.isfinite(ux) & np.isfinite(uy) & np.isfinite(r)
    with np.errstate(all="ignore"):
        q = (ux * ux + uy * uy) / (uLB * uLB)
    return {k: reordered_sum_bound(a[ok]) for k, a in zip(MON_SUMS, (ux, uy, r, q))}


def same_monitor_record(got, u, rho, uLB, what, rows=None, **spec):
    """A device record against monitor.host_monitor of the fields: exact fields exactly, the sums within monitor_sum_bounds."""
    want = monitor.host_monitor(u, rho, uLB, rows=rows, step=got["step"], **spec)
    for k in MON_EXACT:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    assert np.array_equal(got["probe"], want["probe"], equal_nan=True), f"{what}: probes"
    tol = monitor_sum_bounds(u, rho, uLB, rows)
    for k in MON_SUMS:
        assert abs(got[k] - want[k]) <= tol[k], f"{what}: {k} off by {abs(got[k] - want[k])}, bound {tol[k]}"
    return want


def residual_terms(prev, cur, rows=None):
    """(ok, d2, u2, dr2) of two (u, rho) samples in float64, restricted to the rows of a slab."""
    y0, n = (0, cur[0].shape[2]) if rows is None else rows
    a = [x[..., y0:y0 + n].astype(np.float64) for x in (prev[0][0], prev[0][1], prev[1], cur[0][0], cur[0][1], cur[1])]
    ok = np.all([np.isfinite(x) for x in a], axis=0)
    with np.errstate(all="ignore"):
        dux, duy, dr = a[3] - a[0], a[4] - a[1], a[5] - a[2]
        return ok, dux * dux + duy * duy, a[3] * a[3] + a[4] * a[4], dr * dr


def residual_sum_bounds(prev, cur, rows=None):
    """reordered_sum_bound for the residual's three sums, over the cells that are finite in both samples."""
    ok, d2, u2, dr2 = residual_terms(prev, cur, rows)
    return {k: reordered_sum_bound(t[ok]) for k, t in zip(RES_SUMS, (d2, u2, dr2))}


def same_residual_record(got, prev, cur, what, rows=None):
    """got: a record of the device; prev, cur: (step, u, rho) of the two samples."""
    want = residual.host_residual(prev[1], prev[2], cur[1], cur[2], rows=rows, step=cur[0], step_prev=prev[0])
    for k in RES_EXACT:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    tol = residual_sum_bounds(prev[1:], cur[1:], rows)
    for k in RES_SUMS:
        print(f"{what}: {k} device {got[k]!r} host {want[k]!r} bound {tol[k]!r}")
        assert abs(got[k] - want[k]) <= tol[k], f"{what}: {k} off by {abs(got[k] - want[k])}, bound {tol[k]}"
    return want


class HostStats:
    """The host loop of the time statistics: acc += u.astype(f64); acc2 += u64 * u64; ...; acc / count."""

    def __init__(self):
        self.S, self.n = None, 0

    def add(self, u, rho):
        u, rho = u.astype(np.float64), rho.astype(np.float64)
        ux, uy = u[..., 0, :, :], u[..., 1, :, :]
        terms = [u, rho, np.stack([ux * ux, uy * uy, ux * uy], axis=-3)]
        self.S = terms if self.S is None else [a + b for a, b in zip(self.S, terms)]
        self.n += 1

    def means(self):
        return [a / self.n for a in self.S] + [self.n]


def raw_stats(s):
    """lbm_stats_get as it comes: (E[u], E[rho], [E[uu], E[vv], E[uv]], count), float64, whole-lattice shaped."""
    lead = s._lead
    mu, mrho, sec = np.zeros(lead + (2, s.nx, s.ny)), np.zeros(lead + (s.nx, s.ny)), np.zeros(lead + (3, s.nx, s.ny))
    n = ctypes.c_longlong(-1)
    rc = s.lib.lbm_stats_get(s._h, mu.ctypes.data, mrho.ctypes.data, sec.ctypes.data, ctypes.byref(n))
    assert rc == 0, s.lib.lbm_last_error(s._h)
    return mu, mrho, sec, n.value


def same_stats(s, host, what):
    """The device statistics of s are the bits of a HostStats."""
    got = raw_stats(s)
    if host.n == 0:
        assert got[3] == 0, f"{what}: {got[3]} samples, host none"
        return
    want = host.means()
    assert got[3] == want[3], f"{what}: {got[3]} samples, host {want[3]}"
    for name, a, b in zip(("u", "rho", "second"), got[:3], want[:3]):
        assert np.array_equal(a, b), f"{what}: E[{name}] differs, max abs {np.abs(a - b).max()}"


def same_topology_record(got, want, what):
    assert got["step"] == want["step"], f"{what}: step {got['step']} != {want['step']}"
    assert got["closure"] == want["closure"], f"{what}: closure {got['closure']} != {want['closure']}"
    assert len(got["window"]) == len(want["window"]), what
    for i, (g, w) in enumerate(zip(got["window"], want["window"])):
        for side in ("min", "max"):
            for k in ("psi", "x", "y", "omega"):
                assert nan_equal(g[side][k], w[side][k]), f"{what}: window {i} {side} {k}: {g[side]} != {w[side]}"


def check_topology(s, what, out_dtypes, wins=None):
    """topology() and stream_function() of a solver against the host statements of its get_fields(), for every out_dtype."""
    wins = windows(s.nx, s.ny) if wins is None else wins
    for dt in out_dtypes:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            u, _ = s.get_fields(out_dtype=dt)
        tag = f"{what} out={np.dtype(dt).name} after {s.steps_done}"
        want = T.host_topology(u, s.uLB, wins, step=s.steps_done)
        same_topology_record(s.topology(wins, out_dtype=dt), want, tag)
        psi, omega = s.stream_function(out_dtype=dt)
        hpsi, homega = T.host_stream_function(u)
        assert psi.dtype == omega.dtype == np.float64
        assert np.array_equal(psi, hpsi, equal_nan=True), f"{tag}: psi differs in {np.count_nonzero(~((psi == hpsi) | (np.isnan(psi) & np.isnan(hpsi))))} cells"
        assert np.array_equal(omega, homega, equal_nan=True), f"{tag}: omega differs"
        for w_ in want["window"]:      # the record's omega is the field's, the same bits
            for e in (w_["min"], w_["max"]):
                if e["x"] >= 0:
                    assert nan_equal(e["omega"], omega[e["x"], e["y"]]) and e["psi"] == psi[e["x"], e["y"]]
    return want
