"""CPU tests of the run monitor: monitor.host_monitor (the NumPy statement of the device record) against ghia.locate_vortices on
seeded fields with ties and NaN cells, the column forms of the Ghia metrics, the ABI's structs and argument checks (no device), the
slab combination, and run_cavity(monitor="device") driven by a stand-in solver."""
import ctypes
import os
import re

import numpy as np
import pytest

from front_end_standin import standin
from latticeboltzmannsimulations_amd import _lib, ghia, monitor, relaxation
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
from oracle.lbm_ref import CavityOracleC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULB = 0.08


def _fields(X, Y, seed, dtype=np.float32, ties=False, nans=0):
    rng = np.random.default_rng(seed)
    u = (ULB * rng.standard_normal((2, X, Y))).astype(dtype)
    rho = (1.0 + 0.01 * rng.standard_normal((X, Y))).astype(dtype)
    if ties:     # a few distinct speeds only: many cells share the minimum
        u = (ULB * rng.integers(1, 4, size=(2, X, Y)) / 4.0).astype(dtype)
    for _ in range(nans):
        x, y, k = rng.integers(0, X), rng.integers(0, Y), rng.integers(0, 3)
        (u[0], u[1], rho)[k][x, y] = (np.nan, np.inf, -np.inf)[rng.integers(0, 3)]
    return u, rho


@pytest.mark.parametrize("X,Y", [(36, 33), (97, 80), (192, 160), (40, 41), (81, 64)])
@pytest.mark.parametrize("kind", ["random", "ties"])
def test_two_monitor_records_compose_to_locate_vortices(X, Y, kind):
    for seed in range(4):
        u, rho = _fields(X, Y, seed + 10 * X, ties=kind == "ties")
        assert monitor.host_locate_vortices(u, rho, ULB) == ghia.locate_vortices(u, ULB), (X, Y, kind, seed)


def test_locate_vortices_skips_nan_velocities_like_nanargmin():
    """NaN velocity cells are NaN in the reference's usq too, so both searches skip them (rho plays no part in the reference's)."""
    for seed in range(6):
        u, rho = _fields(64, 48, seed, nans=0)
        rng = np.random.default_rng(seed)
        for _ in range(40):
            u[rng.integers(0, 2), rng.integers(0, 64), rng.integers(0, 48)] = np.nan
        want = ghia.locate_vortices(u, ULB)
        assert monitor.host_locate_vortices(u, rho, ULB) == want
        # the minimum itself: blank it and the search moves on
        u[0, want[0][0], want[0][1]] = np.nan
        assert monitor.host_locate_vortices(u, rho, ULB) == ghia.locate_vortices(u, ULB) != want


def test_record_fields_window_boxes_ties_and_nonfinite_cells():
    X, Y = 37, 29
    u, rho = _fields(X, Y, 3, dtype=np.float64, nans=7)
    bad = ~(np.isfinite(u[0]) & np.isfinite(u[1]) & np.isfinite(rho))
    r = monitor.host_monitor(u, rho, ULB, window=(3, 30, 2, 20), exclude=((5, 9, 0, 29),), probes=((0, 0), (36, 28), (5, 5)), step=12)
    assert r["step"] == 12 and r["nonfinite"] == bad.sum() > 0
    q = (u[0] * u[0] + u[1] * u[1]) / (ULB * ULB)
    assert r["sum_ux"] == pytest.approx(u[0][~bad].sum(), rel=1e-13) and r["sum_q"] == pytest.approx(q[~bad].sum(), rel=1e-13)
    assert r["max_q"] == q[~bad].max()
    best = min((q[x, y], x, y) for x in range(3, 30) for y in range(2, 20) if not bad[x, y] and not 5 <= x < 9)
    assert (r["min_q"], r["min_x"], r["min_y"]) == best
    assert np.array_equal(r["probe"], [[u[0, x, y], u[1, x, y], rho[x, y]] for x, y in ((0, 0), (36, 28), (5, 5))], equal_nan=True)
    # ties: a constant field has its minimum at the window's first cell, x before y
    u[:], rho[:] = 0.01, 1.0
    r = monitor.host_monitor(u, rho, ULB, window=(4, 30, 7, 20), exclude=((4, 5, 7, 9),))
    assert (r["min_x"], r["min_y"]) == (4, 9) and r["nonfinite"] == 0
    # a window covered by a box, an empty window, and no finite cell at all
    for kw in (dict(window=(4, 10, 4, 10), exclude=((0, 20, 0, 20),)), dict(window=(4, 4, 0, Y))):
        r = monitor.host_monitor(u, rho, ULB, **kw)
        assert (r["min_q"], r["min_x"], r["min_y"]) == (np.inf, -1, -1)
    u[:] = np.nan
    r = monitor.host_monitor(u, rho, ULB)
    assert r["nonfinite"] == X * Y and r["max_q"] == -np.inf and r["sum_rho"] == 0.0 and r["min_x"] == -1
    # a slab owns its rows only
    u, rho = _fields(X, Y, 5)
    whole = monitor.host_monitor(u, rho, ULB, window=(1, 36, 1, 28), probes=((3, 4), (3, 20)))
    parts = [monitor.host_monitor(u, rho, ULB, window=(1, 36, 1, 28), probes=((3, 4), (3, 20)), rows=rw) for rw in ((0, 10), (10, 10), (20, 9))]
    assert np.isnan(parts[0]["probe"][1]).all() and np.isnan(parts[1]["probe"][0]).all()
    both = monitor.combine(parts)
    for k in ("nonfinite", "max_q", "min_q", "min_x", "min_y"):
        assert both[k] == whole[k], k
    assert np.array_equal(both["probe"], whole["probe"])
    assert both["sum_q"] == pytest.approx(whole["sum_q"], rel=1e-13)


def test_spec_arguments_are_checked_on_the_host():
    for kw in (dict(window=(0, 65, 0, 48)), dict(window=(5, 4, 0, 48)), dict(window=(0, 64, -1, 48)), dict(exclude=((0, 10, 0, 49),)),
               dict(probes=((64, 0),)), dict(probes=((0, -1),)), dict(exclude=[(0, 1, 0, 1)] * 5), dict(probes=[(0, 0)] * 9)):
        with pytest.raises(ValueError):
            monitor.make_spec(64, 48, _lib.LBM_F32, **kw)
        with pytest.raises(ValueError):
            monitor.host_monitor(np.zeros((2, 64, 48)), np.ones((64, 48)), ULB, **kw)
    s = monitor.make_spec(64, 48, _lib.LBM_F64, window=(1, 63, 2, 47), exclude=((3, 4, 5, 6),), probes=((7, 8), (9, 10)))
    assert (s.struct_size, s.host_dtype, s.x_lo, s.x_hi, s.y_lo, s.y_hi, s.nboxes, s.nprobes) == (ctypes.sizeof(s), 1, 1, 63, 2, 47, 1, 2)
    assert list(s.box[0]) == [3, 4, 5, 6] and list(s.probe[1]) == [9, 10]


@pytest.mark.parametrize("Re", [100, 1000, 10000])
def test_column_forms_of_the_ghia_metrics_are_bit_identical(Re):
    for X, Y, dt in ((64, 64, np.float32), (97, 80, np.float64), (160, 129, np.float32)):
        u, _ = _fields(X, Y, Re + X, dtype=dt)
        col = np.ascontiguousarray(u[0, int(X / 2), :])
        assert ghia.r2_from_column(col, Re, ULB) == ghia.r2_value(u, Re, ULB)
        assert ghia.regression_from_column(col, Re, ULB) == ghia.regression_value(u, Re, ULB)
        # (what r2_value computed before it was expressed through the column form)
        y_true = ghia.ghia_profiles(Re)[1][:-1]
        y_pred = np.fliplr(np.atleast_2d(u[0, int(X / 2), ghia.sample_rows(Y)] / ULB + 0.001))[0]
        assert ghia.r2_value(u, Re, ULB) == 1.0 - np.sum((y_true - y_pred) ** 2) / np.sum((y_true - np.mean(y_true)) ** 2)


# -- the C ABI, without a device ----------------------------------------------------------------
def _header_struct(name):
    """[(field, C type, number of elements)] of a typedef struct of include/lbm.h."""
    hdr = open(os.path.join(ROOT, "include", "lbm.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)], flags=re.S)
    out = []
    for ctype, field, dims in re.findall(r"^\s+(int32_t|double)\s+(\w+)((?:\[\d+\])*);", body, re.M):
        out.append((field, ctype, int(np.prod([int(d) for d in re.findall(r"\d+", dims)] or [1]))))
    return out


@pytest.mark.parametrize("name", ["lbm_monitor_spec", "lbm_monitor_record"])
def test_struct_mirrors_match_the_header(name):
    fields = _header_struct(name)
    cls = getattr(_lib, name)
    assert getattr(monitor, name) is cls
    assert [f[0] for f in fields] == [f[0] for f in cls._fields_]
    size = {"int32_t": 4, "double": 8}
    assert ctypes.sizeof(cls) == sum(size[t] * n for _, t, n in fields)
    off = 0
    for field, t, n in fields:
        assert getattr(cls, field).offset == off and getattr(cls, field).size == size[t] * n, field
        off += size[t] * n
    hdr = open(os.path.join(ROOT, "include", "lbm.h")).read()
    assert int(re.search(r"LBM_MONITOR_MAX_BOXES = (\d+)", hdr).group(1)) == _lib.LBM_MONITOR_MAX_BOXES == monitor.MAX_BOXES
    assert int(re.search(r"LBM_MONITOR_MAX_PROBES = (\d+)", hdr).group(1)) == _lib.LBM_MONITOR_MAX_PROBES == monitor.MAX_PROBES
    assert ctypes.sizeof(_lib.lbm_monitor_record) == 8 * monitor.RECORD_DOUBLES


def test_null_arguments_are_rejected_not_dereferenced():
    """Every entry point with a NULL context, whatever the spec (a good one, one that is out of range, none), is LBM_ERR_INVALID.
    The spec's own checks need a context's lattice size; monitor.make_spec states the same checks on the host
    (test_spec_arguments_are_checked_on_the_host) and the GPU life-cycle test runs the library's."""
    L = _lib.lib()
    good = monitor.make_spec(64, 48, _lib.LBM_F32)
    bad = monitor.make_spec(64, 48, _lib.LBM_F32)
    bad.x_hi, bad.nprobes, bad.struct_size = 1 << 20, 99, 3
    rec = (_lib.lbm_monitor_record * 1)()
    n = ctypes.c_longlong(0)
    for spec in (None, ctypes.byref(good), ctypes.byref(bad)):
        assert L.lbm_monitor(None, spec, rec) == -1                      # LBM_ERR_INVALID
        assert L.lbm_monitor_begin(None, spec, 1, 8) == -1
    assert L.lbm_monitor_sample(None) == -1
    assert L.lbm_monitor_read(None, rec, 1, ctypes.byref(n), ctypes.byref(n)) == -1
    assert L.lbm_monitor_end(None) == -1
    assert L.lbm_get_lines(None, 0, 0, None, None, 0) == -1


# -- the rank drivers' combination, one slab per "rank" ---------------------------------------------
class SlabStandIn:
    """monitor() / lines() of a CavitySolver that holds rows (y0, ny_local) of the fields u, rho."""

    def __init__(self, u, rho, rows):
        self.u, self.rho, (self.y0, self.ny_local) = u, rho, rows

    def monitor(self, **spec):
        return monitor.host_monitor(self.u, self.rho, ULB, rows=(self.y0, self.ny_local), step=5, **spec)

    def lines(self, x=None, y=None, out_dtype=None):
        _, X, Y = self.u.shape
        x, y = int(X / 2) if x is None else x, int(Y / 2) if y is None else y
        col = np.zeros((3, Y), dtype=self.u.dtype)
        own = slice(self.y0, self.y0 + self.ny_local)
        col[:, own] = np.stack([self.u[0, x, own], self.u[1, x, own], self.rho[x, own]])
        row = np.stack([self.u[0, :, y], self.u[1, :, y], self.rho[:, y]]) if self.y0 <= y < self.y0 + self.ny_local else None
        return col, row


def test_rank_drivers_combine_their_slabs(monkeypatch):
    """slab.global_monitor / global_lines: alone (world = 1), and with three ranks whose all-gather is stood in for."""
    from latticeboltzmannsimulations_amd import slab
    X, Y = 37, 29
    u, rho = _fields(X, Y, 9)
    spec = dict(window=(1, 36, 1, 28), exclude=((5, 9, 3, 20),), probes=((3, 4), (3, 20), (36, 28)))
    whole = monitor.host_monitor(u, rho, ULB, step=5, **spec)
    want_lines = SlabStandIn(u, rho, (0, Y)).lines(x=7, y=21)
    alone = slab.global_monitor(SlabStandIn(u, rho, (0, Y)), **spec)
    for k in monitor.SCALARS:
        assert alone[k] == whole[k], k
    assert np.array_equal(alone["probe"], whole["probe"])
    got = slab.global_lines(SlabStandIn(u, rho, (0, Y)), x=7, y=21)
    assert np.array_equal(got[0], want_lines[0]) and np.array_equal(got[1], want_lines[1])
    # three ranks: dist.all_gather_object replaced by one that asks every rank's stand-in
    import torch.distributed as dist
    rows = [(0, 10), (10, 10), (20, 9)]
    ranks = [SlabStandIn(u, rho, r) for r in rows]

    def gather(box, obj, group=None):
        if isinstance(obj, dict):
            box[:] = [r.monitor(**spec) for r in ranks]
        elif isinstance(obj[0], np.ndarray):
            box[:] = [r.lines(x=7, y=21) for r in ranks]
        else:
            box[:] = rows
    monkeypatch.setattr(dist, "all_gather_object", gather)
    for me in ranks:
        both = slab.global_monitor(me, world=3, **spec)
        for k in ("step", "nonfinite", "max_q", "min_q", "min_x", "min_y"):
            assert both[k] == whole[k], k
        assert np.array_equal(both["probe"], whole["probe"])
        assert both["sum_ux"] == pytest.approx(whole["sum_ux"], rel=1e-12, abs=1e-15)
        col, row = slab.global_lines(me, world=3, x=7, y=21)
        assert np.array_equal(col, want_lines[0]) and np.array_equal(row, want_lines[1])


# -- run_cavity(monitor="device") with a stand-in solver ------------------------------------------
MonitorStepper = standin()        # counts the field downloads, the monitor passes and the line reads


@pytest.fixture(autouse=True)
def _no_blow_up():
    MonitorStepper.blow_up_at = None


def test_device_mode_checks_every_pinterval_without_files_or_downloads(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=251, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=False,
                   monitor="device", solver_factory=MonitorStepper)
    log = MonitorStepper.log
    assert log["steps"] == [1, 100, 100, 50]                   # output iterations although no file is written
    assert log["downloads"] == 1                               # the result's fields, at the end
    assert log["monitors"] == 2 * 3 and log["lines"] == 3          # per check: one pass for the record and the first vortex, one for the second
    assert not os.path.exists(tmp_path / "output")
    o = CavityOracleC(32, 32, 100.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32, turb=0)
    want, vort = [], []
    for it in (0, 100, 200):
        o.step(it + 1 - (want[-1][0] + 1 if want else 0))
        want.append((it, float(ghia.r2_value(o.u, 100.0, 0.08))))
        vort.append((it,) + ghia.locate_vortices(o.u, 0.08))
    assert r.regression == want and r.vortices == vort
    assert not r.diverged and not r.converged and r.iterations == 251 and r.series is None
    out = capsys.readouterr().out
    assert "current iteration : 200" in out and "current regression value is " + str(want[2][1]) in out
    mean = float(np.sum(o.u.astype(np.float64))) / (2 * 32 * 32) / 0.08
    line = [ln for ln in out.split("\n") if ln.startswith("current mean velocity value is ")][-1]
    assert float(line.split()[-1]) == pytest.approx(mean, rel=1e-12)
    assert "current vortex locations are " + str(vort[2][1]) + " and " + str(vort[2][2]) in out


def test_device_mode_downloads_fields_only_for_files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=201, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=True,
                   monitor="device", solver_factory=MonitorStepper, quiet=True)
    assert MonitorStepper.log["downloads"] == 3 + 1
    assert all(os.path.exists(tmp_path / "output" / f"ldc.{i:05d}.vtr") for i in range(3))
    h = run_cavity(maxIt=201, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=True,
                   convergence="device", solver_factory=MonitorStepper, quiet=True)
    assert r.regression == h.regression and np.array_equal(r.u, h.u) and r.iterations == h.iterations


def test_a_diverged_record_stops_the_run(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    MonitorStepper.blow_up_at = 150
    r = run_cavity(maxIt=1000, Re=100.0, RT="SRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=False, monitor="device",
                   solver_factory=MonitorStepper)
    assert r.diverged and not r.converged and r.iterations == 201
    assert MonitorStepper.log["steps"] == [1, 100, 100]
    assert [it for it, _ in r.regression] == [0, 100]
    out = capsys.readouterr().out
    assert "diverged: 2 cells are not finite at iteration 200" in out


def test_monitor_every_returns_the_series(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=101, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=50, SavePlot=False, monitor="device",
                   MonitorEvery=10, solver_factory=MonitorStepper, quiet=True)
    assert MonitorStepper.log["begin"] == dict(every=10, capacity=11, probes=((16, 16),))
    assert r.series["count"] == 10 and list(r.series["step"]) == list(range(10, 101, 10))
    r = run_cavity(maxIt=21, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=50, SavePlot=False, monitor="device",
                   MonitorEvery=10, Probes=((1, 2), (3, 4)), solver_factory=MonitorStepper, quiet=True)
    assert MonitorStepper.log["begin"]["probes"] == ((1, 2), (3, 4)) and r.series["probe"].shape == (2, 2, 3)
    with pytest.raises(ValueError):
        run_cavity(maxIt=21, MonitorEvery=10, solver_factory=MonitorStepper, quiet=True)
    with pytest.raises(ValueError):
        run_cavity(maxIt=21, monitor="gpu", solver_factory=MonitorStepper, quiet=True)


def test_default_mode_is_unchanged(tmp_path, monkeypatch, capsys):
    """monitor='host' (the default): the same steps, downloads, prints and result as before -- no monitor call at all."""
    monkeypatch.chdir(tmp_path)
    kw = dict(maxIt=251, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=True,
              solver_factory=MonitorStepper)
    r = run_cavity(**kw)
    log = MonitorStepper.log
    assert log["steps"] == [1, 100, 100, 50] and log["monitors"] == 0 and log["lines"] == 0 and log["begin"] is None
    assert log["downloads"] == 3 + 1
    out = [ln for ln in capsys.readouterr().out.split("\n") if "time elapsed" not in ln]
    o = CavityOracleC(32, 32, 100.0, semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1)
    want = ["the value of uLB is  0.08", "xsize value is  32", "Re chosen  is  100.0", "RT chosen is  SRT", "Turbulence is on",
            "the value of tau(/Dt) is  " + str(1 / r_omega()), " the value of omega is  " + str(r_omega())]
    done = 0
    for it in (0, 100, 200):
        o.step(it + 1 - done)
        done = it + 1
        want += ["current iteration : " + str(it), "current regression value is " + str(ghia.r2_value(o.u, 100.0, 0.08)),
                 "current mean velocity value is " + str(np.mean(o.u) / 0.08)]
    assert out == want + [""]
    assert not r.diverged and r.vortices == [] and r.series is None
    r2 = run_cavity(maxIt=251, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=False,
                    solver_factory=MonitorStepper, quiet=True)
    assert MonitorStepper.log["steps"] == [251] and r2.regression == []     # no files, host mode: one batch, no output iteration


def r_omega():
    return relaxation(100.0, 32, 0.08)["omega"]
