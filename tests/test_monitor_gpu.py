"""GPU tests of the run monitor (lbm_monitor*, lbm_get_lines): every field of a device record equals monitor.host_monitor of
get_fields() of the same context exactly -- the four sums within the bound of a reordered double sum -- on every kernel route,
semantics and arithmetic; the tie-break and the cells that are not finite; a series equals one-shot records bit for bit and leaves
the stepping alone, also beside the time statistics; batches and slabs; the walls-inside streaming route; the front end."""
import warnings

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, ghia, monitor
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
from latticeboltzmannsimulations_amd.slab import LocalSlabs, partition_rows
from oracle.lbm_ref import CavityOracleC

from cases import route_cases, route_id
from checks import MON_EXACT as EXACT
from checks import MON_SUMS as SUMS
from checks import HostStats, monitor_sum_bounds, perturbed, rest, same_bits, same_monitor_record

pytestmark = pytest.mark.gpu

ULB = 0.08
# every route with each of its semantics and arithmetics once, then a seeded sample of the rest (cases.route_cases)
CASES = route_cases(["generic", "vec", "tb", "stream", "push"], ["strict", "fast", "promoted"], (192, 160), seed=2027, sample=8,
                    extras=[("tb", np.float64, "MRT", 0, "mrt_gpu", "strict"), ("stream", np.float64, "SRT", 1, "mrt_gpu", "strict")])
KEYS = EXACT + SUMS + ("probe",)


def _check_all(s, what, out_dtypes):
    nx, ny = s.nx, s.ny
    spec = dict(window=(5, nx - 7, 3, ny - 2), exclude=((nx // 3, nx // 2, 0, ny // 2), (0, 9, ny // 2, ny)),
                probes=((0, 0), (nx - 1, ny - 1), (nx // 2, ny // 2), (17, 1), (nx - 2, 0)))
    for dt in out_dtypes:
        u, rho = s.get_fields(out_dtype=dt)
        tag = f"{what} out={np.dtype(dt).name} after {s.steps_done}"
        rec = s.monitor(out_dtype=dt, **spec)
        assert rec["step"] == s.steps_done
        same_monitor_record(rec, u, rho, s.uLB, tag, **spec)
        same_monitor_record(s.monitor(out_dtype=dt), u, rho, s.uLB, tag + " (whole lattice)")
        col, row = s.lines(out_dtype=dt)
        assert col.dtype == row.dtype == np.dtype(dt)
        assert np.array_equal(col, np.stack([u[0, nx // 2], u[1, nx // 2], rho[nx // 2]])), tag + ": middle column"
        assert np.array_equal(row, np.stack([u[0, :, ny // 2], u[1, :, ny // 2], rho[:, ny // 2]])), tag + ": middle row"
        col, row = s.lines(x=nx - 1, y=0, out_dtype=dt)
        assert np.array_equal(col[0], u[0, nx - 1]) and np.array_equal(row[2], rho[:, 0]), tag + ": last column, lid row"
        assert s.locate_vortices(out_dtype=dt) == ghia.locate_vortices(u, s.uLB), tag + ": vortices"


@pytest.mark.parametrize("cfg", CASES, ids=route_id)
def test_one_shot_record_lines_and_vortices_equal_the_host_statement(cfg):
    """From an upload: after 1 step (the sample is the raw lattice), 7 and 37 steps."""
    kernel, dtype, coll, turb, sem, arith = cfg
    nx, ny = (97, 80) if kernel == "generic" else (192, 160)
    outs = (np.float32, np.float64) if dtype == np.float64 else (np.float32,)
    with CavitySolver(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, semantics=sem, kernel=kernel, arith=arith) as s:
        s.set_state(perturbed(nx, ny, dtype, CASES.index(cfg)))
        for n in (1, 7, 37):
            s.step(n - s.steps_done)
            _check_all(s, route_id(cfg), outs)


@pytest.mark.parametrize("kernel,dtype", [("auto", np.float32), ("generic", np.float64)])
def test_vortex_search_on_a_lattice_narrower_than_forty_cells(kernel, dtype):
    """X < 40: off = 0, the second search's box is empty and finds the first minimum again, as the reference's does."""
    with CavitySolver(36, 33, 400.0, dtype=dtype, kernel=kernel) as s:
        s.set_state(perturbed(36, 33, dtype, 7))
        for n in (1, 12):
            s.step(n - s.steps_done)
            u, _ = s.get_fields(out_dtype=np.float32)
            got = s.locate_vortices()
            assert got == ghia.locate_vortices(u, s.uLB) and got[0] == got[1]


@pytest.mark.parametrize("nx,ny", [(192, 160), (641, 449)])
def test_ties_go_to_the_smaller_x_then_y_and_cells_that_are_not_finite_are_left_out(nx, ny):
    """A rest state (populations = weights): after one step the sample is the uploaded state, every interior q is exactly 0, so the
    minimum is the window's first cell in (x, y) order -- the device visits the cells x fastest, in workgroups of 256 that do not
    line up with the rows, and (641 x 449) more than once per lane.  Then the same state with NaN / inf written into a few cells."""
    dtype = np.float64
    fin = rest(nx, ny, dtype)
    with CavitySolver(nx, ny, 1000.0, dtype=dtype) as s:
        s.set_state(fin)
        s.step(1)
        u, rho = s.get_fields()
        assert not u[:, 1:-1, 1:-1].any()
        for win in ((70, 150, 3, 100), (1, nx - 1, 1, ny - 1), (nx // 2 + 1, nx - 1, ny // 2 + 3, ny - 1), (97, 98, 5, ny - 1)):
            rec = s.monitor(window=win)
            assert (rec["min_q"], rec["min_x"], rec["min_y"]) == (0.0, win[0], win[2]), win
            same_monitor_record(rec, u, rho, s.uLB, f"rest {win}", window=win)
        rec = s.monitor(window=(70, 150, 3, 100), exclude=((70, 71, 3, 50), (70, 80, 50, 100)))
        assert (rec["min_x"], rec["min_y"]) == (71, 3)
        rec = s.monitor(window=(70, 150, 3, 100), exclude=((0, 100, 0, ny), (100, nx, 0, 100)))
        assert (rec["min_q"], rec["min_x"], rec["min_y"]) == (np.inf, -1, -1)
        # cells that are not finite: computed with, never faulted on
        cells = [(70, 3), (71, 3), (5, 5), (nx - 2, ny - 2), (nx // 2, ny // 2), (130, 77), (0, 40)]
        for i, (x, y) in enumerate(cells):
            fin[i % 9, x, y] = (np.nan, np.inf, -np.inf)[i % 3]
        s.set_state(fin)
        s.step(1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            u, rho = s.get_fields()
            spec = dict(window=(70, 150, 3, 100), probes=((70, 3), (72, 3)))
            rec = s.monitor(**spec)
            want = same_monitor_record(rec, u, rho, s.uLB, "not finite", **spec)
        assert rec["nonfinite"] == want["nonfinite"] >= 5
        assert (rec["min_x"], rec["min_y"]) == (70, 4) and np.isfinite(rec["max_q"]) and np.isfinite(rec["sum_rho"])
        assert not np.isfinite(rec["probe"][0]).all() and np.isfinite(rec["probe"][1]).all()


def test_tie_break_inside_one_wave_and_inside_one_lane():
    """The rest state on 641 x 449, windows cut by boxes to an L so that the orders (q, x, y) and (q, y, x) -- or "first seen" --
    name different cells among equal q = 0.  One wave: the wave of cells 3840 .. 3903 straddles rows 5 and 6; the candidates left are
    (636 .. 639, 5) and (1 .. 56, 6), all in it.  One lane: the pass covers 1024 x 256 cells per sweep, so the lane that visits
    (100, 2) visits (75, 411) next (262144 = 408 x 641 + 616); the only candidates are these two."""
    nx, ny = 641, 449
    with CavitySolver(nx, ny, 1000.0, dtype=np.float64) as s:
        s.set_state(rest(nx, ny, np.float64))
        s.step(1)
        u, rho = s.get_fields()
        assert (3841 // 64 == 3902 // 64) and (2 * nx + 100 + 1024 * 256 == 411 * nx + 75)
        wave = dict(window=(1, 640, 5, 7), exclude=((1, 636, 5, 6), (57, 640, 6, 7)))
        lane = dict(window=(75, 101, 2, 412), exclude=((75, 100, 2, 411), (100, 101, 3, 412), (76, 100, 411, 412)))
        for spec, want in ((wave, (1, 6)), (lane, (75, 411))):
            rec = s.monitor(**spec)
            assert (rec["min_q"], rec["min_x"], rec["min_y"]) == (0.0,) + want, spec
            same_monitor_record(rec, u, rho, s.uLB, f"L-shaped {want}", **spec)


SPEC = dict(window=(4, 180, 4, 150), exclude=((60, 90, 40, 80),), probes=((96, 80), (1, 1), (190, 3)))
SERIES = [(every, kernel, False) for kernel in ("tb", "stream") for every in (1, 3, 8, 13)] + \
         [(3, "generic", False), (8, "push", False), (13, "vec", False), (3, "tb", True), (3, "stream", True), (3, "generic", True)]


@pytest.mark.parametrize("every,kernel,with_stats", SERIES)
def test_series_equals_one_shot_records_and_leaves_the_stepping_alone(every, kernel, with_stats):
    """lbm_step calls that do not line up with `every`; the series is bitwise the one-shot records of a second context stepped to the
    same counts, and fin / u / rho equal that context's.  with_stats: the time statistics sample every 5 beside it; both stay exact."""
    nx, ny, dtype = 192, 160, np.float32
    kw = dict(dtype=dtype, kernel=kernel, turb=0 if kernel == "push" else 1)
    with CavitySolver(nx, ny, 1000.0, **kw) as s, CavitySolver(nx, ny, 1000.0, **kw) as ref:
        f = perturbed(nx, ny, dtype, every)
        s.set_state(f); ref.set_state(f)
        s.begin_monitor(every=every, capacity=64, **SPEC)
        host = HostStats()
        if with_stats:
            s.begin_statistics(5)
        want = []
        for k in (5, 20, 1, 13):
            s.step(k)
            for n in range(ref.steps_done + 1, s.steps_done + 1):
                if n % every == 0 or (with_stats and n % 5 == 0):
                    ref.step(n - ref.steps_done)
                    if n % every == 0:
                        want.append(ref.monitor(**SPEC))
                    if with_stats and n % 5 == 0:
                        host.add(*ref.get_fields())
            ref.step(s.steps_done - ref.steps_done)
            got = s.monitor_series()
            assert got["count"] == len(want) == s.steps_done // every and got["dropped"] == 0
            for i, w in enumerate(want):
                same_bits({k: got[k][i] for k in KEYS}, w, KEYS, f"every={every} {kernel} sample {i}")
            a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"stepping perturbed at {s.steps_done}"
        assert list(got["step"]) == list(range(every, 40, every))
        if with_stats:
            st = s.statistics()
            assert st["samples"] == host.n == 7
            assert np.array_equal(st["u"], host.S[0] / host.n) and np.array_equal(st["rho"], host.S[1] / host.n)
        same_bits(s.monitor(**SPEC), ref.monitor(**SPEC), KEYS, "one-shot beside the series")


def test_series_life_cycle_capacity_and_refusals():
    nx, ny = 192, 160
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as s, CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as ref:
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.monitor()                                   # no step yet
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_monitor()                            # no series
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.monitor_series()
        s.step(4); ref.step(4)
        rec = (monitor.lbm_monitor_record * 1)()
        for field, value in (("x_hi", nx + 1), ("y_lo", -1), ("nboxes", 5), ("nprobes", 9), ("struct_size", 8), ("host_dtype", 2)):
            spec = monitor.make_spec(nx, ny, 0, probes=((1, 1),))
            setattr(spec, field, value)
            assert s.lib.lbm_monitor(s._h, spec, rec) == -1, field          # LBM_ERR_INVALID
            assert s.lib.lbm_monitor_begin(s._h, spec, 1, 4) == -1, field
        spec = monitor.make_spec(nx, ny, 0, probes=((1, 1),))
        spec.probe[0][1] = ny
        assert s.lib.lbm_monitor(s._h, spec, rec) == -1 and s.lib.lbm_monitor(s._h, None, rec) == -1
        assert s.lib.lbm_monitor_begin(s._h, monitor.make_spec(nx, ny, 0), 1, 0) == -1
        col = np.zeros((3, ny), dtype=np.float32)
        assert s.lib.lbm_get_lines(s._h, nx, 0, col.ctypes.data, None, 0) == -1
        assert s.lib.lbm_get_lines(s._h, 0, ny, None, np.zeros((3, nx), dtype=np.float32).ctypes.data, 0) == -1
        s.begin_monitor(every=3, capacity=4)
        s.step(18); ref.step(18)                          # due at 7, 10, 13, 16, 19, 22: six samples, room for four
        got = s.monitor_series()
        assert got["count"] == 4 and got["dropped"] == 2 and list(got["step"]) == [7, 10, 13, 16]
        a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.step_unit(3)                                # automatic monitoring runs inside lbm_step only
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.step_edges()
        s.begin_monitor(every=0, capacity=3, probes=((5, 6),))   # restart: manual samples
        s.step(5).sample_monitor().step(1).sample_monitor()
        got = s.monitor_series()
        assert got["count"] == 2 and list(got["step"]) == [27, 28] and got["probe"].shape == (2, 1, 3)
        ref.step(5)
        same_bits({k: got[k][0] for k in KEYS}, ref.monitor(probes=((5, 6),)), KEYS, "manual sample")
        s.step_unit(3)                                    # every = 0 does not refuse
        s.set_state(perturbed(nx, ny, np.float32, 3))    # ends the series
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.monitor_series()
        s.begin_monitor(every=2, capacity=8).step(4)
        s.init_equilibrium()                              # ends it too
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_monitor()
        s.begin_monitor(every=1, capacity=8).step(3)
        assert s.monitor_series()["count"] == 3
        s.end_monitor()
        s.end_monitor()                                   # (twice is fine)
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.monitor_series()
    with CavitySolver(nx, 300, 1000.0, dtype=np.float32, rows=(100, 96)) as slab:
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            slab.begin_monitor(every=8)                   # no automatic sampling on a slab
        slab.begin_monitor(every=0)


def test_batch_of_mixed_reynolds_numbers_gives_each_lattice_its_own_record():
    Res = [100.0, 400.0, 1000.0]
    nx, ny = 128, 96
    spec = dict(window=(3, 120, 3, 90), probes=((64, 48), (1, 95)))
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=np.float32, turb=1) as bt:
        bt.begin_monitor(every=3, capacity=16, **spec)
        for k in (5, 20, 1):
            bt.step(k)
        series, one = bt.monitor_series(), bt.monitor(**spec)
        cols, rows = bt.lines()
        vort = bt.locate_vortices()
        ub, rb = bt.get_fields()
    assert series["count"] == 8 and series["sum_ux"].shape == (8, 3) and series["probe"].shape == (8, 3, 2, 3)
    for b, Re in enumerate(Res):
        with CavitySolver(nx, ny, Re, RT="MRT", dtype=np.float32, turb=1) as s:
            s.begin_monitor(every=3, capacity=16, **spec)
            for k in (5, 20, 1):
                s.step(k)
            lone, lone_one = s.monitor_series(), s.monitor(**spec)
            c, r = s.lines()
            assert np.array_equal(c, cols[b]) and np.array_equal(r, rows[b])
            assert s.locate_vortices() == vort[b] == ghia.locate_vortices(ub[b], s.uLB)
        same_bits({k: series[k][:, b] for k in KEYS}, lone, KEYS, f"series, Re {Re}")
        same_bits({k: one[k][b] for k in KEYS}, lone_one, KEYS, f"one-shot, Re {Re}")
        same_monitor_record(lone_one, ub[b], rb[b], ULB, f"Re {Re}", **spec)


def test_three_slabs_combine_to_the_lone_lattice():
    nx, ny = 192, 160
    parts = partition_rows(ny, 3)
    mr = min(n for _, n in parts)
    spec = dict(window=(5, 185, 4, 155), exclude=((80, 100, 50, 60),), probes=((96, 80), (3, 2), (100, 159), (7, parts[1][0])))
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, turb=1) as whole:
        slabs = [CavitySolver(nx, ny, 1000.0, dtype=np.float32, turb=1, rows=r, min_rows=mr) for r in parts]
        try:
            f = perturbed(nx, ny, np.float32, 11)
            whole.set_state(f)
            for sl in slabs:
                sl.set_state(f)
            drv = LocalSlabs(slabs)
            for k in (1, 7, 20):
                whole.step(k); drv.step(k)
                u, rho = whole.get_fields()
                want, got = whole.monitor(**spec), drv.monitor(**spec)
                for key in EXACT:
                    assert got[key] == want[key], (key, k)
                assert np.array_equal(got["probe"], want["probe"])
                tol = monitor_sum_bounds(u, rho, ULB)
                for key in SUMS:
                    assert abs(got[key] - want[key]) <= tol[key], (key, k)
                same_monitor_record(got, u, rho, ULB, f"slabs after {whole.steps_done}", **spec)
                for sl in slabs:   # every slab's own record is the host statement of its rows; probes in other rows are NaN
                    rec = same_monitor_record(sl.monitor(**spec), u, rho, ULB, f"slab {sl.y0}", rows=(sl.y0, sl.ny_local), **spec)
                    assert np.isnan(rec["probe"]).all(axis=1).sum() >= 2
                col, row = drv.lines()
                wc, wr = whole.lines()
                assert np.array_equal(col, wc) and np.array_equal(row, wr)
                assert slabs[0].lines()[1] is None and slabs[1].lines()[1] is not None and slabs[2].lines()[1] is None
                col, row = drv.lines(x=0, y=ny - 1)
                assert np.array_equal(col[0], u[0, 0]) and np.array_equal(row[1], u[1, :, ny - 1])
        finally:
            for sl in slabs:
                sl.close()


def test_auto_route_with_the_walls_inside_the_streaming_kernel():
    """kernel='auto' at 8 Mi cells plans k_stream_walls: units of up to 8 steps, cut by every = 8 and every = 3."""
    nx, ny = 4096, 2048
    spec = dict(window=(102, 3993, 102, 1945), probes=((2048, 1024), (0, 0)))
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32) as s, CavitySolver(nx, ny, 1000.0, dtype=np.float32) as ref:
        assert s.describe()["kernel"] == "k_stream_walls"
        s.step(40); ref.step(40)
        for every, calls in ((8, (5, 20, 1)), (3, (4, 9))):
            s.begin_monitor(every=every, capacity=8, **spec)
            n0 = s.steps_done
            for k in calls:
                s.step(k)
            got = s.monitor_series()
            steps = list(range(n0 + every, s.steps_done + 1, every))
            assert list(got["step"]) == steps and got["dropped"] == 0
            for i, n in enumerate(steps):
                ref.step(n - ref.steps_done)
                same_bits({k: got[k][i] for k in KEYS}, ref.monitor(**spec), KEYS, f"auto every={every} step {n}")
            ref.step(s.steps_done - ref.steps_done)
            a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        u, rho = a[0], a[1]
        same_monitor_record(s.monitor(**spec), u, rho, ULB, "auto one-shot", **spec)
        assert s.locate_vortices() == ghia.locate_vortices(u, ULB)


def test_front_end_on_the_device_matches_the_host_mode(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    kw = dict(maxIt=3000, Re=100.0, RT="MRT", turb=0, xsize=64, ysize=64, Pinterval=500, SavePlot=False, quiet=True)
    dev = run_cavity(monitor="device", MonitorEvery=250, Probes=((32, 32), (10, 50)), **kw)
    host = run_cavity(SaveVTK=True, OutputFolder=str(tmp_path / "out"), convergence="device", **kw)
    assert dev.regression == host.regression and len(dev.regression) == 6
    assert dev.iterations == host.iterations and dev.converged == host.converged and not dev.diverged
    assert np.array_equal(dev.u, host.u) and np.array_equal(dev.rho, host.rho)
    assert [v[0] for v in dev.vortices] == [it for it, _ in dev.regression]
    assert not (tmp_path / "output").exists()
    assert dev.series["count"] == 12 and list(dev.series["step"]) == list(range(250, 3001, 250)) and dev.series["probe"].shape == (12, 2, 3)
    assert np.array_equal(dev.series["probe"][-1, 0], [dev.u[0, 32, 32], dev.u[1, 32, 32], dev.rho[32, 32]])


def test_front_end_stops_a_run_that_has_blown_up(tmp_path, monkeypatch, capsys):
    """SRT at Re 10000 with uLB = 0.3 on 32 x 32 (tau = 0.50288) blows up within a few hundred steps; the strict arithmetic is
    bit-identical to the oracle, which therefore names the first check that sees it."""
    monkeypatch.chdir(tmp_path)
    kw = dict(Re=10000.0, RT="SRT", turb=0, xsize=32, ysize=32, uLB=0.3)
    o = CavityOracleC(32, 32, 10000.0, uLB=0.3, semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=0)
    first = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for It in range(0, 2000, 250):
            o.step(1 if It == 0 else 250)
            if not (np.isfinite(o.u).all() and np.isfinite(o.rho).all()):
                first = It
                break
    assert first is not None and first > 0
    r = run_cavity(maxIt=2000, Pinterval=250, SavePlot=False, monitor="device", **kw)
    assert r.diverged and not r.converged and r.iterations == first + 1
    assert f"cells are not finite at iteration {first}" in capsys.readouterr().out
