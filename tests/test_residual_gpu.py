"""GPU tests of the field residual (lbm_residual_*): every field of a device record equals residual.host_residual of the two
get_fields() results of the same context exactly -- the three sums within the bound of a reordered double sum -- on every kernel
route, semantics and arithmetic; ties and cells that are not finite; automatic samples equal manual ones bit for bit and leave the
stepping alone, also beside the time statistics and a monitor series; batches and slabs; the life cycle; the two front ends."""
import warnings

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, datagen, residual
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
from latticeboltzmannsimulations_amd.slab import LocalSlabs, partition_rows

from cases import route_cases, route_id
from checks import RES_EXACT as EXACT
from checks import RES_SUMS as SUMS
from checks import HostStats, perturbed, residual_sum_bounds, residual_terms, rest, same_bits, same_residual_record

pytestmark = pytest.mark.gpu

ULB = 0.08
# the monitor tests' smallest shapes: the odd width leaves a padded last lane group; the tile route; the smallest lattice the
# streaming tests force kernel="stream" on
SIZE = {"generic": (97, 80), "tb": (192, 160), "stream": (132, 200), "push": (192, 160)}


# every route with each of its semantics and arithmetics once, then a sample of the rest drawn with seed 2029, then two fp64 lattices
# on the multi-step routes (both out_dtypes) and the closure on the streaming route (cases.route_cases)
CASES = route_cases(["generic", "tb", "stream", "push"], ["strict", "fast"], SIZE, seed=2029, sample=6,
                    extras=[("tb", np.float64, "MRT", 1, "mrt_gpu", "strict"), ("stream", np.float64, "SRT", 1, "mrt_gpu", "fast"),
                            ("stream", np.float32, "MRT", 1, "mrt_gpu", "strict")])


@pytest.mark.parametrize("cfg", CASES, ids=route_id)
def test_device_record_equals_the_host_statement(cfg):
    """From an upload: samples after 1 step (the sample is the raw lattice), 7 and 37 steps -- two records, the second over an uneven
    number of steps and several launch units."""
    kernel, dtype, coll, turb, sem, arith = cfg
    nx, ny = SIZE[kernel]
    outs = (np.float32, np.float64) if dtype == np.float64 else (np.float32,)
    with CavitySolver(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, semantics=sem, kernel=kernel, arith=arith) as s:
        for dt in outs:
            s.set_state(perturbed(nx, ny, dtype, CASES.index(cfg)))
            s.begin_residual(out_dtype=dt)
            samples = []
            for n in (1, 7, 37):
                s.step(n - s.steps_done)
                samples.append((s.steps_done,) + s.get_fields(out_dtype=dt))
                s.sample_residual()
            got = s.residual_series()
            assert got["count"] == 2 and got["dropped"] == 0
            for i in range(2):
                rec = residual.record_at(got, i)
                want = same_residual_record(rec, samples[i], samples[i + 1], f"{route_id(cfg)} out={np.dtype(dt).name} record {i}")
                assert want["cells"] == nx * ny and want["max_du2"] > 0.0
            assert list(got["step"]) == [7, 37] and list(got["step_prev"]) == [1, 7]


@pytest.mark.parametrize("kernel,dtype,sem", [("generic", np.float64, "mrt_py"), ("tb", np.float32, "mrt_gpu"), ("tb", np.float64, "mrt_gpu")])
def test_ties_go_to_the_smaller_x_then_y_and_cells_that_are_not_finite_are_left_out(kernel, dtype, sem):
    """(lbm_set_state ends a series, so both samples come from one upload.)  A rest state with two horizontal strips of cells that
    carry an excess in one population, on rows that different workgroups reduce, the later row starting at the smaller x; the four
    end cells of the strips hold NaN / inf.  Far from the walls the update is invariant under translation, so the cells of a strip's
    interior change by the same bits in both strips: the maximum of d2 is tied between neighbouring cells (one lane group), along a
    strip (one wave) and between the strips (two workgroups), and the order (d2, x, y) names a cell of the later row while the
    device meets the earlier row first.  The non-finite cells spread by one cell per step and hide what the strips' ends would
    change; they are ordinary data.  The test checks these premises on the downloaded fields before it compares."""
    nx, ny = SIZE[kernel]
    ya, yb = ny // 4, 3 * ny // 4
    strips = ((nx // 3, nx // 3 + 41, ya), (nx // 3 - 9, nx // 3 + 32, yb))
    fin = rest(nx, ny, dtype)
    for a, b, y in strips:
        fin[1, a:b, y] += dtype(0.25)
        fin[3, a, y] = np.nan
        fin[5, b - 1, y] = np.inf
    with CavitySolver(nx, ny, 1000.0, RT="MRT" if sem == "mrt_gpu" else "SRT", dtype=dtype, semantics=sem, kernel=kernel) as s, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s.set_state(fin)
        s.begin_residual()
        s.step(1)
        first = (s.steps_done,) + s.get_fields()
        s.sample_residual().step(2)
        second = (s.steps_done,) + s.get_fields()
        s.sample_residual()
        rec = residual.record_at(s.residual_series(), 0)
        # the premises
        ok, d2, _, _ = residual_terms(first[1:], second[1:])
        ties = np.argwhere(ok & (d2 == d2[ok].max()))
        assert {yb - 1, yb, yb + 1} & set(ties[:, 1]) and {ya - 1, ya, ya + 1} & set(ties[:, 1]), "ties on both strips"
        assert len(ties) >= 40 and (np.diff(ties[:, 0]) == 1).any(), "ties between neighbouring cells"
        x_major = tuple(ties[0])
        y_major = min(map(tuple, ties), key=lambda t: (t[1], t[0]))
        assert x_major != y_major and x_major[1] > y_major[1]
        # the record
        want = same_residual_record(rec, first, second, f"ties {kernel} {np.dtype(dtype).name}")
        assert (rec["max_x"], rec["max_y"]) == x_major and rec["max_du2"] > 1e-4
        assert rec["nonfinite"] == want["nonfinite"] >= 4 * 9 and rec["cells"] + rec["nonfinite"] == nx * ny
        assert np.isfinite([rec[k] for k in SUMS]).all()


SERIES = [(every, kernel, False) for kernel in ("tb", "stream") for every in (1, 3, 8, 13)] + \
         [(3, "generic", False), (8, "push", False), (3, "tb", True), (3, "stream", True), (4, "stream", True), (5, "tb", True)]
MON = dict(window=(4, 120, 4, 150), probes=((66, 80), (1, 1)))


@pytest.mark.parametrize("every,kernel,beside", SERIES)
def test_automatic_samples_equal_manual_samples_and_leave_the_stepping_alone(every, kernel, beside):
    """lbm_step calls that do not line up with `every` (below and above the steps per launch); the series is bitwise the manual
    samples of a second context stepped to the same counts, and fin / u / rho equal that context's.  beside: the time statistics
    sample every 5 and a monitor series every 4 next to it; all three stay exact.  With the residual every 4 or 5 as well, two
    samplers fall due together at many step counts and all three at step 20."""
    (nx, ny), dtype = SIZE[kernel], np.float32
    kw = dict(dtype=dtype, kernel=kernel, turb=0 if kernel == "push" else 1)
    with CavitySolver(nx, ny, 1000.0, **kw) as s, CavitySolver(nx, ny, 1000.0, **kw) as ref:
        f = perturbed(nx, ny, dtype, every)
        s.set_state(f); ref.set_state(f)
        s.begin_residual(every=every, capacity=64)
        ref.begin_residual(every=0, capacity=64)
        host, mon = HostStats(), []
        if beside:
            s.begin_statistics(5)
            s.begin_monitor(every=4, capacity=16, **MON)
        for k in (5, 20, 1, 13):
            s.step(k)
            for n in range(ref.steps_done + 1, s.steps_done + 1):
                due = n % every == 0, beside and n % 5 == 0, beside and n % 4 == 0
                if any(due):
                    ref.step(n - ref.steps_done)
                    if due[0]:
                        ref.sample_residual()
                    if due[1]:
                        host.add(*ref.get_fields())
                    if due[2]:
                        mon.append(ref.monitor(**MON))
            ref.step(s.steps_done - ref.steps_done)
            got, want = s.residual_series(), ref.residual_series()
            assert got["count"] == want["count"] == max(s.steps_done // every - 1, 0) and got["dropped"] == 0
            same_bits(got, want, residual.FIELDS, f"every={every} {kernel} after {s.steps_done}")
            a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"stepping perturbed at {s.steps_done}"
        assert list(got["step"]) == list(range(2 * every, 40, every)) and list(got["step_prev"]) == list(range(every, 40 - every, every))
        if beside:
            st, ms = s.statistics(), s.monitor_series()
            assert st["samples"] == host.n == 7
            assert np.array_equal(st["u"], host.S[0] / host.n) and np.array_equal(st["rho"], host.S[1] / host.n)
            assert ms["count"] == len(mon) == 9
            for i, w in enumerate(mon):
                assert all(np.array_equal(ms[k][i], w[k], equal_nan=True) for k in ("step", "sum_ux", "sum_q", "min_q", "min_x", "min_y", "probe"))


def test_capacity_and_dropped_samples():
    """every = 3 from step 4 on: samples at 7, 10, ..., 22; the first fills the snapshot, room for two records, three are dropped
    (each still replaces the snapshot; nothing reads a later record to show it, the buffer stays full).  Stepping is unaffected."""
    nx, ny = 192, 160
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as s, CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as ref:
        s.step(4); ref.step(4)
        s.begin_residual(every=3, capacity=2)
        ref.begin_residual(capacity=8)
        s.step(18)
        for n in (7, 10, 13):
            ref.step(n - ref.steps_done).sample_residual()
        ref.step(22 - ref.steps_done)
        got, want = s.residual_series(), ref.residual_series()
        assert got["count"] == 2 and got["dropped"] == 3 and list(got["step"]) == [10, 13] and list(got["step_prev"]) == [7, 10]
        same_bits(got, want, residual.FIELDS, "kept records")
        a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        s.begin_residual(every=0, capacity=1)              # restart: the next sample fills the snapshot again
        s.sample_residual().step(3).sample_residual().step(2).sample_residual()
        got = s.residual_series()
        assert got["count"] == 1 and got["dropped"] == 1 and (got["step"][0], got["step_prev"][0]) == (25, 22)


def test_monitor_and_residual_series_are_independent():
    """A monitor series with room for 2 records and a residual series with room for 64, both every 3, over 20 steps in calls of 7 and
    13: samples at 3, 6, ..., 18.  The monitor keeps 2 records and drops 4; the residual keeps all 5 (steps 6 .. 18), bitwise the manual
    samples of a second context; the stepping is unaffected; ending the monitor series leaves the residual series readable and
    sampling on schedule."""
    nx, ny = SIZE["tb"]
    kw = dict(dtype=np.float32, kernel="tb")
    with CavitySolver(nx, ny, 1000.0, **kw) as s, CavitySolver(nx, ny, 1000.0, **kw) as ref:
        f = perturbed(nx, ny, np.float32, 17)
        s.set_state(f); ref.set_state(f)
        s.begin_monitor(every=3, capacity=2, **MON)
        s.begin_residual(every=3, capacity=64)
        ref.begin_residual(every=0, capacity=64)
        s.step(7).step(13)
        mon = []
        for n in range(3, 21, 3):
            ref.step(n - ref.steps_done).sample_residual()
            if len(mon) < 2:
                mon.append(ref.monitor(**MON))
        ref.step(20 - ref.steps_done)
        ms, got, want = s.monitor_series(), s.residual_series(), ref.residual_series()
        assert ms["count"] == 2 and ms["dropped"] == 4 and list(ms["step"]) == [3, 6]
        for i, w in enumerate(mon):
            assert all(np.array_equal(ms[k][i], w[k], equal_nan=True) for k in ("step", "sum_ux", "sum_q", "min_q", "min_x", "min_y", "probe"))
        assert got["count"] == want["count"] == 5 and got["dropped"] == 0 and list(got["step"]) == list(range(6, 21, 3))
        same_bits(got, want, residual.FIELDS, "beside a full monitor series")
        a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        s.end_monitor()
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.monitor_series()
        same_bits(s.residual_series(), want, residual.FIELDS, "after the monitor series ended")
        s.step(3)                                          # (the sample of step count 21 is taken where the unit from 20 starts)
        ref.step(1).sample_residual().step(2)
        got, want = s.residual_series(), ref.residual_series()
        assert got["count"] == 6 and got["dropped"] == 0 and (got["step"][5], got["step_prev"][5]) == (21, 18)
        same_bits(got, want, residual.FIELDS, "on schedule after the monitor series ended")


def test_batch_of_mixed_reynolds_numbers_gives_each_lattice_its_own_record():
    Res = [100.0, 400.0, 1000.0]
    nx, ny = 128, 96
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=np.float32, turb=1) as bt:
        bt.begin_residual(every=3, capacity=16)
        for k in (5, 20, 1):
            bt.step(k)
        bt.sample_residual()                               # (a manual sample beside the automatic ones: step 26 against 24)
        series = bt.residual_series()
    assert series["count"] == 8 and series["sum_du2"].shape == (8, 3) and series["max_x"].dtype == np.int64
    for b, Re in enumerate(Res):
        with CavitySolver(nx, ny, Re, RT="MRT", dtype=np.float32, turb=1) as s:
            s.begin_residual(every=3, capacity=16)
            for k in (5, 20, 1):
                s.step(k)
            s.sample_residual()
            lone = s.residual_series()
        same_bits({k: series[k][:, b] for k in residual.FIELDS}, lone, residual.FIELDS, f"Re {Re}")
    assert len({tuple(series["sum_du2"][:, b]) for b in range(3)}) == 3


def test_three_slabs_combine_to_the_lone_lattice():
    nx, ny = 192, 160
    parts = partition_rows(ny, 3)
    mr = min(n for _, n in parts)
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, turb=1) as whole:
        slabs = [CavitySolver(nx, ny, 1000.0, dtype=np.float32, turb=1, rows=r, min_rows=mr) for r in parts]
        try:
            f = perturbed(nx, ny, np.float32, 11)
            whole.set_state(f)
            for sl in slabs:
                sl.set_state(f)
            drv = LocalSlabs(slabs)
            for st in [whole] + slabs:
                st.begin_residual()
            samples = []
            for k in (1, 7, 20):
                whole.step(k); drv.step(k)
                samples.append((whole.steps_done,) + whole.get_fields())
                for st in [whole] + slabs:
                    st.sample_residual()
            want = whole.residual_series()
            each = [sl.residual_series() for sl in slabs]
            assert want["count"] == 2 and all(e["count"] == 2 for e in each)
            for i in range(2):
                got = residual.combine([residual.record_at(e, i) for e in each])
                w = residual.record_at(want, i)
                for key in EXACT:
                    assert got[key] == w[key], (key, i)
                tol = residual_sum_bounds(samples[i][1:], samples[i + 1][1:])
                for key in SUMS:
                    assert abs(got[key] - w[key]) <= tol[key], (key, i)
                same_residual_record(got, samples[i], samples[i + 1], f"slabs combined, record {i}")
                for sl, e in zip(slabs, each):             # every slab's own record is the host statement of its rows
                    same_residual_record(residual.record_at(e, i), samples[i], samples[i + 1], f"slab {sl.y0}", rows=(sl.y0, sl.ny_local))
        finally:
            for sl in slabs:
                sl.close()


def test_life_cycle_refusals_and_repeatability():
    nx, ny = 192, 160
    runs = []
    for _ in range(2):
        with CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as s:
            s.begin_residual(every=4, capacity=32).step(41)
            runs.append(s.residual_series())
    assert runs[0]["count"] == 9
    for k in residual.FIELDS:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="tb") as s:
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_residual()                           # the residual is off
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.residual_series()
        s.begin_residual()
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_residual()                           # no step yet
        assert s.residual_series()["count"] == 0
        for args in ((2, 0, 4), (-1, 0, 4), (0, -1, 4), (0, 0, 0), (0, 0, -3)):
            assert s.lib.lbm_residual_begin(s._h, *args) == -1, args        # LBM_ERR_INVALID
        assert s.lib.lbm_residual_read(s._h, None, 1, None, None) == -1
        assert s.lib.lbm_residual_read(s._h, None, -1, None, None) == -1
        s.step(4)
        s.begin_residual(every=3, capacity=4)
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.step_unit(3)                                # the automatic residual runs inside lbm_step only
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.step_edges()
        s.begin_residual(every=0, capacity=4)
        s.step_unit(3)                                    # every = 0 does not refuse
        s.sample_residual().step(2).sample_residual()
        assert s.residual_series()["count"] == 1
        s.set_state(perturbed(nx, ny, np.float32, 3))    # ends the series
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.residual_series()
        s.begin_residual(every=2, capacity=8).step(6)
        assert s.residual_series()["count"] == 2
        s.init_equilibrium()                              # ends it too
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_residual()
        s.begin_residual(every=1, capacity=8).step(3)
        assert s.residual_series()["count"] == 2
        s.end_residual()
        s.end_residual()                                  # (twice is fine)
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.residual_series()
        s.step(5)                                         # stepping goes on without it
    with CavitySolver(nx, 300, 1000.0, dtype=np.float32, rows=(100, 96)) as slab:
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            slab.begin_residual(every=8)                  # no automatic sampling on a slab
        slab.begin_residual(every=0)


def test_front_end_stops_on_the_residual_at_the_check_the_host_statement_names(tmp_path, monkeypatch, capsys):
    """64 x 64, Re 100, MRT, fp32, a check every 250 iterations.  The host statement first: the same solver, get_fields at every check
    and host_residual, which gives the sequence of relative L2 changes per step.  residual_tol is the geometric mean of the values
    at iterations 8000 and 8250 (step counts 8001 and 8251), far above the rounding of either summation order, so run_cavity must
    stop at iteration 8250 exactly; its fields are those of the host-driven run."""
    monkeypatch.chdir(tmp_path)
    kw = dict(Re=100.0, RT="MRT", turb=0, xsize=64, ysize=64)
    values, prev = {}, None
    with CavitySolver(64, 64, 100.0, RT="MRT", dtype=np.float32, turb=0) as s:
        for It in range(0, 8251, 250):
            s.step(It + 1 - s.steps_done)
            cur = (s.steps_done,) + s.get_fields(out_dtype=np.float32)
            if prev is not None:
                values[It] = residual.norms(residual.host_residual(prev[1], prev[2], cur[1], cur[2], step=cur[0], step_prev=prev[0]), ULB)["rel_l2_per_step"]
            prev = cur
        u_host, rho_host = cur[1], cur[2]
    print("host residuals:", values)
    tol = float(np.sqrt(values[8000] * values[8250]))
    assert values[8250] < tol < values[8000] and all(v > tol for It, v in values.items() if It < 8250)
    assert values[8000] / values[8250] > 1.01             # (the two orders of summation differ by parts in 1e12)
    for mode in ("host", "device"):
        r = run_cavity(maxIt=20000, Pinterval=250, SavePlot=False, criterion="residual", residual_tol=tol, monitor=mode, **kw)
        assert r.converged and r.iterations == 8251 and not r.diverged, mode
        assert [It for It, _ in r.residuals] == list(range(250, 8251, 250))
        got = [residual.norms(rec, ULB)["rel_l2_per_step"] for _, rec in r.residuals]
        assert np.allclose(got, [values[It] for It, _ in r.residuals], rtol=1e-9, atol=0.0)
        assert np.array_equal(r.u, u_host) and np.array_equal(r.rho, rho_host), mode
        out = capsys.readouterr().out
        assert "current residual is " + str(got[-1]) in out and "breaking out of loop because of convergence" in out
    assert not (tmp_path / "output").exists()


def test_datagen_stops_each_lattice_where_run_cavity_stops_it_alone(tmp_path):
    """Three Reynolds numbers at 64 x 64 in one batch under the residual rule; the tolerance 1e-4 per step is a property of the
    scenario (well below the first checks' values, far above the fp32 floor: on the CPU oracle the three lattices pass it after
    about 2 300, 3 500 and 5 300 iterations), not a bound on anything."""
    Res = [100.0, 200.0, 400.0]
    kw = dict(xsize=64, ysize=64, RT="MRT", turb=0, Pinterval=250)
    out = datagen.generate(Re_range=Res, maxIt=8001, OutputFolder=str(tmp_path), quiet=True, criterion="residual", residual_tol=1e-4, **kw)
    feq, f_final, u_final, Re_range, its, res_final = out
    assert np.array_equal(np.load(tmp_path / "residual_final.npy"), res_final) and res_final.shape == (3,)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["Re_range.npy", "f_final.npy", "feq_initial.npy", "residual_final.npy", "u_final.npy"]
    assert (its < 8001).all() and (res_final < 1e-4).all() and len(set(its)) > 1
    for i, Re in enumerate(Res):
        r = run_cavity(maxIt=8001, Re=Re, SavePlot=False, quiet=True, criterion="residual", residual_tol=1e-4, **kw)
        assert r.converged and r.iterations == its[i], (Re, r.iterations, its[i])
        assert residual.norms(r.residuals[-1][1], ULB)["rel_l2_per_step"] == res_final[i]
        assert np.array_equal(r.u, u_final[i])
    plain = datagen.generate(Re_range=Res[:1], maxIt=501, save=False, quiet=True, **kw)
    assert len(plain) == 5                                # the default criterion returns what it always did
