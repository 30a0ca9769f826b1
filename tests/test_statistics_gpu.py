"""GPU tests of the time statistics (lbm_stats_*): the device sums are bit-identical to the float64 host loop over get_fields() at the
same step counts on every kernel route, dtype, operator, closure, semantics and arithmetic; automatic sampling does not change the
stepping; batches and slabs reproduce the lone lattice; the life cycle; a steady flow has a mean equal to its final field; and the
time-mean of the reference's LES default run (SRT, Smagorinsky, Re 7500 / 10000, 160^2) against Ghia's columns."""
import ctypes

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, ghia
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
from latticeboltzmannsimulations_amd.slab import LOW, HIGH, LocalSlabs, partition_rows

from cases import route_cases, route_id
from checks import HostStats, perturbed, raw_stats, same_stats

pytestmark = pytest.mark.gpu


# every route with each of its semantics and arithmetics once, then a seeded sample of the rest (cases.route_cases)
CASES = route_cases(["generic", "vec", "tb", "stream", "push"], ["strict", "fast", "promoted"], (192, 160), seed=2026, sample=16)
EVERY = (1, 3, 8, 13)


@pytest.mark.parametrize("cfg", CASES, ids=route_id)
def test_bit_identical_to_host_loop_and_stepping_unchanged(cfg):
    """From an upload (the first sample is the raw step's), lbm_step calls that do not line up with `every`; then statistics begun
    again mid-run after a multi-step unit.  After every call: the device statistics equal the host loop over get_fields() of a second
    context at the same step counts, and fin / u / rho equal that context's (automatic sampling does not perturb the stepping)."""
    _sampled_run_equals_host_loop(cfg, CASES.index(cfg))


def _sampled_run_equals_host_loop(cfg, i, tuning=None, described=None):
    """The body of the tests above and below; i picks `every` of the two phases and the uploaded state, `described` is what
    describe() must say of both contexts."""
    kernel, dtype, coll, turb, sem, arith = cfg
    nx, ny = (97, 80) if kernel == "generic" else (192, 160)
    kw = dict(RT=coll, dtype=dtype, turb=turb, semantics=sem, kernel=kernel, arith=arith, tuning=tuning)
    with CavitySolver(nx, ny, 1000.0, **kw) as s, CavitySolver(nx, ny, 1000.0, **kw) as ref:
        for name, value in (described or {}).items():
            assert s.describe()[name] == value and ref.describe()[name] == value, (name, s.describe()[name])
        f = perturbed(nx, ny, dtype, i)
        s.set_state(f); ref.set_state(f)
        for phase, (every, calls) in enumerate(((EVERY[i % 4], (5, 20, 1, 13)), (EVERY[(i + 1) % 4], (17, 5, 20, 1)))):
            if phase == 1:   # mid-run, behind a call that ends in a multi-step unit
                s.step(17); ref.step(17)
            s.begin_statistics(every)
            n0, host = s.steps_done, HostStats()
            for k in calls:
                s.step(k)
                for n in range(n0 + every, s.steps_done + 1, every):
                    if n > ref.steps_done:
                        ref.step(n - ref.steps_done)
                        host.add(*ref.get_fields())
                if ref.steps_done < s.steps_done:
                    ref.step(s.steps_done - ref.steps_done)
                same_stats(s, host, f"{route_id(cfg)} every={every} after {s.steps_done}")
                a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"{route_id(cfg)}: stepping perturbed at {s.steps_done}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_samples_between_two_stream_units_of_a_lone_lattice(dtype):
    """The same run where the wall frame of a lone lattice runs beside the streaming kernel, on the second stream: calls (5, 20, 1, 13)
    with every = 3, then (17, 5, 20, 1) with every = 8, so that automatic samples (one-stream work, which waits for the frame kernels
    lazily and leaves the bulk kernel's event stale) fall between two-stream units.  Without the switch the register rule picks this
    route for some variants only."""
    assert (EVERY[1], EVERY[2]) == (3, 8)
    _sampled_run_equals_host_loop(("stream", dtype, "MRT", 0, "mrt_gpu", "strict"), 1, tuning={"frame_beside": True, "stream_walls": False},
                                  described={"frame_beside": 1})


def test_auto_route_with_the_walls_inside_the_streaming_kernel():
    """kernel='auto' at 8 Mi cells plans k_stream_walls: units of up to 8 steps, cut by every = 8 and every = 3."""
    nx, ny = 4096, 2048
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32) as s, CavitySolver(nx, ny, 1000.0, dtype=np.float32) as ref:
        assert s.describe()["kernel"] == "k_stream_walls"
        s.step(40); ref.step(40)
        for every, calls in ((8, (5, 20, 1)), (3, (4, 9))):
            s.begin_statistics(every)
            n0, host = s.steps_done, HostStats()
            for k in calls:
                s.step(k)
            for n in range(n0 + every, s.steps_done + 1, every):
                ref.step(n - ref.steps_done)
                host.add(*ref.get_fields())
            ref.step(s.steps_done - ref.steps_done)
            same_stats(s, host, f"auto every={every}")
            a, b = s.get_fields(want_fin=True), ref.get_fields(want_fin=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_batch_of_mixed_reynolds_numbers_gives_each_lattice_its_own_statistics():
    Res = [100.0, 400.0, 1000.0]
    nx, ny = 128, 96
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=np.float32, turb=1) as bt:
        bt.begin_statistics(3)
        for k in (5, 20, 1):
            bt.step(k)
        mu, mrho, sec, n = raw_stats(bt)
        st = bt.statistics()
    for b, Re in enumerate(Res):
        with CavitySolver(nx, ny, Re, RT="MRT", dtype=np.float32, turb=1) as s:
            s.begin_statistics(3)
            for k in (5, 20, 1):
                s.step(k)
            one = raw_stats(s)
        assert one[3] == n == 8
        assert np.array_equal(one[0], mu[b]) and np.array_equal(one[1], mrho[b]) and np.array_equal(one[2], sec[b]), Re
        assert st["u"].shape == (3, 2, nx, ny) and st["uu"].shape == (3, nx, ny)
        assert np.array_equal(st["uu"][b], sec[b, 0] - mu[b, 0] * mu[b, 0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_three_slabs_with_caller_driven_halos_reproduce_the_lone_lattice(dtype):
    nx, ny = 128, 3 * 70 + 1
    parts = partition_rows(ny, 3)
    mr = min(n for _, n in parts)
    with CavitySolver(nx, ny, 1000.0, dtype=dtype, turb=1) as whole:
        slabs = [CavitySolver(nx, ny, 1000.0, dtype=dtype, turb=1, rows=r, min_rows=mr) for r in parts]
        try:
            with pytest.raises(RuntimeError, match=r"\(-4\)"):
                slabs[1].begin_statistics(5)
            drv = LocalSlabs(slabs)
            whole.step(3); drv.step(3)
            whole.begin_statistics(0)
            for sl in slabs:
                sl.begin_statistics(0)
            for k in (1, 7, 20, 5):
                whole.step(k); drv.step(k)
                whole.sample_statistics()
                for sl in slabs:
                    sl.sample_statistics()
            want = raw_stats(whole)
            got = [np.zeros_like(a) for a in want[:3]]
            for sl in slabs:   # (each slab writes its own rows only)
                mu, mrho, sec, n = raw_stats(sl)
                y0, m = sl.y0, sl.ny_local
                got[0][..., y0:y0 + m] = mu[..., y0:y0 + m]
                got[1][..., y0:y0 + m] = mrho[..., y0:y0 + m]
                got[2][..., y0:y0 + m] = sec[..., y0:y0 + m]
                assert n == want[3] == 4
                assert not mrho[:, :y0].any() and not mrho[:, y0 + m:].any()
            assert all(np.array_equal(a, b) for a, b in zip(got, want[:3]))
        finally:
            for sl in slabs:
                sl.close()


def test_loopback_slab_with_manual_samples():
    """The in-library exchange path (a middle slab that is its own periodic neighbour) against the same slab stepped through the
    externally driven API with the wrap done through host buffers; manual samples at the same step counts."""
    nx, NY, rows = 512, 300, (100, 96)
    a = CavitySolver(nx, NY, 1000.0, dtype=np.float32, rows=rows, kernel="tb")
    b = CavitySolver(nx, NY, 1000.0, dtype=np.float32, rows=rows, kernel="generic")
    try:
        a.comm_loopback()
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            a.begin_statistics(8)
        fin0 = perturbed(nx, NY, np.float32, 5)
        a.set_state(fin0); b.set_state(fin0)
        a.begin_statistics(0); b.begin_statistics(0)
        up = np.empty(b.halo_elems(), dtype=np.float32); down = np.empty(b.halo_elems(), dtype=np.float32)
        for steps in (23, 8, 1, 10):
            a.step(steps)
            for _ in range(steps):
                b.step_edges(); b.step_interior(); b.step_finish()
                b.halo_export(LOW, up.ctypes.data); b.halo_export(HIGH, down.ctypes.data)
                b.halo_import(HIGH, up.ctypes.data); b.halo_import(LOW, down.ctypes.data)
            a.sample_statistics(); b.sample_statistics()
        ra, rb = raw_stats(a), raw_stats(b)
        assert ra[3] == rb[3] == 4
        assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3]))
        assert np.isfinite(ra[0][..., rows[0]:rows[0] + rows[1]]).all()
    finally:
        a.close(); b.close()


def test_life_cycle():
    nx, ny = 96, 64
    with CavitySolver(nx, ny, 400.0, dtype=np.float64, kernel="tb") as s:
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_statistics()                      # statistics off
        s.begin_statistics(0)
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_statistics()                      # no step yet
        s.step(10).sample_statistics()
        assert raw_stats(s)[3] == 1
        s.begin_statistics(4)                          # begin resets the sums
        mu, mrho, sec = np.full((2, nx, ny), 7.0), np.full((nx, ny), 7.0), np.full((3, nx, ny), 7.0)
        n = ctypes.c_longlong(-1)
        assert s.lib.lbm_stats_get(s._h, mu.ctypes.data, mrho.ctypes.data, sec.ctypes.data, ctypes.byref(n)) == 0
        assert n.value == 0 and (mu == 7.0).all() and (mrho == 7.0).all() and (sec == 7.0).all()   # count == 0 writes nothing else
        assert s.statistics()["samples"] == 0 and s.statistics()["u"] is None
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.step_unit(3)                             # automatic sampling runs inside lbm_step only
        s.step(9)
        assert s.statistics()["samples"] == 2          # n0 + 4, n0 + 8
        s.init_equilibrium()                           # ends statistics
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.statistics()
        s.step(5)
        s.begin_statistics(1).step(3)
        assert s.statistics()["samples"] == 3
        s.set_state(perturbed(nx, ny, np.float64, 1))  # ends statistics
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.sample_statistics()
        s.step(2).begin_statistics(2).step(4)
        s.end_statistics()
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            s.statistics()
        s.end_statistics()                             # (twice is fine)
        s.begin_statistics(2).step(4)                  # end, then begin again
        host = HostStats()
        with CavitySolver(nx, ny, 400.0, dtype=np.float64, kernel="tb") as ref:
            ref.set_state(perturbed(nx, ny, np.float64, 1))
            for n in (8, 10):
                ref.step(n - ref.steps_done)
                host.add(*ref.get_fields())
        same_stats(s, host, "end + begin")


def test_steady_flow_mean_is_the_final_field():
    """Re 100, 64^2, MRT fp64 run to the reference's criterion (|d mean(u)| / uLB < 1e-8 on more than five checks 3000 steps apart,
    MRT_GPU.py:883-889); the time-mean of the last 2000 steps is the final field, and the stresses vanish.  (The density is held
    to 1e-5: the wet-node walls do not conserve mass, and rho drifts slowly -- 4e-6 between the window's mean and its last step.)"""
    uLB = 0.08
    with CavitySolver(64, 64, 100.0, RT="MRT", dtype=np.float64, turb=0) as s:
        past, hits = 0.0, 0
        while hits <= 5:
            s.step(3000)
            m = s.mean_u()
            hits += abs(m - past) / uLB < 1e-8
            past = m
            assert s.steps_done < 600000
        s.begin_statistics(1).step(2000)
        st = s.statistics()
        u, rho = s.get_fields()
    assert st["samples"] == 2000
    assert np.abs(st["u"] - u).max() <= 1e-6 * np.abs(u).max()
    assert np.abs(st["rho"] - rho).max() <= 1e-5 * np.abs(rho).max()
    for k in ("uu", "vv", "uv"):
        assert np.abs(st[k]).max() <= 1e-10 * uLB ** 2, k


# The reference's default LES run (SRT, Smagorinsky, 160^2) at the two Reynolds numbers of the last Ghia columns.  Bounds: the
# largest centreline error of the time-mean this run measured on the MI355X (0.084 at Re 7500, 0.135 at Re 10000,
# in lid-velocity units, Ghia's typos masked) with about 20 % headroom.
LES_ITERS, LES_FROM, LES_EVERY = 240000, 120000, 50
LES_BOUND = {7500: 0.10, 10000: 0.16}


@pytest.mark.parametrize("Re", [7500, 10000])
def test_reference_default_run_time_mean_against_ghia(Re, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=LES_ITERS, Re=float(Re), RT="SRT", turb=1, xsize=160, ysize=160, Pinterval=20000, SavePlot=False,
                   SaveVTK=False, quiet=True, AverageFrom=LES_FROM, AverageEvery=LES_EVERY)
    assert r.samples == (LES_ITERS - LES_FROM) // LES_EVERY
    em = ghia.profile_errors(r.u_mean, Re, 0.08, mask_typos=True)
    ei = ghia.profile_errors(r.u.astype(np.float64), Re, 0.08, mask_typos=True)
    k = (r.uu + r.vv) / 0.08 ** 2
    print(f"Re {Re}: mean errors {em}, last-field errors {ei}, max (uu + vv) / uLB^2 {k.max():.3e} mean {k.mean():.3e}, "
          f"max |uv| / uLB^2 {np.abs(r.uv).max() / 0.08 ** 2:.3e}, regression of the mean {r.regression_mean[-1:]}")
    assert np.isfinite(r.u_mean).all() and (r.uu >= -1e-12).all() and (r.vv >= -1e-12).all()
    assert max(em) <= LES_BOUND[Re]
