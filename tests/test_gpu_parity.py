"""GPU parity tests proper (run with -m gpu on an MI355X): the HIP path, called through the C
ABI (ctypes -> liblbm_hip.so), against the CPU oracle on identical inputs.

Tolerances: the library is compiled with -ffp-contract=off and keeps the reference's operation
order, so fp64 AND fp32 results are required to be BIT-IDENTICAL to the oracle (np.array_equal);
north_star's 1e-6 relative tolerance on the centrelines is asserted on top for config C1.
Nothing here reads /root/reference.
"""
import json
import os

import numpy as np
import pytest

from oracle.lbm_ref import CavityOracleC, set_threads, max_threads
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, ghia
from latticeboltzmannsimulations_amd.slab import LocalSlabs, partition_rows

from checks import same_as_oracle, smooth_state

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KERNELS = ["generic", "auto"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("sem", ["mrt_py", "mrt_gpu"])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hip_step_is_bit_identical_to_oracle(kernel, sem, coll, dtype):
    for nx, ny in ((16, 16), (40, 24), (300, 20), (24, 300), (1028, 12)):
        o = CavityOracleC(nx, ny, 100.0, semantics=sem, collision=coll, dtype=dtype)
        with CavitySolver(nx, ny, 100.0, RT=coll, semantics=sem, dtype=dtype, kernel=kernel) as s:
            assert np.array_equal(s.get_fields(want_fin=True)[2], o.fin), "initial equilibrium differs"
            for n in (1, 1, 1, 7, 90):
                o.step(n); s.step(n)
                same_as_oracle(s, o, f"{nx}x{ny} after {o.nsteps} steps")
            assert s.steps_done == 100


@pytest.mark.parametrize("layout", ["planes", "rows"])
@pytest.mark.parametrize("kernel", ["generic", "vec"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_layouts_give_identical_results(layout, kernel, dtype):
    nx, ny = 260, 37
    o = CavityOracleC(nx, ny, 400.0, semantics="mrt_gpu", collision="MRT", dtype=dtype).step(60)
    with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=dtype, kernel=kernel, layout=layout) as s:
        s.step(60)
        same_as_oracle(s, o, f"layout={layout} kernel={kernel}")
    if kernel == "generic":
        o = CavityOracleC(nx, ny, 400.0, semantics="mrt_py", collision="SRT", dtype=dtype).step(60)
        with CavitySolver(nx, ny, 400.0, RT="SRT", semantics="mrt_py", dtype=dtype, layout=layout) as s:
            s.step(60)
            same_as_oracle(s, o, f"mrt_py layout={layout}")


@pytest.mark.parametrize("kernel", ["generic", "vec", "tb"])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_smagorinsky_closure_is_bit_identical_to_oracle(kernel, coll, dtype):
    """turb = 1 (MRT_GPU.py:368-387): per-cell relaxation rate from the previous step's equilibrium."""
    for nx, ny, layout in ((40, 34, "rows"), (260, 41, "planes")):
        o = CavityOracleC(nx, ny, 5000.0, semantics="mrt_gpu", collision=coll, dtype=dtype, turb=1)
        with CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=1, kernel=kernel, layout=layout) as s:
            for n in (1, 2, 57):
                o.step(n); s.step(n)
                same_as_oracle(s, o, f"turb {coll} {nx}x{ny} after {o.nsteps}")
            # upload convention: history := equilibrium / density of the uploaded state
            _, _, fin = s.get_fields(want_fin=True)
            s.set_state(fin); o.set_state(fin)
            o.step(9); s.step(9)
            same_as_oracle(s, o, "turb after set_state")


def test_smagorinsky_on_slabs():
    nx, ny, steps = 132, 45, 30
    with CavitySolver(nx, ny, 5000.0, RT="SRT", dtype=np.float32, turb=1) as one:
        one.step(steps)
        u1, r1, f1 = one.get_fields(want_fin=True)
    slabs = [CavitySolver(nx, ny, 5000.0, RT="SRT", dtype=np.float32, turb=1, rows=r) for r in partition_rows(ny, 3)]
    LocalSlabs(slabs).step(steps)
    u = np.zeros_like(u1); rho = np.zeros_like(r1); fin = np.zeros_like(f1)
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, f1) and np.array_equal(u, u1) and np.array_equal(rho, r1)


@pytest.mark.parametrize("sem", ["mrt_gpu", "mrt_py"])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_steps_per_launch_is_bit_identical_to_oracle(sem, coll, dtype):
    """kernel='tb': temporal blocking through LDS on the interior + single steps on the frame.  Sizes with partial
    tiles in x and y, one tile only, and many tiles; step counts that mix single and double steps."""
    for nx, ny, layout in ((260, 75, "rows"), (64, 33, "planes"), (132, 131, "rows")):
        o = CavityOracleC(nx, ny, 400.0, semantics=sem, collision=coll, dtype=dtype)
        with CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype, kernel="tb", layout=layout) as s:
            for n in (1, 2, 3, 4, 5, 64):
                o.step(n); s.step(n)
                same_as_oracle(s, o, f"tb {sem} {coll} {nx}x{ny} after {o.nsteps} steps")
            _, _, fin = s.get_fields(want_fin=True)
            s.set_state(fin); o.set_state(fin)
            o.step(11); s.step(11)
            same_as_oracle(s, o, "tb after set_state")


@pytest.mark.parametrize("sem,coll", [("mrt_gpu", "MRT"), ("mrt_py", "SRT")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_step_on_thin_and_wide_lattices(sem, coll, dtype):
    """Shapes at the limits of the multi-step path: 64 cells in one direction (the frame of width 8 leaves 48), very wide and
    very tall; frame segments of every default length (16 / 32) and the LDS windows of the fused frame passes."""
    for nx, ny, steps in ((1028, 64, 23), (64, 516, 23), (2052, 68, 12), (640, 640, 11)):
        o = CavityOracleC(nx, ny, 400.0, semantics=sem, collision=coll, dtype=dtype).step(steps)
        with CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype) as s:      # kernel = auto
            s.step(steps)
            same_as_oracle(s, o, f"{nx}x{ny} {sem} {coll}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_and_three_steps_per_launch_agree(dtype):
    """The interior advances three to five steps per launch by default (two with tuning tb_steps=2): same bits either way."""
    o = CavityOracleC(132, 99, 400.0, semantics="mrt_gpu", collision="MRT", dtype=dtype).step(47)
    for steps in (2, 3, 4, 5):   # (fp64: the x rim of the tiles is two vectors wide from four steps on)
        for eager in (False, True):     # lazy one-step lag (u / rho recomputed on demand) and a single last step
            with CavitySolver(132, 99, 400.0, RT="MRT", dtype=dtype, kernel="tb", tuning=dict(tb_steps=steps, eager_lag=eager)) as s:
                s.step(47)
                same_as_oracle(s, o, f"tb_steps={steps} eager_lag={eager}")
    for sem, coll in (("mrt_py", "SRT"), ("mrt_gpu", "TRT")):
        o = CavityOracleC(260, 71, 400.0, semantics=sem, collision=coll, dtype=dtype).step(33)
        with CavitySolver(260, 71, 400.0, RT=coll, semantics=sem, dtype=dtype, kernel="tb", tuning=dict(tb_steps=4)) as s:
            s.step(33)
            same_as_oracle(s, o, f"four steps {sem} {coll}")
    # the other routes of the frame passes: one launch per pass on the second stream (row strips by vector cells), and the
    # fused passes through scratch lattices instead of LDS windows; segment lengths that do / do not fit the LDS budget
    o = CavityOracleC(260, 131, 400.0, semantics="mrt_gpu", collision="MRT", dtype=dtype).step(27)
    for tune in (dict(frame_fused=False), dict(frame_lds=False), dict(frame_seg=64), dict(frame_seg=8), dict(nt=True), dict(nt=False)):
        with CavitySolver(260, 131, 400.0, RT="MRT", dtype=dtype, kernel="tb", tuning=tune) as s:
            s.step(27)
            same_as_oracle(s, o, f"{tune}")
    # with the Smagorinsky closure: two-phase kernel (history through LDS) and in-place kernel (history in registers)
    o = CavityOracleC(132, 99, 5000.0, semantics="mrt_gpu", collision="MRT", dtype=dtype, turb=1).step(29)
    for steps in (2, 3, 4, 5):
        with CavitySolver(132, 99, 5000.0, RT="MRT", dtype=dtype, turb=1, kernel="tb", tuning=dict(tb_steps=steps)) as s:
            s.step(29)
            same_as_oracle(s, o, f"turb tb_steps={steps}")


@pytest.mark.parametrize("dtype,coll,turb", [(np.float32, "MRT", 0), (np.float64, "SRT", 1), (np.float64, "MRT", 0)])
def test_one_step_lag_after_every_kind_of_last_unit(dtype, coll, turb):
    """lbm_get_fields returns the u / rho computed in the LAST iteration.  After a multi-step launch unit
    the lattice that iteration started from is recomputed on demand; every call length 1 .. 14 (last unit: single step,
    3-, 4-, 5-step launch), fields asked for once, twice, or not at all between calls; mean_u and tau from the same state."""
    nx, ny = 132, 99
    o = CavityOracleC(nx, ny, 1000.0, semantics="mrt_gpu", collision=coll, dtype=dtype, turb=turb)
    with CavitySolver(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, kernel="tb") as s:
        for n in range(1, 15):
            o.step(n); s.step(n)
            if n % 3 == 0:
                continue                                   # no read between these calls
            same_as_oracle(s, o, f"after a call of {n} steps")
            if n % 2:
                same_as_oracle(s, o, "asked twice")
            m = s.mean_u()
            assert abs(m - float(np.mean(o.u.astype(np.float64)))) < 1e-6 * 0.08
        tau = s.get_tau()
        if turb == 0:
            assert np.all(tau == dtype(1.0) / dtype(s.relax["omega"]))
        else:
            assert tau.min() >= (1.0 / s.relax["omega"]) * (1 - 1e-6) and tau.max() > tau.min()


@pytest.mark.parametrize("sem,coll,turb", [("mrt_gpu", "MRT", 0), ("mrt_gpu", "SRT", 1), ("mrt_gpu", "TRT", 0), ("mrt_py", "SRT", 0), ("mrt_gpu", "MRT", 1)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["pairs", "walls", "frame"])
def test_streaming_kernel_is_bit_identical_to_oracle(sem, coll, turb, dtype, mode):
    """kernel='stream' (lbm_stream.hpp): up to 8 time steps per launch streamed down column strips -- rows in registers,
    neighbour rows through LDS, x neighbours by DPP.  Sizes with one and several strips (partial last strip), one and several
    row segments, every steps-per-launch setting 2 .. 8 (frame widths 4 / 8 / 12), call lengths that leave every remainder
    (tail units of 3 .. 7 steps, single steps), fields read after units of every length (lagged lattice recomputed by the same
    kernel).  mode: "frame" = k_stream, the cells next to the walls as a frame of single-step passes (slabs, MRT.py semantics, the
    operator variants that would spill); "walls" = the walls inside the streaming kernel (k_stream_walls, r03: side walls on the lane
    shifts, lid / bottom row as rows of the pipeline, corner kept slots carried; the default for a lone MRT / fp64 SRT lattice in
    MRT_GPU.py semantics); "pairs" = that with two rows per wave, twelve waves, up to 10 steps per launch (k_stream_pairs, an r03
    experiment kept for A/B).  All three bit-identical to the oracle."""
    if mode != "frame" and sem == "mrt_py":
        pytest.skip("the walls inside the streaming kernel: MRT_GPU.py semantics only (MRT.py lattices keep the frame: the other leg)")
    walls = mode != "frame"
    sizes = ((320, 192, 8), (1028, 80, 0), (132, 600, 5), (516, 300, 7), (260, 131, 2), (64, 64, 8), (772, 257, 6), (304, 99, 3), (288, 160, 4),
             (256, 70, 8), (252, 75, 8), (496, 64, 8), (500, 67, 7), (64, 200, 8))
    if mode == "pairs":      # ... and the step counts only this kernel takes; odd row counts (a pair without a B row), one-pair segments
        sizes += ((320, 193, 10), (516, 301, 10), (1028, 81, 9), (260, 64, 10), (128, 65, 9))
    for nx, ny, tbs in sizes:
        o = CavityOracleC(nx, ny, 1000.0, semantics=sem, collision=coll, dtype=dtype, turb=turb)
        # (the wall frame inside the launch or as a kernel of its own beside the streaming workgroups: alternate, whatever the default)
        with CavitySolver(nx, ny, 1000.0, RT=coll, semantics=sem, dtype=dtype, turb=turb, kernel="stream",
                          tuning=dict(tb_steps=tbs, frame_beside=bool((nx // 4) % 2), stream_walls=mode != "frame", stream_pairs=mode == "pairs")) as s:
            assert s.describe()["kernel"] == {"pairs": "k_stream_pairs", "walls": "k_stream_walls", "frame": "k_stream"}[mode], s.describe()
            for n in (1, 8, 19, 3, 7, 12):
                o.step(n); s.step(n)
                same_as_oracle(s, o, f"stream {nx}x{ny} tb_steps={tbs} {sem} {coll} turb={turb} after {o.nsteps} steps")
            assert s.next_unit(100) == (tbs or (10 if mode == "pairs" else 8)) or min(nx, ny) < 80


def test_seeded_random_configurations_against_oracle():
    """40 seeded random (size, steps, semantics, collision, dtype, kernel, layout, turb) draws; every kernel variant must
    reproduce the oracle bit for bit, including ragged sizes and step counts that mix 1-, 2- and 3-step launches."""
    rng = np.random.default_rng(20261004)
    for case in range(40):
        sem = "mrt_gpu" if rng.random() < 0.7 else "mrt_py"
        coll = ["SRT", "TRT", "MRT"][rng.integers(3)]
        dtype = [np.float32, np.float64][rng.integers(2)]
        turb = int(sem == "mrt_gpu" and rng.random() < 0.3)
        nx = int(rng.integers(8, 90)) * 4
        ny = int(rng.integers(32, 140))
        kernel = ["auto", "generic", "vec", "tb"][rng.integers(4)]
        if sem == "mrt_py" and kernel == "vec":
            kernel = "generic"
        if kernel in ("auto", "generic") and rng.random() < 0.5:
            nx = int(rng.integers(9, 333))            # any width: auto falls back to the one-thread-per-cell kernel
            ny = int(rng.integers(5, 140))
        layout = ["rows", "planes"][rng.integers(2)]
        Re = [100.0, 400.0, 1000.0, 5000.0][rng.integers(4)]
        chunks = [int(v) for v in rng.integers(1, 12, size=3)]
        o = CavityOracleC(nx, ny, Re, semantics=sem, collision=coll, dtype=dtype, turb=turb)
        with CavitySolver(nx, ny, Re, RT=coll, semantics=sem, dtype=dtype, turb=turb, kernel=kernel, layout=layout) as s:
            for n in chunks:
                o.step(n); s.step(n)
            same_as_oracle(s, o, f"case {case}: {nx}x{ny} {sem} {coll} {np.dtype(dtype).name} turb={turb} {kernel} {layout} {chunks}")


def test_seeded_random_configurations_of_the_streaming_kernel():
    """30 seeded random draws for kernel = stream: ragged widths (last strip partly outside the lattice, one to four strips), heights
    that no segment count divides, every steps-per-launch 3 .. 8, call lengths that leave every kind of tail (tail units of a lone
    fp32 lattice go to the tile kernel, the others stay), lone lattices and 2 - 3 slabs driven through the launch-unit API, the
    closure; strict arithmetic against the oracle, bit for bit, fields (one-step lag) included.  A third of the draws (a second
    generator, so the strict draws are those of round 2) run `arith = fast`: same bits as the one-cell-per-thread kernel in fast
    arithmetic, within the fast tolerance of the oracle."""
    rng = np.random.default_rng(20261005)
    rng_fast = np.random.default_rng(20261105)
    for case in range(30):
        dtype = [np.float32, np.float64][rng.integers(2)]
        V = 4 if dtype == np.float32 else 2
        coll = ["SRT", "TRT", "MRT"][rng.integers(3)]
        turb = int(rng.random() < 0.25)
        sem = "mrt_py" if (not turb and rng.random() < 0.2) else "mrt_gpu"
        nx = int(rng.integers(64 // V, 900 // V)) * V
        nslabs = 1 if sem == "mrt_py" else int(rng.integers(1, 4))
        ny = int(rng.integers(64, 200)) * nslabs + int(rng.integers(0, nslabs))
        tbs = int(rng.integers(3, 9))
        Re = [100.0, 1000.0, 5000.0][rng.integers(3)]
        chunks = [int(v) for v in rng.integers(1, 23, size=3)]
        tune = dict(tb_steps=tbs, tail_tiles=bool(rng.integers(2)), xcd_bands=bool(rng.integers(2)), stream_walls=bool(rng_fast.integers(2)), stream_pairs=bool(rng_fast.integers(2)))
        arith = "fast" if (sem == "mrt_gpu" and rng_fast.random() < 0.34) else "strict"
        what = f"case {case}: {nx}x{ny} {sem} {coll} {np.dtype(dtype).name} turb={turb} S={tbs} slabs={nslabs} {chunks} {tune} {arith}"
        o = CavityOracleC(nx, ny, Re, semantics=sem, collision=coll, dtype=dtype, turb=turb)
        for n in chunks:
            o.step(n)
        want = (o.u, o.rho, o.fin)
        if arith == "fast":
            with CavitySolver(nx, ny, Re, RT=coll, dtype=dtype, turb=turb, kernel="generic", arith="fast") as g:
                g.step(sum(chunks))
                want = g.get_fields(want_fin=True)
            tol = 2e-5 if dtype == np.float32 else 1e-9
            assert np.abs(want[2] - o.fin).max() / np.abs(o.fin).max() < tol, what
        if nslabs == 1:
            with CavitySolver(nx, ny, Re, RT=coll, semantics=sem, dtype=dtype, turb=turb, kernel="stream", arith=arith, tuning=tune) as s:
                for n in chunks:
                    s.step(n)
                got = s.get_fields(want_fin=True)
            assert all(np.array_equal(a, b) for a, b in zip(want, got)), what
            continue
        parts = partition_rows(ny, nslabs)
        mr = min(n for _, n in parts)
        slabs = [CavitySolver(nx, ny, Re, RT=coll, semantics=sem, dtype=dtype, turb=turb, kernel="stream", arith=arith, rows=r, min_rows=mr,
                              tuning=tune) for r in parts]
        drv = LocalSlabs(slabs)
        for n in chunks:
            drv.step(n)
        u = np.zeros_like(o.u); rho = np.zeros_like(o.rho); fin = np.zeros_like(o.fin)
        for sl in slabs:
            sl.get_fields(u=u, rho=rho, fin=fin)
            sl.close()
        assert np.array_equal(fin, want[2]) and np.array_equal(u, want[0]) and np.array_equal(rho, want[1]), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_step_streaming_slabs_keep_the_wall_frame(dtype):
    """Slabs that would take the walls inside the streaming kernel, run with two steps per launch: a two-step unit has no edge
    launch, so they plan k_stream (frame passes + bulk launch) and stay bit-identical to the oracle."""
    nx, ny, chunks = 320, 600, (1, 7, 12, 5)
    o = CavityOracleC(nx, ny, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=dtype)
    for n in chunks:
        o.step(n)
    parts = partition_rows(ny, 3)
    slabs = [CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=dtype, kernel="stream", rows=r, tuning=dict(tb_steps=2)) for r in parts]
    try:
        for sl in slabs:
            d = sl.describe()
            assert d["kernel"] == "k_stream" and d["steps_per_launch"] == 2, d
        drv = LocalSlabs(slabs)
        for n in chunks:
            drv.step(n)
        u = np.zeros_like(o.u); rho = np.zeros_like(o.rho); fin = np.zeros_like(o.fin)
        for sl in slabs:
            sl.get_fields(u=u, rho=rho, fin=fin)
    finally:
        for sl in slabs:
            sl.close()
    assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho)


def test_two_steps_per_launch_needs_its_preconditions():
    with pytest.raises(RuntimeError, match="kernel = TB"):
        CavitySolver(24, 64, 100.0, kernel="tb")
    with pytest.raises(RuntimeError, match="kernel = TB"):
        CavitySolver(66, 64, 100.0, kernel="tb", dtype=np.float32)


def test_config_c1_128_re100_1000_steps():
    """BASELINE.json configs[0]: 128x128, Re = 100, fp64, 1000 steps, MRT.py semantics."""
    rec = json.load(open(os.path.join(GOLDEN, "survey_appendix_c.json")))
    o = CavityOracleC(128, 128, 100.0, semantics="mrt_py", collision="SRT").step(1000)
    with CavitySolver(128, 128, 100.0, RT="SRT", semantics="mrt_py", dtype=np.float64) as s:
        assert s.relax["omega"] == rec["omega"]
        s.step(1000)
        same_as_oracle(s, o, "C1")
        u, rho = s.get_fields()
    # north_star gate: centreline u / v within 1e-6 relative (fp64)
    cx, cy = ghia.centrelines(u, 0.08)
    ox, oy = ghia.centrelines(o.u, 0.08)
    assert np.allclose(cx, ox, rtol=1e-6, atol=0) and np.allclose(cy, oy, rtol=1e-6, atol=0)
    # recorded cross-check (provenance in the JSON)
    for y, v in zip(rec["ux_mid_column"]["y"], rec["ux_mid_column"]["value_over_uLB"]):
        assert cx[y] == pytest.approx(v, rel=1e-6, abs=1e-15)
    for x, v in zip(rec["uy_mid_row"]["x"], rec["uy_mid_row"]["value_over_uLB"]):
        assert cy[x] == pytest.approx(v, rel=1e-6, abs=1e-15)
    assert ghia.regression_value(u, 100, 0.08) == pytest.approx(rec["regression_value"], rel=1e-9)


@pytest.mark.parametrize("coll,sem", [("MRT", "mrt_gpu"), ("SRT", "mrt_py")])
def test_config_c2_1024_re1000_100_steps(coll, sem):
    """BASELINE.json configs[1]: 1024x1024, Re = 1000, fp64, fused pull kernel."""
    set_threads(min(16, max_threads()))
    try:
        o = CavityOracleC(1024, 1024, 1000.0, semantics=sem, collision=coll).step(100)
    finally:
        set_threads(1)
    with CavitySolver(1024, 1024, 1000.0, RT=coll, semantics=sem, dtype=np.float64) as s:
        s.step(100)
        same_as_oracle(s, o, "C2")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batched_steps_equal_single_steps(dtype):
    a = CavitySolver(96, 80, 400.0, RT="MRT", dtype=dtype)
    b = CavitySolver(96, 80, 400.0, RT="MRT", dtype=dtype)
    a.step(37)
    for _ in range(37):
        b.step(1)
    ua, ra, fa = a.get_fields(want_fin=True)
    ub, rb, fb = b.get_fields(want_fin=True)
    assert np.array_equal(fa, fb) and np.array_equal(ua, ub) and np.array_equal(ra, rb)
    a.close(); b.close()


@pytest.mark.parametrize("sem", ["mrt_py", "mrt_gpu"])
def test_set_state_roundtrip_and_exact_restart(sem):
    nx, ny = 72, 56
    with CavitySolver(nx, ny, 100.0, RT="TRT", semantics=sem, dtype=np.float64) as s:
        s.step(25)
        _, _, fin25 = s.get_fields(want_fin=True)
        s.step(30)
        u55, rho55, fin55 = s.get_fields(want_fin=True)
    with CavitySolver(nx, ny, 100.0, RT="TRT", semantics=sem, dtype=np.float64) as r:
        r.set_state(fin25)
        _, _, back = r.get_fields(want_fin=True)
        assert np.array_equal(back, fin25)                      # a10 layout contract round trip
        r.step(30)
        u, rho, fin = r.get_fields(want_fin=True)
        assert np.array_equal(fin, fin55) and np.array_equal(u, u55) and np.array_equal(rho, rho55)
    # host dtype conversion on the boundary
    with CavitySolver(nx, ny, 100.0, RT="TRT", semantics=sem, dtype=np.float32) as r:
        r.set_state(fin25)                                      # fp64 host -> fp32 device
        _, _, back = r.get_fields(want_fin=True, out_dtype=np.float64)
        assert np.array_equal(back, fin25.astype(np.float32).astype(np.float64))


def test_reynolds_sweep_datagen(tmp_path):
    """datagen.generate (MRT_GPU_datagen.py): concurrent lattices == each solved alone by the oracle; file set."""
    from latticeboltzmannsimulations_amd.datagen import generate
    Re = np.array([100, 400, 1000, 2500])
    feq0, f_final, u_final, Re_out, its = generate(Re, xsize=48, ysize=48, maxIt=2500, Pinterval=400, concurrent=3,
                                                   OutputFolder=str(tmp_path / "out"), quiet=True)
    assert f_final.shape == (4, 9, 48, 48) and u_final.shape == (4, 2, 48, 48) and np.array_equal(Re_out, Re)
    for name in ("feq_initial.npy", "f_final.npy", "u_final.npy", "Re_range.npy"):
        assert os.path.exists(tmp_path / "out" / name)
    assert np.array_equal(np.load(tmp_path / "out" / "f_final.npy"), f_final)
    for i, re in enumerate(Re):
        o = CavityOracleC(48, 48, float(re), semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1)
        assert np.array_equal(feq0, o.fin)
        o.step(int(its[i]))
        assert np.array_equal(f_final[i], o.fin) and np.array_equal(u_final[i], o.u), re
    assert (its == 2500).all()          # not converged within maxIt at tolerance 1e-7: the loop ran to its end
    # a loose tolerance makes the lattices stop at different checks: each is recorded where the reference's loop
    # (MRT_GPU_datagen.py:862-871), run on the oracle alone, would have stopped it
    Re = np.array([100, 150, 400, 1000, 2500])
    _, f2, u2, _, its2 = generate(Re, xsize=48, ysize=48, maxIt=6000, Pinterval=100, tolerance=2e-3, concurrent=4, save=False, quiet=True)
    for i, re in enumerate(Re):
        o = CavityOracleC(48, 48, float(re), semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1)
        count, past, It = 0, 0.0, 0
        while True:
            o.step(It + 1 - o.nsteps)
            m = float(np.mean(o.u))
            count += abs(m - past) / 0.08 < 2e-3
            past = m
            if count > 5:
                break
            if It + 100 > 6000 - 1:
                o.step(6000 - o.nsteps)
                break
            It += 100
        assert its2[i] == o.nsteps, (re, its2[i], o.nsteps)
        assert np.array_equal(f2[i], o.fin) and np.array_equal(u2[i], o.u), re
    assert len(set(its2.tolist())) > 1 and its2.min() < 6000
    # the same criterion evaluated on lbm_mean_u -- mean(u) reduced on the device in double, B doubles per check
    # over PCIe instead of B fields.  Same stop iteration as the host criterion for every lattice of this sweep (the two means
    # differ by ~1e-9 relative, the decisive differences here are ~1e-3 of the tolerance away), same final populations.
    _, f3, u3, _, its3 = generate(Re, xsize=48, ysize=48, maxIt=6000, Pinterval=100, tolerance=2e-3, concurrent=4, save=False, quiet=True,
                                  convergence="device")
    assert np.array_equal(its3, its2) and np.array_equal(f3, f2) and np.array_equal(u3, u2)


def test_mean_u_and_tau_exports():
    """lbm_mean_u == mean of the u that lbm_get_fields returns (accumulated in double, run-to-run identical), for a single
    lattice, a batch and after single-step and multi-step units; lbm_get_tau == taus_g of the closure recomputed from the
    oracle's state (MRT_GPU.py:385-387), 1 / omega without the closure."""
    with CavitySolver(132, 99, 5000.0, RT="SRT", dtype=np.float32, turb=1, kernel="tb") as s:
        o = CavityOracleC(132, 99, 5000.0, semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1)
        for n in (1, 7, 1, 13):
            s.step(n)
            u, rho = s.get_fields()
            m = s.mean_u()
            assert m == s.mean_u()
            assert abs(m - float(np.mean(u.astype(np.float64)))) < 1e-12
            # the oracle one step behind holds the state (fin) and history (feq, rho of the step before) the last iteration started from
            o.step(s.steps_done - 1 - o.nsteps)
            f = o.fin.astype(np.float64)
            q = (f[5] - f[6] + f[7] - f[8]) - (o.feq[5].astype(np.float64) - o.feq[6] + o.feq[7] - o.feq[8])
            tau0 = 1.0 / s.relax["omega"]
            tau = 0.5 * (tau0 + np.sqrt(tau0 * tau0 + 18 * 1.4142 * 0.025 * np.abs(q) / o.rho.astype(np.float64)))
            got = s.get_tau(out_dtype=np.float64)
            assert np.abs(got - tau).max() < 2e-6 * tau0, n
            assert got.min() >= tau0 * (1 - 1e-6)
            if s.steps_done > 5:                       # (the very first iteration starts from the equilibrium: tau = tau0 everywhere)
                assert got.max() > tau0 * (1 + 1e-4)
    with CavityBatch(64, 64, [100.0, 1000.0, 5000.0], RT="MRT", dtype=np.float64) as b:
        b.step(30)
        u, _ = b.get_fields()
        m = b.mean_u()
        assert m.shape == (3,) and np.allclose(m, u.reshape(3, -1).mean(axis=1), rtol=0, atol=1e-15)
        tau = b.get_tau()
        assert tau.shape == (3, 64, 64) and all(np.all(tau[i] == 1.0 / b.relax_list[i]["omega"]) for i in range(3))


@pytest.mark.parametrize("kernel", ["generic", "vec", "tb"])
@pytest.mark.parametrize("dtype,coll,sem,turb", [(np.float32, "SRT", "mrt_gpu", 1), (np.float32, "MRT", "mrt_gpu", 0),
                                                 (np.float64, "TRT", "mrt_gpu", 0), (np.float64, "MRT", "mrt_gpu", 1),
                                                 (np.float64, "SRT", "mrt_py", 0)])
def test_batch_of_lattices_equals_lattices_run_alone(kernel, dtype, coll, sem, turb):
    """lbm_params.batch: B cavities with their own Reynolds numbers in one set of launches (the sweep of
    MRT_GPU_datagen.py:55-57); every lattice must evolve bit for bit as the oracle runs it alone."""
    if sem == "mrt_py" and kernel == "vec":
        pytest.skip("the vector kernel implements MRT_GPU.py semantics only")
    Res = [100.0, 400.0, 1000.0, 3200.0, 5000.0]
    nx, ny = 132, 75
    oracles = [CavityOracleC(nx, ny, Re, semantics=sem, collision=coll, dtype=dtype, turb=turb) for Re in Res]
    with CavityBatch(nx, ny, Res, RT=coll, semantics=sem, dtype=dtype, turb=turb, kernel=kernel) as b:
        def check(what, macros=True):
            u, rho, fin = b.get_fields(want_fin=True)
            assert fin.shape == (5, 9, nx, ny) and u.shape == (5, 2, nx, ny) and rho.shape == (5, nx, ny)
            for i, o in enumerate(oracles):
                assert np.array_equal(fin[i], o.fin), f"{what}: lattice {i} (Re {Res[i]}) fin differs"
                if macros:
                    assert np.array_equal(u[i], o.u) and np.array_equal(rho[i], o.rho), f"{what}: lattice {i} macros differ"
        check("initial state", macros=False)
        for n in (1, 2, 40):
            b.step(n)
            for o in oracles:
                o.step(n)
            check(f"after {oracles[0].nsteps} steps")
        # upload of a whole batch, then new rates for one lattice mid-run
        _, _, fin = b.get_fields(want_fin=True)
        fin = np.ascontiguousarray(fin[::-1])                      # lattice i restarts from the state of lattice 4 - i
        b.set_state(fin)
        for i, o in enumerate(oracles):
            o.set_state(fin[i])
        r = b.set_relaxation(2, Re=250.0)
        oracles[2] = CavityOracleC(nx, ny, 250.0, semantics=sem, collision=coll, dtype=dtype, turb=turb)
        oracles[2].set_state(fin[2])
        assert r["omega"] == pytest.approx(2.0 / (6.0 * 0.08 * ny / 250.0 + 1.0))
        b.step(13)
        for o in oracles:
            o.step(13)
        check("after set_state + set_relaxation")


def test_batch_argument_checks():
    with pytest.raises(RuntimeError, match="slab"):
        CavitySolver(64, 64, 100.0, rows=(0, 32), batch=3)
    with pytest.raises(ValueError):
        CavityBatch(64, 64, [])
    with CavityBatch(32, 32, [100.0, 200.0]) as b:
        with pytest.raises(RuntimeError, match="index"):
            b.set_relaxation(2, Re=100.0)
        with pytest.raises(ValueError):
            b.set_state(np.zeros((9, 32, 32), dtype=np.float32))      # the [B] axis is missing
        with pytest.raises(RuntimeError, match="batch"):
            b.halo_export(0, 0x1000)
    with CavityBatch(32, 32, [100.0]) as one, CavitySolver(32, 32, 100.0) as ref:      # a batch of one
        one.step(7); ref.step(7)
        assert np.array_equal(one.get_fields(want_fin=True)[2][0], ref.get_fields(want_fin=True)[2])
    with CavitySolver(32, 32, 100.0, dtype=np.float64) as s, CavitySolver(32, 32, 700.0, dtype=np.float64) as ref:
        s.set_relaxation(0, Re=700.0)                                   # single lattice: rates changed at run time
        s.step(9); ref.step(9)
        assert np.array_equal(s.get_fields(want_fin=True)[2], ref.get_fields(want_fin=True)[2])


def test_checkpoint_restart(tmp_path):
    with CavitySolver(96, 64, 400.0, RT="MRT", dtype=np.float64) as a:
        a.step(40)
        a.save_checkpoint(tmp_path / "ck.npz")
        a.step(25)
        ref = a.get_fields(want_fin=True)
    with CavitySolver(96, 64, 400.0, RT="MRT", dtype=np.float64) as b:
        assert b.load_checkpoint(tmp_path / "ck.npz") == 40
        b.step(25)
        assert all(np.array_equal(x, y) for x, y in zip(ref, b.get_fields(want_fin=True)))
    with CavitySolver(64, 64, 400.0) as c, pytest.raises(ValueError):
        c.load_checkpoint(tmp_path / "ck.npz")


def test_argument_checks():
    with CavitySolver(32, 32, 100.0) as s:
        with pytest.raises(ValueError):
            s.set_state(np.zeros((9, 32, 31)))
        with pytest.raises(ValueError):
            s.set_state(np.zeros((9, 32, 32), dtype=np.int32))
        with pytest.raises(ValueError):
            s.get_fields(u=np.zeros((2, 32, 32), order="F")[:, ::2])
    with pytest.raises(ValueError):
        CavitySolver(32, 32, 100.0, RT="BGK")
    with pytest.raises(RuntimeError, match="turb"):
        CavitySolver(32, 32, 100.0, turb=1, semantics="mrt_py", RT="SRT")
    with pytest.raises(RuntimeError, match="nx, ny"):
        CavitySolver(2, 32, 100.0)


@pytest.mark.parametrize("sem,coll", [("mrt_gpu", "MRT"), ("mrt_py", "SRT")])
def test_split_step_equals_fused_step(sem, coll):
    a = CavitySolver(80, 40, 100.0, RT=coll, semantics=sem, dtype=np.float64)
    b = CavitySolver(80, 40, 100.0, RT=coll, semantics=sem, dtype=np.float64)
    a.step(9)
    for _ in range(9):
        b.step_edges(); b.step_interior(); b.step_finish()
    fa, fb = a.get_fields(want_fin=True), b.get_fields(want_fin=True)
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    a.close(); b.close()


@pytest.mark.parametrize("sem,coll,dtype", [("mrt_gpu", "MRT", np.float64), ("mrt_gpu", "MRT", np.float32),
                                            ("mrt_py", "SRT", np.float64), ("mrt_gpu", "TRT", np.float64)])
@pytest.mark.parametrize("nslabs", [2, 3, 8])
def test_slabs_on_one_device_equal_single_slab(sem, coll, dtype, nslabs):
    """T6: S y-slabs (uneven) with halo export/import on ONE device == the undivided lattice."""
    nx, ny, steps = 132, 67, 40
    with CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype) as one:
        one.step(steps)
        u1, r1, f1 = one.get_fields(want_fin=True)
    slabs = [CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype, rows=r) for r in partition_rows(ny, nslabs)]
    LocalSlabs(slabs).step(steps)
    u = np.zeros_like(u1); rho = np.zeros_like(r1); fin = np.zeros_like(f1)
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, f1) and np.array_equal(u, u1) and np.array_equal(rho, r1)


def test_slab_restart_from_global_state():
    """set_state on slabs reads each slab's rows from the whole-lattice array."""
    nx, ny = 64, 50
    with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=np.float64) as one:
        one.step(20)
        _, _, f20 = one.get_fields(want_fin=True)
        one.step(15)
        u35, r35, f35 = one.get_fields(want_fin=True)
    slabs = [CavitySolver(nx, ny, 100.0, RT="MRT", dtype=np.float64, rows=r) for r in partition_rows(ny, 3)]
    for s in slabs:
        s.set_state(f20)
    LocalSlabs(slabs).step(15)
    u = np.zeros_like(u35); rho = np.zeros_like(r35); fin = np.zeros_like(f35)
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, f35) and np.array_equal(u, u35) and np.array_equal(rho, r35)


@pytest.mark.parametrize("Re,n,RT,dtype,tol,arith", [(100, 128, "MRT", np.float64, 0.03, "strict"), (1000, 256, "MRT", np.float32, 0.05, "strict"),
                                                     (1000, 256, "SRT", np.float64, 0.05, "strict"), (1000, 256, "MRT", np.float32, 0.05, "fast"),
                                                     (100, 128, "MRT", np.float64, 0.03, "fast"),
                                                     # the streaming kernel (what the benchmark lattices run), eight steps per launch
                                                     (1000, 256, "MRT", np.float32, 0.05, "fast:stream"), (100, 128, "MRT", np.float64, 0.03, "strict:stream"),
                                                     # the fused SRT / TRT fast operators (r03: the equilibrium is never formed, lbm_device.hpp equ_collide),
                                                     # and SRT with the closure -- the reference script's default mode
                                                     (1000, 256, "SRT", np.float32, 0.05, "fast:stream"), (1000, 256, "TRT", np.float32, 0.05, "fast:stream"),
                                                     (1000, 256, "TRT", np.float64, 0.05, "fast"), (1000, 256, "SRT", np.float64, 0.06, "fast:auto:turb")])
def test_converged_cavity_matches_ghia(Re, n, RT, dtype, tol, arith):
    """T7 (physics): run to the reference's convergence criterion (MRT_GPU.py:883-889) and compare the centrelines
    with Ghia et al. at the geometrically correct positions; global mass drift stays small."""
    arith, _, kernel = arith.partition(":")
    kernel, _, turb = kernel.partition(":")
    with CavitySolver(n, n, float(Re), RT=RT, dtype=dtype, arith=arith, kernel=kernel or "auto", turb=1 if turb else 0) as s:
        prev, quiet = None, 0
        for _ in range(400):
            s.step(3000)
            u, rho = s.get_fields(out_dtype=np.float64)
            m = float(np.mean(u))
            if prev is not None and abs(m - prev) / 0.08 < 1e-8:
                quiet += 1
                if quiet > 5:
                    break
            prev = m
        _, _, fin = s.get_fields(want_fin=True, out_dtype=np.float64)
    ex, ey = ghia.profile_errors(u, Re, 0.08)
    assert ex < tol and ey < tol, (ex, ey, s.steps_done)
    # the reference's own metric (MRT_GPU.py:815-821) samples the column at approximate, reversed rows: indicative only
    assert ghia.r2_value(u, Re, 0.08) > 0.9
    # (fp32 means never settle to 1e-8: those runs last all 1.2 M steps, over which the wall rules have let 1.7 % (SRT) / 3.7 % (TRT; the
    # strict operator the same: 3.70 against 3.77 %, tools/probes/trt_mass.py) of the mass in; MRT 0.2 %, the fp64 runs stop after ~340 k steps at 1.5 %)
    assert abs(fin.sum() - n * n) / (n * n) < (5e-2 if RT == "TRT" and dtype == np.float32 else 2e-2)


@pytest.mark.parametrize("Re,n,dtype,arith,kernel,cap,tol", [
    (400, 256, np.float64, "strict", "auto", 600_000, 0.04), (400, 256, np.float32, "fast", "stream", 400_000, 0.04),
    (3200, 256, np.float32, "strict", "stream", 800_000, 0.05), (3200, 256, np.float64, "fast", "auto", 1_200_000, 0.05),
    (5000, 384, np.float32, "fast", "auto", 2_400_000, 0.04), (5000, 256, np.float64, "strict", "auto", 1_800_000, 0.055)])
def test_converged_cavity_matches_the_other_ghia_columns_and_the_vortex_table(Re, n, dtype, arith, kernel, cap, tol):
    """the only fixtures the reference holds for this path are GhiaData.csv's centreline columns and its vortex
    table (MRT.py:104-116).  Re = 400, 3200 (configs[3]) and 5000 (configs[4]), MRT, run to the reference's convergence criterion
    (MRT_GPU.py:883-889, on the device mean; fp32 means do not settle to 1e-8, those runs stop at `cap`, past the fp64 runs' count):
    (a) centrelines at the geometrically correct positions against the Ghia columns, the table's known bad entries masked (ghia.TYPOS,
    ghia.PAPER_MISPRINTS) -- measured r03 (max |dUx| / max |dUy|, u_lid): Re 400 0.014 / 0.016, Re 3200 0.038 / 0.039 (fp32) and 0.041 / 0.041
    (fp64) at 256^2, Re 5000 0.028 / 0.024 (384^2), 0.042 / 0.044 (256^2); (b) the primary vortex centre against VORTEX_GHIA rows 0 / 7 within
    two Ghia grid spacings (2 / 128) -- measured: Re 400 on the table value, Re 3200 (-0.0009, -0.0078), Re 5000 (+0.0039, -0.0013 .. -0.0040);
    (c) the two minima of |u|^2 the reference's own search returns (MRT_GPU.py:764-778) each sit on a vortex of the table (within 3 / 128;
    measured <= 0.0142: they are the bottom-left and a bottom-right eddy, not the primary vortex)."""
    with CavitySolver(n, n, float(Re), RT="MRT", dtype=dtype, arith=arith, kernel=kernel) as s:
        prev, quiet = None, 0
        while s.steps_done < cap and quiet <= 5:
            s.step(3000)
            m = s.mean_u()
            quiet = quiet + 1 if (prev is not None and abs(m - prev) / 0.08 < 1e-8) else 0
            prev = m
        u, rho = s.get_fields(out_dtype=np.float64)
        steps = s.steps_done
    assert np.isfinite(u).all()
    ex, ey = ghia.profile_errors(u, Re, 0.08, mask_typos=True)
    dx, dy = ghia.primary_vortex_error(u, Re, 0.08)
    near = [ghia.nearest_vortex_error(l, Re, n, n) for l in ghia.locate_vortices(u, 0.08)]
    print(f"\nRe={Re} {n}^2 {np.dtype(dtype).name} {arith} {kernel}: steps {steps}, max|dUx| {ex:.4f}, max|dUy| {ey:.4f}, primary vortex "
          f"({dx:+.4f}, {dy:+.4f}), reference's two minima -> nearest table vortex (distance, row) {near}")
    assert ex < tol and ey < tol, (ex, ey)
    assert abs(dx) <= 2 / 128 + 1e-9 and abs(dy) <= 2 / 128 + 1e-9, (dx, dy)
    assert all(d <= 3 / 128 for d, _ in near), near


@pytest.mark.parametrize("sem,coll", [("mrt_gpu", "MRT"), ("mrt_gpu", "TRT"), ("mrt_py", "SRT")])
def test_minimum_sizes_and_empty_calls(sem, coll):
    """Edge cases: the smallest lattices the library accepts (4 x 4: every cell is a wall cell or next to one), two-row
    slabs, and lbm_step(0)."""
    for nx, ny in ((4, 4), (5, 4), (4, 7), (8, 5), (6, 6)):
        for dtype in (np.float64, np.float32):
            o = CavityOracleC(nx, ny, 100.0, semantics=sem, collision=coll, dtype=dtype)
            with CavitySolver(nx, ny, 100.0, RT=coll, semantics=sem, dtype=dtype) as s:
                s.step(0)
                assert s.steps_done == 0 and np.array_equal(s.get_fields(want_fin=True)[2], o.fin)
                for n in (1, 2, 22):
                    o.step(n); s.step(n)
                    same_as_oracle(s, o, f"{nx}x{ny} {sem} {coll} after {o.nsteps}")
                s.step(0)
                same_as_oracle(s, o, "after an empty step call")
    nx, ny = 12, 8
    o = CavityOracleC(nx, ny, 100.0, semantics=sem, collision=coll, dtype=np.float64).step(15)
    slabs = [CavitySolver(nx, ny, 100.0, RT=coll, semantics=sem, dtype=np.float64, rows=(y0, 2)) for y0 in range(0, ny, 2)]
    LocalSlabs(slabs).step(15)
    u = np.zeros_like(o.u); rho = np.zeros_like(o.rho); fin = np.zeros_like(o.fin)
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho)


def _threads():
    return max(1, min(max_threads(), 16))


@pytest.mark.parametrize("steps", [13, 20])
def test_config_c3_4096_fp32_against_oracle(steps):
    """BASELINE.json configs[2] at full size -- 4096 x 4096, Re = 1000, fp32, MRT, the lattice bench.py times -- against the C
    oracle: the default kernels (several steps per launch) in the reference's operation order bit for bit; arith = fast (what
    bench.py's headline runs) within 2e-5 of it.  20 steps = the driver's bench shape (raw step + multi-step units)."""
    n = 4096
    set_threads(_threads())
    try:
        o = CavityOracleC(n, n, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32).step(steps)
    finally:
        set_threads(1)
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32) as s:
        s.step(steps)
        assert s.next_unit(100) >= 4                                         # (several steps per launch is what ran)
        same_as_oracle(s, o, f"C3 strict, {steps} steps")
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32, arith="fast") as f:
        f.step(steps)
        u, rho, fin = f.get_fields(want_fin=True)
    assert np.abs(fin - o.fin).max() / np.abs(o.fin).max() < 2e-5
    assert np.abs(u - o.u).max() / 0.08 < 2e-4 and np.abs(rho - o.rho).max() < 2e-5


def test_strict_fp32_path_against_the_promoted_oracle():
    """VERDICT r02 "missing" item 1, quantified on the shipped path: MRT_GPU.py's CUDA text evaluates the sub-expressions that carry
    `double` literals (lines 385, 410, 638-642, 652) in double and rounds once (oracle `promote=True`); the library computes fp32
    lattices in fp32 throughout (== the plain oracle bit for bit, asserted here too).  Distance of the HIP strict fp32 path from the
    PROMOTED oracle, the stated tolerance of that deviation: populations <= 1e-5 relative, u <= 5e-5 uLB after 1, 100, 1000 steps at
    128 x 128 (MRT; SRT + closure = the reference script's default mode) and <= 1e-6 / 1e-5 on the C3 lattice after the 20 steps of
    the driver's bench.  Measured values: DESIGN "Arithmetic contract" (a few 1e-6: a tenth of fp32's own distance from fp64)."""
    n = 128
    rows = []
    for coll, turb in (("MRT", 0), ("SRT", 1)):
        plain = CavityOracleC(n, n, 1000.0, semantics="mrt_gpu", collision=coll, dtype=np.float32, turb=turb)
        prom = CavityOracleC(n, n, 1000.0, semantics="mrt_gpu", collision=coll, dtype=np.float32, turb=turb, promote=True)
        with CavitySolver(n, n, 1000.0, RT=coll, dtype=np.float32, turb=turb) as s:
            done = 0
            for steps in (1, 100, 1000):
                plain.step(steps - done); prom.step(steps - done); s.step(steps - done); done = steps
                u, rho, fin = s.get_fields(want_fin=True)
                assert np.array_equal(fin, plain.fin) and np.array_equal(u, plain.u)
                df, du = np.abs(fin - prom.fin).max() / np.abs(prom.fin).max(), np.abs(u - prom.u).max() / 0.08
                ulp = np.abs(fin.view(np.int32).astype(np.int64) - prom.fin.view(np.int32).astype(np.int64))
                rows.append((coll, turb, steps, df, du, int(ulp.max()), float((ulp > 0).mean())))
                assert df < 1e-5 and du < 5e-5, rows[-1]
    n = 4096
    set_threads(_threads())
    try:
        prom = CavityOracleC(n, n, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32, promote=True).step(20)
    finally:
        set_threads(1)
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32) as s:
        s.step(20)
        u, rho, fin = s.get_fields(want_fin=True)
    df, du = np.abs(fin - prom.fin).max() / np.abs(prom.fin).max(), np.abs(u - prom.u).max() / 0.08
    ulp = np.abs(fin.view(np.int32).astype(np.int64) - prom.fin.view(np.int32).astype(np.int64))
    rows.append(("MRT C3 4096^2", 0, 20, df, du, int(ulp.max()), float((ulp > 0).mean())))
    assert df < 1e-6 and du < 1e-5, rows[-1]
    print("\npromotion gap (HIP strict fp32 vs promoted oracle): operator, closure, steps, max rel populations, max u / uLB, max ulp, share of differing words")
    for r in rows:
        print("  %-14s turb=%d %5d steps  %.3g  %.3g  %d ulp  %.4f" % r)


def test_config_c4_8192_fp64_re3200_slabs_and_oracle():
    """BASELINE.json configs[3]: 8192 x 8192, Re = 3200, fp64, MRT, y-slabs for 8 GPUs.  On one device: the undivided lattice
    (default multi-step kernels) == the C oracle after 10 steps, == the one-step vector kernel, == 8 slabs of 8192 x 1024
    driven through the multi-step launch units with deep halos (what each of the 8 ranks runs), all bit for bit."""
    n, steps, nslabs = 8192, 10, 8
    set_threads(_threads())
    try:
        o = CavityOracleC(n, n, 3200.0, semantics="mrt_gpu", collision="MRT", dtype=np.float64).step(steps)
    finally:
        set_threads(1)
    with CavitySolver(n, n, 3200.0, RT="MRT", dtype=np.float64) as one:
        assert abs(one.relax["omega"] - 0.8973438621679827) < 1e-15
        one.step(steps)
        same_as_oracle(one, o, "C4 undivided")
    u = np.zeros_like(o.u); rho = np.zeros_like(o.rho); fin = np.zeros_like(o.fin)
    with CavitySolver(n, n, 3200.0, RT="MRT", dtype=np.float64, kernel="vec") as v:
        v.step(steps)
        v.get_fields(u=u, rho=rho, fin=fin)
    assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho), "vec"
    for arith in ("strict", "fast"):     # fast: five steps per launch on the slabs (strict fp64 MRT: three, last step single)
        parts = partition_rows(n, nslabs)
        slabs = [CavitySolver(n, n, 3200.0, RT="MRT", dtype=np.float64, rows=r, min_rows=n // nslabs, arith=arith) for r in parts]
        LocalSlabs(slabs).step(steps)
        assert slabs[3].next_unit(100) >= 3
        u[:] = 0; rho[:] = 0; fin[:] = 0
        for sl in slabs:
            sl.get_fields(u=u, rho=rho, fin=fin)
            sl.close()
        if arith == "strict":
            assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho), "8 slabs"
        else:
            assert np.abs(fin - o.fin).max() / np.abs(o.fin).max() < 1e-9 and np.abs(u - o.u).max() / 0.08 < 1e-9


def test_config_c5_16384_fp32_re5000_slabs():
    """BASELINE.json configs[4] (and the edge case 'maximum sizes'): 16384 x 16384, Re = 5000, fp32 = 268 M cells, element
    offsets beyond 2^31 in the [y][k][x] layout (9.7 GB per lattice), cut into 8 slabs of 16384 x 2048 -- the per-GPU share of
    the weak-scaling series, all 8 resident on the one device.  A smooth non-trivial state advanced 12 steps as ONE lattice
    (arith = fast as benched: raw step, eight-step launches of the streaming kernel, the rest) must equal, bit for bit, the same
    state advanced by the 8 slabs through the multi-step launch units with deep halos (edge launch + bulk launch per unit); the first 3 steps also against the C oracle's
    reference-order arithmetic within the fast form's tolerance."""
    n, steps, nslabs = 16384, 12, 8
    x = np.arange(n, dtype=np.float32)
    base = (1.0 + 1e-3 * np.sin(0.01 * x)[:, None] * np.cos(0.013 * x)[None, :]).astype(np.float32)
    t = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    fin0 = np.empty((9, n, n), dtype=np.float32)
    for k in range(9):
        np.multiply(base, t[k] * np.float32(1.0 + 1e-4 * k), out=fin0[k])
    del base
    with CavitySolver(n, n, 5000.0, RT="MRT", dtype=np.float32, arith="fast") as one:
        assert abs(one.relax["omega"] - 0.7773438471679809) < 1e-15         # omega from the global height
        one.set_state(fin0)
        one.step(steps)
        u1, r1, f1 = one.get_fields(want_fin=True)
    assert np.isfinite(f1[:, ::97, ::89]).all() and abs(float(r1[::64, ::64].mean()) - 1.0) < 1e-2
    slabs = [CavitySolver(n, n, 5000.0, RT="MRT", dtype=np.float32, arith="fast", rows=r, min_rows=n // nslabs) for r in partition_rows(n, nslabs)]
    for sl in slabs:
        sl.set_state(fin0)
    LocalSlabs(slabs).step(steps)
    assert slabs[0].ny_local == 2048 and slabs[1].next_unit(100) == 8    # (the streaming kernel, as benched)
    u = np.zeros_like(u1); rho = np.zeros_like(r1); fin = np.zeros_like(f1)
    for sl in slabs:
        sl.get_fields(u=u, rho=rho, fin=fin)
        sl.close()
    assert np.array_equal(fin, f1) and np.array_equal(u, u1) and np.array_equal(rho, r1)
    del u, rho, fin, u1, r1, f1
    # a 16384 x 2048 slab-sized strip of the same state against the oracle (3 steps, strict order; the fast form within 2e-5)
    m = 2048
    sub = np.ascontiguousarray(fin0[:, :, :m])
    del fin0
    set_threads(_threads())
    try:
        o = CavityOracleC(n, m, 5000.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32, ny_global=n)
        o.set_state(sub)
        o.step(3)
    finally:
        set_threads(1)
    with CavitySolver(n, m, 5000.0 * m / n, RT="MRT", dtype=np.float32) as s:
        s.set_relaxation(0, **o.relax)                                      # omega of Re = 5000 at the GLOBAL height (MRT_GPU.py:63)
        s.set_state(sub)
        s.step(3)
        same_as_oracle(s, o, "C5 strip, strict")


@pytest.mark.parametrize("kernel", ["generic", "vec", "tb", "stream"])
@pytest.mark.parametrize("turb", [0, 1])
def test_fast_arithmetic_agrees_with_oracle_to_rounding(kernel, turb):
    """arith='fast': the MRT operator in factored form with fused multiply-adds -- algebraically the same operator, not the
    reference's operation order, so the comparison with the oracle is by tolerance: fp64 full field
    <= 1e-9 relative after 10 steps; fp32 <= 1e-4 relative to the fp64 oracle after 100 steps (and <= 2e-5 to the fp32 one).
    Every kernel variant and all steps-per-launch settings of the multi-step kernel."""
    nx, ny = (320, 192) if kernel == "stream" else (132, 99)
    for tbs in ((2, 3, 4, 5) if kernel == "tb" else (3, 8) if kernel == "stream" else (0,)):
        a64 = CavityOracleC(nx, ny, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=np.float64, turb=turb)
        a32 = CavityOracleC(nx, ny, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32, turb=turb)
        with CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=np.float64, turb=turb, kernel=kernel, arith="fast", tuning=dict(tb_steps=tbs)) as d, \
                CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=np.float32, turb=turb, kernel=kernel, arith="fast", tuning=dict(tb_steps=tbs)) as f:
            d.step(10); a64.step(10)
            u, rho, fin = d.get_fields(want_fin=True)
            assert not np.array_equal(fin, a64.fin)                           # it really is the other operation order
            assert np.abs(fin - a64.fin).max() / np.abs(a64.fin).max() < 1e-9
            assert np.abs(u - a64.u).max() / 0.08 < 1e-9 and np.abs(rho - a64.rho).max() < 1e-9
            d.step(90); a64.step(90); f.step(100); a32.step(100)
            u, rho, fin = d.get_fields(want_fin=True)
            assert np.abs(fin - a64.fin).max() / np.abs(a64.fin).max() < 1e-9
            u32, rho32, fin32 = f.get_fields(want_fin=True, out_dtype=np.float64)
            assert np.abs(fin32 - a64.fin).max() / np.abs(a64.fin).max() < 1e-4
            assert np.abs(u32 - a64.u).max() / 0.08 < 1e-3                     # fp32 itself is this far from fp64
            assert np.abs(fin32 - a32.fin).max() / np.abs(a32.fin).max() < 2e-5
            assert np.abs(u32 - a32.u).max() / 0.08 < 2e-4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_arithmetic_is_the_same_in_every_kernel(dtype):
    """The factored operator spells its fused multiply-adds out, so the one-cell-per-thread kernel, the vector kernel and
    the multi-step kernels (any steps per launch), slabs or not, all give the same bits -- as the strict form does."""
    nx, ny, steps = 132, 99, 37
    with CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=dtype, kernel="generic", arith="fast") as g:
        g.step(steps)
        ref = g.get_fields(want_fin=True)
    for kernel, tbs in (("vec", 0), ("tb", 2), ("tb", 3), ("tb", 4), ("tb", 5), ("stream", 8), ("stream", 5)):
        with CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=dtype, kernel=kernel, arith="fast", tuning=dict(tb_steps=tbs)) as s:
            s.step(steps)
            assert all(np.array_equal(x, y) for x, y in zip(ref, s.get_fields(want_fin=True))), (kernel, tbs)
    slabs = [CavitySolver(nx, ny, 1000.0, RT="MRT", dtype=dtype, arith="fast", rows=r) for r in partition_rows(ny, 3)]
    LocalSlabs(slabs).step(steps)
    u = np.zeros_like(ref[0]); rho = np.zeros_like(ref[1]); fin = np.zeros_like(ref[2])
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, ref[2]) and np.array_equal(u, ref[0]) and np.array_equal(rho, ref[1])


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("turb", [0, 1])
def test_fast_arithmetic_srt_trt_and_closure(coll, turb):
    """arith='fast' beyond the MRT operator: u = j * rcp(rho) and the closure's divisions / square root use the hardware's
    reciprocal and square-root instructions (fp32: 1 ulp; fp64: v_rcp_f64 / v_rsq_f64 refined by Newton steps).  Tolerance
    against the oracle after 100 steps: fp32 2e-5 on the populations, 2e-4 on u / uLB; fp64 1e-9.  All kernel variants give
    the same bits."""
    nx, ny, steps = 132, 99, 100
    for dtype, tol_f, tol_u in ((np.float32, 2e-5, 2e-4), (np.float64, 1e-9, 1e-9)):
        o = CavityOracleC(nx, ny, 5000.0, semantics="mrt_gpu", collision=coll, dtype=dtype, turb=turb).step(steps)
        ref = None
        for kernel, tbs in (("generic", 0), ("vec", 0), ("tb", 3), ("tb", 5), ("stream", 8), ("stream", 3)):
            with CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=turb, kernel=kernel, arith="fast", tuning=dict(tb_steps=tbs)) as s:
                s.step(steps)
                got = s.get_fields(want_fin=True)
            if ref is None:
                ref = got
                assert np.abs(got[2] - o.fin).max() / np.abs(o.fin).max() < tol_f
                assert np.abs(got[0] - o.u).max() / 0.08 < tol_u
            else:
                assert all(np.array_equal(x, y) for x, y in zip(ref, got)), (kernel, tbs, np.dtype(dtype).name)


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("turb", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_streaming_kernel_fast_arithmetic_every_instantiation(coll, turb, dtype):
    """Every `arith = fast` instantiation of k_stream (lbm_stream.hpp LBM_STREAM_ALL: C_SRT_FAST / C_TRT_FAST / C_MRT_FAST, each with
    and without the Smagorinsky closure, fp32 and fp64; `turb = 1` SRT is the reference script's default mode, MRT_GPU.py:368-387,
    427-529): 3 and 8 steps per launch on a lattice with two (fp32) / three (fp64) strips, call lengths that leave tail units of every
    length, fields read after every call (the lagged lattice is replayed by the same fast kernel).  The streaming kernel must give the
    SAME BITS as the one-cell-per-thread kernel in fast arithmetic, and both sit within the fast tolerance of the oracle (fp32 2e-5
    on the populations, 2e-4 on u / uLB; fp64 1e-9)."""
    nx, ny = 320, 192
    tol_f, tol_u = (2e-5, 2e-4) if dtype == np.float32 else (1e-9, 1e-9)
    calls = (1, 8, 19, 3, 7, 12, 50)
    o = CavityOracleC(nx, ny, 5000.0, semantics="mrt_gpu", collision=coll, dtype=dtype, turb=turb)
    with CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=turb, kernel="generic", arith="fast") as g, \
            CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=turb, kernel="stream", arith="fast", tuning=dict(tb_steps=8, stream_pairs=True)) as s8, \
            CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=turb, kernel="stream", arith="fast",
                         tuning=dict(tb_steps=3, frame_beside=True, tail_tiles=False, stream_walls=False)) as s3, \
            CavitySolver(nx, ny, 5000.0, RT=coll, dtype=dtype, turb=turb, kernel="stream", arith="fast",
                         tuning=dict(tb_steps=5, stream_walls=True)) as sw:
        for n in calls:
            o.step(n); g.step(n); s8.step(n); s3.step(n); sw.step(n)
            # (the first unit of a freshly initialised lattice is a single step; from then on the streaming plan applies)
            assert s8.next_unit(100) == 8 and s3.next_unit(100) == 3 and sw.next_unit(100) == 5
            assert (s8.describe()["kernel"], sw.describe()["kernel"], s3.describe()["kernel"]) == ("k_stream_pairs", "k_stream_walls", "k_stream")
            ref = g.get_fields(want_fin=True)
            for name, s in (("S=8 pairs", s8), ("S=3 frame", s3), ("S=5 walls", sw)):
                got = s.get_fields(want_fin=True)
                assert all(np.array_equal(x, y) for x, y in zip(ref, got)), (name, coll, turb, np.dtype(dtype).name, o.nsteps)
            assert np.abs(ref[2] - o.fin).max() / np.abs(o.fin).max() < tol_f
            assert np.abs(ref[0] - o.u).max() / 0.08 < tol_u and np.abs(ref[1] - o.rho).max() < tol_u
        if turb:
            assert np.array_equal(g.get_tau(), s8.get_tau()) and np.array_equal(g.get_tau(), s3.get_tau()) and np.array_equal(g.get_tau(), sw.get_tau())


def test_fast_arithmetic_config_c1_centrelines():
    """north_star's tolerance on the fast path: 128 x 128, Re = 100, fp64, 1000 steps (config C1 with the MRT operator):
    centreline velocities within 1e-6 relative of the oracle's; collisions conserve mass as exactly as the strict form."""
    n = 128
    o = CavityOracleC(n, n, 100.0, semantics="mrt_gpu", collision="MRT", dtype=np.float64).step(1000)
    with CavitySolver(n, n, 100.0, RT="MRT", dtype=np.float64, arith="fast") as s:
        s.step(1000)
        u, rho, fin = s.get_fields(want_fin=True)
    for got, ref in ((u[0, n // 2, :], o.u[0, n // 2, :]), (u[1, :, n // 2], o.u[1, :, n // 2])):
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-6
    assert np.abs(fin - o.fin).max() / np.abs(o.fin).max() < 1e-9
    assert abs(fin.sum() - o.fin.sum()) / o.fin.sum() < 1e-12
    with CavityBatch(96, 64, [100.0, 1000.0], RT="MRT", dtype=np.float64, arith="fast") as b:      # in a batch as well
        b.step(40)
        fb = b.get_fields(want_fin=True)[2]
    for i, Re in enumerate((100.0, 1000.0)):
        ob = CavityOracleC(96, 64, Re, semantics="mrt_gpu", collision="MRT", dtype=np.float64).step(40)
        assert np.abs(fb[i] - ob.fin).max() / np.abs(ob.fin).max() < 1e-9


@pytest.mark.parametrize("sem", ["mrt_gpu", "mrt_py"])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_push_scheme_equals_pull_kernels_and_oracle(sem, coll, dtype):
    """kernel='push' is the reference's own two-launch scheme (collide-and-push into a persistent array, then wall
    rules + copy: funRT + funBC); it must give the same bits as the fused pull kernels and the oracle, for odd and even step
    counts, after an upload, and in the lagged u / rho."""
    for nx, ny in ((40, 24), (132, 99), (17, 33)):
        o = CavityOracleC(nx, ny, 400.0, semantics=sem, collision=coll, dtype=dtype)
        with CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype, kernel="push") as p, \
                CavitySolver(nx, ny, 400.0, RT=coll, semantics=sem, dtype=dtype) as q:
            assert np.array_equal(p.get_fields(want_fin=True)[2], o.fin)
            for n in (1, 2, 3, 40):
                o.step(n); p.step(n); q.step(n)
                same_as_oracle(p, o, f"push {sem} {coll} {nx}x{ny} after {o.nsteps}")
                assert all(np.array_equal(a, b) for a, b in zip(p.get_fields(want_fin=True), q.get_fields(want_fin=True)))
            _, _, fin = p.get_fields(want_fin=True)
            p.set_state(fin); o.set_state(fin)
            o.step(7); p.step(7)
            same_as_oracle(p, o, "push after set_state")
    with pytest.raises(RuntimeError, match="PUSH"):
        CavitySolver(64, 64, 100.0, kernel="push", turb=1)
    with pytest.raises(RuntimeError, match="PUSH"):
        CavitySolver(64, 64, 100.0, kernel="push", rows=(0, 32))


@pytest.mark.parametrize("n,dtype,arith,steps", [(1024, np.float32, "fast", 20003), (1024, np.float64, "strict", 10001),
                                                 (160, np.float32, "strict", 40005)])
def test_long_run_multi_step_equals_one_step_kernel(n, dtype, arith, steps):
    """Soak: tens of thousands of steps in irregular call lengths through the multi-step path (tile + fused frame workgroups,
    LDS windows) against ONE call of the one-step-per-launch kernel: the same bits, run to run and path to path.
    (`profiles/r01_logs/soak.log`: the same at 4096^2 and up to 300 000 steps.)"""
    def run(kernel, chunks):
        with CavitySolver(n, n, 1000.0, RT="MRT", dtype=dtype, arith=arith, kernel=kernel) as s:
            for c in chunks:
                s.step(c)
            assert s.steps_done == steps
            return s.get_fields(want_fin=True)
    per = steps // 7
    chunks = [per + (i % 3) for i in range(7)]
    chunks[-1] += steps - sum(chunks)
    a = run("auto", chunks)
    b = run("auto", chunks)
    c = run("vec", [steps])
    assert np.isfinite(a[2]).all()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "run to run"
    assert all(np.array_equal(x, y) for x, y in zip(a, c)), "multi-step path vs one step per launch"


def test_fp32_tracks_fp64():
    with CavitySolver(256, 256, 1000.0, RT="MRT", dtype=np.float64) as d, \
            CavitySolver(256, 256, 1000.0, RT="MRT", dtype=np.float32) as f:
        d.step(500); f.step(500)
        ud, rd = d.get_fields()
        uf, rf = f.get_fields(out_dtype=np.float64)
    assert np.abs(uf - ud).max() / 0.08 < 2e-4
    assert np.abs(rf - rd).max() < 2e-5


@pytest.mark.parametrize("arith", ["strict", "fast"])
def test_full_size_properties_4096_fp32(arith):
    """BASELINE.json configs[2] size (4096^2, fp32, MRT; both arithmetic forms -- `fast` is what bench.py times): properties
    that need no CPU oracle run -- 4 slabs == 1 lattice bit for bit, one-step kernels == default (multi-step) kernel, mass
    drift bounded; the fast form within 2e-5 of the strict one."""
    n, steps = 4096, 13           # raw first step, two multi-step launches, one single step
    with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32, arith=arith) as one:
        one.step(steps)
        u1, r1, f1 = one.get_fields(want_fin=True)
    assert np.isfinite(f1).all()
    mass0 = float(n) * n                                   # rho = 1 everywhere at t = 0
    assert abs(f1.sum(dtype=np.float64) - mass0) / mass0 < 1e-4
    for kern in ("generic", "vec"):
        with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32, kernel=kern, arith=arith) as g:
            g.step(steps)
            ug, rg, fg = g.get_fields(want_fin=True)
        assert np.array_equal(fg, f1) and np.array_equal(ug, u1) and np.array_equal(rg, r1), kern
        del ug, rg, fg
    slabs = [CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32, rows=r, arith=arith) for r in partition_rows(n, 4)]
    LocalSlabs(slabs).step(steps)
    u = np.zeros_like(u1); rho = np.zeros_like(r1); fin = np.zeros_like(f1)
    for s in slabs:
        s.get_fields(u=u, rho=rho, fin=fin)
        s.close()
    assert np.array_equal(fin, f1) and np.array_equal(u, u1) and np.array_equal(rho, r1)
    if arith == "fast":
        with CavitySolver(n, n, 1000.0, RT="MRT", dtype=np.float32) as ref:
            ref.step(steps)
            fs = ref.get_fields(want_fin=True)[2]
        assert not np.array_equal(fs, f1) and np.abs(fs - f1).max() / np.abs(fs).max() < 2e-5


def test_rccl_single_rank_communicator_is_transparent():
    from latticeboltzmannsimulations_amd import comm_unique_id
    with CavitySolver(64, 64, 100.0, RT="MRT", dtype=np.float64) as a, \
            CavitySolver(64, 64, 100.0, RT="MRT", dtype=np.float64) as b:
        b.comm_init(1, 0, comm_unique_id())
        a.step(12); b.step(12)
        assert all(np.array_equal(x, y) for x, y in zip(a.get_fields(want_fin=True), b.get_fields(want_fin=True)))


@pytest.mark.parametrize("deep", [True, False])
@pytest.mark.parametrize("kernel,layout", [("auto", "rows"), ("tb", "rows"), ("tb", "planes"), ("stream", "rows"), ("stream", "planes")])
@pytest.mark.parametrize("dtype,coll,turb,arith", [(np.float32, "MRT", 0, "strict"), (np.float64, "SRT", 1, "strict"),
                                                   (np.float32, "MRT", 0, "fast"), (np.float32, "TRT", 1, "strict")])
def test_rccl_exchange_path_in_loopback(dtype, coll, turb, arith, kernel, layout, deep):
    """lbm_step's in-library exchange (edge/interior split, comm stream, events, ncclSend/ncclRecv straight from
    lattice rows into ghost rows) on ONE GPU: a middle slab exchanges with itself (periodic in y).  Expected
    result: the same slab stepped with the externally driven API and the same wrap done through host buffers.
    kernel='tb': multi-step launches between slabs -- one deep exchange per launch (the default: the frame
    passes recompute a shrinking band of the neighbour's rows) or one one-row exchange per pass (tuning deep_halo=False).
    kernel='stream': units of 8 steps; the rows next to the interfaces are short segments of the streaming kernel that start in
    the deep halo (the edge launch of a unit), the column strips of the wall frame run the slab's whole height.
    u / rho are read after calls that end in a multi-step unit (recomputed from the unit's deep halo) and in a single step."""
    from latticeboltzmannsimulations_amd.slab import LOW, HIGH
    nx, NY, rows = 512, 300, (100, 96)
    a = CavitySolver(nx, NY, 1000.0, RT=coll, dtype=dtype, rows=rows, turb=turb, kernel=kernel, layout=layout, arith=arith,
                     tuning=dict(deep_halo=deep))
    b = CavitySolver(nx, NY, 1000.0, RT=coll, dtype=dtype, rows=rows, turb=turb, kernel="generic", layout=layout, arith=arith)
    a.comm_loopback()
    fin0 = smooth_state(nx, NY, dtype)     # (from the rest state a slab in loopback would stay uniform: a stale row would not show)
    a.set_state(fin0); b.set_state(fin0)
    up = np.empty(b.halo_elems(), dtype=dtype); down = np.empty(b.halo_elems(), dtype=dtype)
    for steps in (23, 8, 1, 10):   # several calls: each starts from the one-row halo the previous one left
        a.step(steps)
        for _ in range(steps):
            b.step_edges(); b.step_interior(); b.step_finish()
            b.halo_export(LOW, up.ctypes.data); b.halo_export(HIGH, down.ctypes.data)
            b.halo_import(HIGH, up.ctypes.data); b.halo_import(LOW, down.ctypes.data)
        fa, fb = a.get_fields(want_fin=True), b.get_fields(want_fin=True)
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb)), steps
    assert np.isfinite(fa[2][:, :, rows[0]:rows[0] + rows[1]]).all()
    a.close(); b.close()


@pytest.mark.parametrize("kernel", ["tb", "stream"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rccl_loopback_with_mrt_py_windows(kernel, dtype):
    """MRT.py's truncated streaming windows between slabs: no deep halo (the left wall reads values parked in ghost columns), so a
    multi-step unit exchanges one row after every frame pass -- with the tile kernel and with the streaming kernel as the bulk
    launch (frame width S + 1).  Expected: the same slab stepped one step at a time with the caller moving the rows."""
    from latticeboltzmannsimulations_amd.slab import LOW, HIGH
    nx, NY, rows = 512, 300, (100, 96)
    a = CavitySolver(nx, NY, 1000.0, RT="SRT", semantics="mrt_py", dtype=dtype, rows=rows, kernel=kernel)
    b = CavitySolver(nx, NY, 1000.0, RT="SRT", semantics="mrt_py", dtype=dtype, rows=rows, kernel="generic")
    a.comm_loopback()
    fin0 = smooth_state(nx, NY, dtype)
    a.set_state(fin0); b.set_state(fin0)
    up = np.empty(b.halo_elems(), dtype=dtype); down = np.empty(b.halo_elems(), dtype=dtype)
    units = set()
    for steps in (19, 8, 1, 10):
        units.add(a.next_unit(steps))
        a.step(steps)
        for _ in range(steps):
            b.step_edges(); b.step_interior(); b.step_finish()
            b.halo_export(LOW, up.ctypes.data); b.halo_export(HIGH, down.ctypes.data)
            b.halo_import(HIGH, up.ctypes.data); b.halo_import(LOW, down.ctypes.data)
        fa, fb = a.get_fields(want_fin=True), b.get_fields(want_fin=True)
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb)), steps
    assert max(units) >= 3, units
    a.close(); b.close()


@pytest.mark.parametrize("nx,rows,dtype", [(4096, 512, np.float32), (4096, 1024, np.float32), (16384, 2048, np.float32), (8192, 1024, np.float64)])
def test_streaming_slab_units_at_benchmark_sizes_in_loopback(nx, rows, dtype):
    """The two-stream schedule of a slab's unit under the streaming kernel at the sizes the scaling runs use, where launches really
    overlap: edge launch + bulk launch + exchange under the bulk launch, with the bulk launch planned on fewer CUs (4096 x 512), in
    one round (4096 x 1024) or released behind the edge launch (16384 x 2048, 8192 x 1024 fp64).  A middle slab in RCCL loopback,
    several calls, 173 steps; expected: the same slab advanced one step per launch with one exchange per step (kernel = vec, same
    loopback), bit for bit -- same arithmetic (fast) in both."""
    a = CavitySolver(nx, 3 * rows, 3200.0, RT="MRT", dtype=dtype, rows=(rows, rows), arith="fast")
    b = CavitySolver(nx, 3 * rows, 3200.0, RT="MRT", dtype=dtype, rows=(rows, rows), arith="fast", kernel="vec")
    a.comm_loopback(); b.comm_loopback()
    fin0 = smooth_state(nx, 3 * rows, dtype)
    a.set_state(fin0); b.set_state(fin0)
    del fin0
    assert a.describe()["kernel"] == "k_stream_walls" and a.describe()["slab"] == 1
    for steps in (1, 64, 27, 81):
        a.step(steps); b.step(steps)
    assert a.next_unit(100) == 8 and b.next_unit(100) == 1
    fa, fb = a.get_fields(want_fin=True), b.get_fields(want_fin=True)
    own = slice(rows, 2 * rows)
    assert np.array_equal(fa[2][:, :, own], fb[2][:, :, own]) and np.array_equal(fa[0][:, :, own], fb[0][:, :, own])
    assert np.array_equal(fa[1][:, own], fb[1][:, own]) and np.isfinite(fa[2][:, :, own]).all()
    a.close(); b.close()


@pytest.mark.parametrize("kernel", ["auto", "tb"])
def test_deep_exchange_after_a_single_step_waits_for_the_interior_kernel(kernel):
    """The exchange of a unit is enqueued on the communication stream ahead of the wait for the previous bulk kernel.  After a
    SINGLE step (the raw first step of a run, a tail) only the slab's first / last row was written on that stream: the S rows of a
    deep exchange must wait for the interior kernel.  The race only showed on the second and later solvers of a process (the
    first is slowed by code loading): same slab four times in one process, short calls that start with single steps; expected:
    every run equals one step and one exchange per launch (kernel = vec)."""
    nx, rows = 4096, 1024
    fin0 = smooth_state(nx, 3 * rows, np.float32)
    def run(k):
        with CavitySolver(nx, 3 * rows, 1000.0, RT="MRT", dtype=np.float32, rows=(rows, rows), arith="fast", kernel=k) as s:
            s.comm_loopback()
            s.set_state(fin0)
            for n in (9, 1, 17, 2, 10):
                s.step(n)
            return s.get_fields(want_fin=True)[2][:, :, rows:2 * rows].copy()
    ref = run("vec")
    for _ in range(4):
        assert np.array_equal(run(kernel), ref)


def test_unit_api_messages_quote_the_accepted_ranges():
    """lbm_halo_export_rows / lbm_step_unit: what the error text says is what the call accepts."""
    import ctypes
    from latticeboltzmannsimulations_amd import _lib
    L = _lib.lib()
    with CavitySolver(320, 600, 100.0, rows=(200, 200), dtype=np.float32, kernel="stream", tuning=dict(tb_steps=8)) as s:
        n9 = L.lbm_halo_rows_elems(s._h, 9)
        assert n9 > 0 and L.lbm_halo_rows_elems(s._h, 10) == 0
        buf = np.zeros(n9, dtype=np.float32)
        s.halo_export_rows(_lib.LBM_SIDE_LOW, 9, buf.ctypes.data)                       # the largest accepted
        with pytest.raises(RuntimeError, match=r"1 <= nrows <= 9"):
            s.halo_export_rows(_lib.LBM_SIDE_LOW, 10, buf.ctypes.data)
        s.step_edges(); s.step_interior(); s.step_finish()                              # (the first step after init is a single step)
        with pytest.raises(RuntimeError, match=r"3 \.\. 8"):
            s.step_unit(9)
        with pytest.raises(RuntimeError, match=r"3 \.\. 8"):
            s.step_unit(2)
    with pytest.raises(RuntimeError, match=r"2 \.\. 10"):
        CavitySolver(320, 200, 100.0, tuning=dict(tb_steps=12))
    with pytest.raises(RuntimeError, match=r"6 \.\. 10 need kernel = STREAM"):
        CavitySolver(320, 200, 100.0, kernel="tb", tuning=dict(tb_steps=6))
    with pytest.raises(RuntimeError, match=r"9 \.\. 10 need the streaming kernel with two rows per wave"):
        CavitySolver(320, 400, 100.0, kernel="stream", rows=(0, 200), tuning=dict(tb_steps=9, stream_pairs=True))        # (a slab: 8 at most)
    with CavitySolver(320, 200, 100.0, kernel="stream", tuning=dict(tb_steps=10, stream_pairs=True)) as s:
        assert s.describe()["kernel"] == "k_stream_pairs" and s.describe()["steps_per_launch"] == 10


def test_slab_without_a_communicator_is_refused():
    """lbm_step / lbm_time_steps on a slab with no transport attached would read ghost rows nobody fills: LBM_ERR_STATE."""
    with CavitySolver(256, 128, 100.0, rows=(0, 64)) as s:
        with pytest.raises(RuntimeError, match="without a communicator"):
            s.step(3)
        with pytest.raises(RuntimeError, match="without a communicator"):
            s.time_steps(3)
        s.step_edges(); s.step_interior(); s.step_finish()      # the externally driven calls are what such a slab takes
        assert s.steps_done == 1


SLAB_CASES = [(np.float32, "MRT", 0, "strict"), (np.float32, "MRT", 0, "fast"), (np.float64, "SRT", 1, "strict"),
              (np.float64, "MRT", 0, "strict"), (np.float64, "MRT", 0, "fast")]


@pytest.mark.parametrize("kernel", ["tb", "stream", "stream_frame"])
@pytest.mark.parametrize("nslabs", [2, 3, 8])
@pytest.mark.parametrize("dtype,coll,turb,arith", SLAB_CASES)
def test_slabs_through_multi_step_units_equal_single_lattice(dtype, coll, turb, arith, nslabs, kernel):
    """What every rank of a decomposition runs between its RCCL calls -- first slab (lid, one neighbour below), middle slabs,
    last slab (bottom wall): launch units of S steps, each preceded by the exchange of the S complete rows next to every
    interface (lbm_halo_export_rows -> lbm_halo_import_rows) and run by lbm_step_unit = lbm_step's own multi-step launch
    sequence (frame passes that recompute a shrinking band of the neighbour's rows + tile kernel, two streams; kernel = stream:
    edge launch + bulk launch -- "stream": the walls inside, k_stream_walls_slab, the edge launch is the interface bands alone (the
    library's choice where the operator variant does not spill; forced here); "stream_frame": k_stream, edge launch = column strips +
    the interface rows as segments of the streaming kernel).  Uneven slab
    heights, several calls whose lengths leave every remainder, fields read after every call (one-step lag recomputed from
    the deep halo on slabs).  Expected: the undivided lattice, bit for bit (and the C oracle for strict arithmetic)."""
    nx, ny = 512, 75 * 8 + 5
    calls = (1, 13, 5, 9, 4, 16, 3)
    parts = partition_rows(ny, nslabs)
    mr = min(n for _, n in parts)
    o = CavityOracleC(nx, ny, 1000.0, semantics="mrt_gpu", collision=coll, dtype=dtype, turb=turb) if arith == "strict" else None
    one = CavitySolver(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, arith=arith, kernel="vec")
    tuning = {} if kernel == "tb" else dict(stream_walls=kernel == "stream")
    slabs = [CavitySolver(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, arith=arith, kernel=kernel.split("_")[0], rows=r, min_rows=mr, tuning=tuning)
             for r in parts]
    if kernel != "tb":
        assert {sl.describe()["kernel"] for sl in slabs} == {"k_stream_walls" if kernel == "stream" else "k_stream"}
    assert slabs[0].next_unit(1) == 1                                       # raw lattice: a single step first
    drv = LocalSlabs(slabs)
    units = set()
    for n in calls:
        units.add(slabs[-1].next_unit(n))
        drv.step(n); one.step(n)
        ref = one.get_fields(want_fin=True)
        u = np.zeros_like(ref[0]); rho = np.zeros_like(ref[1]); fin = np.zeros_like(ref[2])
        for sl in slabs:
            sl.get_fields(u=u, rho=rho, fin=fin)
        assert np.array_equal(fin, ref[2]) and np.array_equal(u, ref[0]) and np.array_equal(rho, ref[1]), n
        if o is not None:
            o.step(n)
            assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho), n
    assert max(units) >= (8 if kernel != "tb" else 3), units                # the multi-step path really ran
    means = [sl.mean_u() * sl.ny_local for sl in slabs]
    assert abs(sum(means) / ny - one.mean_u()) < 1e-12
    for sl in slabs:
        sl.close()
    one.close()


def test_slabs_derive_one_plan_from_the_smallest_slab():
    """Two neighbours on opposite sides of a size threshold (768 x 1535 rows cut in two: 768 and 767 rows) must still run the
    same protocol: with min_rows = the smallest slab both report the same launch units; without it they may not, and the
    driver refuses to continue instead of posting mismatched exchanges."""
    nx, ny = 768, 1535
    parts = partition_rows(ny, 2)
    mr = min(n for _, n in parts)
    good = [CavitySolver(nx, ny, 1000.0, dtype=np.float32, rows=r, min_rows=mr) for r in parts]
    for left in (1, 5, 9, 40):
        assert good[0].next_unit(left) == good[1].next_unit(left)
    LocalSlabs(good).step(12)
    with CavitySolver(nx, ny, 1000.0, dtype=np.float32, kernel="vec") as one:
        one.step(12)
        ref = one.get_fields(want_fin=True)
    u = np.zeros_like(ref[0]); rho = np.zeros_like(ref[1]); fin = np.zeros_like(ref[2])
    for sl in good:
        sl.get_fields(u=u, rho=rho, fin=fin)
        sl.close()
    assert np.array_equal(fin, ref[2]) and np.array_equal(u, ref[0]) and np.array_equal(rho, ref[1])
    with pytest.raises(RuntimeError, match="ny_local_min"):
        CavitySolver(nx, ny, 1000.0, dtype=np.float32, rows=parts[1], min_rows=parts[1][1] + 1)


def test_timing_and_bandwidth_probes():
    with CavitySolver(1024, 1024, 1000.0, RT="MRT", dtype=np.float32) as s:
        s.step(5); s.sync()
        ms = s.time_steps(20)
        assert 0 < ms < 1000
        assert s.copy_bandwidth(1 << 28, 5) > 500.0     # GB/s, any healthy MI355X
        assert 20.0 < s.fma_rate(5.0) < 200.0           # TFLOP/s of packed fp32 FMAs (vector peak 157)


def test_front_end_drop_in(tmp_path, monkeypatch):
    """run_cavity with the reference's knobs: outputs at It = 0, P, 2P; VTK files; u / rho shapes."""
    from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=2001, Re=100.0, RT="MRT", turb=0, xsize=64, ysize=64, Pinterval=1000,
                   SavePlot=False, SaveVTK=True, quiet=True)
    assert r.iterations == 2001 and [it for it, _ in r.regression] == [0, 1000, 2000]
    assert r.u.shape == (2, 64, 64) and r.rho.shape == (64, 64) and r.u.dtype == np.float32
    for i in range(3):
        assert os.path.exists(tmp_path / "output" / f"ldc.{i:05d}.vtr")
    assert r.regression[-1][1] > r.regression[0][1]
    o = CavityOracleC(64, 64, 100.0, semantics="mrt_gpu", collision="MRT", dtype=np.float32).step(2001)
    assert np.array_equal(r.u, o.u) and np.array_equal(r.rho, o.rho)
    # the reference's default mode: SRT + Smagorinsky at Re = 10000 (MRT_GPU.py:47-49)
    r = run_cavity(maxIt=301, Pinterval=100, xsize=96, ysize=96, SavePlot=True, SaveVTK=False, quiet=True)
    o = CavityOracleC(96, 96, 10000.0, semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1).step(301)
    assert np.array_equal(r.u, o.u) and np.array_equal(r.rho, o.rho)
    assert os.path.exists(tmp_path / "output" / "ldc_00003.png")
