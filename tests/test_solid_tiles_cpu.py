"""CPU tests of solid obstacles on the multi-step tile kernel (LBM_FLAG_SOLID_TILES, tuning=dict(solid_tiles=True)): the
flag bit, the dry-run plan -- the units, steps per launch and frame of plain bounce-back with kernel='tb' for the same lattice, ten
planes instead of nine --, the plans without the flag as tests/test_solid_cpu.py pins them, every refused combination with its reason,
and the front ends' argument check and command lines through the stand-ins of tests/front_end_standin.py."""

import numpy as np
import pytest


import front_end_standin as FS
from solid_ref import SolidOracle
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import datagen, launch_plan, mrt_gpu
from latticeboltzmannsimulations_amd.solver import _tuning

TILES = dict(solid_tiles=True)
SOLID = dict(semantics="bounce_back", solid=True)
NX, NY = 48, 40


def test_the_flag_is_a_tuning_switch_and_a_new_bit():
    assert L.LBM_FLAG_SOLID_TILES == 524288
    assert _tuning(dict(solid_tiles=True)) == (0, 0, L.LBM_FLAG_SOLID_TILES)
    assert _tuning(dict(solid_tiles=False)) == (0, 0, 0)
    assert _tuning(dict(solid_tiles=True, tb_steps=4, frame_lds=False)) == (4, 0, L.LBM_FLAG_SOLID_TILES | L.LBM_FLAG_NO_FRAME_LDS)
    text = open(L.HEADER).read()
    assert "LBM_FLAG_SOLID_TILES = 524288" in text and "#define LBM_ABI_VERSION 4" in text and L.ABI_VERSION == 4


# (size, keywords): the sizes of the issue -- the flagship lattice, the GPU tests' smallest fp32 shape, the sweep's batch -- and the GPU
# tests' fp64 and F = 8 shapes
PLANS = [((4096, 4096), {}), ((128, 72), {}), ((384, 384), dict(batch=64, arith="fast")), ((72, 72), dict(dtype=np.float64)),
         ((136, 80), dict(tuning=dict(tb_steps=4))), ((4096, 4096), dict(dtype=np.float64, RT="TRT")), ((1024, 1024), dict(arith="fast", RT="SRT"))]


@pytest.mark.parametrize("size,kw", PLANS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
@pytest.mark.parametrize("steps", [1, 6, 23, 100])
def test_plan_is_the_plain_bounce_back_tile_plan_with_ten_planes(size, kw, steps):
    kw = dict(kw)
    tune = kw.pop("tuning", {})
    got = launch_plan(*size, 1000.0, steps=steps, tuning=dict(tune, **TILES), **SOLID, **kw)
    want = launch_plan(*size, 1000.0, steps=steps, semantics="bounce_back", kernel="tb", tuning=tune, **kw)
    for key in ("units", "steps_per_launch", "frame", "frame_seg", "workgroups", "frame_fused", "kernel"):
        assert got[key] == want[key], key
    assert got["kernel"] == "k_stepS_deep" and got["steps_per_launch"] in (3, 4, 5) and sum(got["units"]) == steps
    assert got["semantics"] == "bounce_back_solid" and want["semantics"] == "bounce_back"
    assert got["lattice_bytes"] * 9 == want["lattice_bytes"] * 10
    assert got["units"][0] == 1                                           # the first step after an upload: k_step_solid
    # kernel='tb' with the flag is the same plan
    assert launch_plan(*size, 1000.0, steps=steps, kernel="tb", tuning=dict(tune, **TILES), **SOLID, **kw) == got


@pytest.mark.parametrize("tb", [3, 4, 5])
def test_tb_steps_and_the_frame_switches_follow_plain_bounce_back(tb):
    for size, dt in (((128, 72), np.float32), ((72, 72), np.float64), ((136, 80), np.float32)):
        for extra in ({}, dict(frame_lds=False), dict(frame_fused=False), dict(eager_lag=True)):
            tune = dict(tb_steps=tb, **extra)
            got = launch_plan(*size, 100.0, steps=37, dtype=dt, tuning=dict(tune, **TILES), **SOLID)
            want = launch_plan(*size, 100.0, steps=37, dtype=dt, semantics="bounce_back", kernel="tb", tuning=tune)
            assert (got["units"], got["steps_per_launch"], got["frame"], got["frame_seg"], got["frame_fused"], got["lazy_lag"]) == \
                (want["units"], want["steps_per_launch"], want["frame"], want["frame_seg"], want["frame_fused"], want["lazy_lag"])
            assert got["steps_per_launch"] == tb and got["frame"] == (4 if tb == 3 else 8)


def test_without_the_flag_nothing_changes():
    """The plans tests/test_solid_cpu.py pins, with the tuning key absent and with it False."""
    for tune in (None, dict(solid_tiles=False)):
        p = launch_plan(4096, 4096, 1000.0, steps=6, tuning=tune, **SOLID)
        assert p["kernel"] == "k_step_solid" and p["steps_per_launch"] == 1 and p["units"] == [1] * 6 and p["frame"] == 0
        assert launch_plan(384, 384, 100.0, batch=64, arith="fast", steps=3, tuning=tune, **SOLID)["units"] == [1, 1, 1]
        assert launch_plan(70, 66, 100.0, tuning=tune, **SOLID)["kernel"] == "k_step_generic"
        for kernel in ("tb", "stream", "vec", "push"):
            with pytest.raises(RuntimeError, match="one step per launch"):
                launch_plan(128, 128, 100.0, kernel=kernel, tuning=tune, **SOLID)
    plain = launch_plan(4096, 4096, 1000.0, steps=6, semantics="bounce_back")
    assert "semantics=bounce_back_solid" not in str(plain) and plain["semantics"] == "bounce_back"


@pytest.mark.parametrize("kw,text", [
    (dict(kernel="stream"), "kernel = AUTO or TB"),
    (dict(kernel="vec"), "kernel = AUTO or TB"),
    (dict(kernel="push"), "kernel = AUTO or TB"),
    (dict(kernel="generic"), "kernel = AUTO or TB"),
    (dict(rows=(0, 64)), "no slabs"),
    (dict(rows=(64, 64)), "no slabs"),
    (dict(turb=1), "turb = 1"),
    (dict(arith="promoted"), "promoted"),
    (dict(tuning=dict(stream_walls=True)), "STREAM_WALLS"),
    (dict(tuning=dict(stream_pairs=True)), "STREAM_WALLS"),
    (dict(tuning=dict(tb_steps=2)), "3 .. 5"),
    (dict(tuning=dict(tb_steps=6)), "tb_steps 6"),
])
def test_plan_refuses_with_a_reason(kw, text):
    kw = dict(kw)
    tune = dict(kw.pop("tuning", {}), **TILES)
    with pytest.raises(RuntimeError, match=text):
        launch_plan(128, 128, 100.0, tuning=tune, **SOLID, **kw)


def test_plan_refuses_the_flag_without_a_mask_and_the_sizes_the_tile_kernel_refuses():
    for sem in ("bounce_back", "mrt_gpu", "mrt_py"):
        with pytest.raises(RuntimeError, match="needs a solid mask"):
            launch_plan(128, 128, 100.0, semantics=sem, tuning=TILES)
    # every size plain bounce-back refuses kernel='tb' for is refused here, and so is nx % V != 0
    for size, dt in (((28, 64), np.float32), ((64, 28), np.float32), ((30, 30), np.float64), ((70, 66), np.float32), ((67, 66), np.float64)):
        with pytest.raises(RuntimeError, match="kernel = TB needs"):
            launch_plan(*size, 100.0, dtype=dt, semantics="bounce_back", kernel="tb")
        with pytest.raises(RuntimeError, match="LBM_FLAG_SOLID_TILES needs what kernel = TB needs"):
            launch_plan(*size, 100.0, dtype=dt, tuning=TILES, **SOLID)
    assert launch_plan(70, 66, 100.0, dtype=np.float64, tuning=TILES, **SOLID)["kernel"] == "k_stepS_deep"        # 70 % 2 == 0
    assert launch_plan(32, 32, 100.0, tuning=TILES, **SOLID)["steps_per_launch"] == 3


# ---- the front ends, through the stand-ins ------------------------------------------------------------------------------------------
def _mask():
    m = np.zeros((NX, NY), dtype=bool)
    m[20:28, 14:20] = True
    return m


def _standin():
    """A stand-in with CavitySolver's solid=... and tuning=..., stepping the reference of tests/solid_ref.py."""
    class S(FS.standin()):
        source = "solid"
        tunings = []

        def __init__(self, xsize, ysize, Re, solid=None, tuning=None, **kw):
            type(self).tunings.append(tuning)
            FS.SOURCES["solid"] = lambda X, Y, R, k: SolidOracle(X, Y, R, mask=solid, uLB=k["uLB"], collision=k["RT"], dtype=np.float64)
            super().__init__(xsize, ysize, Re, **kw)

        def solid_force(self):
            F = self.o.force()
            return dict(step=self.steps_done, links=F["links"], fx=F["fx"], fy=F["fy"])
    return S


def test_run_cavity_passes_the_switch_and_refuses_it_without_a_mask():
    S = _standin()
    kw = dict(maxIt=11, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=5, SavePlot=False, BC="BB", quiet=True, solver_factory=S)
    r = mrt_gpu.run_cavity(solid=_mask(), solid_tiles=True, **kw)
    assert S.tunings == [dict(solid_tiles=True)] and [it for it, _ in r.forces] == [0, 5, 10]
    mrt_gpu.run_cavity(solid=_mask(), **kw)
    assert S.tunings[-1] is None                                         # without the switch the solver is made as before
    made = len(S.made)
    with pytest.raises(ValueError, match="solid_tiles.*needs solid"):
        mrt_gpu.run_cavity(solid_tiles=True, **kw)
    with pytest.raises(ValueError, match="solid_tiles.*needs solid"):
        mrt_gpu.run_cavity(solid_tiles=True, **dict(kw, BC="EB-NEBB "))
    with pytest.raises(ValueError, match="BC='BB'"):
        mrt_gpu.run_cavity(solid=_mask(), solid_tiles=True, **dict(kw, BC="EB-NEBB "))
    assert len(S.made) == made


def test_sweep_passes_the_switch_and_refuses_it_without_a_mask():
    seen = []

    class B(FS.BatchStandIn):
        def __init__(self, xsize, ysize, Re_list, solid=None, tuning=None, **kw):
            seen.append(tuning)
            lone = _standin()
            self.lattices = [lone(xsize, ysize, float(Re), solid=solid[i], **kw) for i, Re in enumerate(Re_list)]
            self.journal = []
    kw = dict(xsize=NX, ysize=NY, RT="MRT", turb=0, maxIt=7, Pinterval=5, BC="BB", save=False, quiet=True, batch_factory=B)
    out = datagen.generate([100.0, 200.0], solid=_mask(), solid_tiles=True, **kw)
    assert seen == [dict(solid_tiles=True)] and not out[2][0][:, _mask()].any()
    datagen.generate([100.0], solid=_mask(), **kw)
    assert seen[-1] is None
    with pytest.raises(ValueError, match="solid_tiles.*needs solid"):
        datagen.generate([100.0], solid_tiles=True, **kw)
    assert len(seen) == 2


def test_command_lines_parse_the_switch(monkeypatch, capsys):
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return mrt_gpu.CavityResult()
    monkeypatch.setattr(mrt_gpu, "run_cavity", fake)
    size = ["--xsize", str(NX), "--ysize", str(NY), "--turb", "0", "--BC", "BB"]
    box = ["--solid-box", "20", "28", "14", "20"]
    assert mrt_gpu.main(size + box + ["--solid-tiles"]) == 0
    assert seen["solid_tiles"] is True and np.array_equal(seen["solid"], _mask())
    seen.clear()
    assert mrt_gpu.main(size + box) == 0 and "solid_tiles" not in seen and np.array_equal(seen["solid"], _mask())
    seen.clear()
    with pytest.raises(SystemExit) as e:
        mrt_gpu.main(size + ["--solid-tiles"])
    assert e.value.code == 2 and "needs solid" in capsys.readouterr().err and not seen

    got = {}
    monkeypatch.setattr(datagen, "generate", lambda *a, **kw: got.update(kw))
    assert datagen.main(["--size", str(NX), "--BC", "BB", "--solid-box", "1", "3", "2", "4", "--solid-tiles"]) == 0
    assert got["solid_tiles"] is True and got["solid"].sum() == 4 and got["turb"] == 0
    got.clear()
    assert datagen.main(["--size", str(NX), "--BC", "BB", "--solid-box", "1", "3", "2", "4"]) == 0 and "solid_tiles" not in got
    got.clear()
    with pytest.raises(SystemExit) as e:
        datagen.main(["--size", str(NX), "--BC", "BB", "--solid-tiles"])
    assert e.value.code == 2 and "needs solid" in capsys.readouterr().err and not got
