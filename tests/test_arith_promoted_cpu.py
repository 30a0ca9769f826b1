"""arith='promoted' without a GPU: the C ABI constant and version, the dry-run launch plans (lbm_plan) and the front ends' plumbing."""
import os
import re

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import datagen, mrt_gpu
from latticeboltzmannsimulations_amd.solver import launch_plan
from front_end_standin import standin

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lbm.h")


def test_header_constant_and_abi_version():
    text = open(HEADER).read()
    assert re.search(r"LBM_ARITH_PROMOTED\s*=\s*2\b", text)
    assert int(re.search(r"#define LBM_ABI_VERSION (\d+)", text).group(1)) == 4
    assert L.LBM_ARITH_PROMOTED == 2 and L.ABI_VERSION == 4
    assert L.lib().lbm_abi_version() == 4


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("RT", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("turb", [0, 1])
def test_launch_plan_promoted(dtype, RT, turb):
    for kw in (dict(xsize=384, ysize=384), dict(xsize=4096, ysize=4096), dict(xsize=96, ysize=80, batch=3),
               dict(xsize=2048, ysize=2048, rows=(512, 1024), min_rows=1024)):
        p = launch_plan(Re=1000.0, steps=30, RT=RT, turb=turb, dtype=dtype, arith="promoted", **kw)
        assert p["kernel"] and sum(p["units"]) == 30, kw
        if dtype == np.float64:      # the promotion's casts are no-ops in fp64: the strict variants and plan
            assert p == launch_plan(Re=1000.0, steps=30, RT=RT, turb=turb, dtype=dtype, arith="strict", **kw), kw


def test_promoted_routes():
    """The AUTO routes DESIGN documents for the promoted fp32 operators: the walls inside the streaming kernel for the C3 lattice
    (4096^2 MRT), the tile kernel with five steps per launch for the datagen lattice (384^2 SRT + closure)."""
    c3 = launch_plan(4096, 4096, 1000.0, steps=20, RT="MRT", arith="promoted")
    assert c3["kernel"] == "k_stream_walls" and c3["steps_per_launch"] == 8 and c3["units"] == [1, 8, 8, 3]
    dg = launch_plan(384, 384, 1000.0, steps=20, RT="SRT", turb=1, arith="promoted")
    assert dg["kernel"] == "k_stepS_deep" and dg["steps_per_launch"] == 5
    forced = launch_plan(4096, 4096, 1000.0, RT="TRT", turb=1, arith="promoted", kernel="stream", tuning=dict(stream_walls=True))
    assert forced["kernel"] == "k_stream_walls"


def test_promoted_rejections():
    with pytest.raises(RuntimeError, match="MRT_GPU semantics"):
        launch_plan(128, 128, 100.0, semantics="mrt_py", arith="promoted")
    with pytest.raises(RuntimeError, match="two rows per wave"):
        launch_plan(4096, 4096, 1000.0, arith="promoted", kernel="stream", tuning=dict(stream_pairs=True))
    with pytest.raises(ValueError, match="arith"):
        launch_plan(128, 128, 100.0, arith="promote")


PromotedOracleStepper = standin()        # `made` records the arith it was given


def test_run_cavity_passes_promoted(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    PromotedOracleStepper.made.clear()
    r = mrt_gpu.run_cavity(maxIt=21, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=10, SavePlot=False, SaveVTK=False,
                           solver_factory=PromotedOracleStepper, arith="promoted", quiet=True)
    assert [kw["arith"] for kw in PromotedOracleStepper.made] == ["promoted"] and r.iterations == 21


def test_command_lines_accept_promoted(monkeypatch):
    got = {}
    monkeypatch.setattr(mrt_gpu, "run_cavity", lambda **kw: got.setdefault("mrt_gpu", kw) and type("R", (), {"mlups": 0.0})())
    monkeypatch.setattr(datagen, "generate", lambda *a, **kw: got.setdefault("datagen", kw))
    assert mrt_gpu.main(["--arith", "promoted", "--maxIt", "1"]) == 0
    assert datagen.main(["--arith", "promoted"]) == 0
    assert got["mrt_gpu"]["arith"] == "promoted" and got["datagen"]["arith"] == "promoted"
    with pytest.raises(SystemExit):
        mrt_gpu.main(["--arith", "double"])
