"""CPU tests of the half-way bounce-back walls (semantics='bounce_back'): the NumPy reference the GPU tests check against
(tests/bounce_back_ref.py), the launch plans and refusals of lbm_plan, and the front end (run_cavity's BC, datagen's BC, ghia's walls)."""

import numpy as np
import pytest


from bounce_back_ref import BOUNCE, BounceBackOracle
from front_end_standin import standin
from oracle import lbm_numpy as on
from latticeboltzmannsimulations_amd import datagen, ghia, launch_plan, mrt_gpu
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd.solver import _SEM


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_bounce_is_the_opposite_direction():
    for k in range(9):
        assert on.CX[BOUNCE[k]] == -on.CX[k] and on.CY[BOUNCE[k]] == -on.CY[k]


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_reference_conserves_mass(coll):
    """fp64, 2000 steps on a non-square lattice: the total mass is X * Y to 1e-12 relative (the lid terms of a cell cancel)."""
    o = BounceBackOracle(64, 48, 100.0, collision=coll)
    m0 = o.mass()
    assert m0 == pytest.approx(64 * 48, rel=1e-14)
    o.step(2000)
    drift = abs(o.mass() - m0) / m0
    assert drift < 1e-12, drift
    assert np.abs(o.u[0]).max() > 0.05          # (the lid drives a flow)


def test_wet_node_walls_drift_far_more():
    """The same run under the wet-node walls of semantics='mrt_gpu' gains mass (1.6e-4 relative), the bounce-back one does not."""
    n = on.CavityOracle(64, 48, 100.0, semantics="mrt_gpu", collision="MRT")
    m0 = float(n.fin.sum())
    n.step(2000)
    nebb = abs(float(n.fin.sum()) - m0) / m0
    b = BounceBackOracle(64, 48, 100.0, collision="MRT")
    b0 = b.mass()
    b.step(2000)
    bb = abs(b.mass() - b0) / b0
    assert 1e-4 < nebb < 3e-4, nebb
    assert nebb > 100 * bb, (nebb, bb)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_resting_lattice_stays_at_rest(coll, dtype):
    """uLB = 0 from f = w_k: the walls inject nothing -- the state stays uniform bit for bit and u exactly 0.  It stays at w_k bit
    for bit where the equilibrium of the rest state is w_k itself: in fp32 sum_k w_k rounds to 1 (SRT and TRT reproduce w_k; the
    MRT back transform rounds once more), in fp64 to 1 + 2^-52, and the first step moves f by that rounding, walls or not."""
    o = BounceBackOracle(20, 14, 100.0, collision=coll, dtype=dtype)
    o.uLB = 0.0
    w = np.broadcast_to(on.weights(dtype)[:, None, None], o.fin.shape).copy()
    o.set_state(w)
    o.step(200)
    for k in range(9):
        assert np.all(o.fin[k] == o.fin[k, 0, 0]), k
    assert not np.any(o.u)
    if dtype == np.float32 and coll != "MRT":
        assert np.array_equal(o.fin, w)
    else:
        assert np.abs(o.fin - w).max() <= 4 * np.finfo(dtype).eps


def test_lid_terms_of_every_lid_cell_cancel():
    """One step from the initial state: beyond the lid, slot 8 gains t and slot 7 loses it, corners included; slot 4 is the plain bounce."""
    o = BounceBackOracle(12, 10, 100.0, collision="SRT")
    rho, ux, uy = o.macros(o.fin)
    fpost = o.collide(o.fin, rho, on.equ(rho, ux, uy, o.t))
    fin = o.stream_bb(fpost, rho)
    t = (rho[:, 0] * 0.08) * (1.0 / 6.0)
    assert np.array_equal(fin[8, :, 0], fpost[6, :, 0] + t)
    assert np.array_equal(fin[7, :, 0], fpost[5, :, 0] - t)
    assert np.array_equal(fin[4, :, 0], fpost[2, :, 0])
    assert np.array_equal(fin[1, 0, :], fpost[3, 0, :]) and np.array_equal(fin[3, -1, :], fpost[1, -1, :])
    assert np.array_equal(fin[2, :, -1], fpost[4, :, -1])
    assert np.array_equal(fin[1, 1:, 3], fpost[1, :-1, 3])          # (the interior streams as before)


# ---- the library's plan and its refusals ------------------------------------------------------------------------------------
def test_abi_constant():
    assert L.LBM_SEM_BOUNCE_BACK == 2 and _SEM["bounce_back"] == 2
    assert L.ABI_VERSION == 4


def test_bounce_back_plans():
    d = launch_plan(160, 160, 100.0, semantics="bounce_back", steps=20)
    assert d["kernel"] == "k_stepS_deep" and d["frame"] > 0 and d["semantics"] == "bounce_back" and sum(d["units"]) == 20
    d = launch_plan(4096, 4096, 1000.0, semantics="bounce_back", steps=20)
    assert d["kernel"] == "k_stream" and d["frame"] == 8 and d["semantics"] == "bounce_back"
    d = launch_plan(4096, 4096, 1000.0, semantics="bounce_back", arith="fast", dtype=np.float64)
    assert d["kernel"] == "k_stream" and d["frame"] == 8
    d = launch_plan(384, 384, 1000.0, semantics="bounce_back", batch=64)
    assert d["kernel"] == "k_stepS_deep" and d["frame"] > 0
    d = launch_plan(256, 256, 100.0, semantics="bounce_back", kernel="generic", steps=5)
    assert d["kernel"] == "none" and d["units"] == [1] * 5
    d = launch_plan(320, 600, 100.0, semantics="bounce_back", rows=(200, 200), kernel="stream")
    assert d["kernel"] == "k_stream" and d["deep_halo"] == 0 and d["slab"] == 1
    # the wet-node plans do not carry the field (their text is unchanged)
    assert "semantics" not in launch_plan(160, 160, 100.0) and "semantics" not in launch_plan(160, 160, 100.0, semantics="mrt_py")


@pytest.mark.parametrize("kw, text", [(dict(arith="promoted"), "promoted"), (dict(kernel="push"), "PUSH"), (dict(kernel="vec"), "VEC"),
                                      (dict(tuning={"stream_walls": True}), "STREAM_WALLS"), (dict(tuning={"stream_pairs": True}), "STREAM_PAIRS"),
                                      (dict(turb=1), "turb")])
def test_bounce_back_refusals(kw, text):
    with pytest.raises(RuntimeError, match=text):
        launch_plan(4096, 4096, 1000.0, semantics="bounce_back", **kw)


def test_stream_walls_off_is_accepted():
    assert launch_plan(4096, 4096, 1000.0, semantics="bounce_back", tuning={"stream_walls": False})["kernel"] == "k_stream"


# ---- front end --------------------------------------------------------------------------------------------------------------
_StandIn = standin(source="bounce_back")


def test_run_cavity_passes_bounce_back_through(tmp_path):
    _StandIn.made.clear()
    r = mrt_gpu.run_cavity(maxIt=30, Re=100.0, RT="MRT", turb=0, xsize=24, ysize=20, Pinterval=10, SavePlot=False, quiet=True,
                           OutputFolder=str(tmp_path), solver_factory=_StandIn, BC="BB")
    assert _StandIn.made[-1]["semantics"] == "bounce_back"
    assert r is not None
    mrt_gpu.run_cavity(maxIt=10, Re=100.0, RT="MRT", turb=0, xsize=24, ysize=20, Pinterval=10, SavePlot=False, quiet=True,
                       OutputFolder=str(tmp_path), solver_factory=_StandIn)
    assert _StandIn.made[-1]["semantics"] == "mrt_gpu"          # (default unchanged)
    with pytest.raises(ValueError, match="turb=0"):
        mrt_gpu.run_cavity(maxIt=10, turb=1, xsize=24, ysize=20, SavePlot=False, quiet=True, solver_factory=_StandIn, BC="BB")
    with pytest.raises(ValueError, match="BC"):
        mrt_gpu.run_cavity(maxIt=10, turb=0, xsize=24, ysize=20, SavePlot=False, quiet=True, solver_factory=_StandIn, BC="XX")


def test_cli_and_datagen_take_bc():
    import inspect
    assert inspect.signature(datagen.generate).parameters["BC"].default == "EB-NEBB "
    assert inspect.signature(mrt_gpu.run_cavity).parameters["BC"].default == "EB-NEBB "
    with pytest.raises(ValueError, match="turb=0"):
        datagen.generate([100.0], xsize=32, ysize=32, BC="BB", turb=1, save=False, quiet=True)
    with pytest.raises(ValueError, match="BC"):
        datagen.generate([100.0], xsize=32, ysize=32, BC="NEBB", save=False, quiet=True)


def test_profile_errors_halfway_reproduces_a_linear_profile():
    """A Couette-like field u_x = height, u_y = 0 with the cells at the half-way positions: the interpolated centrelines are the
    linear profile itself, so the errors are those of the linear profile against Ghia's table, to rounding."""
    X, Y, uLB = 40, 30, 0.1
    h = 1.0 - (np.arange(Y) + 0.5) / Y
    u = np.zeros((2, X, Y))
    u[0] = uLB * h[None, :]
    Yg, Uxg, Xg, Uyg = ghia.ghia_profiles(100.0)
    ex, ey = ghia.profile_errors(u, 100.0, uLB, walls="halfway")
    assert ex == pytest.approx(np.max(np.abs(Yg - Uxg)), abs=1e-12)
    assert ey == pytest.approx(np.max(np.abs(Uyg)), abs=1e-12)
    # the node convention reads the same cells at other heights
    assert abs(ghia.profile_errors(u, 100.0, uLB)[0] - ex) > 1e-3
    assert ghia.profile_errors(u, 100.0, uLB) == ghia.profile_errors(u, 100.0, uLB, walls="nodes")
    with pytest.raises(ValueError):
        ghia.profile_errors(u, 100.0, uLB, walls="wet")


def test_primary_vortex_error_halfway_position():
    X, Y = 41, 31
    u = np.ones((2, X, Y))
    i, j = 20, 12
    u[:, i, j] = 0.0
    dx, dy = ghia.primary_vortex_error(u, 100.0, 0.1, walls="halfway")
    dxn, dyn = ghia.primary_vortex_error(u, 100.0, 0.1)
    px, py = (i + 0.5) / X, 1.0 - (j + 0.5) / Y
    assert dx - dxn == pytest.approx(px - i / X) and dy - dyn == pytest.approx(py - (Y - 1 - j) / Y)
