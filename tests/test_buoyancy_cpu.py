"""CPU tests of Boussinesq buoyancy (lbm_set_buoyancy, CavitySolver.set_buoyancy, latticeboltzmannsimulations_amd.convection): the ABI
names; B_k against drive_terms; the reference tests/buoyancy_ref.py against a second restatement without image cells, bit for bit; its
two degenerate cases (no acceleration: PeriodicOracle alone; a uniform C = c_ref + 1: a driving force (ax, ay) alone); the front ends
through the stand-in tests/buoyancy_standin.py; the physics of the reference in fp64 (tests/buoyancy_cases.py).  The refusals need a
context and are in tests/test_buoyancy_gpu.py."""
import re

import numpy as np
import pytest

import buoyancy_cases as P
from buoyancy_ref import BuoyantOracle, Coupled, RollBuoyant
from buoyancy_standin import OracleSolver
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import CavitySolver, channel, periodic
from latticeboltzmannsimulations_amd import convection as CV
from open_flow_ref import feq
from oracle import lbm_numpy as on
from periodic_ref import PeriodicOracle, drive_terms
from scalar_ref import ScalarOracle

BUOY = (3e-4, 7e-4, 0.5)
D = 0.07


def test_abi_names_are_present():
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for n in ("lbm_set_buoyancy", "lbm_get_buoyancy", "lbm_set_buoyancy_plane"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert sorted(L.SIGNATURES) == sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", hdr)))
    assert L.ABI_VERSION == 4 and "#define LBM_ABI_VERSION 4" in text and lib.lbm_abi_version() == 4
    assert "buoyancy=1" in text and "unless lbm_set_buoyancy" in text and "B_k = (3 w_k) (cx_k ax + cy_k ay)" in text
    assert lib.lbm_set_buoyancy(None, 0.0, 1e-4, 0.5) == -1 and lib.lbm_get_buoyancy(None, None, None, None) == -1
    assert lib.lbm_set_buoyancy_plane(None, None, 0) == -1
    assert hasattr(CavitySolver, "set_buoyancy") and isinstance(CavitySolver.buoyancy, property)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_b_k_is_drive_terms(dtype):
    o = BuoyantOracle(8, 8, 100.0, dtype=dtype, buoyancy=BUOY)
    want = drive_terms(BUOY[0], BUOY[1])
    assert [float(v) for v in o.B] == [float(dtype(v)) for v in want] and float(o.c_ref) == 0.5
    for k in range(1, 9):
        w3 = 1.0 / 3.0 if k <= 4 else 1.0 / 12.0
        assert want[k] == w3 * (float(on.CX[k]) * BUOY[0] + float(on.CY[k]) * BUOY[1])
    assert o.set_buoyancy(0.0, 0.0, 0.3).buoy is None


def _case(nx, ny, per, seed):
    r = np.random.default_rng(seed)
    m = periodic.wrap(r.random((nx, ny)) < 0.2, *per)
    wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan), *per)
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    c0 = periodic.wrap(0.5 + 0.4 * np.sin(2 * np.pi * xs / nx) * np.cos(2 * np.pi * ys / ny) + 0.1 * r.random((nx, ny)), *per)
    st = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny)))
    return m, wv, c0, periodic.wrap(st, *per)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("per", [(1, 0), (0, 1), (1, 1), (0, 0)], ids=["x", "y", "xy", "closed"])
def test_the_two_references_agree(dtype, per):
    """The image-cell reference coupled with ScalarOracle equals the restatement on np.roll bit for bit on the real cells: flow populations,
    moments, scalar populations and C, 20 % random solid with Dirichlet cells, with and without a driving force, after 1, 2, 7, 37 steps."""
    nx, ny = 14, 11
    m, wv, c0, st = _case(nx, ny, per, seed=5)
    for coll in ("SRT", "TRT", "MRT"):
        for force in ((0.0, 0.0), (1e-5, -2e-5)):
            o = BuoyantOracle(nx, ny, 100.0, mask=m, periodic=per, force=force, collision=coll, dtype=dtype, buoyancy=BUOY)
            o.set_state(st.astype(dtype))
            sc = ScalarOracle(m, D, c0, dtype, wall_value=wv, periodic=per)
            pair = Coupled(o, sc)
            real = o.real()
            rs = (slice(None),) + real
            w = RollBuoyant(m[real], 100.0, per, ny, D, c0[real], wall_value=wv[real], force=force, buoyancy=BUOY, fin=o.fin[rs], collision=coll, dtype=dtype)
            done = 0
            for n in (1, 2, 7, 37):
                pair.step(n - done); w.step(n - done)
                done = n
                what = (coll, force, n)
                assert np.array_equal(o.fin[rs], w.w.fin) and np.array_equal(o.u[rs], w.w.u) and np.array_equal(o.rho[real], w.w.rho), what
                assert np.array_equal(sc.populations()[rs], w.g), what
                assert np.array_equal(sc.populations(stored=True)[rs], w.gpost), what
                assert np.array_equal(sc.conc()[real], w.C), what
            assert np.abs(o.u).max() > 1e-4 and np.isfinite(o.fin).all() and np.isfinite(sc.s).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_degenerate_cases(dtype):
    """No acceleration: the bits of PeriodicOracle alone.  A uniform C = c_ref + 1: the bits of a driving force (ax, ay) alone.  And the
    buoyancy does act: another C gives other bits."""
    nx, ny = 14, 11
    per = (1, 0)
    m, wv, c0, st = _case(nx, ny, per, seed=9)
    kw = dict(mask=m, periodic=per, collision="TRT", dtype=dtype)
    plain = PeriodicOracle(nx, ny, 100.0, force=(1e-5, -2e-5), **kw)
    a = BuoyantOracle(nx, ny, 100.0, force=(1e-5, -2e-5), buoyancy=(0.0, 0.0, 0.5), **kw)
    a.Cp = c0.astype(dtype)
    forced = PeriodicOracle(nx, ny, 100.0, force=BUOY[:2], **kw)
    b = BuoyantOracle(nx, ny, 100.0, buoyancy=BUOY, **kw)
    b.Cp = np.full((nx, ny), 1.5, dtype)
    c = BuoyantOracle(nx, ny, 100.0, buoyancy=BUOY, **kw)
    c.Cp = c0.astype(dtype)
    for o in (plain, a, forced, b, c):
        o.set_state(st.astype(dtype))
        o.step(9)
    assert np.array_equal(a.fin, plain.fin) and np.array_equal(b.fin, forced.fin)
    assert not np.array_equal(c.fin, forced.fin) and np.isfinite(c.fin).all()


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------
def test_numbers_and_geometry():
    a = CV.acceleration(1e4, 1.0, 32, 0.05, 0.05 / 0.71)
    assert CV.rayleigh(a, 1.0, 32, 0.05, 0.05 / 0.71) == pytest.approx(1e4, rel=1e-14)
    assert CV.nusselt(0.1 * 2.0 / 16.0 * 7, 0.1, 2.0, 7, 16.0) == pytest.approx(1.0)
    u, rho, C = np.ones((2, 3, 3)), 2.0 * np.ones((3, 3)), 1.5 * np.ones((3, 3))
    v = CV.velocity(u, rho, C, (0.4, -0.8), 0.5, force=(0.4, 0.0))
    assert np.array_equal(v, np.stack([1.2 * np.ones((3, 3)), 0.8 * np.ones((3, 3))]))
    g = CV.heated_cavity(6)
    assert g["solid"].shape == (8, 8) and g["solid"].sum() == 64 - 36 and g["nbodies"] == 3 and g["periodic"] == (False, False)
    assert (g["labels"][0] == 0).all() and (g["labels"][-1] == 1).all() and (g["labels"][1:-1, [0, -1]] == 2).all()
    assert (g["wall_value"][0] == 1.0).all() and (g["wall_value"][-1] == 0.0).all() and np.isnan(g["wall_value"][1:-1]).all()
    b = CV.benard(8)
    assert b["solid"].shape == (18, 10) and b["periodic"] == (True, False) and b["H"] == 8 and b["L"] == 16
    assert (b["wall_value"][:, -1] == 1.0).all() and (b["wall_value"][:, 0] == 0.0).all() and b["s"][1] == 0.5 / 8
    c0 = CV.benard_start(b)
    assert np.array_equal(c0, periodic.wrap(c0, True, False)) and abs(c0[1:-1, 1:-1].mean() - 0.5) < 1e-12
    assert np.allclose(CV.benard_start(b, 0.0)[3, 1:-1], b["s"][1:-1])
    t = np.arange(0, 400, 10)
    assert CV.growth_rate(t, 3.0 * np.exp(2e-3 * t)) == pytest.approx(2e-3, rel=1e-9)


def test_runs_through_the_stand_in(capsys):
    r = CV.run_heated_cavity(8, 1e3, steps=40, solver_factory=OracleSolver)
    order = [c[0] for c in OracleSolver.journal]
    assert order.index("set_periodic") < order.index("begin_scalar") < order.index("set_buoyancy") < order.index("step") and order[-1] == "close"
    assert OracleSolver.journal[0][1] == dict(RT="TRT", dtype="float64", arith="strict")
    sb = [c for c in OracleSolver.journal if c[0] == "set_buoyancy"][0]
    assert sb[1:] == (0.0, r["a"], 0.5) and r["a"] == CV.acceleration(1e3, 1.0, 8, 0.05, r["D"]) and r["D"] == 0.05 / 0.71
    assert r["Nu_hot"] > 1.0 and r["Nu_cold"] < -0.0 and np.isfinite(r["u"]).all() and r["steps"] == 40
    assert "Nu = " in capsys.readouterr().out
    b = CV.run_benard(6, 3000.0, steps=60, every=10, solver_factory=OracleSolver, quiet=True)
    assert list(b["step"]) == [10, 20, 30, 40, 50, 60] and np.isfinite(b["rate"]) and len(b["amplitude"]) == 6
    assert [c[1] for c in OracleSolver.journal if c[0] == "step"] == [10] * 6
    assert CV.main(["cavity", "--n", "6", "--Ra", "1e3", "--steps", "20"], solver_factory=OracleSolver) == 0
    assert "heated cavity 6 x 6, Ra = 1000" in capsys.readouterr().out
    assert CV.main(["benard", "--h", "6", "--steps", "40"], solver_factory=OracleSolver) == 0
    out = capsys.readouterr().out
    assert out.count("growth rate") == 2 and "critical Rayleigh number at H = 6" in out


class _Recorder:
    """What run_channel asks of a solver, recorded."""
    calls = []

    def __init__(self, nx, ny, Re, **kw):
        type(self).calls = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def call(*a, **kw):
            type(self).calls.append((name, a, kw))
            if name == "force_series":
                return dict(fx=np.array([[0.0, 0.0, 0.25]]), fy=np.array([[0.0, 0.0, 0.125]]))
            if name == "scalar_flux":
                return dict(flux=np.array([0.0, -0.5, 1.0]))
            return self
        return call


def test_channel_passes_the_buoyancy_through():
    kw = dict(umax=0.05, disc=(15.0, 10.5, 4.0), steps=10, force_every=5, solver_factory=_Recorder, quiet=True)
    channel.run_channel(60, 22, 20.0, scalar=dict(D=0.04), buoyancy=(0.0, 1e-4, 0.5), **kw)
    order = [c[0] for c in _Recorder.calls]
    assert order.index("begin_scalar") < order.index("set_buoyancy") < order.index("step")
    assert [c[1] for c in _Recorder.calls if c[0] == "set_buoyancy"] == [(0.0, 1e-4, 0.5)]
    channel.run_channel(60, 22, 20.0, scalar=dict(D=0.04), **kw)
    assert "set_buoyancy" not in [c[0] for c in _Recorder.calls]


# ---- the physics of the reference, fp64 ----------------------------------------------------------------------------------------------------
def test_hydrostatic_rest():
    P.check_hydrostatic(OracleSolver)


def test_onset_of_convection():
    """The critical Rayleigh number at H = 16 and 24 against linear theory, within 1.5 x the recorded deviations, and second order in H."""
    P.check_onset(OracleSolver)


@pytest.mark.parametrize("Ra", [1e4, 1e3], ids=["Ra1e4", "Ra1e3"])
def test_heated_cavity(Ra):
    P.check_cavity(OracleSolver, Ra)
