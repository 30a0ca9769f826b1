"""CPU tests of the sub-grid closure of the obstacle lattices (lbm_set_subgrid, CavitySolver.set_subgrid): header, bindings and what a
library without a device can answer; the reference of tests/subgrid_ref.py against its parents; the front ends on the stand-ins of tests/subgrid_standin.py; and the physics of the reference in fp64 -- the
under-resolved block at Re 20000, periodic Couette flow against its closed form, and a resolved cavity that the closure leaves alone.
The refusals that need a context (another semantics, the tile kernel, buoyancy) run where a context exists: tests/test_subgrid_gpu.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, channel, datagen, launch_plan, relaxation
from latticeboltzmannsimulations_amd import mrt_gpu as MG
from latticeboltzmannsimulations_amd.stopping import subgrid_constant
from open_flow_ref import feq
from periodic_ref import PeriodicOracle
from solid_ref import SolidOracle
from subgrid_ref import SubgridOracle, SubgridSolidOracle, subgrid_k
from subgrid_standin import SubgridBatch, SubgridSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")

# What the reference measured once, fp64; the tests assert FACTOR times these and nothing wider.
#   periodic Couette, H = 8 rows between a wall at rest and a wall sliding at U = 0.1, nu0 = 0.01, Cs2 = 0.1 (the eddy term is an eighth
#   of nu0), SRT, 6000 steps from the linear profile: max |(tau - tau0) / (3 Cs2 U / H) - 1| over the fluid cells, and
#   |wall force per unit length / (rho (nu0 + Cs2 U / H) U / H) - 1| on the wall at rest
COUETTE_TAU_ERR, COUETTE_FORCE_ERR = 3.14e-5, 1.45e-6
FACTOR = 2.0


def _block(n=48):
    m = np.zeros((n, n), bool)
    m[n // 2 - 4:n // 2 + 4, n // 2 - 4:n // 2 + 4] = True
    return m


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_names_are_present():
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    for n in ("lbm_set_subgrid", "lbm_get_subgrid"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert sorted(L.SIGNATURES) == sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", hdr)))
    assert L.ABI_VERSION == 4 and "#define LBM_ABI_VERSION 4" in text and lib.lbm_abi_version() == 4      # (no struct changes)
    assert "subgrid=<cs2>" in text and "k = 18 sqrt(2) cs2" in text and "a solid cell and a hold cell" in text
    assert lib.lbm_set_subgrid(None, 0.025) == -1 and lib.lbm_set_subgrid(None, 0.0) == -1 and lib.lbm_get_subgrid(None, None) == -1
    for cls in (CavitySolver, CavityBatch):
        assert hasattr(cls, "set_subgrid") and isinstance(cls.subgrid, property) and hasattr(cls, "get_tau")
    assert inspect.signature(CavitySolver.set_subgrid).parameters["cs2"].default == 0.025
    assert "subgrid" not in " ".join(inspect.signature(CavitySolver.__init__).parameters)      # (a setter, no new keyword)


def test_the_plan_is_untouched():
    """The constant is run state: lbm_params and the dry-run plan know nothing of it, and turb = 1 stays refused on these lattices."""
    assert not any("subgrid" in f[0] for f in L.lbm_params._fields_)
    plan = launch_plan(64, 64, 1000.0, steps=10, semantics="bounce_back", solid=True) if "solid" in inspect.signature(launch_plan).parameters \
        else launch_plan(64, 64, 1000.0, steps=10, semantics="bounce_back")
    assert "subgrid" not in str(plan)
    with pytest.raises((RuntimeError, ValueError), match="turb"):
        launch_plan(64, 64, 1000.0, steps=10, semantics="bounce_back", turb=1)


def test_the_constant_and_the_units():
    """k = 18 sqrt(2) cs2 as the reference forms it, and the new instantiations have translation units of their own."""
    assert subgrid_k(0.025) == (18.0 * math.sqrt(2.0)) * 0.025 and subgrid_k(0.0) == 0.0
    for u in ("", "_move", "_shape"):
        for t in ("f32", "f64"):
            assert os.path.exists(os.path.join(CSRC, f"lbm_solid_sgs{u}_{t}.hip"))


# ---- the reference against its parents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_reference_round_trip_and_degenerate_cases(dtype):
    """cs2 = 0 is the parent, bit for bit; set, get, clear; setting restarts nothing; tau is tau0 on solid cells and at rest, and grows
    with the shear; each operator takes the rate where its viscous rate goes."""
    nx, ny = 14, 11
    r = np.random.default_rng(4)
    m = r.random((nx, ny)) < 0.15
    st = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 * r.standard_normal((nx, ny)), 0.01 * r.standard_normal((nx, ny))).astype(dtype)
    for coll in ("SRT", "TRT", "MRT"):
        plain = SolidOracle(nx, ny, 400.0, mask=m, collision=coll, dtype=dtype)
        a = SubgridSolidOracle(nx, ny, 400.0, mask=m, collision=coll, dtype=dtype)
        b = SubgridOracle(nx, ny, 400.0, cs2=0.05, mask=m, collision=coll, dtype=dtype)
        assert a.cs2 == 0.0 and b.cs2 == 0.05 and a.turb == 0 and b.turb == 0
        for o in (plain, a, b):
            o.set_state(st)
            o.step(5)
        assert np.array_equal(a.fin, plain.fin) and not np.array_equal(b.fin, plain.fin) and np.isfinite(b.fin).all()
        assert np.all(a.peek_tau() == a.tau0()) and a.peek_tau().dtype == np.dtype(dtype)
        t = b.peek_tau()
        assert np.all(t[m] == b.tau0()) and np.all(t[~m] > b.tau0()) and t.dtype == np.dtype(dtype)
        b.set_subgrid(0.0); a.set_subgrid(0.05)
        assert b.nsteps == 5 and a.nsteps == 5 and np.all(b.peek_tau() == b.tau0())
        b.set_state(plain.fin); a.set_subgrid(0.0)
        b.step(3); plain.step(3); a.step(3)
        assert np.array_equal(b.fin, plain.fin) and np.array_equal(a.fin, plain.fin)
        # the rest state has no non-equilibrium flux to rounding: tau stays within a few ulp-sized steps of tau0
        q = SubgridSolidOracle(nx, ny, 400.0, cs2=0.05, mask=m, collision=coll, dtype=dtype)
        q.set_state(np.broadcast_to(np.asarray(q.t)[:, None, None], (9, nx, ny)).astype(dtype))
        assert float(np.abs(q.peek_tau() - q.tau0()).max()) < 1e-3
    with pytest.raises(AssertionError):
        a.set_subgrid(-0.1)
    with pytest.raises(AssertionError):
        a.set_subgrid(float("nan"))


def test_reference_composes_with_the_other_rules():
    """Periodic sides, a driving force, a motion: the closure changes the collision's rate and nothing else -- with cs2 = 0 the composed
    reference is PeriodicOracle bit for bit, with cs2 > 0 it stays finite, conserves the fluid's mass under the force-free closed
    rules and differs."""
    from latticeboltzmannsimulations_amd import periodic as P
    nx, ny = 16, 12
    r = np.random.default_rng(8)
    m = P.wrap(r.random((nx, ny)) < 0.12, True, True)
    kw = dict(mask=m, periodic=(1, 1), force=(2e-5, -1e-5), collision="TRT", dtype=np.float64)
    plain = PeriodicOracle(nx, ny, 400.0, **kw).step(20)
    a = SubgridOracle(nx, ny, 400.0, **kw).step(20)
    b = SubgridOracle(nx, ny, 400.0, cs2=0.1, **kw).step(20)
    assert np.array_equal(a.fin, plain.fin) and np.isfinite(b.fin).all() and not np.array_equal(b.fin, plain.fin)
    real = b.real()
    assert np.all(b.tau[real][~m[real]] >= b.tau0())
    t = b.peek_tau()
    assert np.all(t[b.hold] == b.tau0()) and np.all(t[m] == b.tau0()) and np.any(t > b.tau0())      # (image cells are hold cells: tau0)


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------
def test_subgrid_constant_is_checked_once():
    assert subgrid_constant(None, "EB-NEBB ") is None and subgrid_constant(0.0, "EB-NEBB ") is None and subgrid_constant(0.025, "BB") == 0.025
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite constant >= 0"):
            subgrid_constant(bad, "BB")
    with pytest.raises(ValueError, match="pass BC='BB'"):
        subgrid_constant(0.025, "EB-NEBB ")
    with pytest.raises(ValueError, match="one step per launch"):
        subgrid_constant(0.025, "BB", True)
    # the messages of the walls' own check stay word for word
    with pytest.raises(ValueError, match=re.escape("BC='BB' runs without the Smagorinsky closure: pass turb=0")):
        MG.run_cavity(maxIt=1, BC="BB", turb=1, subgrid=0.025, SavePlot=False, quiet=True, solver_factory=SubgridSolver)
    with pytest.raises(ValueError, match=re.escape("solid obstacles need the bounce-back walls: pass BC='BB' (and turb=0)")):
        MG.run_cavity(maxIt=1, solid=_block(16), xsize=16, ysize=16, SavePlot=False, quiet=True, solver_factory=SubgridSolver)


def test_run_cavity_through_the_stand_in(capsys):
    kw = dict(Re=20000.0, RT="SRT", turb=0, xsize=24, ysize=24, Pinterval=20, SavePlot=False, BC="BB", dtype=np.float64, solver_factory=SubgridSolver)
    r = MG.run_cavity(maxIt=41, subgrid=0.025, **kw)
    j = SubgridSolver.journal
    assert j[0] == ("init", dict(RT="SRT", semantics="bounce_back", turb=0, solid=0))      # (no mask given: an empty one)
    order = [c[0] for c in j]
    assert order.index("set_subgrid") < order.index("step") and order[-1] == "close" and [c for c in j if c[0] == "set_subgrid"] == [("set_subgrid", 0.025)]
    out = capsys.readouterr().out
    assert "Sub-grid closure is on, Cs2 =  0.025" in out and out.count("current mean relaxation time is ") == 3 and "force on the obstacles" not in out
    assert [it for it, _ in r.tau_mean] == [0, 20, 40] and all(t > 1.0 / relaxation(20000.0, 24)["omega"] for _, t in r.tau_mean[1:])
    assert np.isfinite(r.u).all() and r.iterations == 41
    # with a mask: the mean is taken over the fluid cells, and the obstacle output stays
    m = _block(24)
    r2 = MG.run_cavity(maxIt=21, subgrid=0.025, solid=m, **kw)
    out = capsys.readouterr().out
    assert SubgridSolver.journal[0][1]["solid"] == 64 and out.count("current force on the obstacles is") == 2
    o = SubgridSolidOracle(24, 24, 20000.0, cs2=0.025, mask=m, collision="SRT", dtype=np.float64).step(21)
    assert r2.tau_mean[-1] == (20, float(np.mean(o.peek_tau()[~m], dtype=np.float64)))
    # without the constant nothing changes: no mask, no call, no line
    MG.run_cavity(maxIt=21, quiet=True, **dict(kw, solver_factory=_refuse_solid))
    MG.run_cavity(maxIt=21, subgrid=0.0, quiet=True, **dict(kw, solver_factory=_refuse_solid))
    with pytest.raises(SystemExit):
        MG.main(["--subgrid", "0.025", "--BC", "EB-NEBB"])
    with pytest.raises(SystemExit):
        MG.main(["--subgrid", "0.025", "--BC", "BB", "--turb", "1"])
    assert "pass turb=0" in capsys.readouterr().err


class _refuse_solid(SubgridSolver):
    def __init__(self, *a, **kw):
        assert "solid" not in kw
        super().__init__(*a, solid=np.zeros((a[0], a[1]), bool), **kw)

    def set_subgrid(self, cs2=0.025):
        raise AssertionError("set_subgrid without a constant")


class _Recorder:
    """What run_channel asks of a solver, recorded."""
    calls = []

    def __init__(self, nx, ny, Re, **kw):
        type(self).calls = []
        self.shape = (nx, ny)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def call(*a, **kw):
            type(self).calls.append((name, a, kw))
            if name == "force_series":
                return dict(fx=np.array([[0.0, 0.0, 0.25]]), fy=np.array([[0.0, 0.0, 0.125]]))
            if name == "get_tau":
                return np.full(self.shape, 0.75)
            return self
        return call


def test_channel_and_datagen_pass_the_constant_through(capsys):
    kw = dict(umax=0.05, disc=(15.0, 10.5, 4.0), steps=10, force_every=5, solver_factory=_Recorder, quiet=True)
    out = channel.run_channel(60, 22, 200.0, subgrid=0.025, **kw)
    order = [c[0] for c in _Recorder.calls]
    assert order.index("set_wall_velocity") < order.index("set_subgrid") < order.index("step") and out["tau_mean"] == 0.75 and out["subgrid"] == 0.025
    assert [c[1] for c in _Recorder.calls if c[0] == "set_subgrid"] == [(0.025,)]
    out = channel.run_channel(60, 22, 200.0, **kw)
    assert "set_subgrid" not in [c[0] for c in _Recorder.calls] and "tau_mean" not in out
    with pytest.raises(ValueError, match="exclude each other"):
        channel.run_channel(60, 22, 200.0, subgrid=0.025, scalar=dict(D=0.04), buoyancy=(0.0, 1e-4, 0.5), **kw)
    with pytest.raises(SystemExit):
        channel.main(["--subgrid", "0.025", "--buoyancy", "0", "1e-4", "0.5", "--scalar-D", "0.04", "--disc", "15", "10.5", "4"])
    capsys.readouterr()
    res = datagen.generate(Re_range=[5000.0, 20000.0], xsize=16, ysize=16, RT="SRT", turb=0, maxIt=30, Pinterval=10, save=False, quiet=True,
                           BC="BB", subgrid=0.025, batch_factory=SubgridBatch, dtype=np.float64)
    j = SubgridBatch.journal
    assert j[0] == ("init", dict(n=2, semantics="bounce_back", solid=(2, 16, 16))) and j[1] == ("set_subgrid", 0.025) and j[2][0] == "step"
    assert np.isfinite(res[1]).all() and res[1].shape == (2, 9, 16, 16)
    with pytest.raises(ValueError, match="pass BC='BB'"):
        datagen.generate(Re_range=[100.0], xsize=16, ysize=16, subgrid=0.025, save=False, quiet=True, batch_factory=SubgridBatch)
    with pytest.raises(SystemExit):
        datagen.main(["--subgrid", "0.025"])


# ---- the physics of the reference, fp64 ----------------------------------------------------------------------------------------------------
def test_the_block_at_re_20000_needs_the_closure():
    """48 x 48, Re 20000, an 8 x 8 block in the middle, SRT.  Without the closure the run is lost by step 200 -- densities of both signs
    beyond 1e30 and |u| in the thousands; the doubles themselves overflow near step 600, which the second assertion waits for.  With
    cs2 = 0.025 it is finite with max |u| < 1 after 4000 steps and the fluid's mass has moved by less than 1e-6 of itself."""
    m = _block()
    with np.errstate(all="ignore"):
        o = SolidOracle(48, 48, 20000.0, mask=m, collision="SRT", dtype=np.float64).step(200)
        lost = not np.isfinite(o.fin).all() or float(np.abs(o.u).max()) > 1.0 or float(o.rho.min()) < 0.0
        print(f"without the closure after 200 steps: max |u| {np.abs(o.u).max():.3e}, rho in [{o.rho.min():.3e}, {o.rho.max():.3e}]")
        assert lost
        assert not np.isfinite(o.step(500).fin).all()
    o = SubgridSolidOracle(48, 48, 20000.0, cs2=0.025, mask=m, collision="SRT", dtype=np.float64)
    m0 = o.fluid_mass()
    o.step(4000)
    drift = abs(o.fluid_mass() - m0) / m0
    print(f"with the closure after 4000 steps: max |u| {np.abs(o.u).max():.4f}, max tau {o.tau.max():.4f} (tau0 {o.tau0():.6f}), mass drift {drift:.2e}")
    assert np.isfinite(o.fin).all() and float(np.abs(o.u).max()) < 1.0 and drift < 1e-6
    assert float(o.tau.max()) > float(o.tau0()) + 1e-3


def test_couette_flow_against_the_closed_form():
    """Between a wall at rest and a wall sliding at U, periodic in x, the shear is uniform, |S| = U / H, so nu_t = Cs2 U / H everywhere:
    tau - tau0 = 3 Cs2 U / H in every fluid cell and the wall feels rho (nu0 + Cs2 U / H) U / H per unit length.  The check is against
    the closed form; the margins are twice what the reference measured (top of this file)."""
    H, U, nu0, cs2, nx = 8, 0.1, 0.01, 0.1, 6
    ny = H + 2
    m = np.zeros((nx, ny), bool)
    m[:, 0] = m[:, ny - 1] = True
    lab = np.zeros((nx, ny), np.int32)
    lab[:, ny - 1] = 1
    uw = np.zeros((2, nx, ny))
    uw[0, :, 0] = U                                         # (row 0 slides; the lid behind it drives nothing)
    o = SubgridOracle(nx, ny, U * ny / nu0, uLB=U, cs2=cs2, mask=m, labels=lab, centres=np.array([[(nx - 1) / 2.0, 0.0], [(nx - 1) / 2.0, ny - 1.0]]),
                      periodic=(1, 0), wall_velocity=uw, collision="SRT", dtype=np.float64)
    assert cs2 * U / H >= 0.1 * nu0
    prof = U * (1.0 - (np.arange(ny) - 0.5) / H)
    prof[0] = prof[-1] = 0.0
    o.set_state(feq(1.0, np.broadcast_to(prof[None, :], (nx, ny)), 0.0))
    o.step(6000)
    S = U / H
    e_tau = float(np.abs((o.tau[1:-1, 1:-1] - o.tau0()) / (3.0 * cs2 * S) - 1.0).max())
    rho = float(o.rho[1:-1, 1:-1].mean())
    fx = float(o.body_force()["fx"][1]) / (nx - 2)
    e_f = abs(fx / (rho * (nu0 + cs2 * S) * S) - 1.0)
    print(f"Couette with the closure: tau error {e_tau:.3e} (measured {COUETTE_TAU_ERR:.2e}), wall force error {e_f:.3e} (measured {COUETTE_FORCE_ERR:.2e})")
    assert e_tau < FACTOR * COUETTE_TAU_ERR and e_f < FACTOR * COUETTE_FORCE_ERR
    assert float(np.abs(o.u[0][1:-1, 1:-1] - prof[None, 1:-1]).max()) / U < 1e-5      # (the profile stays linear)


def test_a_resolved_cavity_is_left_alone():
    """Re 100 on 32 x 32, TRT, 2000 steps: the closure with cs2 = 0.025 changes u by less than 1 % of uLB."""
    a = SubgridSolidOracle(32, 32, 100.0, collision="TRT", dtype=np.float64).step(2000)
    b = SubgridSolidOracle(32, 32, 100.0, cs2=0.025, collision="TRT", dtype=np.float64).step(2000)
    d = float(np.abs(a.u - b.u).max()) / a.uLB
    print(f"Re 100, 32 x 32, TRT: the closure moves u by {100 * d:.3f} % of uLB")
    assert 0.0 < d < 0.01
