"""CPU tests of the relaxation field of the obstacle lattices (lbm_set_relaxation_field, CavitySolver.set_relaxation_field,
set_viscosity): header, bindings and units; the reference of tests/viscosity_ref.py against its parents; the helpers of viscosity.py
against hand values; the front ends on the stand-in of tests/viscosity_standin.py; and the physics of the reference in fp64 -- the
two-layer Poiseuille flow against its closed form, with both rates per cell and with a uniform omega-, and the vortex that leaves through
a held column with and without a sponge.  What needs a context (the refusals, the checkpoint) runs in tests/test_viscosity_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, channel, periodic, viscosity
from latticeboltzmannsimulations_amd import mrt_gpu as MG
from open_flow_ref import feq
from periodic_ref import PeriodicOracle
from solid_ref import SolidOracle
from subgrid_ref import SubgridOracle, SubgridSolidOracle
import viscosity_cases as VC
from viscosity_ref import ViscosityOracle, ViscositySolidOracle
from viscosity_standin import ViscositySolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")

# What the reference measured once, fp64 TRT: the relative max error of the two-layer Poiseuille profile after 40 H^2
# steps at H = 16 and 32 fluid rows, (a) with the magic parameter 3/16 kept in every cell, (b) with the lattice's uniform omega-.
# (a) is asserted below FACTOR times its measured value, (b) by its ratio between the two heights, within RATIO_TOL of the measured one.
TWO_LAYER_A = {16: 2.22e-11, 32: 1.58e-11}
TWO_LAYER_B = {16: 5.9809e-3, 32: 1.49581e-3}
FACTOR, RATIO_TOL = 10.0, 0.15


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_names_and_units_are_present():
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert re.search(r"\bint\s+lbm_set_relaxation_field\s*\(\s*lbm_ctx\s*\*\s*c\s*,\s*const\s+double\s*\*\s*omega\s*,\s*const\s+double\s*\*\s*omegam\s*\)", hdr)
    assert re.search(r"\bint\s+lbm_get_relaxation_field\s*\(\s*lbm_ctx\s*\*\s*c\s*,\s*double\s*\*\s*omega_out\s*,\s*double\s*\*\s*omegam_out\s*\)", hdr)
    for n in ("lbm_set_relaxation_field", "lbm_get_relaxation_field"):
        assert n in L.SIGNATURES and hasattr(lib, n), n
    assert sorted(L.SIGNATURES) == sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", hdr)))
    assert L.ABI_VERSION == 4 and "#define LBM_ABI_VERSION 4" in text and lib.lbm_abi_version() == 4      # (no struct changes)
    assert "relax_field+m" in text and "MRT's other rates" in text and "first offending cell" in text
    assert lib.lbm_set_relaxation_field(None, None, None) == -1 and lib.lbm_get_relaxation_field(None, None, None) == -1
    for cls in (CavitySolver, CavityBatch):
        assert hasattr(cls, "set_relaxation_field") and hasattr(cls, "set_viscosity") and isinstance(cls.relaxation_field, property)
    assert not any("relax_field" in f[0] or "viscosity" in f[0] for f in L.lbm_params._fields_)      # (run state, not a parameter)
    for u in ("", "_move", "_shape", "_sgs", "_sgs_move", "_sgs_shape"):
        for t in ("f32", "f64"):
            assert os.path.exists(os.path.join(CSRC, f"lbm_solid_relax{u}_{t}.hip")), (u, t)
    dev = open(os.path.join(CSRC, "lbm_device.hpp")).read()
    assert "constexpr int WALL_RELAX = 16" in dev


# ---- the reference against its parents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_uniform_field_is_the_parent_bit_for_bit(dtype):
    """A field equal to the lattice's rate everywhere (and, TRT, a second one equal to its omega-) gives the parent reference bit for
    bit, with and without the closure and with the other rules; a random field differs; set and clear restart nothing."""
    nx, ny = 14, 11
    r = np.random.default_rng(4)
    m = r.random((nx, ny)) < 0.15
    st = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 * r.standard_normal((nx, ny)), 0.01 * r.standard_normal((nx, ny))).astype(dtype)
    for coll in ("SRT", "TRT", "MRT"):
        for cs2 in (0.0, 0.05):
            plain = (SubgridSolidOracle(nx, ny, 400.0, cs2=cs2, mask=m, collision=coll, dtype=dtype) if cs2 else
                     SolidOracle(nx, ny, 400.0, mask=m, collision=coll, dtype=dtype))
            a = ViscositySolidOracle(nx, ny, 400.0, cs2=cs2, mask=m, collision=coll, dtype=dtype)
            w = np.full((nx, ny), a.relax["omega"])
            a.set_relaxation_field(w, np.full((nx, ny), a.relax["omegam"]) if coll == "TRT" else None)
            b = ViscositySolidOracle(nx, ny, 400.0, cs2=cs2, mask=m, collision=coll, dtype=dtype, omega_field=VC.random_rates((nx, ny), 5))
            for o in (plain, a, b):
                o.set_state(st)
                o.step(5)
            assert np.array_equal(a.fin, plain.fin) and np.isfinite(b.fin).all() and not np.array_equal(b.fin, plain.fin), (coll, cs2)
            if cs2:
                assert np.array_equal(a.peek_tau(), plain.peek_tau())
            else:
                assert np.all(a.peek_tau() == a.lattice_tau0())
                t = b.peek_tau()
                assert t.dtype == np.dtype(dtype) and np.all(t[m] == b.lattice_tau0()) and np.array_equal(t[~m], (dtype(1.0) / b.w_field)[~m])
            b.set_relaxation_field(None)
            assert b.nsteps == 5
            b.set_state(plain.fin)
            b.step(3); plain.step(3)
            assert np.array_equal(b.fin, plain.fin)
    with pytest.raises(AssertionError):
        a.set_relaxation_field(np.full((nx, ny), 2.0))
    with pytest.raises(AssertionError):
        ViscositySolidOracle(nx, ny, 400.0, collision="MRT").set_relaxation_field(w, w)      # (omega- is TRT's)


def test_reference_composes_with_the_other_rules():
    """Periodic sides, a driving force, a mask: a uniform field under the composed reference is PeriodicOracle (SubgridOracle) bit for bit;
    TRT with a random second plane stays finite and differs; hold and solid cells report the lattice's tau0."""
    nx, ny = 16, 12
    r = np.random.default_rng(8)
    m = periodic.wrap(r.random((nx, ny)) < 0.12, True, True)
    kw = dict(mask=m, periodic=(1, 1), force=(2e-5, -1e-5), collision="TRT", dtype=np.float64)
    plain = PeriodicOracle(nx, ny, 400.0, **kw).step(20)
    w = np.full((nx, ny), plain.relax["omega"])
    a = ViscosityOracle(nx, ny, 400.0, omega_field=w, omegam_field=np.full((nx, ny), plain.relax["omegam"]), **kw).step(20)
    assert np.array_equal(a.fin, plain.fin)
    sg = SubgridOracle(nx, ny, 400.0, cs2=0.1, **kw).step(20)
    a = ViscosityOracle(nx, ny, 400.0, omega_field=w, cs2=0.1, **kw).step(20)
    assert np.array_equal(a.fin, sg.fin) and np.array_equal(a.peek_tau(), sg.peek_tau())
    b = ViscosityOracle(nx, ny, 400.0, omega_field=VC.random_rates((nx, ny), 1), omegam_field=VC.random_rates((nx, ny), 2), cs2=0.1, **kw).step(20)
    assert np.isfinite(b.fin).all() and not np.array_equal(b.fin, sg.fin)
    t = b.peek_tau()
    assert np.all(t[b.hold] == b.lattice_tau0()) and np.all(t[m] == b.lattice_tau0())
    fl = ~m & ~b.hold
    assert np.all(t[fl] >= (1.0 / b.w_field)[fl])      # (the closure only adds to the cell's own tau0)


# ---- viscosity.py against hand values ----------------------------------------------------------------------------------------------------
def test_rates_layers_sponge_and_profile_against_hand_values():
    w, wm = viscosity.rates(np.array([[0.1, 0.4], [1.0 / 6.0, 0.5]]))
    assert wm is None and np.allclose(w, [[1.25, 1.0 / 1.7], [1.0, 0.5]], rtol=1e-15)
    w, wm = viscosity.rates(np.array([0.1, 0.4]), magic=3.0 / 16.0)
    assert np.allclose(wm, [1.0 / (0.5 + 0.1875 / 0.3), 1.0 / (0.5 + 0.1875 / 1.2)], rtol=1e-15)
    assert np.allclose((1.0 / w - 0.5) * (1.0 / wm - 0.5), 3.0 / 16.0, rtol=1e-14)
    for bad in (np.array([0.1, 0.0]), np.array([np.nan]), np.array([-1.0])):
        with pytest.raises(ValueError):
            viscosity.rates(bad)
    with pytest.raises(ValueError):
        viscosity.rates(np.array([0.1]), magic=0.0)
    nu = viscosity.layers(3, 6, [2, 4], [0.1, 0.2, 0.3])
    assert nu.shape == (3, 6) and np.array_equal(nu[1], [0.1, 0.1, 0.2, 0.2, 0.3, 0.3]) and np.array_equal(nu[0], nu[2])
    with pytest.raises(ValueError):
        viscosity.layers(3, 6, [4, 2], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        viscosity.layers(3, 6, [2], [0.1])
    s = viscosity.sponge(10, 3, 4, 9.0)
    assert s.shape == (10, 3) and np.array_equal(s[:, 0], s[:, 2])
    assert np.allclose(s[:, 1], [1, 1, 1, 1, 1, 1, 1.5, 3.0, 5.5, 9.0], rtol=1e-15)      # 1 + 8 (d / 4)^2, d = 0 .. 4
    assert np.allclose(viscosity.sponge(10, 3, 4, 9.0, side="west")[:, 1], s[::-1, 1], rtol=1e-15)
    assert np.allclose(viscosity.sponge(3, 10, 4, 9.0, side="south")[1], s[:, 1], rtol=1e-15)
    assert np.allclose(viscosity.sponge(3, 10, 4, 9.0, side="north")[1], s[::-1, 1], rtol=1e-15)
    assert np.allclose(viscosity.sponge(10, 3, 4, 9.0, power=1)[:, 1], [1, 1, 1, 1, 1, 1, 3, 5, 7, 9], rtol=1e-15)
    assert np.all(viscosity.sponge(10, 3, 0, 9.0) == 1.0)
    with pytest.raises(ValueError):
        viscosity.sponge(10, 3, 4, 9.0, side="up")
    # one fluid is the parabola F s (H - s) / (2 nu); two fluids: H = 4, h = 2, nu = 1 | 2, F = 1 -- s0 = (2 + 3) / (2 + 1) = 5/3,
    # u(1) = 5/3 - 1/2 = 7/6, u(2) = 10/3 - 2 = 4/3, u(3) = 4/3 + (5/3 - 5/2) / 2 = 11/12, u(4) = 4/3 + (10/3 - 6) / 2 = 0
    u = viscosity.two_layer_profile(8, 3, 0.2, 0.2, 1e-3)
    sc = np.arange(8) + 0.5
    assert np.allclose(u, 1e-3 * sc * (8 - sc) / 0.4, rtol=1e-13)
    u = viscosity.two_layer_profile(4, 2, 1.0, 2.0, 1.0, s=[0.0, 1.0, 2.0, 3.0, 4.0])
    assert np.allclose(u, [0.0, 7.0 / 6.0, 4.0 / 3.0, 11.0 / 12.0, 0.0], rtol=1e-14, atol=1e-15)
    with pytest.raises(ValueError):
        viscosity.two_layer_profile(4, 4, 1.0, 2.0, 1.0)


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------
def test_run_cavity_through_the_stand_in(capsys):
    nx = ny = 20
    nu = viscosity.layers(nx, ny, [ny // 2], [0.02, 0.08])
    kw = dict(Re=400.0, turb=0, xsize=nx, ysize=ny, Pinterval=10, SavePlot=False, BC="BB", dtype=np.float64, solver_factory=ViscositySolver)
    r = MG.run_cavity(maxIt=21, RT="TRT", viscosity_field=nu, **kw)
    j = ViscositySolver.journal
    order = [c[0] for c in j]
    assert j[0][0] == "init" and j[0][1]["solid"] == 0 and order.index("set_viscosity") < order.index("step") and order[-1] == "close"
    call = [c for c in j if c[0] == "set_viscosity"]
    rl = CavitySolver.__init__.__globals__["relaxation"](400.0, ny)
    assert len(call) == 1 and np.array_equal(call[0][1], nu) and call[0][2] == (1.0 / rl["omega"] - 0.5) * (1.0 / rl["omegam"] - 0.5)
    assert "Viscosity field is on, nu from  0.02  to  0.08" in capsys.readouterr().out and np.isfinite(r.u).all()
    w, wm = viscosity.rates(nu, call[0][2])
    o = ViscositySolidOracle(nx, ny, 400.0, collision="TRT", dtype=np.float64, omega_field=w, omegam_field=wm).step(21)
    assert np.array_equal(r.u, o.u.astype(r.u.dtype))
    MG.run_cavity(maxIt=11, RT="MRT", viscosity_field=nu, quiet=True, **kw)
    assert [c[2] for c in ViscositySolver.journal if c[0] == "set_viscosity"] == [None]      # (no magic outside TRT)
    MG.run_cavity(maxIt=11, RT="MRT", quiet=True, **kw, solid=np.zeros((nx, ny), bool))
    assert "set_viscosity" not in [c[0] for c in ViscositySolver.journal]                     # (without the argument nothing is called)
    with pytest.raises(ValueError, match="pass BC='BB'"):
        MG.run_cavity(maxIt=1, viscosity_field=nu, **dict(kw, BC="EB-NEBB "))
    with pytest.raises(ValueError, match="must have shape"):
        MG.run_cavity(maxIt=1, viscosity_field=nu[:, 1:], **kw)


class _Recorder:
    """What run_channel asks of a solver, recorded."""
    calls = []

    def __init__(self, nx, ny, Re, **kw):
        type(self).calls = []
        self.shape = (nx, ny)
        self.relax = dict(omega=1.6, omegam=1.2)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def __getattr__(self, name):
        def call(*a, **kw):
            type(self).calls.append((name, a, kw))
            if name == "force_series":
                return dict(fx=np.array([[0.0, 0.0, 0.25]]), fy=np.array([[0.0, 0.0, 0.125]]))
            if name == "get_fields":
                rho = np.ones(self.shape)
                rho[-5, 7] = 1.25
                rho[3, 3] = 2.0
                return np.zeros((2,) + self.shape), rho
            return self
        return call


def test_channel_passes_the_sponge_through(capsys):
    kw = dict(umax=0.05, disc=(15.0, 10.5, 4.0), steps=10, force_every=5, solver_factory=_Recorder, quiet=True)
    out = channel.run_channel(60, 22, 200.0, sponge=(12, 30.0), RT="TRT", **kw)
    order = [c[0] for c in _Recorder.calls]
    assert order.index("set_wall_velocity") < order.index("set_viscosity") < order.index("step")
    (nu, magic), = [c[1] for c in _Recorder.calls if c[0] == "set_viscosity"]
    assert np.allclose(nu, out["nu"] * viscosity.sponge(60, 22, 12, 30.0), rtol=1e-15) and nu[0, 0] == out["nu"] and np.isclose(nu[-1, 5], 30.0 * out["nu"])
    assert magic == (1.0 / 1.6 - 0.5) * (1.0 / 1.2 - 0.5)
    assert out["sponge"] == (12, 30.0) and out["outlet_drho"] == 0.25      # (the last 20 columns; the cell at x = 3 is outside them)
    out = channel.run_channel(60, 22, 200.0, sponge=(12, 30.0), **kw)
    assert [c[1][1] for c in _Recorder.calls if c[0] == "set_viscosity"] == [None]      # (MRT: no omega- plane)
    out = channel.run_channel(60, 22, 200.0, **kw)
    assert "set_viscosity" not in [c[0] for c in _Recorder.calls] and "outlet_drho" not in out and "get_fields" not in [c[0] for c in _Recorder.calls]
    with pytest.raises(ValueError, match="exclude each other"):
        channel.run_channel(60, 22, 200.0, sponge=(12, 30.0), scalar=dict(D=0.04), buoyancy=(0.0, 1e-4, 0.5), **kw)
    with pytest.raises(SystemExit):
        channel.main(["--sponge", "12", "30", "--buoyancy", "0", "1e-4", "0.5", "--scalar-D", "0.04", "--disc", "15", "10.5", "4"])
    capsys.readouterr()
    assert "sponge" in inspect.signature(channel.run_channel).parameters and "viscosity_field" in inspect.signature(MG.run_cavity).parameters


# ---- the physics of the reference, fp64 ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_layer_errors():
    """{(H, per_cell): error} of the reference, computed once."""
    out = {}
    for H in (16, 32):
        for per_cell in (True, False):
            o, c = VC.two_layer_reference(H, per_cell)
            out[H, per_cell] = VC.two_layer_error(o.u, o.rho, c)
    return out


def test_two_layer_poiseuille_is_exact_with_both_rates_per_cell(two_layer_errors):
    """nu = 0.1 | 0.4, the interface on the link midpoint at mid-height, x periodic, force 1e-6, 40 H^2 steps: with omega+ and omega- per
    cell such that the magic parameter is 3/16 in both layers, the profile with the half-force shift matches the closed form of stress
    continuity as well as the one-fluid channel does.  Measured on this reference: 2.22e-11 at 16 rows, 1.58e-11 at 32."""
    for H in (16, 32):
        e = two_layer_errors[H, True]
        print(f"two-layer Poiseuille, H = {H}, magic per cell: {e:.3e} (measured {TWO_LAYER_A[H]:.2e})")
        assert e < FACTOR * TWO_LAYER_A[H], (H, e)


def test_two_layer_poiseuille_is_second_order_with_a_uniform_odd_rate(two_layer_errors):
    """The same with omega+ per cell only and the lattice's omega- (the magic parameter is 3/16 in the lower layer alone): the error
    falls by the ratio the reference measured, 5.981e-3 / 1.496e-3 = 3.998 -- second order -- within 15 %."""
    e16, e32 = two_layer_errors[16, False], two_layer_errors[32, False]
    want = TWO_LAYER_B[16] / TWO_LAYER_B[32]
    print(f"two-layer Poiseuille, uniform omega-: {e16:.4e} at 16 rows, {e32:.4e} at 32, ratio {e16 / e32:.4f} (measured {want:.4f})")
    assert abs((e16 / e32) / want - 1.0) < RATIO_TOL
    assert e16 > 1e3 * two_layer_errors[16, True]      # (which is why the field carries both rates)


def test_a_sponge_lowers_the_pressure_spike_at_the_held_outlet():
    """A Gaussian vortex (amp 0.02, R = 5) in a uniform stream U = 0.05 leaves a 120 x 48 lattice, periodic in y, through a held column;
    nu = 0.01, TRT with the magic parameter 3/16 per cell, 1800 steps.  The peak of max |rho - 1| over the domain from the step at which
    the vortex's rim reaches the outlet is smaller with sponge(120, 48, 40, 30) than without.  Measured on this reference: 1.320e-3
    without, 2.820e-4 with; the upstream half afterwards holds 4.5e-7 and 2.8e-7 -- recorded, not asserted."""
    c = VC.vortex_outlet()
    res = {}
    for sp in (False, True):
        o = ViscosityOracle(c["nx"], c["ny"], c["Re"], collision="TRT", dtype=np.float64,
                            omegam=periodic.trt_omegam(1.0 / (3.0 * c["nu"] + 0.5), VC.MAGIC))
        o.set_periodic(False, True)
        o.set_open_cells(c["hold"], c["held"])
        o.set_state(c["fin"])
        if sp:
            o.set_relaxation_field(*viscosity.rates(c["sponge"], VC.MAGIC))
        res[sp] = VC.run_vortex(o, c)
        print(f"vortex through the held outlet, sponge {sp}: peak max |rho - 1| {res[sp][0]:.3e}, upstream half afterwards {res[sp][1]:.3e}")
    assert res[True][0] < res[False][0]
