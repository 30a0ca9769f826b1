"""CPU tests of the rheology table (lbm_set_rheology): the C ABI and the bindings, the table builder of rheology.py, the
reference of tests/rheology_ref.py against its parents, the index function of csrc/lbm_rheology.hpp in a host program of its own, the
physics of the reference in fp64 -- power-law Poiseuille flow against its closed form at two heights and two indices, periodic Couette
flow -- and the front ends on the stand-in."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, channel, periodic
from latticeboltzmannsimulations_amd import mrt_gpu as MG
from latticeboltzmannsimulations_amd import rheology as RH
from checks import perturbed
from periodic_ref import PeriodicOracle
import rheology_cases as RC
from rheology_ref import RheologyOracle, RheologySolidOracle
from rheology_standin import RheologySolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")


# ---- 1. the C ABI and the bindings -------------------------------------------------------------------------------------------------------
def test_abi_names_and_units_are_present():
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert re.search(r"\bint\s+lbm_set_rheology\s*\(\s*lbm_ctx\s*\*\s*c\s*,\s*const\s+double\s*\*\s*omega\s*,\s*const\s+double\s*\*\s*omegam\s*,\s*int\s+n\s*,"
                     r"\s*double\s+g_max\s*\)", hdr)
    assert re.search(r"\bint\s+lbm_get_rheology\s*\(\s*lbm_ctx\s*\*\s*c\s*,\s*double\s*\*\s*omega_out\s*,\s*double\s*\*\s*omegam_out\s*,\s*int\s*\*\s*n_out\s*,"
                     r"\s*double\s*\*\s*g_max_out\s*\)", hdr)
    assert re.search(r"\bint\s+lbm_get_shear\s*\(\s*lbm_ctx\s*\*\s*c\s*,\s*void\s*\*\s*g_host\s*,\s*int\s+host_dtype\s*\)", hdr)
    for n in ("lbm_set_rheology", "lbm_get_rheology", "lbm_get_shear"):
        assert n in L.SIGNATURES and hasattr(lib, n), n
    assert sorted(L.SIGNATURES) == sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", hdr)))
    assert L.ABI_VERSION == 4 and "#define LBM_ABI_VERSION 4" in text and lib.lbm_abi_version() == 4      # (no struct changes)
    assert "rheology=<n>+m" in text and "names its index" in text
    assert lib.lbm_set_rheology(None, None, None, 0, 0.0) == -1 and lib.lbm_get_rheology(None, None, None, None, None) == -1
    for cls in (CavitySolver, CavityBatch):
        assert hasattr(cls, "set_rheology") and hasattr(cls, "get_shear") and isinstance(cls.rheology, property)
    assert not any("rheo" in f[0] for f in L.lbm_params._fields_)      # (run state, not a parameter)
    for u in ("", "_move", "_shape"):
        for t in ("f32", "f64"):
            assert os.path.exists(os.path.join(CSRC, f"lbm_solid_rheo{u}_{t}.hip")), (u, t)
    dev = open(os.path.join(CSRC, "lbm_device.hpp")).read()
    assert "constexpr int WALL_RHEO = 32" in dev


# ---- 2. the table builder ----------------------------------------------------------------------------------------------------------------
def _implicit_residual(law, omega, g_max):
    tau = 1.0 / omega
    g = np.linspace(0.0, g_max, omega.size)
    return float(np.abs((0.5 + 3.0 * law(RH.shear_rate(g, tau))) / tau - 1.0).max())


def test_table_builder():
    w, wm = RH.table(lambda gd: np.full_like(gd, 0.1), 17, 0.01)
    assert wm is None and np.all(w == 1.0 / (0.5 + 3.0 * 0.1))
    for n in (0.5, 1.5):
        K, F, gw = RH.power_law_channel(16, n, 0.05, 0.05)
        law = RH.power_law(K, n, 1e-3, 2.0)
        w, wm = RH.table(law, 4096, 2.0 * gw, magic=3.0 / 16.0)
        assert w.shape == wm.shape == (4096,) and _implicit_residual(law, w, 2.0 * gw) < 1e-10, n
        assert float(np.abs((1.0 / w - 0.5) * (1.0 / wm - 0.5) - 3.0 / 16.0).max()) < 1e-14, n
        assert (np.diff(w) >= 0).all() if n < 1.0 else (np.diff(w) <= 0).all()      # (thinning: tau falls with the shear, omega rises)
    law = RH.carreau(0.1, 0.01, 50.0, 0.5)
    w, _ = RH.table(law, 256, 0.05)
    assert _implicit_residual(law, w, 0.05) < 1e-10
    law = RH.bingham(0.05, 1e-4, 1e3)
    w, _ = RH.table(law, 256, 0.05)
    assert _implicit_residual(law, w, 0.05) < 1e-10 and abs(1.0 / w[0] - (0.5 + 3.0 * (0.05 + 1e-4 * 1e3))) < 1e-12
    with pytest.raises(ValueError, match="not strictly increasing"):
        RH.table(lambda gd: 10.0 / gd ** 2, 64, 0.05)      # (the stress 10 / gdot falls)
    with pytest.raises(ValueError, match=r"\(0, 2\)|> 0"):
        RH.table(lambda gd: np.full_like(gd, -0.1), 64, 0.05)      # (tau < 1/2)
    with pytest.raises(ValueError):
        RH.table(lambda gd: np.full_like(gd, np.nan), 64, 0.05)
    with pytest.raises(ValueError):
        RH.table(law, 1, 0.05)
    with pytest.raises(ValueError):
        RH.table(law, 64, 0.0)
    # the helpers against hand values
    assert RH.g_of(0.3, 0.1) == pytest.approx(np.sqrt(2.0) / 3.0 * 0.3 * 0.8) and RH.shear_rate(RH.g_of(0.3, 0.1), 0.8) == pytest.approx(0.3)
    assert RH.apparent_viscosity(0.8) == pytest.approx(0.1)
    K, F, gw = RH.power_law_channel(16, 0.5, 0.05, 0.05)
    gdw = 0.05 * 1.5 / (0.5 * 8.0)                  # umax (n + 1) / (n h)
    assert K == pytest.approx(0.05 * gdw ** 0.5) and F == pytest.approx(0.05 * gdw / 8.0) and gw == pytest.approx(np.sqrt(2.0) / 3.0 * gdw * 0.65)
    u = RH.power_law_profile(16, K, 0.5, F, s=np.array([0.0, 8.0, -4.0]))
    assert u[0] == pytest.approx(0.05) and u[1] == pytest.approx(0.0, abs=1e-15) and u[2] == pytest.approx(0.05 * (1.0 - 0.5 ** 3))
    assert RH.power_law_profile(16, K, 0.5, F).shape == (16,)
    # n = 1 is Poiseuille's parabola
    K1, F1, _ = RH.power_law_channel(16, 1.0, 0.05, 0.05)
    assert np.allclose(RH.power_law_profile(16, K1, 1.0, F1), periodic.poiseuille_profile(18, 0.05, F1)[1:-1], rtol=1e-13)


# ---- 3. the reference against its parents ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_a_constant_table_is_the_plain_reference_bit_for_bit(dtype):
    """A table whose every entry is the lattice's rate (and, TRT, a second one of its omega-) gives PeriodicOracle bit for bit under the
    composed rules -- periodic sides, a force, a mask, hold cells; the hostile table differs; solid and hold cells report tau0."""
    nx, ny = 16, 12
    r = np.random.default_rng(8)
    m = periodic.wrap(r.random((nx, ny)) < 0.12, True, True)
    st = periodic.wrap(perturbed(nx, ny, dtype, 11), True, True)
    for coll, with_m in (("SRT", False), ("TRT", False), ("TRT", True), ("MRT", False)):
        kw = dict(mask=m, periodic=(1, 1), force=(2e-5, -1e-5), collision=coll, dtype=dtype)
        plain = PeriodicOracle(nx, ny, 400.0, **kw)
        a = RheologyOracle(nx, ny, 400.0, **kw)
        a.set_rheology(np.full(17, a.relax["omega"]), np.full(17, a.relax["omegam"]) if with_m else None, 1e-3)
        b = RheologyOracle(nx, ny, 400.0, **kw)
        for o in (plain, a, b):
            o.set_state(st)
        b.set_rheology(*RC.hostile_table(3, with_m), RC.hostile_gmax(b))
        for o in (plain, a, b):
            o.step(7)
        assert np.array_equal(a.fin, plain.fin), (coll, with_m)
        assert np.isfinite(b.fin).all() and not np.array_equal(b.fin, plain.fin), (coll, with_m)
        t = b.peek_tau()
        pinned = b._pinned()
        assert t.dtype == np.dtype(dtype) and pinned.any() and np.all(t[pinned] == b.lattice_tau0()) and np.all(b.peek_shear()[pinned] == 0)
        assert np.all(a.peek_tau() == a.lattice_tau0())
        b.set_rheology(None)
        assert b.nsteps == 7
        b.set_state(plain.fin)
        b.step(3); plain.step(3)
        assert np.array_equal(b.fin, plain.fin)
    with pytest.raises(AssertionError):
        a.set_rheology(np.full(17, 2.0), None, 1.0)
    with pytest.raises(AssertionError):
        RheologySolidOracle(nx, ny, 400.0, collision="MRT").set_rheology(np.full(4, 1.0), np.full(4, 1.0), 1.0)      # (omega- is TRT's)


# ---- 4. the index function, on the host ------------------------------------------------------------------------------------------------------
def test_index_function_is_safe_for_any_input(tmp_path):
    """tests/rheology_index_model.cpp: for NaN, +-Inf, -1, 0, subnormals, values in range, n - 1, 1e30 and the integer limits, in both real
    types and six table sizes, i lies in [0, n - 2], fr in [0, 1] and the loads stay inside the table; built with the address and
    undefined-behaviour sanitizers where the compiler has them."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "rheology_index_model")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "rheology_index_model.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)     # (a compiler without the sanitizers' runtimes)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "FAILED" not in p.stdout, p.stdout + p.stderr
    assert [l.split()[:2] for l in p.stdout.splitlines()] == [["ok", "float"], ["ok", "double"], ["ok", "slopes"]]


# ---- 5. the physics of the reference, fp64 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poiseuille_runs():
    out = {}
    for H, n in RC.POISEUILLE:
        o, c = RC.power_law_reference(H, n)
        top, _ = RC.coverage(o)
        out[(H, n)] = dict(error=RC.power_law_error(o.u, o.rho, c), newtonian=c["newtonian"], top=top,
                           g=float(o.peek_shear().max()) / c["g_max"], tau=(float(o.tau[1:-1, 1:-1].min()), float(o.tau[1:-1, 1:-1].max())))
    return out


@pytest.mark.parametrize("case", RC.POISEUILLE, ids=lambda c: f"H{c[0]}-n{c[1]}")
def test_power_law_poiseuille_against_the_closed_form(poiseuille_runs, case):
    """TRT with omega- per entry for the magic parameter 3/16, 40 H^2 steps: the profile with the half-force shift against
    rheology.power_law_profile.  The error is below a tenth of the profile's distance from the Newtonian parabola of equal peak -- the
    scheme tells the fluids apart with a margin -- and at most twice what the reference measured; no cell clamps."""
    r = poiseuille_runs[case]
    print(f"power-law Poiseuille H = {case[0]}, n = {case[1]}: error {r['error']:.6e} (measured {RC.POISEUILLE_ERROR[case]:.6e}), Newtonian distance "
          f"{r['newtonian']:.4e}, largest shear {r['g']:.4f} g_max, tau {r['tau'][0]:.4f} .. {r['tau'][1]:.4f}")
    assert r["error"] < 0.1 * r["newtonian"]
    assert r["error"] <= RC.FACTOR * RC.POISEUILLE_ERROR[case]
    assert r["top"] == 0.0 and r["g"] < 1.0


@pytest.mark.parametrize("n", [0.5, 1.5])
def test_power_law_poiseuille_is_second_order(poiseuille_runs, n):
    ratio = poiseuille_runs[(16, n)]["error"] / poiseuille_runs[(32, n)]["error"]
    want = RC.POISEUILLE_ERROR[(16, n)] / RC.POISEUILLE_ERROR[(32, n)]
    print(f"power-law Poiseuille n = {n}: error ratio H 16 / H 32 = {ratio:.4f} (measured {want:.4f})")
    assert abs(ratio / want - 1.0) <= RC.RATIO_TOL and ratio > 3.0


# ---- 6. Couette ----------------------------------------------------------------------------------------------------------------------------
def test_couette_flow_has_the_law_s_tau_in_every_cell():
    """The shear rate is U / H everywhere, so every interior tau is 1/2 + 3 nu(U / H) of the law; the margin is twice what the reference
    measured (tests/rheology_cases.py)."""
    o, tau, prof = RC.couette_reference()
    e = float(np.abs(o.tau[1:-1, 1:-1] / tau - 1.0).max())
    print(f"Couette with a power-law table: tau error {e:.6e} (measured {RC.COUETTE_TAU_ERR:.2e}), tau = {tau:.6f}")
    assert e <= RC.FACTOR * RC.COUETTE_TAU_ERR
    assert float(np.abs(o.u[0][1:-1, 1:-1] - prof[None, 1:-1]).max()) / RC.COUETTE_U < 1e-4      # (the profile stays linear)
    top, _ = RC.coverage(o)
    assert top == 0.0


# ---- 7. the front ends on the stand-in -------------------------------------------------------------------------------------------------------
def test_run_cavity_and_run_poiseuille_through_the_stand_in(capsys):
    law = RH.power_law(0.01, 0.7)
    spec = dict(law=law, g_max=0.1, entries=64, magic=3.0 / 16.0)
    res = MG.run_cavity(maxIt=41, Re=100.0, RT="TRT", turb=0, xsize=16, ysize=16, Pinterval=20, SavePlot=False, SaveVTK=False, dtype=np.float64,
                        BC="BB", solver_factory=RheologySolver, rheology=spec)
    j = RheologySolver.journal
    calls = [c for c in j if c[0] == "set_rheology"]
    w, wm = RH.table(law, 64, 0.1, magic=3.0 / 16.0)
    assert len(calls) == 1 and np.array_equal(calls[0][1], w) and np.array_equal(calls[0][2], wm) and calls[0][3] == 0.1
    assert j[0][1]["solid"] == 0 and [c[0] for c in j].count("get_shear") == 3      # (an empty mask; one look per output iteration)
    out = capsys.readouterr().out
    assert "Rheology table is on" in out and "warning" not in out and not res.diverged
    # under MRT the magic parameter reaches no second table; a g_max far too small warns at every output iteration
    MG.run_cavity(maxIt=21, Re=100.0, RT="MRT", turb=0, xsize=16, ysize=16, Pinterval=10, SavePlot=False, SaveVTK=False, dtype=np.float64,
                  BC="BB", solver_factory=RheologySolver, rheology=dict(law=law, g_max=1e-6, entries=8, magic=3.0 / 16.0))
    calls = [c for c in RheologySolver.journal if c[0] == "set_rheology"]
    assert calls[0][2] is None and calls[0][1].shape == (8,)
    out = capsys.readouterr().out
    assert out.count("exceeds the rheology table's g_max 1e-06") == 3
    with pytest.raises(ValueError, match="pass BC='BB'"):
        MG.run_cavity(maxIt=1, xsize=16, ysize=16, turb=0, solver_factory=RheologySolver, rheology=spec)
    with pytest.raises(ValueError, match="excludes"):
        MG.run_cavity(maxIt=1, xsize=16, ysize=16, turb=0, BC="BB", subgrid=0.025, solver_factory=RheologySolver, rheology=spec)
    # the periodic channel, in pieces, with a table it leaves: one warning per piece
    K, F, gw = RH.power_law_channel(8, 0.5, 0.05, 0.05)
    r = periodic.run_poiseuille(4, 10, 0.05, F, steps=300, solver_factory=RheologySolver, output_every=100,
                                rheology=dict(law=RH.power_law(K, 0.5), power=(K, 0.5), g_max=0.1 * gw, entries=32, magic=3.0 / 16.0))
    calls = [c for c in RheologySolver.journal if c[0] == "set_rheology"]
    w, wm = RH.table(RH.power_law(K, 0.5), 32, 0.1 * gw, magic=3.0 / 16.0)
    assert np.array_equal(calls[0][1], w) and np.array_equal(calls[0][2], wm) and r["g_top"] > 0.1 * gw
    assert capsys.readouterr().out.count("warning: the largest shear") == 3


def test_command_lines_pass_the_law_through(monkeypatch):
    seen = {}
    monkeypatch.setattr(channel, "run_channel", lambda *a, **kw: seen.update(kw))
    channel.main(["--xsize", "64", "--ysize", "32", "--power-law", "0.01", "0.7", "--g-max", "0.05"])
    w, wm, g_max = RH.resolve(seen["rheology"], "TRT")
    want = RH.table(RH.power_law(0.01, 0.7), 4096, 0.05, magic=3.0 / 16.0)
    assert g_max == 0.05 and np.array_equal(w, want[0]) and np.array_equal(wm, want[1])
    assert RH.resolve(seen["rheology"], "MRT")[1] is None
    channel.main(["--xsize", "64", "--ysize", "32", "--carreau", "0.1", "0.01", "50", "0.5"])
    w, _, g_max = RH.resolve(seen["rheology"], "MRT")
    assert g_max == RH.G_MAX_DEFAULT and np.array_equal(w, RH.table(RH.carreau(0.1, 0.01, 50.0, 0.5), 4096, RH.G_MAX_DEFAULT)[0])
    with pytest.raises(SystemExit):
        channel.main(["--power-law", "0.01", "0.7", "--subgrid", "0.025"])
    monkeypatch.setattr(periodic, "run_poiseuille", lambda *a, **kw: seen.update(kw))
    periodic.main(["poiseuille", "--power-law", "0.02", "0.5"])
    assert seen["rheology"]["power"] == (0.02, 0.5) and seen["rheology"]["g_max"] == RH.G_MAX_DEFAULT
    assert np.array_equal(RH.resolve(seen["rheology"], "TRT")[0], RH.table(RH.power_law(0.02, 0.5), 4096, RH.G_MAX_DEFAULT, magic=3.0 / 16.0)[0])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="excludes"):
        channel.run_channel(64, 32, 100.0, subgrid=0.025, rheology=(w, None, 0.1))
