"""CPU tests of the open boundaries (lbm_set_open_cells, lbm_set_wall_velocity): header, bindings and the sizes that must not change; the
table builders of csrc/lbm_wall_motion.hpp and csrc/lbm_wall_shape.hpp with hold cells and a wall velocity per solid cell, driven by
tests/open_flow_model.cpp, against the reference tests/open_flow_ref.py bit for bit, and the public restatement
solid.host_open_tables against both; the flux check and its waiver; the geometry of channel(); and the reference itself -- without the
two pieces it is CurvedWallOracle, a free stream started from rest becomes uniform, and a channel carries one flux through every column
with a parabolic profile.  The program is built with the host g++ (with the address and undefined-behaviour sanitizers where the compiler
has them); its tests are skipped where there is no g++."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_cases
from curved_wall_ref import CurvedWallOracle, circle_fractions
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import channel as CH
from latticeboltzmannsimulations_amd import solid
from latticeboltzmannsimulations_amd.solver import CavitySolver
from open_flow_ref import OpenFlowOracle, feq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")
NX, NY = 72, 40


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_four_calls_and_keeps_version_and_sizes():
    assert L.ABI_VERSION == 4 and ctypes.sizeof(L.lbm_params) == 18 * 4 + 6 * 8
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert lib.lbm_abi_version() == 4 and "#define LBM_ABI_VERSION 4" in text
    for n in ("lbm_set_open_cells", "lbm_get_open_cells", "lbm_set_wall_velocity", "lbm_get_wall_velocity"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert sorted(L.SIGNATURES) == sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", hdr)))      # (the two lists stay equal)
    assert "open_cells=1" in text and "wall_velocity=1" in text and "(6 w_k) (cx_k uwx(S) + cy_k uwy(S))" in text
    a = np.zeros(4)
    assert lib.lbm_set_open_cells(None, None, None) == -1 and lib.lbm_get_open_cells(None, None, None) == -1
    assert lib.lbm_set_wall_velocity(None, a.ctypes.data) == -1 and lib.lbm_get_wall_velocity(None, a.ctypes.data) == -1
    for name in ("set_open_cells", "open_cells", "set_wall_velocity", "wall_velocity"):
        assert hasattr(CavitySolver, name), name
    import inspect
    assert "open" not in " ".join(inspect.signature(CavitySolver.__init__).parameters)      # (no new keyword: the stand-ins mirror it)


# ---- the table builder -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    tmp = tmp_path_factory.mktemp("open")
    exe = str(tmp / "open_flow_model")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "open_flow_model.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)     # (a compiler without the sanitizers' runtimes)

    def run(mask, labels, centres, motion, hold=None, uw=None, q=None, f32=False):
        path = str(tmp / "case.txt")
        hx = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())      # noqa: E731
        with open(path, "w") as f:
            f.write(f"{mask.shape[0]} {mask.shape[1]} {len(centres)} {int(uw is not None)} {int(q is not None)}\n")
            for a in (mask, labels, np.zeros(mask.shape, bool) if hold is None else hold):
                f.write(" ".join(str(int(v)) for v in np.asarray(a).ravel()) + "\n")
            for c, m in zip(centres, motion):
                f.write(hx(list(c) + list(m)) + "\n")
            for a in (uw, q):
                if a is not None:
                    f.write(hx(a) + "\n")
        out = {}
        for line in subprocess.run([exe, path, str(int(f32))], check=True, capture_output=True, text=True).stdout.splitlines():
            w = line.split()
            out.setdefault(w[0], []).append(w[1:])
        return out
    return run


def _case(name):
    """(mask, labels, nbodies, hold): a body_cases mask with hold cells beside solid cells, in column 0 and in the interior."""
    mask, labels, nb = body_cases.cases(NX, NY)[name]
    lab = body_cases.labels_of(mask, labels)
    hold = np.zeros((NX, NY), bool)
    hold[NX - 1, 3:NY - 3] = True
    hold[0, 20:24] = True
    hold[40:44, 25] = True
    free = np.argwhere(~mask)
    sel = np.random.default_rng(3).choice(len(free), 60, replace=False)
    hold[free[sel, 0], free[sel, 1]] = True
    near = np.argwhere(np.any(solid.links(mask), axis=0))[::5]                 # every fifth fluid cell that has a link: beside a solid cell
    hold[near[:, 0], near[:, 1]] = True
    hold &= ~mask
    return mask, lab, nb, hold


def _uw(mask, seed):
    return np.where(mask[None], np.random.default_rng(seed).uniform(-0.05, 0.05, (2,) + mask.shape), 0.0)


def _motions(nb, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.01, 0.01, nb)], axis=1)


@pytest.mark.parametrize("name", ["two_blocks", "walls", "random", "ring"])
def test_builder_equals_the_reference_bit_for_bit(builder, name):
    """The link list without the links that start at a hold cell; delta with the cell term in double and rounded to float; the rows of
    the table; with a shape the a, d, near and effective q, a hold cell counting as no fluid cell behind a link.  The public
    restatement solid.host_open_tables says the same."""
    mask, lab, nb, hold = _case(name)
    cen = solid.centroids(mask, lab, nb)
    mot, uw = _motions(nb, 11), _uw(mask, 12)
    q = 1.0 - np.random.default_rng(13).random((8, NX, NY))
    for with_motion in (False, True):
        m_ = mot if with_motion else np.zeros((nb, 3))
        o = OpenFlowOracle(NX, NY, 100.0, mask=mask, labels=lab, centres=cen, motion=m_, hold=hold, f=feq(1.0, 0.02 * np.ones((NX, NY)), 0.0),
                           wall_velocity=uw)
        assert o.links and not any(hold[x, y] for x, y, _, _ in o.links)
        assert len(o.links) < len(CurvedWallOracle(NX, NY, 100.0, mask=mask, labels=lab, centres=cen).links)      # (some were dropped)
        for f32 in (False, True):
            got = builder(mask, np.where(mask, lab, 0), cen, m_, hold, uw, q, f32)
            assert [tuple(int(v) for v in l) for l in got["link"]] == o.links, name
            assert got["refusal"][0][0] == "0"                                  # (open: whatever S is)
            rnd = (lambda d: float(np.float32(d))) if f32 else float
            assert [float.fromhex(v[0]) for v in got["ld"]] == [rnd(d) for d in o.delta64], (name, f32)
            dd = {(x, y, k): rnd(d) for (x, y, k, _), d in zip(o.links, o.delta64)}
            cells = got["cell"]
            assert sorted((int(c[1]), int(c[0])) for c in cells) == sorted({(y, x) for x, y, _, _ in o.links})
            for c in cells:
                x, y = int(c[0]), int(c[1])
                assert [float.fromhex(v) for v in c[3:]] == [dd.get((x, y, k), 0.0) for k in range(1, 9)], (name, x, y)
            # the shape's table of the same lattice
            os_ = OpenFlowOracle(NX, NY, 100.0, mask=mask, labels=lab, centres=cen, motion=m_, q=q, hold=hold,
                                 f=feq(1.0, 0.02 * np.ones((NX, NY)), 0.0), wall_velocity=uw, dtype=np.float32 if f32 else np.float64)
            assert [float.fromhex(v[0]) for v in got["lq"]] == os_.l_q.tolist()
            fig = {(x, y, k): (float(a), float(d), bool(n)) for (x, y, k, _), a, d, n in zip(os_.links, os_.l_a, os_.l_d, os_.l_near)}
            for r in got["srow"]:
                x, y, near = int(r[0]), int(r[1]), int(r[3])
                vals = [float.fromhex(v) for v in r[4:]]
                for k in range(1, 9):
                    a, d, n = fig.get((x, y, k), (1.0, 0.0, False))
                    assert (vals[k - 1], vals[8 + k - 1], bool((near >> (k - 1)) & 1)) == (a, d, n), (name, x, y, k)
            t = solid.host_open_tables(mask, lab, cen, m_, uw, hold, q, np.float32 if f32 else None)
            assert [tuple(r) for r in t["links"].tolist()] == o.links and t["delta"].tolist() == [rnd(d) for d in o.delta64]
            assert t["S"] == o.S and t["A"] == o.A and t["closed"] and t["q"].tolist() == os_.l_q.tolist()
            assert t["a"].tolist() == [float(v) for v in os_.l_a] and t["d"].tolist() == [float(v) for v in os_.l_d]
            assert t["near"].tolist() == os_.l_near.tolist()
    # a hold cell behind a link is no fluid cell: somewhere the fallback to q = 1/2 applies because of one
    plain = CurvedWallOracle(NX, NY, 100.0, mask=mask, labels=lab, centres=cen, q=q)
    eff = {(x, y, k): v for (x, y, k, _), v in zip(plain.links, plain.l_q)}
    assert name != "random" or any(eff[(x, y, k)] != v for (x, y, k, _), v in zip(os_.links, os_.l_q))


def test_flux_check_is_waived_exactly_when_the_lattice_has_a_hold_cell(builder):
    m = np.zeros((NX, NY), bool)
    m[0, :] = True                                                             # an inlet column with a wall-normal velocity: a net inflow
    lab = np.zeros((NX, NY), np.int32)
    cen, rest = [[0.0, 0.0]], np.zeros((1, 3))
    uw = np.zeros((2, NX, NY))
    uw[0, 0, :] = 0.03
    o = OpenFlowOracle(NX, NY, 100.0, mask=m, wall_velocity=uw)
    got = builder(m, lab, cen, rest, None, uw)
    assert got["refusal"][0][0] == "1" and "ld" not in got and not o.closed() and abs(o.S) > 0.01
    assert float.fromhex(got["refusal"][0][2]) == o.S and float.fromhex(got["refusal"][0][3]) == o.A and int(got["refusal"][0][4]) == len(o.links)
    t = solid.host_open_tables(m, lab, cen, rest, uw)
    assert not t["closed"] and t["S"] == o.S and t["A"] == o.A
    hold = np.zeros((NX, NY), bool)
    hold[NX - 1, 5] = True                                                     # one hold cell opens the lattice
    oh = OpenFlowOracle(NX, NY, 100.0, mask=m, hold=hold, f=feq(1.0, 0.03 * np.ones((NX, NY)), 0.0), wall_velocity=uw)
    got = builder(m, lab, cen, rest, hold, uw)
    assert got["refusal"][0][0] == "0" and oh.closed() and len(got["ld"]) == len(oh.links)
    assert solid.host_open_tables(m, lab, cen, rest, uw, hold)["closed"]
    belt = np.zeros((2, NX, NY))
    belt[1, 0, :] = 0.04                                                       # the same column sliding along itself: tangential, closed
    ob = OpenFlowOracle(NX, NY, 100.0, mask=m, wall_velocity=belt)
    got = builder(m, lab, cen, rest, None, belt)
    assert got["refusal"][0][0] == "0" and ob.closed() and any(float.fromhex(v[0]) != 0.0 for v in got["ld"])
    # a body's normal motion cancelled by its cells' own velocity: the one table holds both, and S is formed from the sum
    both = np.zeros((2, NX, NY))
    both[0, 0, :] = -0.03
    oc = OpenFlowOracle(NX, NY, 100.0, mask=m, motion=[[0.03, 0.0, 0.0]], wall_velocity=both)
    got = builder(m, lab, oc.centres, oc.motion, None, both)
    assert got["refusal"][0][0] == "0" and oc.closed() and all(float.fromhex(v[0]) == 0.0 for v in got["ld"])
    assert builder(m, lab, oc.centres, oc.motion)["refusal"][0][0] == "1"       # (the motion alone is refused as before)


def test_defaults_leave_the_tables_of_the_parent(builder):
    """Without hold cells and without a velocity the builders give what they gave: the list and the deltas of MovingWallOracle."""
    from moving_wall_ref import MovingWallOracle
    mask, labels, nb = body_cases.cases(NX, NY)["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    cen, mot = solid.centroids(mask, lab, nb), _motions(nb, 5)
    o = MovingWallOracle(NX, NY, 100.0, mask=mask, labels=lab, centres=cen, motion=mot)
    got = builder(mask, np.where(mask, lab, 0), cen, mot)
    assert [tuple(int(v) for v in l) for l in got["link"]] == o.links and [float.fromhex(v[0]) for v in got["ld"]] == o.delta64
    assert float.fromhex(got["refusal"][0][2]) == 0.0                         # (S is reported only with a refusal)


# ---- channel() -----------------------------------------------------------------------------------------------------------------------
def test_channel_geometry():
    nx, ny, um = 64, 34, 0.05
    g = CH.channel(nx, ny, um)
    m, lab = g["solid"], g["labels"]
    assert m[:, 0].all() and m[:, ny - 1].all() and m[0, :].all() and not m[1:, 1:ny - 1].any()
    assert (lab[1:, 0] == 0).all() and (lab[:, ny - 1] == 0).all() and (lab[0, 1:ny - 1] == 1).all() and (lab[~m] == -1).all() and g["nbodies"] == 2
    assert g["hold"][nx - 1, 1:ny - 1].all() and g["hold"].sum() == ny - 2 and not (g["hold"] & m).any()
    p = g["profile"]
    y = np.arange(ny)
    assert p[0] == p[ny - 1] == 0.0
    # the parabola vanishes half a cell outside rows 1 and ny - 2, and peaks at umax in the middle
    par = lambda t: um * 4.0 * (t - 0.5) * (ny - 1.5 - t) / (ny - 2.0) ** 2      # noqa: E731
    assert par(0.5) == 0.0 and par(ny - 1.5) == 0.0 and np.array_equal(p[1:ny - 1], par(y[1:ny - 1].astype(float)))
    assert abs(par((ny - 1) / 2.0) - um) < 1e-15 and abs(g["mean"] - 2.0 / 3.0 * um) < um / (ny - 2) ** 2
    uw = g["wall_velocity"]
    assert np.array_equal(uw[0, 0, :], p) and not uw[1].any() and not uw[0, 1:, :].any()
    assert np.array_equal(g["f"], solid.equilibrium(1.0, np.broadcast_to(p[None, :], (nx, ny)), 0.0))
    assert np.array_equal(solid.equilibrium(1.0, 0.03, -0.01), feq(1.0, 0.03, -0.01)) and abs(solid.equilibrium(1.2, 0.03, 0.01).sum() - 1.2) < 1e-15
    s = CH.channel(nx, ny, um, profile="plug", walls="stream")
    assert (s["wall_velocity"][0, :, 0] == um).all() and (s["wall_velocity"][0, :, ny - 1] == um).all() and (s["profile"][1:ny - 1] == um).all()
    d = CH.channel(nx, ny, um, disc=(20, 16.5, 4.0), curved=True)
    disc = d["solid"] & ~m
    assert disc.sum() > 30 and (d["labels"][disc] == 2).all() and d["nbodies"] == 3 and d["shape"].shape == (8, nx, ny)
    q = d["shape"]
    ln = solid.body_links(d["solid"], d["labels"])
    on_disc = ln[ln[:, 3] == 2]
    assert (q[on_disc[:, 2] - 1, on_disc[:, 0], on_disc[:, 1]] != 0.5).any() and ((q > 0) & (q <= 1)).all()
    off = ln[ln[:, 3] != 2]
    assert (q[off[:, 2] - 1, off[:, 0], off[:, 1]] == 0.5).all()
    assert abs(CH.solver_re(20.0, 20.0, 0.05, 2.0 / 3.0 * 0.05, 84) - 0.05 * 84 / (2.0 / 3.0 * 0.05 * 20.0 / 20.0)) < 1e-9
    with pytest.raises(ValueError):
        CH.channel(nx, ny, um, disc=(nx - 1, 16, 3.0))


def test_run_channel_through_a_stand_in(capsys):
    """The driver sets the geometry first, then the shape, then the velocities, and reads the obstacle's force from the series."""
    calls = []

    class StandIn:
        def __init__(self, nx, ny, Re, **kw):
            calls.append(("create", nx, ny, Re, kw["uLB"], kw["semantics"], kw["solid"].sum(), int(kw["bodies"].max())))

        def __enter__(self):
            return self

        def __exit__(self, *a):
            pass

        def __getattr__(self, name):
            def f(*a, **k):
                calls.append((name,) + tuple(v for v in a if np.isscalar(v)) + tuple(sorted(k.items())))
                if name == "force_series":
                    return dict(fx=np.array([[0.0, 0.0, 0.125]]), fy=np.array([[0.0, 0.0, -0.25]]))
                return self
            return f
    r = CH.run_channel(64, 34, 20.0, umax=0.05, disc=(20, 16.5, 4.0), curved=True, steps=50, force_every=10, solver_factory=StandIn)
    names = [c[0] for c in calls]
    assert names == ["create", "set_open_cells", "set_shape", "set_wall_velocity", "step", "begin_force", "step", "sample_force", "force_series", "end_force"]
    mean, D = CH.channel(64, 34, 0.05)["mean"], 8.0
    assert r["Cd"] == 2.0 / (mean ** 2 * D) * 0.125 and r["Cl"] == 2.0 / (mean ** 2 * D) * -0.25
    assert abs(mean * D / r["nu"] - 20.0) < 1e-12 and abs(calls[0][3] - 0.05 * 34 / r["nu"]) < 1e-9
    out = capsys.readouterr().out
    assert "Re_D = 20" in out and "the solver's Re" in out and "Cd" in out


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_without_the_two_pieces_the_reference_is_the_curved_wall_oracle(coll):
    mask, labels, nb = body_cases.cases(NX, NY)["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    q = circle_fractions(mask, 11.0, [3.3])
    for dt in (np.float32, np.float64):
        for kw in (dict(), dict(motion=_motions(nb, 4)), dict(q=q, motion=_motions(nb, 4))):
            a = CurvedWallOracle(NX, NY, 100.0, mask=mask, labels=lab, collision=coll, dtype=dt, **kw).step(12)
            b = OpenFlowOracle(NX, NY, 100.0, mask=mask, labels=lab, collision=coll, dtype=dt, **kw).step(12)
            assert np.array_equal(a.fin, b.fin) and np.array_equal(a.u, b.u) and np.array_equal(a.rho, b.rho)
            assert a.body_force()["fx"].tolist() == b.body_force()["fx"].tolist()


def test_hold_cells_keep_their_values_and_feed_their_neighbours():
    mask, lab, nb, hold = _case("two_blocks")
    f = feq(1.03, 0.02 * np.ones((NX, NY)), -0.01)
    o = OpenFlowOracle(NX, NY, 100.0, mask=mask, labels=lab, hold=hold, f=f, collision="TRT").step(9)
    assert np.array_equal(o.fin[:, hold], f[:, hold]) and np.array_equal(o.fpost[:, hold], f[:, hold])
    assert not hold[44, 25] and not mask[44, 25] and o.fin[1, 44, 25] == f[1, 43, 25]      # slot 1 pulls from (x - 1, y), a hold cell
    assert not hold[41, 24] and not mask[41, 24] and o.fin[2, 41, 24] == f[2, 41, 25]      # slot 2 pulls from (x, y + 1)
    assert np.array_equal(o.rho[hold], o.macros(f)[0][hold])
    o.set_state(np.ascontiguousarray(np.broadcast_to(o.t[:, None, None], (9, NX, NY))))
    assert np.array_equal(o.fin[:, hold], f[:, hold])                           # (a set_state pins them again)


# (a) a free stream started from rest becomes uniform; (b) a channel carries one flux and a parabola.  Measured on this reference, fp64
# (DESIGN.md 2.10); the tests assert FREE_FACTOR / FLUX_FACTOR / PROFILE_FACTOR times these and nothing wider: the residue of the free
# stream decays about 5x per 500 steps, so 10x is less than one more block of steps; a wrong inlet rule shows as a profile error >= 0.1.
FREE_STREAM = {"TRT": (1.7237830561567247e-06, 1.1949157530320786e-05), "SRT": (2.389982731165752e-07, 4.6686652957808543e-07)}
CHANNEL_FLUX_SPREAD, CHANNEL_PROFILE_ERR = 9.153486140176345e-07, 0.0023234875175591474
FREE_FACTOR, FLUX_FACTOR, PROFILE_FACTOR = 10.0, 10.0, 2.0


@pytest.mark.parametrize("coll", ["TRT", "SRT"])
def test_free_stream_from_rest_becomes_uniform(coll):
    """40 x 24: the inlet column and both side rows are solid with the wall velocity (U, 0), the outlet column is held at feq(1, U, 0);
    U = 0.05, nu = U ysize / Re with Re = 100; 3000 steps from rest."""
    nx, ny, U = 40, 24, 0.05
    g = CH.channel(nx, ny, U, profile="plug", walls="stream")
    o = OpenFlowOracle(nx, ny, 100.0, uLB=U, mask=g["solid"], hold=g["hold"], f=g["f"], wall_velocity=g["wall_velocity"], collision=coll, dtype=np.float64)
    o.step(3000)
    fl = o.fluid()
    ex, ey = float(np.abs(o.u[0][fl] - U).max() / U), float(np.abs(o.u[1][fl]).max() / U)
    print(f"free stream {coll}: max|ux - U|/U = {ex!r} (measured {FREE_STREAM[coll][0]!r}), max|uy|/U = {ey!r} (measured {FREE_STREAM[coll][1]!r})")
    assert ex <= FREE_FACTOR * FREE_STREAM[coll][0] and ey <= FREE_FACTOR * FREE_STREAM[coll][1]


def test_channel_carries_one_flux_and_a_parabola():
    """64 x 34, walls at rest, a parabolic wall velocity on the inlet column, the outlet held at feq(1, parabola); umax = 0.05, Re 100,
    TRT, 4000 steps: the mass flux through columns 1, nx / 2 and nx - 2, and the profile at 3 nx / 4."""
    nx, ny, um = 64, 34, 0.05
    g = CH.channel(nx, ny, um)
    o = OpenFlowOracle(nx, ny, 100.0, uLB=um, mask=g["solid"], hold=g["hold"], f=g["f"], wall_velocity=g["wall_velocity"], collision="TRT", dtype=np.float64)
    o.step(4000)
    flux = [float((o.rho[c, 1:ny - 1] * o.u[0][c, 1:ny - 1]).sum()) for c in (1, nx // 2, nx - 2)]
    spread = (max(flux) - min(flux)) / float(np.mean(flux))
    err = float(np.abs(o.u[0][3 * nx // 4, 1:ny - 1] - g["profile"][1:ny - 1]).max() / um)
    print(f"channel: flux spread {spread!r} (measured {CHANNEL_FLUX_SPREAD!r}), profile error at 3nx/4 {err!r} (measured {CHANNEL_PROFILE_ERR!r})")
    assert spread <= FLUX_FACTOR * CHANNEL_FLUX_SPREAD and err <= PROFILE_FACTOR * CHANNEL_PROFILE_ERR
    assert min(flux) > 0.5 * um * (ny - 2) * 2.0 / 3.0
