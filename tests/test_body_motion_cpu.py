"""CPU tests of the wall velocity on solid bodies (lbm_set_body_motion): the table builder of csrc/lbm_wall_motion.hpp, driven by
tests/wall_motion_model.cpp, against the NumPy restatement of tests/moving_wall_ref.py bit for bit; the flux check; header, bindings and
the sizes that must not change; the dry-run plans; the front end, its messages and the checkpoint through stand-ins; and the reference
itself -- zero motion is SolidOracle, the fluid mass stays, and the annulus between a rotating disc and a ring at rest is Taylor-Couette
flow, whose torque and profile are known in closed form.  The program is built with the host g++ (with the address and
undefined-behaviour sanitizers where the compiler has them); its tests are skipped where there is no g++."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_cases
import body_force_standin
from body_cases import TC_FACTOR, TC_N, TC_PROFILE_ERR, TC_RE, TC_STEPS, TC_TORQUE_ERR, tc_case, tc_errors
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import launch_plan, mrt_gpu, solid
from latticeboltzmannsimulations_amd.solver import CavitySolver
from moving_wall_ref import MovingWallOracle
from solid_ref import SolidOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")

@pytest.fixture(scope="module")
def tc_reference():
    case = tc_case()
    o = MovingWallOracle(TC_N, TC_N, TC_RE, mask=case["mask"], labels=case["labels"], centres=case["centres"], motion=case["motion"],
                         collision="TRT", dtype=np.float64)
    m0 = o.fluid_mass()
    o.step(TC_STEPS)
    return o, case, m0


# ---- the table builder -----------------------------------------------------------------------------------------------------------------
def _build(tmp, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp / name)
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)     # (a compiler without the sanitizers' runtimes)
    return exe


@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("motion")
    exe = _build(tmp, "wall_motion_model")

    def run(mask, labels, centres, motion):
        path = str(tmp / "case.txt")
        nb = len(centres)
        with open(path, "w") as f:
            f.write(f"{mask.shape[0]} {mask.shape[1]} {nb}\n")
            f.write(" ".join(str(int(v)) for v in mask.ravel()) + "\n" + " ".join(str(int(v)) for v in labels.ravel()) + "\n")
            for c, m in zip(centres, motion):
                f.write(" ".join(float(v).hex() for v in list(c) + list(m)) + "\n")
        out = {}
        for line in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines():
            w = line.split()
            out.setdefault(w[0], []).append(w[1:])
        return out
    return run


def two_bodies_one_cell(nx=72, ny=40):
    """A fluid cell between two bodies with different motions: its links belong to both."""
    m = np.zeros((nx, ny), dtype=bool)
    lab = np.full((nx, ny), -7, dtype=np.int32)
    m[20:23, 10:14] = True; lab[20:23, 10:14] = 0
    m[24:27, 10:14] = True; lab[24:27, 10:14] = 1
    return m, lab, 2


def _motions(nb, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.01, 0.01, nb)], axis=1)


def test_builder_equals_the_numpy_restatement_bit_for_bit(builder):
    """delta of every link in list order, its float rounding, S, A, the verdict of the flux check and the per-cell table (row numbers
    continue a batch's, slot k - 1 holds link k, zero elsewhere)."""
    cases = dict(body_cases.cases(72, 40))
    cases["between"] = two_bodies_one_cell()
    for name, (mask, labels, nb) in cases.items():
        lab = body_cases.labels_of(mask, labels)
        cen = solid.centroids(mask, lab, nb)
        mot = _motions(nb, 11)
        o = MovingWallOracle(72, 40, 100.0, mask=mask, labels=lab, centres=cen, motion=mot)
        got = builder(mask, np.where(mask, lab, 0), cen, mot)
        links = got.get("link", [])
        assert [tuple(int(v) for v in l[:4]) for l in links] == o.links, name
        assert [float.fromhex(l[4]) for l in links] == o.delta64, name
        assert [float.fromhex(l[5]) for l in links] == [float(np.float32(d)) for d in o.delta64], name
        assert float.fromhex(got["S"][0][0]) == o.S and float.fromhex(got["A"][0][0]) == o.A, name
        assert int(got["closed"][0][0]) == int(o.closed()), name
        ln, d = solid.wall_deltas(mask, lab, cen, mot)                       # the public restatement says the same
        assert [tuple(r) for r in ln.tolist()] == o.links and d.tolist() == o.delta64, name
        o32 = MovingWallOracle(72, 40, 100.0, mask=mask, labels=lab, centres=cen, motion=mot, dtype=np.float32)
        assert o32.delta.dtype == np.float32 and np.array_equal(solid.wall_delta_field(mask, lab, cen, mot, np.float32), o32.delta.astype(np.float64)), name
        cells = got.get("cell", [])
        want_cells = sorted({(y, x) for x, y, _, _ in o.links})
        assert [(int(c[1]), int(c[0])) for c in cells] == want_cells and int(got["rows"][0][0]) == len(want_cells), name
        rows = sorted(int(c[2]) for c in cells)
        assert rows == list(range(5, 5 + len(cells))), name
        dd = {(x, y, k): d for (x, y, k, _), d in zip(o.links, o.delta64)}
        for c in cells:
            x, y = int(c[0]), int(c[1])
            assert [float.fromhex(v) for v in c[3:]] == [dd.get((x, y, k), 0.0) for k in range(1, 9)], (name, x, y)
    m, lab, _ = cases["between"]
    o = MovingWallOracle(72, 40, 100.0, mask=m, labels=lab, motion=[[0.01, 0.0, 0.0], [-0.02, 0.0, 0.0]])
    both = {b for x, y, k, b in o.links if (x, y) == (23, 11)}
    assert both == {0, 1} and o.delta[1, 23, 11] != 0.0 and o.delta[3, 23, 11] != 0.0


def _block(nx=72, ny=40, box=(30, 38, 14, 22)):
    m = np.zeros((nx, ny), dtype=bool)
    m[box[0]:box[1], box[2]:box[3]] = True
    return m


def test_flux_check_accepts_what_conserves_mass_and_refuses_what_leaks(builder):
    def closed(mask, labels, motion, centres=None):
        nb = len(motion)
        cen = solid.centroids(mask, labels, nb) if centres is None else centres
        o = MovingWallOracle(mask.shape[0], mask.shape[1], 100.0, mask=mask, labels=labels, centres=cen, motion=motion)
        got = builder(mask, np.where(mask, labels, 0), cen, np.asarray(motion, dtype=np.float64))
        assert int(got["closed"][0][0]) == int(o.closed())
        return o.closed(), o
    zero = np.zeros((72, 40), dtype=np.int32)
    for mot in ([[0.05, -0.03, 0.004]], [[0.0, 0.0, -0.01]], [[0.1, 0.1, 0.0]], [[1e-9, 3.0, 0.25]]):          # a block clear of the edge: any motion
        ok, o = closed(_block(), zero, mot)
        assert ok and abs(o.S) < 1e-15 * max(o.A, 1.0), mot
    belt = np.zeros((72, 40), dtype=bool); belt[0:2, 8:30] = True                   # a belt on the left wall: tangential motion
    assert closed(belt, zero, [[0.0, 0.04, 0.0]])[0]
    lidbelt = np.zeros((72, 40), dtype=bool); lidbelt[20:50, 0] = True              # ... and one in the lid row
    assert closed(lidbelt, zero, [[-0.03, 0.0, 0.0]])[0]
    xs, ys = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    ring = np.hypot(xs - 23.5, ys - 23.5) > 20.6                                   # a rotating ring that touches the whole perimeter
    assert closed(ring, np.zeros((48, 48), dtype=np.int32), [[0.0, 0.0, 0.002]], centres=[[23.5, 23.5]])[0]
    wall = np.zeros((72, 40), dtype=bool); wall[0:4, 10:20] = True                  # a block on the left wall, wall-normal velocity: pumps
    ok, o = closed(wall, zero, [[0.03, 0.0, 0.0]])
    assert not ok and abs(o.S) > 0.01
    m, lab, _ = two_bodies_one_cell()                                               # two touching bodies with different U
    m[23, 10:14] = True; lab[23, 10:14] = 0
    assert not closed(m, np.where(m, lab, 0), [[0.02, 0.0, 0.0], [-0.01, 0.0, 0.0]])[0]
    assert closed(m, np.where(m, lab, 0), [[0.02, 0.01, 0.0], [0.02, 0.01, 0.0]])[0]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_two_calls_and_keeps_version_and_sizes():
    assert L.ABI_VERSION == 4 and ctypes.sizeof(L.lbm_params) == 18 * 4 + 6 * 8
    assert ctypes.sizeof(L.lbm_body_force_record) == 48 and ctypes.sizeof(L.lbm_solid_force_record) == 32
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert lib.lbm_abi_version() == 4 and "#define LBM_ABI_VERSION 4" in text
    for n in ("lbm_set_body_motion", "lbm_get_body_motion"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert "delta = (6 w_k) (cx_k uwx + cy_k uwy)" in text and "wall_motion=1" in text
    m = np.zeros(3)
    assert lib.lbm_set_body_motion(None, m.ctypes.data) == -1 and lib.lbm_get_body_motion(None, m.ctypes.data) == -1


def test_launch_plans_do_not_change():
    """The motion is run state, not plan: the dry-run texts of a mask's plans hold no word of it (tests/test_launch_plans.py pins the
    plain parameters against its golden file)."""
    for size, dt in (((72, 40), np.float32), ((70, 66), np.float32), ((1032, 8), np.float32), ((520, 8), np.float64)):
        p = launch_plan(*size, 100.0, steps=37, dtype=dt, semantics="bounce_back", solid=True)
        assert p["units"] == [1] * 37 and not any("motion" in str(k) or "wall_motion" in str(v) for k, v in p.items())
        assert p["kernel"] == "k_step_solid" if size != (70, 66) else p["kernel"] == "k_step_generic"


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_zero_motion_is_the_solid_oracle(coll):
    mask, labels, nb = body_cases.cases(72, 40)["two_blocks"]
    for dt in (np.float32, np.float64):
        a = SolidOracle(72, 40, 100.0, mask=mask, collision=coll, dtype=dt).step(20)
        for mot in (None, np.zeros((nb, 3))):
            b = MovingWallOracle(72, 40, 100.0, mask=mask, labels=body_cases.labels_of(mask, labels), motion=mot, collision=coll, dtype=dt).step(20)
            assert np.array_equal(a.fin, b.fin) and np.array_equal(a.u, b.u) and np.array_equal(a.rho, b.rho)
            Fa, Fb = a.force(), b.force()
            assert all(Fa[k] == Fb[k] for k in Fa)


def test_fluid_mass_of_the_reference_stays_under_a_motion():
    """About 32 roundings of 2^-53 per cell and step: a relative drift of at most steps * 2^-48.  One leaking link would be 1e-7 a step."""
    mask, labels, nb = body_cases.cases(72, 40)["two_blocks"]
    steps = 400
    o = MovingWallOracle(72, 40, 100.0, mask=mask, labels=body_cases.labels_of(mask, labels), motion=[[0.03, -0.02, 0.004], [0.0, 0.01, -0.006]],
                         collision="TRT", dtype=np.float64)
    assert o.closed()
    m0 = o.fluid_mass()
    o.step(steps)
    drift = abs(o.fluid_mass() - m0) / m0
    print(f"mass drift after {steps} steps: {drift:.3e} (bound {steps * 2.0 ** -48:.3e})")
    assert drift <= steps * 2.0 ** -48
    assert np.abs(o.u[:, ~mask]).max() > 1e-3           # (the motion drives a flow)


def test_taylor_couette_on_the_reference(tc_reference):
    """A disc that rotates inside a ring at rest.  The staircase discs are first-order, so the bound is a measurement: the reference's
    two errors, recorded above and in DESIGN.md 2.10, times TC_FACTOR."""
    o, case, m0 = tc_reference
    assert o.closed()
    F = o.body_force()
    (e_in, e_out), e_prof = tc_errors(o.u, F["tz"], case)
    drift = abs(o.fluid_mass() - m0) / m0
    print(f"Taylor-Couette reference: torque errors {e_in:.6e} {e_out:.6e}, profile error {e_prof:.6e}, mass drift {drift:.3e}, "
          f"tz {F['tz'][0]!r} {F['tz'][1]!r}")
    assert max(e_in, e_out) <= TC_FACTOR * TC_TORQUE_ERR and e_prof <= TC_FACTOR * TC_PROFILE_ERR
    assert F["tz"][0] < 0.0 < F["tz"][1] and abs(F["tz"][0] + F["tz"][1]) <= 1e-6 * abs(F["tz"][1])
    assert drift <= TC_STEPS * 2.0 ** -48


# ---- the front end, through stand-ins ----------------------------------------------------------------------------------------------------
NX, NY = 48, 40
RUN = dict(maxIt=21, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=20, SavePlot=False, BC="BB")


def _moving_standin():
    Base = body_force_standin.make()

    class MovingStandIn(Base):
        def __init__(self, xsize, ysize, Re, solid=None, bodies=None, **kw):
            super().__init__(xsize, ysize, Re, solid=solid, bodies=bodies, **kw)
            self.o = body_force_standin._ForceTap(MovingWallOracle(xsize, ysize, Re, mask=self.mask, labels=self.labels, uLB=self.uLB,
                                                                   collision=kw.get("RT", "MRT"), dtype=np.float64), self)

        def set_body_motion(self, motion):
            self._note("set_body_motion", np.asarray(motion).tolist(), self.steps_done)
            self.o._o.set_motion(motion)
            return self

        def solid_force(self):
            F = self.o._o.force()
            self._note("solid_force", self.steps_done)
            return dict(step=self.steps_done, links=F["links"], fx=F["fx"], fy=F["fy"])
    return MovingStandIn


def _two_boxes():
    return solid.labels_from(NX, NY, [(20, 28, 14, 20), (36, 40, 6, 9)])[:2]


def test_run_cavity_sets_the_motion_before_the_first_step(capsys):
    mask, labels = _two_boxes()
    S = _moving_standin()
    mot = [[0.0, 0.0, 0.004], [0.0, 0.02, 0.0]]
    r = mrt_gpu.run_cavity(solver_factory=S, quiet=True, solid=mask, bodies=labels, body_motion=mot, **RUN)
    assert ("set_body_motion", mot, 0) in S.journal and S.journal.index(("set_body_motion", mot, 0)) < S.journal.index(("step", 1))
    want = MovingWallOracle(NX, NY, 100.0, mask=mask, labels=labels, motion=mot, collision="MRT", dtype=np.float64).step(21).force()
    assert r.forces[-1][1]["fx"] == want["fx"] and r.forces[-1][1]["fy"] == want["fy"]
    S2 = _moving_standin()
    r0 = mrt_gpu.run_cavity(solver_factory=S2, quiet=True, solid=mask, bodies=labels, **RUN)
    assert not body_force_standin.FS._entries(S2.journal, "set_body_motion") and r0.forces[-1][1]["fx"] != want["fx"]


def test_arguments_are_checked_and_reach_the_command_line(monkeypatch, capsys):
    mask, labels = _two_boxes()
    S = _moving_standin()
    mot = [[0.0, 0.0, 0.004], [0.0, 0.0, 0.0]]
    for kw, text in ((dict(body_motion=mot), "needs solid"), (dict(solid=mask, body_motion=[0.0, 0.0, 1.0]), r"\[nbodies, 3\]"),
                     (dict(solid=mask, body_motion=[[0.0, float("nan"), 0.0]]), "finite"),
                     (dict(solid=mask, solid_tiles=True, body_motion=mot), "tile kernel")):
        with pytest.raises(ValueError, match=text):
            mrt_gpu.run_cavity(solver_factory=S, quiet=True, **RUN, **kw)
    assert S.made == []
    with pytest.raises(ValueError, match="needs solid"):                       # (BB walls missing: no mask can be given, the same style)
        mrt_gpu.run_cavity(solver_factory=S, quiet=True, **dict(RUN, BC="EB-NEBB "), body_motion=mot)
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return mrt_gpu.CavityResult()
    monkeypatch.setattr(mrt_gpu, "run_cavity", fake)
    size = ["--xsize", str(NX), "--ysize", str(NY), "--turb", "0", "--BC", "BB"]
    boxes = ["--solid-box", "20", "28", "14", "20", "--solid-box", "36", "40", "6", "9"]
    assert mrt_gpu.main(size + boxes + ["--body-motion", "1", "0.01", "-0.02", "0", "--body-motion", "0", "0", "0", "0.004"]) == 0
    assert np.array_equal(seen["body_motion"], [[0.0, 0.0, 0.004], [0.01, -0.02, 0.0]]) and np.array_equal(seen["bodies"], labels)
    assert np.array_equal(seen["solid"], mask) and "force_every" not in seen
    seen.clear()
    assert mrt_gpu.main(size + boxes + ["--body-motion", "0", "0", "0", "0.004", "--force-every", "5"]) == 0
    assert seen["force_every"] == 5 and seen["body_motion"].shape == (2, 3) and np.array_equal(seen["bodies"], labels)
    seen.clear()
    assert mrt_gpu.main(size + boxes) == 0 and "body_motion" not in seen and "bodies" not in seen
    for extra, text in ((size + ["--body-motion", "0", "0", "0", "0.1"], "needs solid"),
                        (size + boxes + ["--body-motion", "2", "0", "0", "0.1"], "names body 2"),
                        (size + boxes + ["--solid-tiles", "--body-motion", "0", "0", "0", "0.1"], "tile kernel"),
                        (["--xsize", str(NX), "--ysize", str(NY)] + boxes + ["--body-motion", "0", "0", "0", "0.1"], "BB")):
        with pytest.raises(SystemExit) as e:
            mrt_gpu.main(extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra


def test_solver_checks_the_shape_and_the_checkpoint_carries_the_motion(tmp_path):
    """save_checkpoint / load_checkpoint around a context-free double of the solver's state calls: a motion that was set travels with its
    labels and centres and is set again after them; a run at rest writes the file it always wrote."""
    mask, labels = _two_boxes()
    mot = np.array([[0.0, 0.0, 0.004], [0.01, 0.0, 0.0]])

    class Double(CavitySolver):
        def __init__(self, moving):
            self._h, self._lead, self.batch = None, (), 1
            self.nx, self.ny, self.Re, self.RT, self.uLB, self.semantics = NX, NY, 100.0, "MRT", 0.08, "bounce_back"
            self.dtype, self.y0, self.ny_local, self.turb, self.arith = np.dtype(np.float64), 0, NY, 0, "strict"
            self.has_solid, self.state, self.calls, self._bodies_given, self._motion_given = True, None, [], False, moving

        solid = property(lambda self: mask.copy())
        steps_done = property(lambda self: 25)
        nbodies = property(lambda self: 2)
        bodies = property(lambda self: (labels.copy(), np.array([[1.5, 2.5], [30.0, 7.25]])))
        body_motion = property(lambda self: mot.copy())

        def get_fields(self, want_fin=False, **kw):
            return np.zeros((2, NX, NY)), np.ones((NX, NY)), np.zeros((9, NX, NY))

        def set_state(self, fin):
            self.calls.append("state")

        def set_bodies(self, lab, centres=None):
            self.calls.append(("bodies", np.array(lab), np.array(centres)))

        def set_body_motion(self, m):
            self.calls.append(("motion", np.array(m)))
    path = Double(True).save_checkpoint(str(tmp_path / "m"))
    with np.load(path) as z:
        assert np.array_equal(z["body_motion"], mot) and np.array_equal(z["body_labels"], labels) and np.array_equal(z["body_centres"], [[1.5, 2.5], [30.0, 7.25]])
    d = Double(False)
    assert d.load_checkpoint(path) == 25
    assert [c if isinstance(c, str) else c[0] for c in d.calls] == ["state", "bodies", "motion"] and np.array_equal(d.calls[2][1], mot)
    rest = Double(False).save_checkpoint(str(tmp_path / "r"))
    with np.load(rest) as z:
        assert "body_motion" not in z and "body_labels" not in z
    d = Double(False)
    assert d.load_checkpoint(rest) == 25 and d.calls == ["state"]

    class Shape(Double):
        _need_solid = lambda self: None                                         # noqa: E731
    with pytest.raises(ValueError, match=r"\(2, 3\)"):
        CavitySolver.set_body_motion(Shape(False), np.zeros((3, 3)))


def test_host_force_with_delta_is_the_reference(tc_reference):
    """solid.host_force / host_body_force with the optional delta restate the reference's force on public outputs."""
    o, case, _ = tc_reference
    d = solid.wall_delta_field(case["mask"], case["labels"], case["centres"], case["motion"], np.float64)
    assert np.array_equal(d, o.delta)
    F, want = solid.host_body_force(o.fin, case["mask"], case["labels"], case["centres"], d), o.body_force()
    assert all(np.array_equal(F[k], want[k]) for k in ("links", "fx", "fy"))
    # (host_body_force sums the two products of a link's torque apart, the reference their rounded sum: one rounding per link)
    assert np.all(np.abs(F["tz"] - want["tz"]) <= want["links"] * 2.0 ** -52 * want["abs_z"])
    T, wt = solid.host_force(o.fin, case["mask"], d), o.force()
    assert T["links"] == wt["links"] and abs(T["fx"] - wt["fx"]) <= 2.0 ** -52 * wt["abs_x"] and abs(T["fy"] - wt["fy"]) <= 2.0 ** -52 * wt["abs_y"]
    rest = solid.host_body_force(o.fin, case["mask"], case["labels"], case["centres"])
    assert rest["tz"][0] != F["tz"][0] and np.array_equal(rest["tz"][1], F["tz"][1])       # (the ring is at rest: its delta is zero)
