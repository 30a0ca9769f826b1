"""CPU tests of curved obstacle surfaces (lbm_set_solid_shape): the table builder of csrc/lbm_wall_shape.hpp, driven by
tests/wall_shape_model.cpp, against the NumPy restatement of tests/curved_wall_ref.py bit for bit; header, bindings and the sizes that
must not change; the dry-run plans; the helpers of solid.py; the front end, its messages and the checkpoint through stand-ins; and the
reference itself -- all q = 1/2 is the half-way reference, Taylor-Couette flow with the exact fractions re-measures the recorded torque
and profile errors, and the fluid mass drifts by the recorded amount: the interpolated rule does not conserve it.  The program is built
with the host g++ (with the address and undefined-behaviour sanitizers where the compiler has them); its tests are skipped where there
is no g++."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import body_cases
import body_force_standin
from body_cases import tc_case, tc_errors
from curved_wall_ref import (TCQ_FACTOR, TCQ_MASS_DRIFT, TCQ_MASS_DRIFT_AT_REST, TCQ_PROFILE_ERR, TCQ_TORQUE_ERR, CurvedWallOracle, circle_fractions,
                             tc_errors_scaled, tc_scaled)
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import launch_plan, mrt_gpu, solid
from latticeboltzmannsimulations_amd.solver import CavitySolver
from moving_wall_ref import MovingWallOracle
from solid_ref import SolidOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")
HALF_LO, HALF_HI = float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))


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
    tmp = tmp_path_factory.mktemp("shape")
    exe = _build(tmp, "wall_shape_model")

    def run(lattices, f32):
        """lattices: [(mask, labels, centres, motion, q)], all of one size and one number of bodies."""
        path = str(tmp / "case.txt")
        mask0, _, cen0, _, _ = lattices[0]
        with open(path, "w") as f:
            f.write(f"{mask0.shape[0]} {mask0.shape[1]} {len(cen0)} {len(lattices)} {int(f32)}\n")
            for mask, labels, centres, motion, q in lattices:
                f.write(" ".join(str(int(v)) for v in mask.ravel()) + "\n" + " ".join(str(int(v)) for v in labels.ravel()) + "\n")
                for c, m in zip(centres, motion):
                    f.write(" ".join(float(v).hex() for v in list(c) + list(m)) + "\n")
                f.write(" ".join(float(v).hex() for v in np.asarray(q, dtype=np.float64).ravel()) + "\n")
        out = {}
        for line in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines():
            w = line.split()
            out.setdefault(w[0], []).append(w[1:])
        return out
    return run


def two_bodies_one_cell(nx=72, ny=40):
    """A fluid cell between two bodies: its links towards either have no fluid cell behind them."""
    m = np.zeros((nx, ny), dtype=bool)
    lab = np.full((nx, ny), -7, dtype=np.int32)
    m[20:23, 10:14] = True; lab[20:23, 10:14] = 0
    m[24:27, 10:14] = True; lab[24:27, 10:14] = 1
    return m, lab, 2


def _motions(nb, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.01, 0.01, nb)], axis=1)


def _q(mask, labels, seed):
    """q uniform in (0, 1] with 1/2, its two neighbours, 1 and 1e-3 planted on links."""
    q = 1.0 - np.random.default_rng(seed).random((8,) + mask.shape)
    ln = solid.body_links(mask, np.where(mask, labels, 0))
    for i, v in enumerate((0.5, 1.0, 1e-3, HALF_LO, HALF_HI)):
        x, y, k, _ = ln[(i * (len(ln) - 1)) // 4]
        q[k - 1, x, y] = v
    return q


def _cases():
    cases = dict(body_cases.cases(72, 40))
    cases["between"] = two_bodies_one_cell()
    return cases


def test_builder_equals_the_numpy_restatement_bit_for_bit(builder):
    """The effective q of every link in list order; the table: rows in first-seen order, the near masks, a and d rounded once to the
    lattice type (fp32, and fp64: the doubles themselves), 1 and 0 where a cell has no link k; the effective q as lbm_get_solid_shape hands
    it out; the fallback links among them.  (The motions need not pass the flux check: the builder does not ask.)"""
    fell_back = 0
    for ci, (name, (mask, labels, nb)) in enumerate(_cases().items()):
        lab = body_cases.labels_of(mask, labels)
        cen = solid.centroids(mask, lab, nb)
        mot = _motions(nb, 11 + ci)
        q = _q(mask, lab, 50 + ci)
        for f32 in (True, False):
            dt = np.float32 if f32 else np.float64
            o = CurvedWallOracle(72, 40, 100.0, mask=mask, labels=lab, centres=cen, q=q, dtype=dt)
            o.motion = mot                                      # (past the flux check, which the reference's set_motion does not ask either)
            o._build()
            got = builder([(mask, np.where(mask, lab, 0), cen, mot, q)], f32)
            links = got.get("link", [])
            assert len(links) == len(o.links), name
            assert [float.fromhex(l[0]) for l in links] == [f["q"] for f in o.figs], name
            t = solid.shape_table(mask, lab, cen, mot, q, dt)                       # the public restatement says the same
            assert [tuple(r) for r in t["links"].tolist()] == o.links and t["q"].tolist() == o.l_q.tolist() and t["near"].tolist() == o.l_near.tolist(), name
            assert np.array_equal(t["a"], o.l_a.astype(np.float64)) and np.array_equal(t["d"], o.l_d.astype(np.float64)), name
            assert t["rx"].tolist() == [f["rx"] for f in o.figs] and t["ry"].tolist() == [f["ry"] for f in o.figs], name
            # the table: a row per cell with links, numbered as the list first meets the cells
            order = []
            for x, y, k, b in o.links:
                if (x, y) not in order:
                    order.append((x, y))
            cells = got.get("cell", [])
            assert sorted((int(c[1]), int(c[2])) for c in cells) == sorted(order) and int(got["rows"][0][0]) == len(order), name
            fig = {(x, y, k): (o.l_a[i], o.l_d[i], o.l_near[i]) for i, (x, y, k, _) in enumerate(o.links)}
            for c in cells:
                x, y, row, near = int(c[1]), int(c[2]), int(c[3]), int(c[4])
                assert row == order.index((x, y)), (name, x, y)
                vals = [float.fromhex(v) for v in c[5:]]
                for k in range(1, 9):
                    a, d, nr = fig.get((x, y, k), (1.0, 0.0, False))
                    assert vals[k - 1] == float(a) and vals[8 + k - 1] == float(d) and ((near >> (k - 1)) & 1) == int(nr), (name, x, y, k)
            qe = np.zeros((8, 72, 40))
            for w in got.get("qeff", []):
                qe[int(w[1]) - 1, int(w[2]), int(w[3])] = float.fromhex(w[4])
            assert np.array_equal(qe, o.q_eff), name
        fell_back += int(np.count_nonzero((o.q_eff == 0.5) & (q != 0.5) & (o.q_eff != 0.0)))
        if name == "between":                                   # the cell between the bodies: both its axis links fall back whatever q says
            qq = q.copy(); qq[0, 23, 11] = qq[2, 23, 11] = 0.125
            o2 = CurvedWallOracle(72, 40, 100.0, mask=mask, labels=lab, centres=cen, q=qq)
            assert o2.q_eff[0, 23, 11] == 0.5 and o2.q_eff[2, 23, 11] == 0.5 and not any(f["near"] for f, l in zip(o2.figs, o2.links) if l[:2] == (23, 11) and l[2] in (1, 3))
    assert fell_back > 50


def test_builder_numbers_the_rows_of_a_batch_on(builder):
    """Two lattices in one table: the rows of the second follow the first's, cell_row is per lattice, the link list one after the other."""
    mask, labels, nb = _cases()["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    m2, l2, _ = two_bodies_one_cell()
    l2 = body_cases.labels_of(m2, l2)
    A = (mask, np.where(mask, lab, 0), solid.centroids(mask, lab, nb), _motions(nb, 1), _q(mask, lab, 2))
    B = (m2, np.where(m2, l2, 0), solid.centroids(m2, l2, nb), _motions(nb, 3), _q(m2, l2, 4))
    both, a, b = builder([A, B], True), builder([A], True), builder([B], True)
    na = int(a["rows"][0][0])
    assert int(both["rows"][0][0]) == na + int(b["rows"][0][0]) and both["link"] == a["link"] + b["link"]
    assert [c for c in both["cell"] if c[0] == "0"] == a["cell"]
    assert [c[1:3] + [str(int(c[3]) - na)] + c[4:] for c in both["cell"] if c[0] == "1"] == [c[1:] for c in b["cell"]]


def test_builder_refuses_a_q_outside_its_range(builder):
    """0 < q <= 1 and finite on every link, the first offender named (lattices, then cells in [y][x] order, then k); off the links
    anything goes."""
    mask, labels, nb = _cases()["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    cen, mot = solid.centroids(mask, lab, nb), np.zeros((nb, 3))
    ln = solid.body_links(mask, lab)
    first = min((int(y), int(x), int(k)) for x, y, k, _ in ln)                       # the first link in [y][x], k order
    for bad in (0.0, -0.5, 1.0 + 2.0 ** -52, float("inf"), float("nan")):
        q = np.full((8, 72, 40), 0.5)
        x, y, k, _ = ln[len(ln) // 2]
        q[k - 1, x, y] = bad
        q[first[2] - 1, first[1], first[0]] = bad
        got = builder([(mask, np.where(mask, lab, 0), cen, mot, q)], False)
        assert list(got) == ["bad"] and [int(v) for v in got["bad"][0][:4]] == [0, first[1], first[0], first[2]], bad
    q = np.full((8, 72, 40), np.nan)
    q[ln[:, 2] - 1, ln[:, 0], ln[:, 1]] = 1.0
    got = builder([(mask, np.where(mask, lab, 0), cen, mot, q)], False)
    assert "bad" not in got and len(got["link"]) == len(ln)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_two_calls_and_keeps_version_and_sizes():
    assert L.ABI_VERSION == 4 and ctypes.sizeof(L.lbm_params) == 18 * 4 + 6 * 8
    assert ctypes.sizeof(L.lbm_body_force_record) == 48 and ctypes.sizeof(L.lbm_solid_force_record) == 32
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert lib.lbm_abi_version() == 4 and "#define LBM_ABI_VERSION 4" in text
    for n in ("lbm_set_solid_shape", "lbm_get_solid_shape"):
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert "t1 = a own;  b = 1 - a;  t2 = b other;  g_k = (t1 + t2) + d" in text and "wall_shape=1" in text and "NOT conserve" in text
    assert hdr.index("lbm_get_body_motion") < hdr.index("lbm_set_solid_shape") < hdr.index("lbm_halo_elems")
    q = np.zeros(3)
    assert lib.lbm_set_solid_shape(None, q.ctypes.data) == -1 and lib.lbm_get_solid_shape(None, q.ctypes.data) == -1


def test_launch_plans_do_not_change():
    """The shape is run state, not plan: the dry-run texts of a mask's plans hold no word of it."""
    for size, dt in (((72, 40), np.float32), ((70, 66), np.float32), ((1032, 8), np.float32), ((520, 8), np.float64)):
        p = launch_plan(*size, 100.0, steps=37, dtype=dt, semantics="bounce_back", solid=True)
        assert p["units"] == [1] * 37 and not any("shape" in str(k) or "shape" in str(v) for k, v in p.items())
        assert p["kernel"] == "k_step_solid" if size != (70, 66) else p["kernel"] == "k_step_generic"


# ---- the helpers of solid.py -------------------------------------------------------------------------------------------------------------
def test_disc_fractions_are_the_exact_ray_circle_fractions():
    c = tc_scaled(1)
    q = circle_fractions(c["mask"], c["C"], (c["R1"], c["R2"]))
    got = solid.disc_fractions(c["mask"], c["C"], c["C"], c["R2"], solid.disc_fractions(c["mask"], c["C"], c["C"], c["R1"]))
    assert np.array_equal(got, q)
    x, y, k, b = solid.body_links(c["mask"], c["labels"]).T
    t = got[k - 1, x, y]
    wx, wy = x - t * np.array(solid.CX)[k], y + t * np.array(solid.CY)[k]              # every wall point lies on its circle
    assert np.abs(np.hypot(wx - c["C"], wy - c["C"]) - np.where(b == 0, c["R1"], c["R2"])).max() < 1e-12
    assert t.min() > 0.0 and t.max() <= 1.0 and (t < 0.5).any() and (t > 0.5).any()
    assert np.all(got[:, c["mask"]] == 0.5)                                           # (off the links: the default)


def test_fractions_from_a_signed_distance():
    """A plane wall at x = 30.3 (solid beyond it): the linear estimate is exact, 0.3 along the axis and along the diagonals alike; the
    disc's estimate is within the curvature term of the exact fraction."""
    xs, ys = np.meshgrid(np.arange(72), np.arange(40), indexing="ij")
    m = xs > 30.3
    q = solid.fractions_from_distance(m, 30.3 - xs)
    for k in (3, 6, 7):                                                                # the slots that pull from x + 1
        assert np.allclose(q[k - 1, 30, 1:-1], 0.3, rtol=0, atol=1e-14)
    assert np.all(q[[0, 1, 3, 4, 7], 30, 5] == 0.5)                                    # (no link: the default)
    c = tc_scaled(1)
    disc = c["r"] < c["R1"]
    est = solid.fractions_from_distance(disc, c["r"] - c["R1"])
    exact = solid.disc_fractions(disc, c["C"], c["C"], c["R1"])
    lk = np.array(solid.links(disc)[1:])
    assert np.abs(est - exact)[lk].max() < 0.5 / c["R1"] and np.array_equal(est[~lk], exact[~lk])


def test_discs_of_the_command_line():
    m, lab, n = solid.discs_into(48, 40, [(12.0, 20.0, 4.5), (30.5, 18.5, 6.0)])
    assert n == 2 and m.sum() == (lab >= 0).sum() and set(np.unique(lab)) == {-1, 0, 1} and m[12, 20] and lab[30, 18] == 1 and not m[12, 25]
    m0, l0, n0 = solid.labels_from(48, 40, [(2, 6, 30, 34)])
    m2, l2, n2 = solid.discs_into(48, 40, [(12.0, 20.0, 4.5)], m0, l0, n0)
    assert n2 == 2 and np.array_equal(l2[2:6, 30:34], np.zeros((4, 4))) and l2[12, 20] == 1 and not m0[12, 20]
    with pytest.raises(ValueError, match="holds no cell"):
        solid.discs_into(48, 40, [(100.0, 100.0, 3.0)])


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_all_half_is_the_half_way_reference(coll):
    """q = 1/2 on every link: a = 1 selects own + d, the bits of MovingWallOracle (with a motion) and of SolidOracle (at rest)."""
    mask, labels, nb = body_cases.cases(72, 40)["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    half = np.full((8, 72, 40), 0.5)
    mot = [[0.03, -0.02, 0.004], [0.0, 0.01, -0.006]]
    for dt in (np.float32, np.float64):
        a = SolidOracle(72, 40, 100.0, mask=mask, collision=coll, dtype=dt).step(20)
        b = CurvedWallOracle(72, 40, 100.0, mask=mask, labels=lab, q=half, collision=coll, dtype=dt).step(20)
        assert np.array_equal(a.fin, b.fin) and np.array_equal(a.u, b.u) and np.array_equal(a.rho, b.rho)
        Fa, Fb = a.force(), b.force()
        assert all(Fa[k] == Fb[k] for k in Fa)
        a = MovingWallOracle(72, 40, 100.0, mask=mask, labels=lab, motion=mot, collision=coll, dtype=dt).step(20)
        b = CurvedWallOracle(72, 40, 100.0, mask=mask, labels=lab, motion=mot, q=half, collision=coll, dtype=dt).step(20)
        assert np.array_equal(a.fin, b.fin) and np.array_equal(a.u, b.u) and np.array_equal(a.rho, b.rho)
        assert np.array_equal(b.q_eff[b.q_eff != 0.0], np.full(len(b.links), 0.5))


def test_a_motion_set_between_steps_arrives_at_once():
    """The rule is on the read side: after set_motion the arriving populations carry the new term, from a developed state and never from
    plain populations."""
    mask, labels, nb = body_cases.cases(72, 40)["two_blocks"]
    lab = body_cases.labels_of(mask, labels)
    q = _q(mask, lab, 5)
    o = CurvedWallOracle(72, 40, 100.0, mask=mask, labels=lab, q=q).step(5)
    before = o.fin.copy()
    o.set_motion([[0.02, 0.0, 0.0], [0.0, 0.0, 0.0]])
    lk = np.zeros(o.fin.shape, bool)
    for (x, y, k, b), d in zip(o.links, o.l_d):
        lk[k, x, y] = d != 0
    assert lk.any() and np.all(o.fin[lk] != before[lk]) and np.array_equal(o.fin[~lk], before[~lk])
    o.set_state(before)
    o.set_motion(None)
    assert np.array_equal(o.fin, before)


@pytest.fixture(scope="module")
def tc_curved():
    c = tc_scaled(1)
    q = circle_fractions(c["mask"], c["C"], (c["R1"], c["R2"]))
    out = {}
    for key, mot in (("moving", c["motion"]), ("rest", None)):
        o = CurvedWallOracle(c["N"], c["N"], c["Re"], mask=c["mask"], labels=c["labels"], centres=c["centres"], motion=mot, q=q, collision="TRT",
                             dtype=np.float64)
        m0 = o.fluid_mass()
        o.step(6000)
        out[key] = (o, (o.fluid_mass() - m0) / m0)
    return c, q, out


def test_taylor_couette_with_the_exact_fractions(tc_curved):
    """The case of body_cases at 48 x 48 with the wall distances of both circles: torque and profile errors re-measured against the
    figures recorded in curved_wall_ref (and in DESIGN.md 2.10), asserted at TCQ_FACTOR times them.  (At this resolution the staircase
    is the luckier of the two -- 8.48e-3 -- and stays there when the lattice is refined, where this rule gains a factor four:
    tests/test_solid_shape_gpu.py.)"""
    c, q, out = tc_curved
    o, _ = out["moving"]
    assert o.closed()
    F = o.body_force()
    (e_in, e_out), e_prof = tc_errors_scaled(o.u, F["tz"], c)
    assert ((e_in, e_out), e_prof) == tc_errors(o.u, F["tz"], tc_case())               # (scale 1 is body_cases' own case and measure)
    print(f"Taylor-Couette, exact fractions: torque errors {e_in:.6e} {e_out:.6e}, profile error {e_prof:.6e}, tz {F['tz'][0]!r} {F['tz'][1]!r}")
    assert max(e_in, e_out) <= TCQ_FACTOR * TCQ_TORQUE_ERR and e_prof <= TCQ_FACTOR * TCQ_PROFILE_ERR
    assert abs(max(e_in, e_out) / TCQ_TORQUE_ERR - 1.0) < 1e-3 and abs(e_prof / TCQ_PROFILE_ERR - 1.0) < 1e-3        # the record is this run's
    assert F["tz"][0] < 0.0 < F["tz"][1]


def test_a_shaped_lattice_does_not_conserve_its_mass(tc_curved):
    """The interpolation weights two populations, so the fluid mass drifts: by the recorded +5.3e-3 over 6000 steps with the rotating
    disc, asserted at TCQ_FACTOR times the record (and well above rounding: this is the rule, not an error).  At rest the annulus, closed
    off from the lid by the ring, never leaves the rest state, and its mass stays to the bit."""
    c, q, out = tc_curved
    drift, rest = out["moving"][1], out["rest"][1]
    print(f"fluid mass after 6000 steps: {drift:+.6e} with the motion, {rest:+.6e} at rest")
    assert 6000 * 2.0 ** -48 < abs(drift) <= TCQ_FACTOR * TCQ_MASS_DRIFT and abs(drift / TCQ_MASS_DRIFT - 1.0) < 1e-3
    assert abs(rest) <= TCQ_FACTOR * TCQ_MASS_DRIFT_AT_REST


def test_host_force_with_the_shape_is_the_reference(tc_curved):
    c, q, out = tc_curved
    o, _ = out["moving"]
    F, want = solid.host_body_force(o.fin, c["mask"], c["labels"], c["centres"], shape=o.q_eff, fpost=o.fpost), o.body_force()
    assert all(np.array_equal(F[k], want[k]) for k in ("links", "fx", "fy"))
    assert np.all(np.abs(F["tz"] - want["tz"]) <= want["links"] * 2.0 ** -52 * want["abs_z"])
    T, wt = solid.host_force(o.fin, c["mask"], shape=o.fpost), o.force()
    assert T["links"] == wt["links"] and abs(T["fx"] - wt["fx"]) <= 2.0 ** -52 * wt["abs_x"] and abs(T["fy"] - wt["fy"]) <= 2.0 ** -52 * wt["abs_y"]


# ---- the front end, through stand-ins ----------------------------------------------------------------------------------------------------
NX, NY = 48, 40
RUN = dict(maxIt=21, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=20, SavePlot=False, BC="BB")
DISCS = [(14.0, 20.0, 5.3), (34.5, 12.5, 4.2)]


def _curved_standin():
    Base = body_force_standin.make()

    class CurvedStandIn(Base):
        def __init__(self, xsize, ysize, Re, solid=None, bodies=None, **kw):
            super().__init__(xsize, ysize, Re, solid=solid, bodies=bodies, **kw)
            self.o = body_force_standin._ForceTap(CurvedWallOracle(xsize, ysize, Re, mask=self.mask, labels=self.labels, uLB=self.uLB,
                                                                   collision=kw.get("RT", "MRT"), dtype=np.float64), self)

        def set_shape(self, q):
            self._note("set_shape", self.steps_done)
            self.o._o.set_shape(q)
            return self

        def set_body_motion(self, motion):
            self._note("set_body_motion", np.asarray(motion).tolist(), self.steps_done)
            self.o._o.set_motion(motion)
            return self

        def solid_force(self):
            F = self.o._o.force()
            self._note("solid_force", self.steps_done)
            return dict(step=self.steps_done, links=F["links"], fx=F["fx"], fy=F["fy"])
    return CurvedStandIn


def _two_discs():
    mask, labels, _ = solid.discs_into(NX, NY, DISCS)
    q = None
    for x0, y0, R in DISCS:
        q = solid.disc_fractions(mask, x0, y0, R, q)
    return mask, labels, q


def test_run_cavity_sets_the_shape_then_the_motion_before_the_first_step():
    mask, labels, q = _two_discs()
    mot = [[0.0, 0.0, 0.004], [0.0, 0.0, 0.0]]
    S = _curved_standin()
    r = mrt_gpu.run_cavity(solver_factory=S, quiet=True, solid=mask, bodies=labels, body_motion=mot, solid_shape=q, **RUN)
    j = S.journal
    assert j.index(("set_shape", 0)) < j.index(("set_body_motion", mot, 0)) < j.index(("step", 1))
    want = CurvedWallOracle(NX, NY, 100.0, mask=mask, labels=labels, motion=mot, q=q, collision="MRT", dtype=np.float64).step(21).force()
    assert r.forces[-1][1]["fx"] == want["fx"] and r.forces[-1][1]["fy"] == want["fy"]
    S2 = _curved_standin()
    r0 = mrt_gpu.run_cavity(solver_factory=S2, quiet=True, solid=mask, bodies=labels, body_motion=mot, **RUN)          # without the key: nothing of it
    assert not body_force_standin.FS._entries(S2.journal, "set_shape") and r0.forces[-1][1]["fx"] != want["fx"]


def test_arguments_are_checked_and_reach_the_command_line(monkeypatch, capsys):
    mask, labels, q = _two_discs()
    S = _curved_standin()
    for kw, text in ((dict(solid_shape=q), "needs solid"), (dict(solid=mask, solid_shape=q[:7]), r"\[8, xsize, ysize\]"),
                     (dict(solid=mask, solid_tiles=True, solid_shape=q), "tile kernel")):
        with pytest.raises(ValueError, match=text):
            mrt_gpu.run_cavity(solver_factory=S, quiet=True, **RUN, **kw)
    assert S.made == []
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return mrt_gpu.CavityResult()
    monkeypatch.setattr(mrt_gpu, "run_cavity", fake)
    size = ["--xsize", str(NX), "--ysize", str(NY), "--turb", "0", "--BC", "BB"]
    discs = [w for d in DISCS for w in ["--solid-disc"] + [repr(v) for v in d]]
    assert mrt_gpu.main(size + discs + ["--curved", "--body-motion", "0", "0", "0", "0.004"]) == 0
    assert np.array_equal(seen["solid"], mask) and np.array_equal(seen["bodies"], labels) and np.array_equal(seen["solid_shape"], q)
    assert np.array_equal(seen["body_motion"], [[0.0, 0.0, 0.004], [0.0, 0.0, 0.0]])
    seen.clear()
    assert mrt_gpu.main(size + discs) == 0                                             # the discs as a staircase: no shape
    assert np.array_equal(seen["solid"], mask) and np.array_equal(seen["bodies"], labels) and "solid_shape" not in seen
    seen.clear()
    assert mrt_gpu.main(size + ["--solid-box", "2", "6", "30", "34"] + discs[:4] + ["--curved"]) == 0       # a disc is a body after the boxes
    assert seen["bodies"][3, 31] == 0 and seen["bodies"][14, 20] == 1 and np.all(seen["solid_shape"][:, 2:6, 30:34] == 0.5)
    seen.clear()
    assert mrt_gpu.main(size + ["--solid-box", "2", "6", "30", "34"]) == 0 and "solid_shape" not in seen and "bodies" not in seen
    for extra, text in ((size + ["--curved"], "needs --solid-disc"), (size + discs + ["--curved", "--solid-tiles"], "tile kernel"),
                        (size + ["--solid-disc", "100", "100", "2"], "holds no cell"),
                        (["--xsize", str(NX), "--ysize", str(NY)] + discs + ["--curved"], "BB")):
        with pytest.raises(SystemExit) as e:
            mrt_gpu.main(extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra


def test_the_checkpoint_carries_the_shape_and_sets_it_before_the_motion(tmp_path):
    """save_checkpoint / load_checkpoint around a context-free double of the solver's state calls: a shape that is set travels as
    solid_shape and is set again before the motion; a run without one writes the file it always wrote."""
    mask, labels, q = _two_discs()
    mot = np.array([[0.0, 0.0, 0.004], [0.01, 0.0, 0.0]])
    qe = np.where(np.array(solid.links(mask)[1:]), q, 0.0)

    class Double(CavitySolver):
        def __init__(self, shaped, moving=True):
            self._h, self._lead, self.batch = None, (), 1
            self.nx, self.ny, self.Re, self.RT, self.uLB, self.semantics = NX, NY, 100.0, "MRT", 0.08, "bounce_back"
            self.dtype, self.y0, self.ny_local, self.turb, self.arith = np.dtype(np.float64), 0, NY, 0, "strict"
            self.has_solid, self.calls, self._bodies_given, self._motion_given, self._shaped = True, [], False, moving, shaped

        solid = property(lambda self: mask.copy())
        steps_done = property(lambda self: 25)
        nbodies = property(lambda self: 2)
        bodies = property(lambda self: (labels.copy(), np.array([[14.0, 20.0], [34.5, 12.5]])))
        body_motion = property(lambda self: mot.copy())
        shape = property(lambda self: qe.copy() if self._shaped else None)

        def get_fields(self, want_fin=False, **kw):
            return np.zeros((2, NX, NY)), np.ones((NX, NY)), np.zeros((9, NX, NY))

        def set_state(self, fin):
            self.calls.append(("state",))

        def set_bodies(self, lab, centres=None):
            self.calls.append(("bodies",))

        def set_body_motion(self, m):
            self.calls.append(("motion", None if m is None else np.array(m)))

        def set_shape(self, a):
            self.calls.append(("shape", None if a is None else np.array(a)))
            self._shaped = a is not None
    path = Double(True).save_checkpoint(str(tmp_path / "s"))
    with np.load(path) as z:
        assert np.array_equal(z["solid_shape"], qe) and np.array_equal(z["body_motion"], mot)
    d = Double(False, False)
    assert d.load_checkpoint(path) == 25
    names = [c[0] for c in d.calls]
    assert names == ["state", "motion", "shape", "bodies", "motion"] and d.calls[1][1] is None and np.array_equal(d.calls[4][1], mot)
    got = d.calls[2][1]
    lk = np.array(solid.links(mask)[1:])
    assert np.array_equal(got[lk], q[lk]) and np.all(got[~lk] == 0.5)                  # (off the links the file holds 0: any valid value does)
    plain = Double(False).save_checkpoint(str(tmp_path / "p"))
    with np.load(plain) as z:
        assert "solid_shape" not in z
    d = Double(False, False)
    assert d.load_checkpoint(plain) == 25 and [c[0] for c in d.calls] == ["state", "bodies", "motion"]
    d = Double(True, False)                                                            # a shaped solver loads a file without one: the shape goes
    assert d.load_checkpoint(plain) == 25 and [c[0] for c in d.calls][:3] == ["state", "motion", "shape"] and d.calls[2][1] is None

    class Shape(Double):
        _need_solid = lambda self: None                                             # noqa: E731
    with pytest.raises(ValueError, match=r"\(8, 48, 40\)"):
        CavitySolver.set_shape(Shape(False), np.zeros((8, 40, 48)))
