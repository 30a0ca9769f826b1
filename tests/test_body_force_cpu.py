"""CPU tests of the per-body force (lbm_set_solid_bodies, lbm_body_force, lbm_force_*): the link-list builder of csrc/lbm_bodies.hpp,
driven by tests/body_links_model.cpp, against solid.body_links for the labelled masks of tests/body_cases.py; the centroids; the
refusals a library without a device can give; header, bindings and record size; the dry-run plans, which the feature must not touch;
the schedule with the shifted sampler (tests/force_schedule_model.cpp over csrc/lbm_schedule.hpp) against its closed form; and the front
end through the stand-in of tests/body_force_standin.py.  The two programs are built with the host g++ (with the address and
undefined-behaviour sanitizers where the compiler has them); their tests are skipped where there is no g++."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import body_cases  # noqa: E402
import body_force_standin  # noqa: E402
import make_front_end_transcripts as FT  # noqa: E402
from latticeboltzmannsimulations_amd import _lib as L  # noqa: E402
from latticeboltzmannsimulations_amd import launch_plan, mrt_gpu, solid  # noqa: E402
from latticeboltzmannsimulations_amd.solver import CavitySolver  # noqa: E402

CSRC = os.path.join(ROOT, "latticeboltzmannsimulations_amd", "csrc")
CHUNK = 2048
CALLS = ("lbm_set_solid_bodies", "lbm_get_solid_bodies", "lbm_solid_body_count", "lbm_body_force", "lbm_force_begin", "lbm_force_sample",
         "lbm_force_read", "lbm_force_end")


def _build(tmp, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp / name)
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)     # (a compiler without the sanitizers' runtimes)
    return exe


# ---- the link list ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builder(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bodies")
    exe = _build(tmp, "body_links_model")

    def run(mask, labels, nbodies):
        path = str(tmp / "case.txt")
        with open(path, "w") as f:
            f.write(f"{mask.shape[0]} {mask.shape[1]} {nbodies}\n")
            f.write(" ".join(str(int(v)) for v in mask.ravel()) + "\n" + " ".join(str(int(v)) for v in labels.ravel()) + "\n")
        out = {}
        for line in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines():
            w = line.split()
            out.setdefault(w[0], []).append([float(v) if w[0] == "centre" else int(v) for v in w[1:]])
        return out
    return run


SHAPES = [(72, 40), (1032, 8), (13, 9)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_link_list_is_the_host_restatement(builder, shape):
    """Entry count, order and the body of every entry; the bodies' ranges; the chunks cut every 2048 links of one body; the second
    lattice of a batch continues the same vector; the centroids, every bit."""
    cases = body_cases.cases(*shape) if shape[0] >= 72 else {"random": body_cases.cases(72, 40)["random"]}
    for name, (mask, labels, nb) in cases.items():
        mask = mask[:shape[0], :shape[1]]
        lab = body_cases.labels_of(mask, None if labels is None else labels[:shape[0], :shape[1]])
        raw = np.where(mask, lab, -7)                                           # (what a caller hands over: anything on fluid cells)
        got = builder(mask, raw, nb)
        want = solid.body_links(mask, lab)
        assert got["bad"] == [[-1]], name
        links = np.array(got.get("link", []), dtype=np.int64).reshape(-1, 4)
        assert len(links) == 2 * len(want), name
        assert np.array_equal(links[:len(want)], want) and np.array_equal(links[len(want):], want), name
        counts = np.bincount(want[:, 3], minlength=nb)
        start = np.concatenate([[0], np.cumsum(counts)])
        assert got["start"] == [list(start), list(start + len(want))], name
        first, chunks = [0], []
        for lattice in range(2):
            for b in range(nb):
                for i in range(0, counts[b], CHUNK):
                    chunks.append([lattice * len(want) + start[b] + i, min(CHUNK, counts[b] - i), b])
        per = len(chunks) // 2
        for b in range(nb):
            first.append(first[-1] + -(-counts[b] // CHUNK))
        assert got["first"] == [first, first] and got.get("chunk", []) == chunks and first[-1] == per, name
        cen = solid.centroids(mask, lab, nb)
        assert np.array_equal(np.array(got["centre"])[:, 1:], cen), name
        assert [int(c[0]) for c in got["centre"]] == list(range(nb))
    if shape == (1032, 8):
        m, lab, nb = cases["chunk_edge"]
        assert list(np.bincount(solid.body_links(m, lab)[:, 3])) == [CHUNK, CHUNK + 6]      # one full chunk; one full and one of six
    if shape == (72, 40):
        assert np.bincount(solid.body_links(*cases["enclosed"][:2])[:, 3], minlength=2)[1] == 0
        assert np.array_equal(solid.centroids(*cases["unused_label"])[1], [0.0, 0.0])
        assert len(solid.body_links(cases["default"][0], body_cases.labels_of(cases["default"][0], None))) > CHUNK


def test_links_belong_to_the_body_of_their_source_cell(builder):
    """Two bodies that touch share no link; a link's own cell is fluid, its source is solid and carries the entry's label; the entries
    of all bodies together are the links of the mask (solid.links)."""
    mask, labels, nb = body_cases.cases(72, 40)["touching"]
    ln = solid.body_links(mask, labels)
    x, y, k, b = ln.T
    cx, cy = np.array(solid.CX), np.array(solid.CY)
    assert not mask[x, y].any() and mask[x - cx[k], y + cy[k]].all() and np.array_equal(labels[x - cx[k], y + cy[k]], b)
    assert len(ln) == sum(int(l.sum()) for l in solid.links(mask)) and len(np.unique(ln[:, :3], axis=0)) == len(ln)
    assert list(np.bincount(b)) == [40, 27, 31]
    bad = labels.copy()
    bad[16, max(1, 40 // 4)] = 3                                                # a solid cell with the label nbodies
    assert builder(mask, bad, nb)["bad"] == [[16 * 40 + 10]]
    bad[16, 10] = -1
    assert builder(mask, bad, nb)["bad"] == [[16 * 40 + 10]]


def test_labels_from_boxes_and_files(tmp_path):
    """Every --solid-box is a body of its own, in the order given, a later box wins an overlap; the nonzero values of an integer
    --solid-file are body ids, ascending, after the boxes."""
    m, lab, n = solid.labels_from(48, 40, [(20, 28, 14, 20), (26, 30, 18, 22)])
    assert n == 2 and lab[20, 14] == 0 and lab[27, 19] == 1 and lab[29, 21] == 1 and lab[0, 0] == -1
    assert np.array_equal(m, solid.mask_from(48, 40, [(20, 28, 14, 20), (26, 30, 18, 22)]))
    f = np.zeros((48, 40), np.int64); f[2:4, 2:4] = 9; f[10, 10] = 4; f[27, 19] = 4
    path = str(tmp_path / "ids.npy")
    np.save(path, f)
    m, lab, n = solid.labels_from(48, 40, [(20, 28, 14, 20)], path)
    assert n == 3 and lab[20, 14] == 0 and lab[10, 10] == 1 and lab[27, 19] == 1 and lab[2, 2] == 2
    assert np.array_equal(m, solid.mask_from(48, 40, [(20, 28, 14, 20)], path))
    np.save(path, f != 0)
    assert solid.labels_from(48, 40, path=path)[2] == 1
    assert solid.labels_from(48, 40) == (None, None, 0)


def test_host_body_force_sums_to_host_force_and_reads_the_sign_of_one_link():
    """The per-body sums of the restatement add up to solid.host_force's; a single link whose torque can be read off: body 1 is the
    cell (5, 5), enclosed by body 0 but for the fluid cell (6, 5).  Its one link is (cell (6, 5), slot 1): the population that flew in
    -x and came back (fin_1 of that cell in get_fields) pushed the body to the left, tx = -2 f.  About a centre two rows FURTHER from the lid, (5.5, 7), the push acts above the centre in
    the picture with the lid on top, so it turns the body counter-clockwise: tz = ry tx = (5 - 7) (-2 f) = +4 f."""
    rng = np.random.default_rng(3)
    fin = rng.random((9, 72, 40))
    for name, (mask, labels, nb) in body_cases.cases(72, 40).items():
        lab = body_cases.labels_of(mask, labels)
        F = solid.host_body_force(fin, mask, lab, solid.centroids(mask, lab, nb))
        T = solid.host_force(fin, mask)
        assert int(F["links"].sum()) == T["links"], name
        assert abs(F["fx"].sum() - T["fx"]) <= 1e-12 * T["links"] and abs(F["fy"].sum() - T["fy"]) <= 1e-12 * T["links"], name
    mask = np.zeros((12, 12), bool); mask[4:7, 4:7] = True; mask[6, 5] = False
    lab = np.zeros((12, 12), np.int32); lab[5, 5] = 1
    ln = solid.body_links(mask, lab)
    assert [list(r) for r in ln[ln[:, 3] == 1]] == [[6, 5, 1, 1]]
    F = solid.host_body_force(fin[:, :12, :12], mask, lab, [[0.0, 0.0], [5.5, 7.0]])
    f = fin[1, 6, 5]
    assert F["links"][1] == 1 and F["fx"][1] == -2.0 * f and F["fy"][1] == 0.0 and F["tz"][1] == 4.0 * f > 0.0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_new_calls_and_keeps_its_version():
    assert L.ABI_VERSION == 4 and ctypes.sizeof(L.lbm_params) == 18 * 4 + 6 * 8 and ctypes.sizeof(L.lbm_body_force_record) == 48
    assert ctypes.sizeof(L.lbm_solid_force_record) == 32
    text = open(L.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.lib()
    assert lib.lbm_abi_version() == 4 and "#define LBM_ABI_VERSION 4" in text
    for n in CALLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr) and n in L.SIGNATURES and hasattr(lib, n), n
    assert "typedef struct lbm_body_force_record {\n    double step;\n    double body;\n    double links;\n    double fx;\n    double fy;\n    double tz;\n}" in hdr
    assert "positive counter-clockwise" in text and "(rx, ry) = (x - cx_k / 2 - x0, y + cy_k / 2 - y0)" in text


def test_null_context_is_rejected():
    lib = L.lib()
    lab, cen, rec = np.zeros(4, np.int32), np.zeros(2), (L.lbm_body_force_record * 1)()
    n = ctypes.c_longlong(0)
    assert lib.lbm_set_solid_bodies(None, lab.ctypes.data, 1, cen.ctypes.data) == -1
    assert lib.lbm_get_solid_bodies(None, lab.ctypes.data, cen.ctypes.data) == -1
    assert lib.lbm_solid_body_count(None) == 0
    assert lib.lbm_body_force(None, rec) == -1
    assert lib.lbm_force_begin(None, 1, 1) == -1 and lib.lbm_force_sample(None) == -1 and lib.lbm_force_end(None) == -1
    assert lib.lbm_force_read(None, rec, 1, ctypes.byref(n), ctypes.byref(n)) == -1


def test_launch_plans_do_not_change():
    """The feature touches no plan: a mask's plan with and without the tile route, at the sizes of the GPU tests, is the text the
    golden fixture of tests/test_launch_plans.py records for plain parameters plus what tests/test_solid*_cpu.py pin -- here: equal to
    itself across the two ways of asking, and free of any word of the feature."""
    for size, dt in (((72, 40), np.float32), ((1032, 8), np.float32), ((520, 8), np.float64), ((136, 80), np.float32)):
        p = launch_plan(*size, 100.0, steps=37, dtype=dt, semantics="bounce_back", solid=True)
        assert p["units"] == [1] * 37 and not any("force" in str(k) or "bod" in str(k) for k in p)
    p = launch_plan(136, 80, 100.0, steps=37, semantics="bounce_back", solid=True, tuning=dict(solid_tiles=True, tb_steps=5))
    assert p["kernel"] == "k_stepS_deep" and p["steps_per_launch"] == 5 and sum(p["units"]) == 37


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
EVERY, SMAX, CALL_STEPS = (0, 1, 3, 4, 5, 7, 8, 13), (1, 5, 8), (5, 20, 1, 13)
ARM_RES, ARM_FORCE = 2, 3
TOTAL = ARM_FORCE + sum(CALL_STEPS)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("schedule"), "force_schedule_model")
    found, key = {}, None
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "run":
            key = tuple(int(v) for v in w[1:])
            found[key] = []
        else:
            found[key].append((w[0],) + tuple(v if w[0] == "automatic" else int(v) for v in w[1:]))
    return found


def test_force_samples_follow_the_unit_that_ends_at_their_step_count(runs):
    assert sorted(runs) == sorted((a, b, s) for a in EVERY for b in EVERY for s in SMAX)
    returns = [ARM_RES, ARM_FORCE] + [ARM_FORCE + sum(CALL_STEPS[:k + 1]) for k in range(len(CALL_STEPS))]
    for (er, ef, smax), events in runs.items():
        assert events[-1] == ("end", TOTAL)
        # the force: samples n0 + j every, each taken at nsteps == n, right after a unit that ends there and before the call returns
        want_f = list(range(ARM_FORCE + ef, TOTAL + 1, ef)) if ef else []
        want_r = list(range(ARM_RES + er, TOTAL + 1, er)) if er else []      # the residual: n - 1 == nsteps, before the unit from n - 1
        got_f, got_r = [], []
        for i, ev in enumerate(events):
            if ev[0] != "sample":
                continue
            _, s, n, nsteps = ev
            if s == 3:
                assert nsteps == n and events[i - 1][0] == "unit" and events[i - 1][2] == n, (er, ef, smax, ev)
                got_f.append(n)
            else:
                assert s == 2 and nsteps == n - 1 and events[i + 1][:2] in (("unit", n - 1), ("sample", 2)), (er, ef, smax, ev)
                got_r.append(n)
        assert got_f == want_f and got_r == want_r, (er, ef, smax)
        # after any call exactly the samples with n <= steps done have been taken: one due at the call's last step included
        taken = 0
        for ev in events:
            taken += ev[0] == "sample" and ev[1] == 3
            if ev[0] == "return":
                assert taken == len([n for n in want_f if n <= ev[1]]), (er, ef, smax, ev)
        assert [ev[1] for ev in events if ev[0] == "return"] == returns
        # no unit crosses a cut, and none is shorter than it must be
        units = [ev[1:] for ev in events if ev[0] == "unit"]
        assert [u[0] for u in units] == [0] + [u[1] for u in units[:-1]] and units[-1][1] == TOTAL
        for a, b in units:
            cuts = [n for n in want_f if n > a and a >= ARM_FORCE] + [n - 1 for n in want_r if n - 1 > a and a >= ARM_RES]
            assert b == min([a + smax, min(e for e in returns if e > a)] + cuts), (er, ef, smax, (a, b))
        stem = [ev[1] for ev in events if ev[0] == "automatic"]
        assert stem == ["lbm_residual" if er else ("lbm_force" if ef else "-")]


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
NX, NY = 48, 40
RUN = dict(maxIt=41, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=20, SavePlot=False, BC="BB")


def _two_boxes():
    return solid.labels_from(NX, NY, [(20, 28, 14, 20), (36, 40, 6, 9)])[:2]


def _transcript(capsys, **kw):
    S = body_force_standin.make()
    r = mrt_gpu.run_cavity(solver_factory=S, **RUN, **kw)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "elapsed" not in ln]
    return r, S, lines


def test_force_every_writes_the_series(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    mask, labels = _two_boxes()
    r, S, _ = _transcript(capsys, solid=mask, bodies=labels, force_every=7, SaveVTK=True)
    assert body_force_standin.FS._entries(S.journal, "begin_force") == [(1, 7, 41 // 7 + 1)] and ("bodies", 2) in S.journal
    assert S.journal.index(("step", 1)) < S.journal.index(("begin_force", 1, 7, 6))           # (the force exists after the first step)
    fs = r.force_series
    assert fs["count"] == 5 and fs["dropped"] == 0 and fs["step"].tolist() == [[n, n] for n in (8, 15, 22, 29, 36)]
    assert fs["body"].tolist() == [[0, 1]] * 5 and fs["links"][0].tolist() == [6 * (8 + 6) - 4, 6 * (4 + 3) - 4]
    again = body_force_standin.make()(NX, NY, 100.0, RT="MRT", turb=0, semantics="bounce_back", solid=mask, bodies=labels)
    again.step(22)
    want = again.body_force_at(22)
    assert all(np.array_equal(fs[k][2], want[k]) for k in ("links", "fx", "fy", "tz")) and np.abs(fs["tz"][-1]).min() > 0.0
    saved = np.load(tmp_path / "output" / "force.npy")
    assert saved.shape == (5, 2, 6) and saved.dtype == np.float64
    assert all(np.array_equal(saved[..., i], fs[k]) for i, k in enumerate(body_force_standin.KEYS))
    assert [it for it, _ in r.forces] == [0, 20, 40]                                            # (the printed force goes on)


def test_without_force_every_nothing_changes(tmp_path, monkeypatch, capsys):
    """A run with obstacles prints, calls and writes what it did before: the same transcript as with the arguments left out, no
    begin_force, no force.npy; and a recorded case of tests/golden/front_end_transcripts.json replays with them spelt out."""
    monkeypatch.chdir(tmp_path)
    mask, labels = _two_boxes()
    a, A, lines_a = _transcript(capsys, solid=mask, SaveVTK=True)
    b, B, lines_b = _transcript(capsys, solid=mask, SaveVTK=True, bodies=None, force_every=None)
    assert A.journal == B.journal and lines_a == lines_b and not body_force_standin.FS._entries(A.journal, "begin_force")
    assert a.force_series is None and b.force_series is None and ("bodies", None) in A.journal
    assert "force.npy" not in os.listdir(tmp_path / "output") and a.forces == b.forces != []
    import json
    with open(FT.PATH) as f:
        recorded = json.load(f)["device+vtk"]
    _, got = FT.run(dict(FT.CASES["device+vtk"], bodies=None, force_every=None))
    assert all(got[part] == recorded[part] for part in ("result", "files", "journal", "lines"))


def test_arguments_are_checked_and_reach_the_command_line(monkeypatch, capsys):
    mask, labels = _two_boxes()
    S = body_force_standin.make()
    for kw, text in ((dict(force_every=5), "need solid"), (dict(bodies=labels), "need solid"), (dict(solid=mask, force_every=0), ">= 1")):
        with pytest.raises(ValueError, match=text):
            mrt_gpu.run_cavity(solver_factory=S, quiet=True, **RUN, **kw)
    assert S.made == []
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return mrt_gpu.CavityResult()
    monkeypatch.setattr(mrt_gpu, "run_cavity", fake)
    size = ["--xsize", str(NX), "--ysize", str(NY), "--turb", "0", "--BC", "BB"]
    boxes = ["--solid-box", "20", "28", "14", "20", "--solid-box", "36", "40", "6", "9"]
    assert mrt_gpu.main(size + boxes + ["--force-every", "7"]) == 0
    assert seen["force_every"] == 7 and np.array_equal(seen["bodies"], labels) and np.array_equal(seen["solid"], mask)
    seen.clear()
    assert mrt_gpu.main(size + boxes) == 0 and "force_every" not in seen and "bodies" not in seen
    with pytest.raises(SystemExit) as e:
        mrt_gpu.main(size + ["--force-every", "7"])
    assert e.value.code == 2 and "need solid" in capsys.readouterr().err


def test_checkpoint_carries_the_bodies(tmp_path):
    """save_checkpoint / load_checkpoint around a context-free double of the solver's state calls: labels and centres travel in the file
    when they were set, and a file without them loads as before."""
    mask, labels = _two_boxes()

    class Double(CavitySolver):
        def __init__(self, given):
            self._h, self._lead, self.batch = None, (), 1
            self.nx, self.ny, self.Re, self.RT, self.uLB, self.semantics = NX, NY, 100.0, "MRT", 0.08, "bounce_back"
            self.dtype, self.y0, self.ny_local, self.turb, self.arith = np.dtype(np.float64), 0, NY, 0, "strict"
            self.has_solid, self.state, self.set, self._bodies_given = True, None, None, given

        solid = property(lambda self: mask.copy())
        steps_done = property(lambda self: 25)
        bodies = property(lambda self: (labels.copy(), np.array([[1.5, 2.5], [30.0, 7.25]])))

        def get_fields(self, want_fin=False, **kw):
            return np.zeros((2, NX, NY)), np.ones((NX, NY)), np.zeros((9, NX, NY))

        def set_state(self, fin):
            self.state = fin

        def set_bodies(self, lab, centres=None):
            self.set = (np.array(lab), np.array(centres))
    path = Double(True).save_checkpoint(str(tmp_path / "b"))
    with np.load(path) as z:
        assert np.array_equal(z["body_labels"], labels) and np.array_equal(z["body_centres"], [[1.5, 2.5], [30.0, 7.25]])
    d = Double(False)
    assert d.load_checkpoint(path) == 25 and d.state is not None
    assert np.array_equal(d.set[0], labels) and np.array_equal(d.set[1], [[1.5, 2.5], [30.0, 7.25]])
    old = Double(False).save_checkpoint(str(tmp_path / "o"))
    with np.load(old) as z:
        assert "body_labels" not in z and "body_centres" not in z
    d = Double(False)
    assert d.load_checkpoint(old) == 25 and d.set is None
