"""GPU tests of the per-body force and torque (CavitySolver.set_bodies / body_force / begin_force / force_series; lbm_set_solid_bodies,
lbm_body_force, lbm_force_*): every labelled mask of tests/body_cases.py against the host restatement solid.host_body_force
within bounds derived from the number of roundings, and against lbm_solid_force; bit for bit between a series and the one-shot call,
manual and automatic samples, two runs, a batch and its lattices alone, the tile route and one step per launch; the unit cuts of the
schedule leave the lattice alone; the mechanics of the series, the refusals, the sign of the torque from a single link, a mirror-image
pair and a checkpoint.

Shapes: fp32 72 x 40 (one partial workgroup per row of the step kernel); fp32 1032 x 8 and fp64 520 x 8 (a row spans workgroups; wide
enough for a body of exactly one chunk of 2048 links and one of 2054: the seams of THIS reduction are the chunks of the link list);
fp32 136 x 80 on the tile route with five steps per launch.  A random 20 % mask as one body gives several chunks at every shape;
1024 x 160 gives more chunks than the final pass has lanes."""
import math

import numpy as np
import pytest

import body_cases
from checks import FAST_BOUND
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, solid

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")
TILES5 = dict(solid_tiles=True, tb_steps=5)
KEYS = ("step", "body", "links", "fx", "fy", "tz")
EPS = 2.0 ** -52


def _solver(shape, mask, labels, dtype=np.float32, coll="MRT", Re=100.0, tuning=None, **kw):
    return CavitySolver(shape[0], shape[1], Re, RT=coll, dtype=dtype, solid=mask, bodies=labels, tuning=tuning, **BB, **kw)


def _check_against_host(s, mask, labels, nb, what):
    """The issue's bounds, from the lattice as get_fields returns it.  links exactly; fx, fy within links_b 2^-52 sum |terms| of the
    exactly rounded host sum (one rounding per addition); tz within (links_b + 2) 2^-52 sum (|rx ty| + |ry tx|) (the products are
    rounded alike on both sides; one rounding for their sum and one for the addition per link); the bodies together against
    lbm_solid_force: links exactly, fx and fy within twice the bound of a sum over all links."""
    fin = s.get_fields(want_fin=True)[2]
    F, T = s.body_force(), s.solid_force()
    lab, cen = s.bodies
    assert np.array_equal(lab, body_cases.labels_of(mask, labels)) and np.array_equal(cen, solid.centroids(mask, lab, nb)), what
    H = solid.host_body_force(fin, mask, lab, cen)
    b, tx, ty, mx, my = solid.body_force_terms(fin, mask, lab, cen)
    assert F["step"].tolist() == [s.steps_done] * nb and F["body"].tolist() == list(range(nb)), what
    assert np.array_equal(F["links"], H["links"]), (what, F["links"], H["links"])
    for i in range(nb):
        sel = b == i
        n = int(sel.sum())
        for k, t in (("fx", tx), ("fy", ty)):
            bound = n * EPS * math.fsum(np.abs(t[sel]).tolist())
            print(f"{what} body {i} {k}: device {F[k][i]!r} host {H[k][i]!r} bound {bound!r}")
            assert abs(F[k][i] - H[k][i]) <= bound, (what, i, k, F[k][i], H[k][i], bound)
        bound = (n + 2) * EPS * math.fsum((np.abs(mx[sel]) + np.abs(my[sel])).tolist())
        print(f"{what} body {i} tz: device {F['tz'][i]!r} host {H['tz'][i]!r} bound {bound!r}")
        assert abs(F["tz"][i] - H["tz"][i]) <= bound, (what, i, "tz", F["tz"][i], H["tz"][i], bound)
        if n == 0:
            assert F["fx"][i] == 0.0 and F["fy"][i] == 0.0 and F["tz"][i] == 0.0, what
    assert int(F["links"].sum()) == T["links"] == len(b), what
    for k, t in (("fx", tx), ("fy", ty)):
        bound = 2.0 * len(b) * EPS * math.fsum(np.abs(t).tolist())
        assert abs(math.fsum(F[k].tolist()) - T[k]) <= bound, (what, k, F[k], T[k], bound)
    return F


CONFIGS = {"f32-72x40": (np.float32, (72, 40), None), "f32-1032x8": (np.float32, (1032, 8), None), "f64-520x8": (np.float64, (520, 8), None),
           "f32-136x80-tiles5": (np.float32, (136, 80), TILES5)}


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_mask_against_the_host_restatement(config, coll):
    dtype, shape, tuning = CONFIGS[config]
    for name, (mask, labels, nb) in body_cases.cases(*shape).items():
        with _solver(shape, mask, labels, dtype, coll, tuning=tuning) as s:
            assert s.nbodies == nb, name
            for n in (1, 7, 37):
                s.step(n - s.steps_done)
                F = _check_against_host(s, mask, labels, nb, f"{config} {coll} {name} step {n}")
            if name == "enclosed":
                assert F["links"][1] == 0 and F["links"][0] > 0
            if name == "unused_label":
                assert F["links"].tolist()[1] == 0 and np.array_equal(s.bodies[1][1], [0.0, 0.0])
            if name == "chunk_edge":
                assert F["links"].tolist() == [2048, 2054]


def test_fast_arithmetic_and_given_centres():
    shape = (72, 40)
    mask, labels, nb = body_cases.cases(*shape)["random"]
    cen = np.random.default_rng(2).random((nb, 2)) * [72, 40]
    with _solver(shape, mask, labels, np.float32, "MRT", arith="fast", centres=cen) as s:
        s.step(37)
        assert np.array_equal(s.bodies[1], cen)
        fin = s.get_fields(want_fin=True)[2]
        F, H = s.body_force(), solid.host_body_force(fin, mask, body_cases.labels_of(mask, labels), cen)
        b, tx, ty, mx, my = solid.body_force_terms(fin, mask, body_cases.labels_of(mask, labels), cen)
        for i in range(nb):
            sel = b == i
            n = int(sel.sum())
            assert F["links"][i] == n == H["links"][i]
            assert abs(F["fx"][i] - H["fx"][i]) <= n * EPS * math.fsum(np.abs(tx[sel]).tolist())
            assert abs(F["fy"][i] - H["fy"][i]) <= n * EPS * math.fsum(np.abs(ty[sel]).tolist())
            assert abs(F["tz"][i] - H["tz"][i]) <= (n + 2) * EPS * math.fsum((np.abs(mx[sel]) + np.abs(my[sel])).tolist())


def test_more_chunks_than_lanes_of_the_final_pass():
    """1024 x 160, random 20 %, one body: about 200 000 links, about 100 chunks for the 64 lanes of the final pass."""
    shape = (1024, 160)
    mask = np.random.default_rng(9).random(shape) < 0.2
    with _solver(shape, mask, None) as s:
        s.step(7)
        F = _check_against_host(s, mask, None, 1, "1024x160 default")
        assert F["links"][0] > 64 * 2048
        assert all(np.array_equal(F[k], v) for k, v in s.body_force().items())


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.mark.parametrize("config", ["f32-72x40", "f64-520x8"])
def test_series_one_shot_manual_and_rerun_have_the_same_bits(config):
    """begin at n0 = 3 with every = 5: records at 8, 13, ...; each equals body_force() called at that step count in a second run, the
    manual samples of a third, and the series of a fourth.  A sample due at a call's last step is there when the call returns."""
    dtype, shape, _ = CONFIGS[config]
    mask, labels, nb = body_cases.cases(*shape)["random"]

    def series():
        with _solver(shape, mask, labels, dtype) as s:
            s.step(3)
            s.begin_force(every=5, capacity=16)
            s.step(5)
            first = s.force_series()
            assert first["count"] == 1 and first["step"].tolist() == [[8] * nb], "the sample of the call's last step"
            for n in (4, 20, 1, 13):
                s.step(n)
                assert s.force_series()["count"] == (s.steps_done - 3) // 5
            out = s.force_series()
            tail = s.body_force()
        return out, tail
    a, tail = series()
    steps = list(range(8, 47, 5))
    assert a["count"] == len(steps) and a["dropped"] == 0 and a["step"].tolist() == [[n] * nb for n in steps]
    assert a["fx"].shape == (len(steps), nb) and tail["step"][0] == 46
    with _solver(shape, mask, labels, dtype) as s, _solver(shape, mask, labels, dtype) as m:
        s.step(3)
        m.step(3)
        m.begin_force(every=0, capacity=16)
        for j, n in enumerate(steps):
            s.step(n - s.steps_done)
            m.step(n - m.steps_done)
            m.sample_force()
            _same({k: a[k][j] for k in KEYS}, s.body_force(), f"one-shot at {n}")
        manual = m.force_series()
    _same(a, manual, "manual samples")
    _same(a, series()[0], "second run")
    assert np.abs(a["tz"]).max() > 0.0 and np.abs(a["fx"]).max() > 0.0


def test_a_lattice_of_a_batch_has_the_bits_of_the_lattice_alone():
    shape, Res = (72, 40), [100.0, 400.0, 1000.0]
    c = body_cases.cases(*shape)
    masks = np.stack([c["random"][0], c["touching"][0], c["default"][0]])
    labels = np.stack([c["random"][1], c["touching"][1], np.random.default_rng(4).integers(0, 5, shape).astype(np.int32)])
    with CavityBatch(shape[0], shape[1], Res, RT="MRT", dtype=np.float32, solid=masks, bodies=labels, **BB) as b:
        assert b.nbodies == 7
        b.step(2)
        b.begin_force(every=3, capacity=8)
        b.step(13)
        fs, one = b.force_series(), b.body_force()
        lab, cen = b.bodies
    assert fs["fx"].shape == (4, 3, 7) and one["fx"].shape == (3, 7) and fs["step"][:, 0, 0].tolist() == [5, 8, 11, 14]
    for i, Re in enumerate(Res):
        assert np.array_equal(lab[i], body_cases.labels_of(masks[i], labels[i]))
        with _solver(shape, masks[i], labels[i], Re=Re) as s:
            nb = s.nbodies                                         # (3 for the touching blocks, 5 and 7 for the others)
            assert np.array_equal(s.bodies[1], cen[i, :nb])
            s.step(2)
            s.begin_force(every=3, capacity=8)
            s.step(13)
            alone, alone_one = s.force_series(), s.body_force()
        for k in KEYS:
            assert np.array_equal(fs[k][:, i, :nb], alone[k]) and np.array_equal(one[k][i, :nb], alone_one[k]), (i, k)
        assert not fs["links"][:, i, nb:].any() and not fs["fx"][:, i, nb:].any() and not fs["tz"][:, i, nb:].any()


@pytest.mark.parametrize("every", [1, 3, 7])
def test_tile_route_series_equals_one_step_per_launch_and_leaves_the_lattice_alone(every):
    """136 x 80, five steps per launch: a unit ends at every sample; the records are those of the one-step route, and the lattice after
    the run is the lattice of a run without the sampler."""
    shape = (136, 80)
    mask, labels, nb = body_cases.cases(*shape)["random"]
    got = {}
    for name, tuning, sample in (("tiles", TILES5, True), ("one", None, True), ("plain", TILES5, False)):
        with _solver(shape, mask, labels, tuning=tuning) as s:
            s.step(2)
            if sample:
                s.begin_force(every=every, capacity=64)
            s.step(23)
            s.step(12)
            got[name] = (s.force_series() if sample else None, s.get_fields(want_fin=True), s.body_force())
    n = 35 // every
    assert got["tiles"][0]["count"] == n and got["tiles"][0]["step"][:, 0].tolist() == [2 + every * (j + 1) for j in range(n)]
    _same(got["tiles"][0], got["one"][0], "tile route against one step per launch")
    _same(got["tiles"][2], got["one"][2], "one-shot")
    for a, b, c in zip(got["tiles"][1], got["plain"][1], got["one"][1]):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_series_mechanics_and_refusals():
    shape = (136, 80)
    mask, labels, nb = body_cases.cases(*shape)["two_blocks"]
    with _solver(shape, mask, labels, tuning=TILES5) as s:
        lib, h = s.lib, s._h
        rec = (lib.lbm_body_force.argtypes[1]._type_ * nb)()
        assert lib.lbm_body_force(h, rec) == -4 and b"no step yet" in lib.lbm_last_error(h), "LBM_ERR_STATE before the first step"
        assert lib.lbm_force_begin(h, 1, 4) == -4 and lib.lbm_force_sample(h) == -4
        with pytest.raises(RuntimeError, match="no series"):
            s.force_series()
        s.step(4)
        assert lib.lbm_force_begin(h, -1, 4) == -1 and lib.lbm_force_begin(h, 1, 0) == -1
        s.begin_force(every=2, capacity=4)
        s.step(12)                                                  # samples at 6, 8, .., 16: six for a buffer of four
        a, b = s.force_series(), s.force_series()
        assert a["count"] == 4 and a["dropped"] == 2 and a["step"][:, 0].tolist() == [6, 8, 10, 12]
        _same(a, b, "read twice")
        assert lib.lbm_step_unit(h, 5) == -4 and b"lbm_force_begin" in lib.lbm_last_error(h)
        assert lib.lbm_step_edges(h) == -4
        # set_bodies ends the series and nothing else
        before = s.get_fields(want_fin=True)
        s.begin_monitor(every=0, capacity=4)
        s.set_bodies(np.zeros(shape, np.int32), centres=[[1.0, 2.0]])
        assert s.nbodies == 1 and s.steps_done == 16 and np.array_equal(s.bodies[1], [[1.0, 2.0]])
        assert all(np.array_equal(x, y) for x, y in zip(before, s.get_fields(want_fin=True)))
        assert s.monitor_series()["count"] == 0                     # (the monitor's series goes on)
        with pytest.raises(RuntimeError, match="no series"):
            s.force_series()
        assert lib.lbm_step_unit(h, 5) == 0                         # (no sampler is automatic any more)
        one = s.body_force()
        assert one["links"].tolist() == [88] and one["step"].tolist() == [21]
        # ... as do set_state and set_solid; set_solid returns to one body at its centroid
        for end in ("set_state", "set_solid"):
            s.step(1)
            if end == "set_solid":
                s.set_bodies(labels)
                assert s.nbodies == 2
            s.begin_force(every=1, capacity=4)
            s.step(2)
            assert s.force_series()["count"] == 2
            if end == "set_state":
                s.set_state(np.ascontiguousarray(before[2]))
            else:
                s.set_solid(mask)
            with pytest.raises(RuntimeError, match="no series"):
                s.force_series()
            assert lib.lbm_force_sample(h) == -4
        assert s.nbodies == 1 and np.array_equal(s.bodies[1], solid.centroids(mask, np.zeros(shape, int), 1))
        # labels out of range, bad counts, another semantics
        bad = labels.copy(); bad[8, 20] = 2
        assert mask[8, 20] and lib.lbm_set_solid_bodies(h, bad.ctypes.data, 2, None) == -1 and b"label" in lib.lbm_last_error(h)
        bad[8, 20] = -1
        assert lib.lbm_set_solid_bodies(h, bad.ctypes.data, 2, None) == -1
        ok = np.ascontiguousarray(np.where(mask, labels, 999), dtype=np.int32)      # (labels on fluid cells are ignored)
        assert lib.lbm_set_solid_bodies(h, ok.ctypes.data, 2, None) == 0
        for n in (0, -1, 257):
            assert lib.lbm_set_solid_bodies(h, ok.ctypes.data, n, None) == -1
        assert lib.lbm_set_solid_bodies(h, None, 2, None) == -1
        nan = np.full((2, 2), np.nan)
        assert lib.lbm_set_solid_bodies(h, ok.ctypes.data, 2, nan.ctypes.data) == -1
        assert s.nbodies == 2                                       # (the refused calls changed nothing)
        assert lib.lbm_set_solid_bodies(h, ok.ctypes.data, 256, None) == 0 and s.nbodies == 256
        s.step(3)
        assert s.body_force()["links"].tolist() == [56, 32] + [0] * 254
    with CavitySolver(72, 40, 100.0, **BB) as plain:
        lab = np.zeros((72, 40), np.int32)
        assert plain.lib.lbm_set_solid_bodies(plain._h, lab.ctypes.data, 1, None) == -4
        assert plain.lib.lbm_get_solid_bodies(plain._h, lab.ctypes.data, None) == -4 and plain.lib.lbm_solid_body_count(plain._h) == 0
        plain.step(1)
        rec = (plain.lib.lbm_body_force.argtypes[1]._type_ * 1)()
        assert plain.lib.lbm_body_force(plain._h, rec) == -4 and plain.lib.lbm_force_begin(plain._h, 1, 1) == -4
        assert plain.bodies is None and plain.nbodies == 0
        with pytest.raises(RuntimeError, match="no solid mask"):
            plain.set_bodies(lab)
    with pytest.raises(ValueError, match="needs solid"):
        CavitySolver(72, 40, 100.0, bodies=np.zeros((72, 40), np.int32), **BB)


def test_the_sign_of_the_torque_from_a_single_link():
    """Body 1 is the cell (5, 5), enclosed by body 0 but for the fluid cell (6, 5): its one link is (cell (6, 5), slot 1), whose
    population flew in -x and came back (fin_1 of that cell), so tx = -2 f, ty = 0.  About the centre (5.5, 7), two rows further from
    the lid than the link, the push to the left acts ABOVE the centre in the picture with the lid on top and turns the body
    counter-clockwise: tz = ry tx = (5 - 7) (-2 f) = +4 f, exactly."""
    mask = np.zeros((72, 40), bool); mask[4:7, 4:7] = True; mask[6, 5] = False
    lab = np.zeros((72, 40), np.int32); lab[5, 5] = 1
    for dtype in (np.float32, np.float64):
        with _solver((72, 40), mask, lab, dtype, centres=[[0.0, 0.0], [5.5, 7.0]]) as s:
            s.step(37)
            F, f = s.body_force(), float(s.get_fields(want_fin=True)[2][1, 6, 5])
        assert F["links"][1] == 1 and f > 0.0
        assert F["fx"][1] == -2.0 * f and F["fy"][1] == 0.0 and F["tz"][1] == 4.0 * f


def test_mirror_image_halves_under_a_reversed_lid():
    """The pair of tests/test_solid_gpu.py::test_mirror_image_under_a_reversed_lid (128^2, Re 100, MRT fp64, a 16 x 16 block and its
    mirror image under the reversed lid, 2000 steps), the block split into its left and right half as two bodies; the mirror image of
    body i carries the label i.  Per body fx changes sign between the images, fy does not, and the torque changes sign, to that
    test's tolerance: the populations of the two runs differ by err max|f| (measured here, and held below the bound of fast against
    strict fp64 bounce-back as there), so a force term differs by at most 2 err max|f| and a torque term by that times |rx| + |ry|, and
    each device sum carries its own rounding bound."""
    n = 128
    m1 = np.zeros((n, n), bool); m1[32:48, 56:72] = True
    l1 = np.zeros((n, n), np.int32); l1[40:48] = 1
    m2, l2 = m1[::-1].copy(), l1[::-1].copy()
    MIRROR = [0, 3, 2, 1, 4, 6, 5, 8, 7]
    with _solver((n, n), m1, l1, np.float64) as a:
        a.step(2000)
        fa, Fa, ca = a.get_fields(want_fin=True)[2], a.body_force(), a.bodies[1]
    with CavitySolver(n, n, -100.0, RT="MRT", dtype=np.float64, uLB=-0.08, solid=m2, bodies=l2, **BB) as b:
        b.step(2000)
        fb, Fb, cb = b.get_fields(want_fin=True)[2], b.body_force(), b.bodies[1]
    assert np.array_equal(cb, np.stack([n - 1 - ca[:, 0], ca[:, 1]], axis=1)) and ca[0].tolist() == [35.5, 63.5]
    err = float(np.abs(fa - fb[MIRROR][:, ::-1]).max() / np.abs(fa).max())
    fmax = float(np.abs(fa).max())
    assert err < FAST_BOUND[np.float64], err
    body, tx, ty, mx, my = solid.body_force_terms(fa, m1, l1, ca)
    ln = solid.body_links(m1, l1)
    arm = np.abs(ln[:, 0] - 0.5 * np.array(solid.CX)[ln[:, 2]] - ca[body, 0]) + np.abs(ln[:, 1] + 0.5 * np.array(solid.CY)[ln[:, 2]] - ca[body, 1])
    assert Fa["links"].tolist() == Fb["links"].tolist() == [6 * (8 + 16) - 4 - 16 * 3 + 2] * 2
    for i in range(2):
        sel = body == i
        k = int(sel.sum())
        bx = k * 2.0 * err * fmax + 2.0 * k * EPS * math.fsum(np.abs(tx[sel]).tolist())
        by = k * 2.0 * err * fmax + 2.0 * k * EPS * math.fsum(np.abs(ty[sel]).tolist())
        bz = 2.0 * err * fmax * float(arm[sel].sum()) + 2.0 * (k + 2) * EPS * math.fsum((np.abs(mx[sel]) + np.abs(my[sel])).tolist())
        print(f"mirror body {i}: populations {err:.3e}; fx {Fa['fx'][i]!r} {Fb['fx'][i]!r} ({bx:.3e}); fy {Fa['fy'][i]!r} {Fb['fy'][i]!r} "
              f"({by:.3e}); tz {Fa['tz'][i]!r} {Fb['tz'][i]!r} ({bz:.3e})")
        assert abs(Fa["fx"][i] + Fb["fx"][i]) <= bx and abs(Fa["fy"][i] - Fb["fy"][i]) <= by and abs(Fa["tz"][i] + Fb["tz"][i]) <= bz
        assert abs(Fa["fx"][i]) > 1e-6 and abs(Fa["tz"][i]) > 1e-6, "each half feels a drag and a torque"


def test_checkpoint_round_trip_with_labels(tmp_path):
    shape = (72, 40)
    mask, labels, nb = body_cases.cases(*shape)["touching"]
    cen = np.array([[12.0, 10.0], [18.5, 11.0], [0.0, 39.0]])
    with _solver(shape, mask, labels, centres=cen) as s:
        s.step(25)
        path = s.save_checkpoint(str(tmp_path / "bodies"))
        s.step(30)
        want, F = s.get_fields(want_fin=True), s.body_force()
    with np.load(path) as z:
        assert np.array_equal(z["body_labels"], body_cases.labels_of(mask, labels)) and np.array_equal(z["body_centres"], cen)
    with _solver(shape, mask, None) as r:
        assert r.nbodies == 1 and r.load_checkpoint(path) == 25 and r.nbodies == nb
        assert np.array_equal(r.bodies[0], body_cases.labels_of(mask, labels)) and np.array_equal(r.bodies[1], cen)
        r.step(30)
        assert all(np.array_equal(a, b) for a, b in zip(want, r.get_fields(want_fin=True)))
        G = r.body_force()
        assert all(np.array_equal(F[k][[0, 1, 2]], G[k]) for k in ("links", "fx", "fy", "tz"))
    with _solver(shape, mask, None) as plain:            # a checkpoint without labels: the bodies stay as they are
        plain.step(3)
        old = plain.save_checkpoint(str(tmp_path / "old"))
    with np.load(old) as z:
        assert "body_labels" not in z
    with _solver(shape, mask, labels, centres=cen) as r:
        assert r.load_checkpoint(old) == 3 and r.nbodies == nb and np.array_equal(r.bodies[1], cen)
