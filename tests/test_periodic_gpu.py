"""GPU tests of periodic sides and the driving force (CavitySolver.set_periodic, set_driving_force; lbm_set_periodic,
lbm_set_driving_force): strict arithmetic bit for bit against the NumPy reference tests/periodic_ref.py on the vector kernel and the
generic route, image cells included, over x, y and xy, at rest and with a force, with random solid cells, a disc, a motion with a wall
velocity, a shaped disc and a user hold cell beside an image; the force alone in a closed box; translation invariance, which puts the seam
at every lane position; clearing; `fast` arithmetic; a batch; the checkpoint; the force series; every error path; Poiseuille flow."""
import numpy as np
import pytest

from checks import FAST_BOUND, same_as_oracle, same_fields
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, periodic, solid
from open_flow_ref import feq
from periodic_ref import PeriodicOracle

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")
RE_STRICT = 20.0      # (as tests/test_open_flow_gpu.py: tau = 0.596 on an 8-row lattice, every case stays a flow on the reference)
FORCE = (2e-5, -1e-5)
SHAPES = {np.float32: [(72, 40), (70, 66), (1032, 8)], np.float64: [(72, 40), (70, 66), (1032, 8), (520, 8)]}
CASES = [(c, d, s) for d in (np.float32, np.float64) for c in ("SRT", "TRT", "MRT") for s in SHAPES[d]]
# the Poiseuille margins of tests/test_periodic_cpu.py: 10 x what the reference measured
POISEUILLE_ERR, POISEUILLE_BALANCE = 10 * 1.54e-11, 10 * 1.23e-11


def _random(nx, ny, px, py, seed, frac=0.1, nb=3):
    r = np.random.default_rng(seed)
    m = periodic.wrap(r.random((nx, ny)) < frac, px, py)
    lab = periodic.wrap(r.integers(0, nb, (nx, ny)).astype(np.int32), px, py)
    return m, lab, nb


def _disc(nx, ny, px, py):
    """A disc in the middle of the rows, two cells from every seam; (mask, labels, nbodies, (C, R))."""
    C, R = (ny - 1) / 2.0, min(4.3, (ny - 5) / 2.0 - 0.3)
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    m = np.hypot(xs - (C + 3.0), ys - C) < R
    assert m.any() and not m[:3].any() and not m[:, :3].any() and not m[:, ny - 3:].any()
    return m, np.zeros((nx, ny), np.int32), 1, ((C + 3.0, C), R)


def _scenarios(nx, ny):
    """[(tag, (px, py), force, mask, labels, nbodies, q, uw, motion, hold, f)]"""
    out = []
    for i, (per, force) in enumerate((((1, 0), (0.0, 0.0)), ((0, 1), FORCE), ((1, 1), FORCE), ((1, 1), (0.0, 0.0)))):
        m, lab, nb = _random(nx, ny, *per, seed=100 + i)
        out.append((f"random {per}", per, force, m, lab, nb, None, None, None, None, None))
    m, lab, nb, (cen, R) = _disc(nx, ny, 1, 1)
    out.append(("disc xy", (1, 1), FORCE, m, lab, nb, None, None, None, None, None))
    m2, lab2, nb2 = _random(nx, ny, 1, 1, seed=110)
    r = np.random.default_rng(111)
    uw = periodic.wrap(np.where(m2[None], r.uniform(-0.01, 0.01, (2, nx, ny)), 0.0), 1, 1)
    mot = np.stack([r.uniform(-0.01, 0.01, nb2), r.uniform(-0.01, 0.01, nb2), np.zeros(nb2)], axis=1)
    out.append(("motion + wall velocity xy", (1, 1), FORCE, m2, lab2, nb2, None, uw, mot, None, None))
    q = solid.disc_fractions(m, cen[0], cen[1], R)
    out.append(("shaped disc x", (1, 0), FORCE, m, lab, nb, q, None, None, None, None))
    out.append(("shaped disc xy, rotating", (1, 1), FORCE, m, lab, nb, q, None, np.array([[0.0, 0.0, 0.002]]), None, None))
    hold = np.zeros((nx, ny), bool)
    hold[1, ny // 2] = hold[nx - 2, 2] = hold[5, 1] = hold[1, 1] = True      # beside the image columns, the image rows, in a corner
    rr = np.random.default_rng(112)
    f = feq(1.0 + 0.002 * rr.standard_normal((nx, ny)), 0.005 * rr.standard_normal((nx, ny)), 0.005 * rr.standard_normal((nx, ny)))
    out.append(("hold beside images xy", (1, 1), FORCE, np.zeros((nx, ny), bool), np.zeros((nx, ny), np.int32), 1, None, None, None, hold, f))
    return out


def _setup(x, sc):
    tag, per, force, m, lab, nb, q, uw, mot, hold, f = sc
    x.set_driving_force(0.0, 0.0)
    x.set_solid(m).set_bodies(lab, solid.centroids(m, lab, nb))
    x.set_periodic(*per)
    if hold is not None:
        x.set_open_cells(hold, f)
    if q is not None:
        x.set_shape(q)
    if uw is not None:
        x.set_wall_velocity(uw)
    if mot is not None:
        x.set_body_motion(mot)
    x.set_driving_force(*force)
    return x


def _oracle(nx, ny, Re, sc, **kw):
    tag, per, force, m, lab, nb, q, uw, mot, hold, f = sc
    return PeriodicOracle(nx, ny, Re, mask=m, labels=lab, centres=solid.centroids(m, lab, nb), periodic=per, force=force, q=q, wall_velocity=uw,
                          motion=mot, hold=hold, f=f, **kw)


@pytest.mark.parametrize("coll,dtype,shape", CASES, ids=lambda v: v if isinstance(v, str) else (f"{v[0]}x{v[1]}" if isinstance(v, tuple) else np.dtype(v).name))
def test_strict_bit_identical_to_reference(coll, dtype, shape):
    """fin, u and rho, image cells included, after 1, 2, 7 and 37 steps from the setter's state, then from a set_state of the developed
    one; the default route and kernel='generic' against the reference and against each other."""
    nx, ny = shape
    V = 4 if dtype == np.float32 else 2
    with CavitySolver(nx, ny, RE_STRICT, RT=coll, dtype=dtype, solid=np.zeros(shape, bool), **BB) as s, \
            CavitySolver(nx, ny, RE_STRICT, RT=coll, dtype=dtype, kernel="generic", solid=np.zeros(shape, bool), **BB) as g:
        for sc in _scenarios(nx, ny):
            tag, per, force = sc[:3]
            o = _oracle(nx, ny, RE_STRICT, sc, collision=coll, dtype=dtype)
            for x in (s, g):
                _setup(x, sc)
                d = x.describe()
                assert d["periodic"] == ("xy" if all(per) else ("x" if per[0] else "y")) and x.periodic == (bool(per[0]), bool(per[1]))
                assert ("driving_force" in d) == any(force) and x.driving_force == force and x.steps_done == 0
                assert (x.open_cells is None) == (sc[9] is None) and (sc[9] is None or np.array_equal(x.open_cells[0], sc[9]))
            assert s.describe()["kernel"] == ("k_step_solid" if nx % V == 0 else "k_step_generic")
            for phase in range(2):
                if phase:
                    st = o.fin.copy()
                    st[:, o.img] = 0.25                      # (host values on image cells are ignored)
                    o.set_state(st)
                    s.set_state(st); g.set_state(st)
                for n in (1, 1, 5, 30):
                    s.step(n); g.step(n); o.step(n)
                    what = f"{nx}x{ny} {coll} {np.dtype(dtype).name} {tag} phase {phase} after {o.nsteps}"
                    same_as_oracle(s, o, what)
                    same_fields(g, s, what + " generic")
            for x in (s, g):                                # (geometry comes first: back to rest before the next scenario)
                x.set_body_motion(None).set_wall_velocity(None).set_shape(None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_force_alone_in_a_closed_box(dtype):
    """The force needs no periodic side: a closed box with obstacles under gravity, both routes, bits against the reference; the force may
    change between steps without restarting the lattice."""
    nx, ny = 72, 40
    m, lab, nb = _random(nx, ny, 0, 0, seed=7)
    for coll in ("SRT", "TRT", "MRT"):
        o = PeriodicOracle(nx, ny, 100.0, mask=m, force=(0.0, -3e-5), collision=coll, dtype=dtype)
        with CavitySolver(nx, ny, 100.0, RT=coll, dtype=dtype, solid=m, **BB) as s, \
                CavitySolver(nx, ny, 100.0, RT=coll, dtype=dtype, kernel="generic", solid=m, **BB) as g:
            for x in (s, g):
                x.set_driving_force(0.0, -3e-5)
                assert x.describe()["driving_force"] == 1 and "periodic" not in x.describe() and x.periodic == (False, False)
            for n in (1, 1, 5, 30):
                s.step(n); g.step(n); o.step(n)
                same_as_oracle(s, o, f"closed box {coll} after {o.nsteps}")
                same_fields(g, s, f"closed box {coll} generic")
            o.set_driving_force(1e-5, 2e-5)
            for x in (s, g):
                x.set_driving_force(1e-5, 2e-5)
                assert x.steps_done == 37
            s.step(9); g.step(9); o.step(9)
            same_as_oracle(s, o, f"closed box {coll}, new force")
            same_fields(g, s, f"closed box {coll}, new force, generic")


@pytest.mark.parametrize("dtype,kernel", [(np.float32, "auto"), (np.float64, "auto"), (np.float32, "generic")])
def test_translation_invariance_on_the_device(dtype, kernel):
    """A doubly periodic problem shifted cyclically by (3, 5) gives the shifted bits: the seam passes every lane position."""
    nx, ny = 72, 40
    m, lab, nb = _random(nx, ny, 1, 1, seed=21, frac=0.12)
    r = np.random.default_rng(22)
    st = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny))).astype(dtype)

    def shifted(a):
        b = np.array(a)
        b[..., 1:-1, 1:-1] = np.roll(a[..., 1:-1, 1:-1], (3, 5), axis=(-2, -1))
        return periodic.wrap(b, True, True)
    runs = []
    for mm, ss in ((m, periodic.wrap(st, True, True)), (shifted(m), shifted(st))):
        with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, kernel=kernel, solid=mm, **BB) as s:
            s.set_periodic(True, True).set_driving_force(*FORCE)
            s.set_state(np.ascontiguousarray(ss))
            s.step(41)
            runs.append(s.get_fields(want_fin=True))
    for a, b, name in zip(runs[0], runs[1], ("u", "rho", "fin")):
        # (the real cells: an image exports what it stores, its partner's post-collision populations, not its partner's export)
        assert np.isfinite(a).all() and np.array_equal(periodic.interior(shifted(a), True, True), periodic.interior(b, True, True)), name
    assert float(np.abs(runs[0][0]).max()) > 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clearing_gives_the_bits_of_a_context_that_never_set_them(dtype):
    nx, ny = 72, 40
    m, lab, nb = _random(nx, ny, 1, 1, seed=31)
    for kernel in ("auto", "generic"):
        with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, kernel=kernel, solid=m, bodies=lab, **BB) as plain, \
                CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, kernel=kernel, solid=m, bodies=lab, **BB) as s:
            s.set_periodic(True, True).set_driving_force(*FORCE)
            s.step(5)
            s.set_driving_force(0.0, 0.0)
            assert s.steps_done == 5 and "driving_force" not in s.describe() and s.describe()["periodic"] == "xy"
            s.set_periodic()
            assert s.steps_done == 0 and s.periodic == (False, False) and s.open_cells is None and s.describe() == plain.describe()
            for n in (1, 6):
                s.step(n); plain.step(n)
                same_fields(s, plain, f"cleared {kernel} after {s.steps_done}")
            s.set_periodic(True, False)
            s.set_solid(m)                                  # (a new mask clears the periodic sides)
            plain.set_solid(m)
            assert s.periodic == (False, False) and s.describe() == plain.describe()
            s.step(3); plain.step(3)
            same_fields(s, plain, f"new mask {kernel}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_arithmetic(dtype):
    """Poiseuille flow past a disc, 128 x 96, Re 1000, 2000 steps: the two routes agree bit for bit, and the distance from the strict fp64
    run stays inside checks.FAST_BOUND, the bounds of tests/test_open_flow_gpu.py.  A long-run smoke check (MRT, the default rates,
    against the device's own strict run): the bound on `fast` with periodic sides and the driving force, for the three operators
    against a long-double reference, is tests/test_arith_error_budget_rules_gpu.py."""
    nx, ny = 128, 96
    g = periodic.poiseuille(nx, ny)
    m, lab, _ = solid.discs_into(nx, ny, [(40, 47.5, 9.0)], g["solid"], np.where(g["solid"], 0, -1).astype(np.int32), 1)

    def run(**kw):
        with CavitySolver(nx, ny, 1000.0, RT="MRT", solid=m, bodies=lab, **kw, **BB) as s:
            s.set_periodic(True, False).set_driving_force(1e-5, 0.0)
            s.step(2000)
            return s.get_fields(want_fin=True, out_dtype=np.float64)[2], s.describe()["kernel"]
    f_ref, _ = run(dtype=np.float64)
    a, ka = run(dtype=dtype, arith="fast")
    b, kb = run(dtype=dtype, arith="fast", kernel="generic")
    assert (ka, kb) == ("k_step_solid", "k_step_generic") and np.array_equal(a, b), "fast arithmetic differs between the routes"
    err = float(np.abs(a - f_ref).max() / np.abs(f_ref).max())
    print(f"fast periodic Poiseuille with a disc, MRT {np.dtype(dtype).name}: {err:.3e} (bound {FAST_BOUND[dtype]:.1e})")
    assert np.isfinite(a).all() and err < FAST_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_of_three_geometries_equals_the_lone_runs(dtype):
    nx, ny = 72, 40
    masks = np.stack([_random(nx, ny, 1, 1, seed=40 + i)[0] for i in range(3)])
    Res = [100.0, 400.0, 1000.0]
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=dtype, solid=masks, **BB) as b:
        b.set_periodic(True, True).set_driving_force(*FORCE)
        b.step(1); b.step(22)
        u, rho, fin = b.get_fields(want_fin=True)
        F = b.solid_force()
    for i, Re in enumerate(Res):
        with CavitySolver(nx, ny, Re, RT="MRT", dtype=dtype, solid=masks[i], **BB) as s:
            s.set_periodic(True, True).set_driving_force(*FORCE)
            s.step(23)
            u1, r1, f1 = s.get_fields(want_fin=True)
            F1 = s.solid_force()
        assert np.array_equal(fin[i], f1) and np.array_equal(u[i], u1) and np.array_equal(rho[i], r1), Re
        assert {k: F[k][i] for k in F} == F1, Re


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    nx, ny = 72, 40
    m, lab, nb = _random(nx, ny, 1, 0, seed=51)
    hold = np.zeros((nx, ny), bool); hold[1, 5] = hold[30, 20] = True
    hold &= ~m
    f = feq(1.0, 0.003 * np.ones((nx, ny)), 0.0)
    with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, bodies=lab, **BB) as s:
        s.set_periodic(True, False).set_open_cells(hold, f).set_driving_force(*FORCE)
        s.step(25)
        path = s.save_checkpoint(str(tmp_path / "periodic"))
        s.step(30)
        want = s.get_fields(want_fin=True)
    with np.load(path) as z:
        assert z["periodic"].tolist() == [True, False] and z["driving_force"].tolist() == list(FORCE) and np.array_equal(z["open_hold"], hold)
    with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, **BB) as r:
        assert r.load_checkpoint(path) == 25
        assert r.periodic == (True, False) and r.driving_force == FORCE and np.array_equal(r.open_cells[0], hold)
        r.step(30)
        got = r.get_fields(want_fin=True)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, **BB) as plain:      # files of other runs are unchanged
        plain.step(3)
        with np.load(plain.save_checkpoint(str(tmp_path / "plain"))) as z:
            assert not {"periodic", "driving_force"} & set(z.files)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_force_series_on_a_periodic_lattice(dtype):
    """body_force, solid_force and the force series against the reference's exactly rounded sums: links exactly -- every physical link
    once, from its real fluid cell --; fx, fy within links * 2^-52 * sum |terms|."""
    nx, ny = 72, 40
    scs = {sc[0]: sc for sc in _scenarios(nx, ny)}
    for tag in ("random (1, 1)", "motion + wall velocity xy", "shaped disc x"):
        sc = scs[tag]
        if not any(sc[2]):
            sc = sc[:2] + (FORCE,) + sc[3:]
        o = _oracle(nx, ny, 100.0, sc, collision="MRT", dtype=dtype).step(23)
        assert not any(o.img[x, y] for x, y, _, _ in o.links)
        with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, solid=np.zeros((nx, ny), bool), **BB) as s:
            _setup(s, sc)
            s.step(22)
            s.begin_force(every=1, capacity=4)
            s.step(1)
            F, T, series = s.body_force(), s.solid_force(), s.force_series()
        want, wt = o.body_force(), o.force()
        assert F["links"].tolist() == want["links"].tolist() and T["links"] == wt["links"] == len(o.links), tag
        for k, a in (("fx", "abs_x"), ("fy", "abs_y")):
            bound = want["links"] * 2.0 ** -52 * want[a]
            print(f"{tag} {np.dtype(dtype).name} {k}: device {F[k]!r} reference {want[k]!r} bound {bound!r}")
            assert np.all(np.abs(F[k] - want[k]) <= bound), (tag, k)
            assert series["count"] == 1 and np.array_equal(series[k][0], F[k]), (tag, k)
            assert abs(T[k] - wt[k]) <= wt["links"] * 2.0 ** -52 * wt[a], (tag, k)


def test_error_paths():
    nx, ny = 72, 40
    m, lab, nb = _random(nx, ny, 1, 1, seed=61)
    INVALID, STATE = -1, -4
    ip, dp = np.zeros(1, np.int32), np.zeros(1)
    with CavitySolver(nx, ny, 100.0, **BB) as plain:                   # another semantics
        with pytest.raises(RuntimeError, match="no solid mask"):
            plain.set_periodic(True, False)
        assert plain.lib.lbm_set_periodic(plain._h, 1, 0) == STATE and plain.lib.lbm_get_periodic(plain._h, None, None) == STATE
        assert plain.lib.lbm_set_driving_force(plain._h, 1e-6, 0.0) == STATE
        assert plain.lib.lbm_set_driving_force(plain._h, 0.0, 0.0) == 0 and plain.driving_force == (0.0, 0.0) and plain.periodic is None
    with CavitySolver(nx, ny, 100.0, solid=m, bodies=lab, **BB) as s:
        def refused(code, text, call):
            assert call() == code
            assert text in s.lib.lbm_last_error(s._h).decode(), s.lib.lbm_last_error(s._h)
        for v in (np.nan, np.inf):
            refused(INVALID, "not finite", lambda: s.lib.lbm_set_driving_force(s._h, v, 0.0))
            refused(INVALID, "not finite", lambda: s.lib.lbm_set_driving_force(s._h, 0.0, -v))
        assert s.driving_force == (0.0, 0.0)
        # the mask must equal its own wrap: the first offending cell is named
        bad = m.copy(); bad[0, 7] = ~bad[nx - 2, 7]
        s.set_solid(bad)
        refused(INVALID, f"the mask of image cell {0 * ny + 7} differs", lambda: s.lib.lbm_set_periodic(s._h, 1, 0))
        assert s.periodic == (False, False)
        s.set_solid(m)
        x0, y0 = np.argwhere(m[1:-1, 1:2])[0][0] + 1, 1      # a solid real cell of row 1: its image is row ny - 1
        lb = lab.copy(); lb[x0, ny - 1] = (lb[x0, 1] + 1) % nb
        s.set_bodies(lb)
        refused(INVALID, f"the body label of image cell {x0 * ny + ny - 1} differs", lambda: s.lib.lbm_set_periodic(s._h, 1, 1))
        s.set_bodies(lab).set_periodic(True, True)
        with pytest.raises(RuntimeError, match="lbm_set_solid_bodies: lattice 0: the body label of image cell"):
            s.set_bodies(lb)                                  # (checked when called later, too)
        s.set_bodies(lab)
        assert s.periodic == (True, True)                   # (new bodies keep the periodic sides)
        # a user hold cell on an image cell
        fl = np.argwhere(~m[0:1, :])[0]
        h = np.zeros((nx, ny), bool); h[0, fl[1]] = True
        with pytest.raises(RuntimeError, match="is an image cell of a periodic side"):
            s.set_open_cells(h, feq(1.0, np.zeros((nx, ny)), 0.0))
        assert s.open_cells is None and s.periodic == (True, True)
        hb = np.ones((nx, ny), np.uint8)
        assert s.lib.lbm_get_open_cells(s._h, hb.ctypes.data, None) == 0 and not hb.any()      # (the user's hold cells only)
        # geometry comes first
        s.set_shape(np.full((8, nx, ny), 0.5))
        refused(STATE, "geometry comes first", lambda: s.lib.lbm_set_periodic(s._h, 1, 0))
        s.set_shape(None)
        uw = periodic.wrap(np.where(m[None], 0.01, 0.0) * np.array([0.0, 1.0])[:, None, None], True, True)
        s.set_wall_velocity(uw)
        refused(STATE, "geometry comes first", lambda: s.lib.lbm_set_periodic(s._h, 0, 0))
        s.set_wall_velocity(None).set_body_motion(np.array([[0.01, 0.0, 0.0]] * nb))      # (a periodic lattice is open: no flux check)
        refused(STATE, "geometry comes first", lambda: s.lib.lbm_set_periodic(s._h, 1, 1))
        s.set_body_motion(None)
        assert s.lib.lbm_get_periodic(s._h, ip.ctypes.data_as(s.lib.lbm_get_periodic.argtypes[1]), None) == 0 and ip[0] == 1
        assert s.lib.lbm_get_driving_force(s._h, None, dp.ctypes.data_as(s.lib.lbm_get_driving_force.argtypes[2])) == 0 and dp[0] == 0.0
    with CavitySolver(4, 8, 100.0, dtype=np.float64, solid=np.zeros((4, 8), bool), **BB) as t:      # the smallest: two images, two real cells
        t.set_periodic(True, True).set_driving_force(*FORCE)
        o = PeriodicOracle(4, 8, 100.0, periodic=(True, True), force=FORCE, dtype=np.float64)
        t.step(9); o.step(9)
        same_as_oracle(t, o, "4 x 8")
    with CavitySolver(128, 128, 100.0, solid=np.zeros((128, 128), bool), tuning=dict(solid_tiles=True), **BB) as t:      # the tile kernel
        with pytest.raises(RuntimeError, match="tile kernel"):
            t.set_periodic(True, True)
        with pytest.raises(RuntimeError, match="tile kernel"):
            t.set_driving_force(1e-6, 0.0)
        t.set_driving_force(0.0, 0.0)                       # (zero: nothing to refuse)


def test_poiseuille_on_the_device():
    """fp64, TRT at the product 3/16: the shifted velocity is the parabola and the wall force balances the driver, inside the margins of
    the CPU test; the default product leaves the error of the negative control."""
    out = periodic.run_poiseuille(6, 18, nu=0.1, force=1e-6, steps=20000, quiet=True)
    print(f"Poiseuille on the device: profile error {out['error']:.3e}, force balance {out['balance']:.3e}")
    assert out["error"] < POISEUILLE_ERR and out["balance"] < POISEUILLE_BALANCE, out
    ctl = periodic.run_poiseuille(6, 18, nu=0.1, force=1e-6, steps=20000, magic=None, quiet=True)
    assert ctl["error"] > 1e-3, ctl["error"]
