"""GPU tests of the passive scalar (CavitySolver.begin_scalar ...; lbm_scalar_*): the scalar populations bit for bit against the NumPy
reference tests/scalar_ref.py, which is fed the device's own get_fields velocities step by step (so the scalar kernel is pinned whatever
arithmetic the flow runs); the vector route against kernel='generic'; the totals and the flux against host sums; the checkpoint; that
the flow's own bits do not know of the scalar; and three of the physics checks of tests/test_scalar_cpu.py in fp64."""
import numpy as np
import pytest

from latticeboltzmannsimulations_amd import CavitySolver, periodic, scalar, solid
from open_flow_ref import feq
from scalar_ref import CX, CY, OPP, ScalarOracle

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")
RE = 20.0
FORCE = (2e-5, -1e-5)
D = 0.07
SHAPES = {np.float32: [(72, 40), (70, 66), (1032, 8)], np.float64: [(72, 40), (70, 66), (1032, 8), (520, 8)]}
CASES = [(d, s) for d in (np.float32, np.float64) for s in SHAPES[d]]
IDS = [f"{np.dtype(d).name}-{s[0]}x{s[1]}" for d, s in CASES]
CHECKS = (1, 2, 7, 37)


def _nan(shape):
    return np.full(shape, np.nan)


def _scenarios(nx, ny):
    """[dict(tag, mask, wall_value, c0, per, force, hold, f, hold_value, q, motion)]"""
    r = np.random.default_rng(7)
    out = []
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    c0 = 1.0 + 0.1 * np.sin(2 * np.pi * xs / nx) * np.cos(2 * np.pi * ys / ny)

    def sc(tag, mask, wv=None, per=(0, 0), force=(0.0, 0.0), **kw):
        out.append(dict(dict(tag=tag, mask=mask, wall_value=wv, c0=c0, per=per, force=force, hold=None, f=None, hold_value=None, q=None, motion=None), **kw))

    sc("all fluid", np.zeros((nx, ny), bool))
    m = r.random((nx, ny)) < 0.1                                   # 10 % random solid, half of it Dirichlet at random values
    wv = np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan)
    sc("random, half Dirichlet", m, wv)
    C, Rd = (ny - 1) / 2.0, min(4.3, (ny - 5) / 2.0 - 0.3)          # a disc at 1
    disc = np.hypot(xs - (C + 3.0), ys - C) < Rd
    sc("disc", disc, np.where(disc, 1.0, np.nan))
    m = np.zeros((nx, ny), bool)                                   # Dirichlet cells at every lane position, a whole vector, the edge columns,
    yb = ny // 2                                                   # the lid row, the corners
    for lane in range(4):
        m[8 + 8 * lane + lane, yb] = True
    m[48:52, yb - 2] = True
    m[0, 2] = m[nx - 1, 3] = m[0, 0] = m[nx - 1, 0] = m[0, ny - 1] = m[nx - 1, ny - 1] = True
    m[20:27, 0] = True
    m[30:33, ny - 1] = True
    sc("lanes, edges, lid, corners", m, np.where(m, r.uniform(0.5, 1.5, (nx, ny)), np.nan))
    hold = np.zeros((nx, ny), bool)                                # user hold cells with hold values: an outlet column and single cells
    hold[nx - 2, 1:ny - 1] = True
    hold[5, 1] = hold[9, ny // 2] = True
    f = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 + 0.002 * r.standard_normal((nx, ny)), 0.002 * r.standard_normal((nx, ny)))
    inlet = np.zeros((nx, ny), bool)
    inlet[0, :] = True
    sc("hold cells", inlet, np.where(inlet, 0.25, np.nan), hold=hold, f=f, hold_value=r.uniform(0.0, 1.0, (nx, ny)))
    sc("hold cells, initial values", inlet, None, hold=hold, f=f)
    for i, per in enumerate(((1, 0), (0, 1), (1, 1))):             # periodic sides with a force, random solid cells
        m = periodic.wrap(r.random((nx, ny)) < 0.1, *per)
        wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan), *per)
        sc(f"periodic {per}", m, wv, per=per, force=FORCE)
    q = solid.disc_fractions(disc, C + 3.0, C, Rd)                 # a shape and a motion: ignored by the wall rule, followed through u
    sc("shaped rotating disc", disc, np.where(disc, 1.0, np.nan), q=q, motion=np.array([[0.0, 0.0, 0.002]]))
    return out


def _setup(x, sc, magic=0.25):
    x.set_driving_force(0.0, 0.0)
    x.set_body_motion(None).set_wall_velocity(None).set_shape(None)
    x.set_solid(sc["mask"])
    x.set_periodic(*sc["per"])
    if sc["hold"] is not None:
        x.set_open_cells(sc["hold"], sc["f"])
    if sc["q"] is not None:
        x.set_shape(sc["q"])
    if sc["motion"] is not None:
        x.set_body_motion(sc["motion"])
    x.set_driving_force(*sc["force"])
    x.begin_scalar(D, sc["c0"], magic, wall_value=sc["wall_value"], hold_value=sc["hold_value"])
    return x


def _oracle(sc, dtype, magic=0.25):
    return ScalarOracle(sc["mask"], D, sc["c0"], dtype, magic, wall_value=sc["wall_value"], hold=sc["hold"], hold_f=sc["f"],
                        hold_value=sc["hold_value"], periodic=sc["per"])


def _advance(xs, o, checks, what):
    """Step the solvers xs one step at a time up to max(checks) + 1, feed the oracle the velocity each scalar step read -- the moments of
    the flow state its flow step produced, which get_fields exports one step later -- and compare at `checks`."""
    got = {}
    us = []
    for n in range(1, max(checks) + 2):
        for x in xs:
            x.step(1)
        us.append(xs[0].get_fields()[0])               # the velocity scalar step n - 1 read (n = 1: the one before the first, unused)
        if n in checks:
            got[n] = [(x.scalar_populations(), x.scalar_populations(stored=True), x.scalar()) for x in xs]
    base = o.nsteps
    for n in range(1, max(checks) + 1):
        o.step(us[n][0], us[n][1])
        if n in checks:
            for i, (g, st, C) in enumerate(got[n]):
                w = f"{what} after {base + n} ({'default' if i == 0 else 'generic'} route)"
                assert np.array_equal(g, o.populations()), w + ": arriving populations"
                assert np.array_equal(st, o.populations(stored=True)), w + ": stored populations"
                assert np.array_equal(C, o.conc()), w + ": C"


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_bit_identical_to_reference(dtype, shape):
    """Arriving and stored populations and C after 1, 2, 7 and 37 steps from begin_scalar, then after 1, 2, 7 from a set_scalar_state of
    the developed state; the default route (the vector kernel where nx allows) and kernel='generic' against the reference."""
    nx, ny = shape
    V = 4 if dtype == np.float32 else 2
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=dtype, solid=np.zeros(shape, bool), **BB) as s, \
            CavitySolver(nx, ny, RE, RT="TRT", dtype=dtype, kernel="generic", solid=np.zeros(shape, bool), **BB) as g:
        assert s.describe()["vec"] == (1 if nx % V == 0 else 0) and g.describe()["vec"] == 0
        for sc in _scenarios(nx, ny):
            o = _oracle(sc, dtype)
            for x in (s, g):
                _setup(x, sc)
                assert x.scalar_active == dict(D=D, magic=0.25) and [float(v) for v in x.describe()["scalar"].split(",")] == [D, 0.25]
                assert np.array_equal(x.scalar_populations(), o.populations()) and np.array_equal(x.scalar(), o.conc())
            what = f"{nx}x{ny} {np.dtype(dtype).name} {sc['tag']}"
            _advance((s, g), o, CHECKS, what)
            st = o.populations()
            st[:, o.mask | o.hold] = 0.25                  # (host values on solid and hold cells are ignored)
            o.set_state(st)
            s.set_scalar_state(st); g.set_scalar_state(st)
            _advance((s, g), o, (1, 2, 7), what + " from set_scalar_state")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fast_flow_same_scalar_code(dtype):
    """Under arith='fast' the scalar kernel is the same code fed other velocities: bit identity with the reference fed those."""
    nx, ny = 72, 40
    with CavitySolver(nx, ny, RE, RT="MRT", dtype=dtype, arith="fast", solid=np.zeros((nx, ny), bool), **BB) as s:
        for sc in _scenarios(nx, ny)[1:3]:
            _setup(s, sc, magic=3.0 / 16.0)
            _advance((s,), _oracle(sc, dtype, 3.0 / 16.0), CHECKS, f"fast {np.dtype(dtype).name} {sc['tag']}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_totals_and_flux_against_host_sums(dtype):
    """scalar_totals() against the host sum over scalar() within cells 2^-52 sum|terms|; scalar_flux() per body against the sum of
    g_k - own over the body's links formed from scalar_populations() (arriving and stored), within links 2^-52 sum|terms|."""
    nx, ny = 72, 40
    r = np.random.default_rng(11)
    m = periodic.wrap(r.random((nx, ny)) < 0.15, 1, 0)
    lab = periodic.wrap(r.integers(0, 3, (nx, ny)).astype(np.int32), 1, 0)
    wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.6), r.uniform(0.0, 2.0, (nx, ny)), np.nan), 1, 0)
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=dtype, solid=m, **BB) as s:
        s.set_bodies(lab, solid.centroids(m, lab, 3))
        s.set_periodic(True, False)
        s.begin_scalar(D, 1.0, wall_value=wv)
        with pytest.raises(RuntimeError, match="no scalar step yet"):
            s.scalar_flux()
        s.step(25)
        C = s.scalar().astype(np.float64)
        real = scalar.real_cells(m, (True, False))
        t = s.scalar_totals()
        assert t["step"] == 25 and t["cells"] == int(real.sum())
        assert abs(t["sum"] - C[real].sum()) <= real.sum() * 2.0 ** -52 * np.abs(C[real]).sum()
        assert t["min"] == C[real].min() and t["max"] == C[real].max()
        g, st = s.scalar_populations().astype(np.float64), s.scalar_populations(stored=True).astype(np.float64)
        fl = s.scalar_flux()
        hold = ~real & ~m                                           # (the image cells that are not solid: no link starts at one)
        terms = [[] for _ in range(3)]
        for k in range(1, 9):
            for x, y in zip(*np.nonzero(~m & ~hold)):
                sx, sy = x - CX[k], y + CY[k]
                if 0 <= sx < nx and 0 <= sy < ny and m[sx, sy]:
                    terms[lab[sx, sy]].append(g[k, x, y] - st[OPP[k], x, y])
        for b in range(3):
            tb = np.array(terms[b])
            assert fl["links"][b] == len(tb) and fl["step"][b] == 25
            assert abs(fl["flux"][b] - tb.sum()) <= max(len(tb), 1) * 2.0 ** -52 * np.abs(tb).sum(), b
        assert any(abs(v) > 0 for v in fl["flux"])


def test_checkpoint_round_trip(tmp_path):
    """An exact restart: flow and scalar continue bit for bit from a checkpoint, Dirichlet cells, hold cells and their values included."""
    nx, ny = 72, 40
    sc = _scenarios(nx, ny)[4]
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=np.zeros((nx, ny), bool), **BB) as a, \
            CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=sc["mask"], **BB) as b:
        _setup(a, sc, magic=0.2)
        a.step(23)
        path = a.save_checkpoint(str(tmp_path / "ck"))
        a.step(17)
        assert b.load_checkpoint(path) == 23
        assert b.scalar_active == dict(D=D, magic=0.2)
        b.step(17)
        assert np.array_equal(a.scalar_populations(), b.scalar_populations())
        assert np.array_equal(a.get_fields(want_fin=True)[2], b.get_fields(want_fin=True)[2])


def test_flow_does_not_know_of_the_scalar():
    """The flow's bits with a scalar equal those without; after end_scalar the describe text is the parent's; the geometry setters end it,
    set_state and init_equilibrium keep it and leave its populations alone."""
    nx, ny = 72, 40
    sc = _scenarios(nx, ny)[1]
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=sc["mask"], **BB) as a, \
            CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=sc["mask"], **BB) as b:
        text = b.describe()
        assert "scalar" not in text
        a.begin_scalar(D, sc["c0"], wall_value=sc["wall_value"])
        a.step(20); b.step(20)
        assert np.array_equal(a.get_fields(want_fin=True)[2], b.get_fields(want_fin=True)[2])
        g = a.scalar_populations()
        a.set_state(a.get_fields(want_fin=True)[2])
        assert a.scalar_active is not None and np.array_equal(a.scalar_populations(), g)
        a.init_equilibrium()
        assert a.scalar_active is not None and np.array_equal(a.scalar_populations(), g)
        a.end_scalar()
        assert a.scalar_active is None and a.describe() == text
        with pytest.raises(RuntimeError, match="no scalar is active"):
            a.scalar()
        b.init_equilibrium()
        a.step(20); b.step(20)
        assert np.array_equal(a.get_fields(want_fin=True)[2], b.get_fields(want_fin=True)[2])
        for ender in (lambda x: x.set_solid(sc["mask"]), lambda x: x.set_open_cells(None), lambda x: x.set_periodic(False, False)):
            a.begin_scalar(D, 0.5)
            ender(a)
            assert a.scalar_active is None


def test_every_refusal_with_its_text():
    nx, ny = 72, 40
    z = np.zeros((nx, ny), bool)

    def refused(make, match, **kw):
        with make() as x:
            with pytest.raises(RuntimeError, match=match):
                x.has_solid = True                       # (the library's own refusal, not the wrapper's)
                x.begin_scalar(**dict(dict(D=0.1), **kw))

    refused(lambda: CavitySolver(nx, ny, RE, **BB), r"\(-4\).*obstacle lattices only")
    refused(lambda: CavitySolver(nx, ny, RE), r"\(-4\).*obstacle lattices only")
    refused(lambda: CavitySolver(nx, ny, RE, solid=z, tuning=dict(solid_tiles=True), **BB), r"\(-4\).*LBM_FLAG_SOLID_TILES")
    mk = lambda: CavitySolver(nx, ny, RE, solid=z, **BB)      # noqa: E731
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        refused(mk, r"\(-1\).*diffusivity must be finite and > 0", D=bad)
        refused(mk, r"\(-1\).*magic\) must be finite and > 0", magic=bad)
    c0 = np.ones((nx, ny))
    c0[3, 4] = np.nan
    refused(mk, r"\(-1\).*initial value of cell 124 is not finite", c0=c0)
    wv = np.full((nx, ny), np.nan)
    wv[5, 6] = 1.0
    refused(mk, r"\(-1\).*Dirichlet cell 206 is not a solid cell", wall_value=wv)
    m = z.copy()
    m[5, 6] = True
    with CavitySolver(nx, ny, RE, solid=m, **BB) as x:
        lib, h = x.lib, x._h
        one = np.ones((nx, ny))
        flag = m.astype(np.uint8)
        assert lib.lbm_scalar_begin(h, 0.1, 0.25, None, None, None, None) == -1 and b"c0 is NULL" in lib.lbm_last_error(h)
        assert lib.lbm_scalar_begin(h, 0.1, 0.25, one.ctypes.data, flag.ctypes.data, None, None) == -1
        assert b"wall value of Dirichlet cell 206 is missing or not finite" in lib.lbm_last_error(h)
        hold = z.copy()
        hold[9, 9] = True
        x.set_open_cells(hold, solid.equilibrium(1.0, np.zeros((nx, ny)), 0.0))
        with pytest.raises(RuntimeError, match=r"\(-1\).*hold value of hold cell 369 is not finite"):
            x.begin_scalar(0.1, hold_value=np.full((nx, ny), np.inf))
        assert x.scalar_active is None
        for call in (x.scalar, x.scalar_populations, x.scalar_totals, x.scalar_flux, lambda: x.set_scalar_state(np.zeros((9, nx, ny), np.float32))):
            with pytest.raises(RuntimeError, match=r"\(-4\).*no scalar is active"):
                call()
    from latticeboltzmannsimulations_amd import CavityBatch
    with CavityBatch(nx, ny, [RE, RE], solid=z, **BB) as x:
        assert x.lib.lbm_scalar_begin(x._h, 0.1, 0.25, c0.ctypes.data, None, None, None) == -4 and b"no batches" in x.lib.lbm_last_error(x._h)


def test_physics_fp64():
    """Conduction, conservation and diffusion on the device in fp64, with the bounds of tests/test_scalar_cpu.py."""
    import scalar_cases as P
    P.check_conduction(P.DeviceRun)
    P.check_conservation(P.DeviceRun, np.float64)
    P.check_diffusion(P.DeviceRun)
