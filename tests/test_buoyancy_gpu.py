"""GPU tests of Boussinesq buoyancy (CavitySolver.set_buoyancy; lbm_set_buoyancy): strict arithmetic bit for bit against the coupled NumPy
references (tests/buoyancy_ref.py with tests/scalar_ref.py) -- flow populations, u, rho, the scalar's arriving and stored populations and C --
on the vector kernels and the generic route, over the three operators and both types; clearing, a scalar whose buoyancy was never set,
a change mid-run; the checkpoint; `fast` arithmetic; every refusal with its text; the physics once in fp64."""
import numpy as np
import pytest

import buoyancy_cases as P
from buoyancy_ref import BuoyantOracle, Coupled
from checks import same_as_oracle, same_fields
from latticeboltzmannsimulations_amd import CavitySolver, periodic, solid
from latticeboltzmannsimulations_amd import convection as CV
from open_flow_ref import feq
from scalar_ref import ScalarOracle

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")
RE = 20.0             # (as tests/test_periodic_gpu.py: every case stays a flow on the reference)
FORCE = (2e-5, -1e-5)
BUOY = (3e-5, 6e-5, 0.5)
D = 0.07
SHAPES = {np.float32: [(72, 40), (70, 66), (1032, 8)], np.float64: [(72, 40), (70, 66), (1032, 8), (520, 8)]}
CASES = [(c, d, s) for d in (np.float32, np.float64) for c in ("SRT", "TRT", "MRT") for s in SHAPES[d]]
CHECKS = (1, 2, 7, 37)
# `fast` against the strict fp64 device run, heated_cavity(62) at Ra = 1e4 after 2000 steps, max |f_fast - f_ref| / max |f_ref| over the flow
# populations (MI355X), and the headroom of checks.FAST_BOUND over checks.FAST_MEASURED, a factor of four
FAST_MEASURED = {np.float32: 1.687e-5, np.float64: 1.618e-15}
FAST_HEADROOM = 4.0


def _scenarios(nx, ny):
    """[dict(tag, mask, labels, nbodies, wall_value, c0, per, force, hold, f, hold_value, uw, motion)]"""
    r = np.random.default_rng(17)
    out = []
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    c0 = 0.5 + 0.4 * np.sin(2 * np.pi * xs / nx) * np.cos(2 * np.pi * ys / ny)

    def sc(tag, mask, wv=None, per=(0, 0), force=(0.0, 0.0), labels=None, nbodies=1, **kw):
        lab = np.zeros((nx, ny), np.int32) if labels is None else labels
        out.append(dict(dict(tag=tag, mask=mask, labels=lab, nbodies=nbodies, wall_value=wv, c0=periodic.wrap(c0, *per), per=per, force=force, hold=None,
                             f=None, hold_value=None, uw=None, motion=None), **kw))

    sc("all fluid", np.zeros((nx, ny), bool))
    m = r.random((nx, ny)) < 0.1                                   # 10 % random solid, half of it Dirichlet at random values
    sc("random, half Dirichlet", m, np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan))
    m = np.zeros((nx, ny), bool)                                   # solid cells at every lane position, a whole vector, the edge columns,
    yb = ny // 2                                                   # the lid row, the corners
    for lane in range(4):
        m[8 + 8 * lane + lane, yb] = True
    m[48:52, yb - 2] = True
    m[0, 2] = m[nx - 1, 3] = m[0, 0] = m[nx - 1, 0] = m[0, ny - 1] = m[nx - 1, ny - 1] = True
    m[20:27, 0] = True
    m[30:33, ny - 1] = True
    sc("lanes, a whole vector, edges, lid, corners", m, np.where(m, r.uniform(0.5, 1.5, (nx, ny)), np.nan))
    for i, per in enumerate(((1, 0), (0, 1), (1, 1))):             # periodic sides with a driving force too, random solid cells
        m = periodic.wrap(r.random((nx, ny)) < 0.1, *per)
        wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan), *per)
        sc(f"periodic {per} with a driving force", m, wv, per=per, force=FORCE)
    hold = np.zeros((nx, ny), bool)                                # user hold cells: an outlet column and single cells
    hold[nx - 2, 1:ny - 1] = True
    hold[5, 1] = hold[9, ny // 2] = True
    f = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 + 0.002 * r.standard_normal((nx, ny)), 0.002 * r.standard_normal((nx, ny)))
    inlet = np.zeros((nx, ny), bool)
    inlet[0, :] = True
    sc("hold cells", inlet, np.where(inlet, 0.25, np.nan), hold=hold, f=f, hold_value=r.uniform(0.0, 1.0, (nx, ny)))
    m = periodic.wrap(r.random((nx, ny)) < 0.1, 1, 1)              # a body motion with a wall velocity: WALL_MOVE
    lab = periodic.wrap(r.integers(0, 3, (nx, ny)).astype(np.int32), 1, 1)
    uw = periodic.wrap(np.where(m[None], r.uniform(-0.01, 0.01, (2, nx, ny)), 0.0), 1, 1)
    mot = np.stack([r.uniform(-0.01, 0.01, 3), r.uniform(-0.01, 0.01, 3), np.zeros(3)], axis=1)
    wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan), 1, 1)
    sc("motion + wall velocity xy", m, wv, per=(1, 1), force=FORCE, labels=lab, nbodies=3, uw=uw, motion=mot)
    return out


def _setup(x, sc, buoy=BUOY):
    x.set_driving_force(0.0, 0.0)
    x.set_body_motion(None).set_wall_velocity(None).set_shape(None)
    x.set_solid(sc["mask"]).set_bodies(sc["labels"], solid.centroids(sc["mask"], sc["labels"], sc["nbodies"]))
    x.set_periodic(*sc["per"])
    if sc["hold"] is not None:
        x.set_open_cells(sc["hold"], sc["f"])
    if sc["uw"] is not None:
        x.set_wall_velocity(sc["uw"])
    if sc["motion"] is not None:
        x.set_body_motion(sc["motion"])
    x.set_driving_force(*sc["force"])
    x.begin_scalar(D, sc["c0"], wall_value=sc["wall_value"], hold_value=sc["hold_value"])
    if buoy is not None:
        x.set_buoyancy(*buoy)
    return x


def _oracles(nx, ny, sc, coll, dtype, buoy=BUOY):
    o = BuoyantOracle(nx, ny, RE, mask=sc["mask"], labels=sc["labels"], centres=solid.centroids(sc["mask"], sc["labels"], sc["nbodies"]),
                      periodic=sc["per"], force=sc["force"], wall_velocity=sc["uw"], motion=sc["motion"], hold=sc["hold"], f=sc["f"], collision=coll,
                      dtype=dtype, buoyancy=buoy)
    s = ScalarOracle(sc["mask"], D, sc["c0"], dtype, wall_value=sc["wall_value"], hold=sc["hold"], hold_f=sc["f"], hold_value=sc["hold_value"],
                     periodic=sc["per"])
    return o, s


def _same(x, o, sc, what):
    same_as_oracle(x, o, what)
    assert np.array_equal(x.scalar_populations(), sc.populations()), what + ": arriving scalar populations"
    assert np.array_equal(x.scalar_populations(stored=True), sc.populations(stored=True)), what + ": stored scalar populations"
    assert np.array_equal(x.scalar(), sc.conc()), what + ": C"


@pytest.mark.parametrize("coll,dtype,shape", CASES, ids=lambda v: v if isinstance(v, str) else (f"{v[0]}x{v[1]}" if isinstance(v, tuple) else np.dtype(v).name))
def test_strict_bit_identical_to_reference(coll, dtype, shape):
    """Flow populations, u, rho, the scalar's arriving and stored populations and C after 1, 2, 7 and 37 steps from the setters' state, then
    from set_state + set_scalar_state of the developed one; the default route and kernel='generic' against the reference and each other."""
    nx, ny = shape
    V = 4 if dtype == np.float32 else 2
    with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, solid=np.zeros(shape, bool), **BB) as s, \
            CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, kernel="generic", solid=np.zeros(shape, bool), **BB) as g:
        assert s.describe()["vec"] == (1 if nx % V == 0 else 0) and g.describe()["vec"] == 0
        for sc in _scenarios(nx, ny):
            o, so = _oracles(nx, ny, sc, coll, dtype)
            pair = Coupled(o, so)
            for x in (s, g):
                _setup(x, sc)
                assert x.buoyancy == BUOY and x.describe()["buoyancy"] == 1 and x.steps_done == 0
            for phase in range(2):
                if phase:
                    st = o.fin.copy()
                    sg = so.populations()
                    if o.img is not None:
                        st[:, o.img] = 0.25                  # (host values on image cells are ignored)
                    sg[:, so.mask | so.hold] = 0.25          # (and on the scalar's solid and hold cells)
                    o.set_state(st)
                    so.set_state(sg)
                    for x in (s, g):
                        x.set_state(st)
                        x.set_scalar_state(sg)
                done = 0
                for n in CHECKS:
                    s.step(n - done); g.step(n - done); pair.step(n - done)
                    done = n
                    what = f"{nx}x{ny} {coll} {np.dtype(dtype).name} {sc['tag']} phase {phase} after {n}"
                    _same(s, o, so, what)
                    same_fields(g, s, what + " generic")
                    assert np.array_equal(g.scalar_populations(stored=True), s.scalar_populations(stored=True)), what + " generic: scalar"
                    assert np.array_equal(g.scalar(), s.scalar()), what + " generic: C"
            for x in (s, g):                                # (geometry comes first: back to rest before the next scenario)
                x.set_body_motion(None).set_wall_velocity(None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_clearing_never_setting_and_changing(dtype):
    """set_buoyancy(0, 0) gives the passive context's bits and describe text; a scalar whose buoyancy was never set gives the bits of a
    context without a scalar (flow) and of the passive scalar; buoyancy changed mid-run continues as the reference does."""
    nx, ny = 72, 40
    sc = _scenarios(nx, ny)[1]
    for kernel in ("auto", "generic"):
        kw = dict(RT="TRT", dtype=dtype, kernel=kernel, solid=sc["mask"], **BB)
        with CavitySolver(nx, ny, RE, **kw) as bare, CavitySolver(nx, ny, RE, **kw) as passive, CavitySolver(nx, ny, RE, **kw) as s:
            passive.begin_scalar(D, sc["c0"], wall_value=sc["wall_value"])
            s.begin_scalar(D, sc["c0"], wall_value=sc["wall_value"])
            text = passive.describe()
            assert passive.buoyancy is None and "buoyancy" not in text
            s.set_buoyancy(*BUOY)
            assert s.describe() == dict(text, buoyancy=1)
            s.set_buoyancy(0.0, 0.0)
            assert s.buoyancy is None and s.describe() == text and s.steps_done == 0
            for n in (1, 6, 30):
                for x in (bare, passive, s):
                    x.step(n)
                same_fields(passive, bare, f"never set {kernel} after {s.steps_done}")
                same_fields(s, passive, f"cleared {kernel} after {s.steps_done}")
                assert np.array_equal(s.scalar_populations(stored=True), passive.scalar_populations(stored=True))
            # set mid-run, changed mid-run, cleared mid-run: the reference does the same
            o, so = _oracles(nx, ny, sc, "TRT", dtype, buoy=None)
            pair = Coupled(o, so).step(37)
            _same(s, o, so, f"passive {kernel}")
            for buoy in (BUOY, (-2e-5, 4e-5, 0.25), (0.0, 0.0, 0.0), BUOY):
                s.set_buoyancy(*buoy)
                o.set_buoyancy(*buoy)
                assert s.steps_done == o.nsteps and s.buoyancy == (buoy if any(buoy[:2]) else None)
                s.step(9); pair.step(9)
                _same(s, o, so, f"{kernel} buoyancy {buoy}")
            same = np.array_equal(s.get_fields(want_fin=True)[2], passive.step(27).get_fields(want_fin=True)[2])
            assert not same, "the buoyancy acts on the flow"
            for ender in (lambda x: x.end_scalar(), lambda x: x.set_solid(sc["mask"]), lambda x: x.set_open_cells(None), lambda x: x.set_periodic(False, False)):
                s.begin_scalar(D, 0.5).set_buoyancy(*BUOY)
                ender(s)
                assert s.scalar_active is None and s.buoyancy is None and "buoyancy" not in s.describe()
            s.begin_scalar(D, 0.5).set_buoyancy(*BUOY)
            s.set_body_motion(None).set_wall_velocity(None).set_driving_force(1e-6, 0.0).begin_scalar(D, 0.25)      # (these keep it)
            assert s.buoyancy == BUOY


def test_checkpoint_round_trip(tmp_path):
    """An exact restart: flow and scalar continue bit for bit; the file carries the three numbers and the plane."""
    nx, ny = 72, 40
    sc = _scenarios(nx, ny)[3]
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=np.zeros((nx, ny), bool), **BB) as a, \
            CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=sc["mask"], **BB) as b:
        _setup(a, sc)
        a.step(23)
        path = a.save_checkpoint(str(tmp_path / "ck"))
        a.step(17)
        with np.load(path) as z:
            assert z["buoyancy"].tolist() == list(BUOY) and z["buoyancy_plane"].shape == (nx, ny)
        assert b.load_checkpoint(path) == 23
        assert b.buoyancy == BUOY and b.periodic == (True, False) and b.driving_force == FORCE
        b.step(17)
        assert np.array_equal(a.scalar_populations(), b.scalar_populations()) and np.array_equal(a.scalar(), b.scalar())
        same_fields(b, a, "restart")
        a.set_buoyancy(0.0, 0.0)                         # a file without buoyancy clears this solver's
        path = a.save_checkpoint(str(tmp_path / "ck2"))
        b.load_checkpoint(path)
        assert b.buoyancy is None and b.scalar_active is not None


def _cavity(n, dtype, arith="strict", kernel="auto", steps=2000):
    g = CV.heated_cavity(n)
    nu, Dc = 0.05, 0.05 / 0.71
    a = CV.acceleration(1e4, 1.0, n, nu, Dc)
    with CavitySolver(n + 2, n + 2, periodic.solver_re(nu, n + 2), RT="MRT", dtype=dtype, arith=arith, kernel=kernel, solid=g["solid"], bodies=g["labels"],
                      **BB) as s:
        s.begin_scalar(Dc, 0.5, wall_value=g["wall_value"]).set_buoyancy(0.0, a, 0.5)
        s.step(steps)
        return s.get_fields(want_fin=True, out_dtype=np.float64)[2], s.scalar_populations(out_dtype=np.float64), s.describe()["kernel"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fast_arithmetic(dtype):
    """heated_cavity(62), a 64 x 64 lattice, Ra = 1e4, MRT, 2000 steps: the two routes agree bit for bit under `fast`, and the distance of
    the flow populations from the strict fp64 device run stays within FAST_HEADROOM x the recorded figure.  A long-run smoke check (MRT,
    the default rates, against the device's own strict run): the bound on `fast` with buoyancy, for the three operators and both buoyant
    modes against a long-double reference, is tests/test_arith_error_budget_rules_gpu.py."""
    f_ref, _, _ = _cavity(62, np.float64)
    a, ga, ka = _cavity(62, dtype, "fast")
    b, gb, kb = _cavity(62, dtype, "fast", "generic")
    assert (ka, kb) == ("k_step_solid", "k_step_generic") and np.array_equal(a, b) and np.array_equal(ga, gb), "fast arithmetic differs between the routes"
    err = float(np.abs(a - f_ref).max() / np.abs(f_ref).max())
    print(f"fast heated cavity, MRT {np.dtype(dtype).name}: {err:.3e} (recorded {FAST_MEASURED[dtype]}, headroom {FAST_HEADROOM:g})")
    assert np.isfinite(a).all() and err <= FAST_HEADROOM * FAST_MEASURED[dtype], err


def test_every_refusal_with_its_text():
    nx, ny = 72, 40
    z = np.zeros((nx, ny), bool)
    with CavitySolver(nx, ny, RE, solid=z, **BB) as x:
        with pytest.raises(RuntimeError, match=r"\(-4\).*no scalar is active \(lbm_scalar_begin first"):
            x.set_buoyancy(0.0, 1e-4, 0.5)
        assert x.buoyancy is None
        x.begin_scalar(0.1, 0.5)
        for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 1e-4, float("nan"))):
            with pytest.raises(RuntimeError, match=r"\(-1\).*must be finite"):
                x.set_buoyancy(*bad)
        assert x.buoyancy is None and x.lib.lbm_set_buoyancy_plane(x._h, np.zeros((nx, ny)).ctypes.data, 1) == -4
    with CavitySolver(nx, ny, RE, solid=z, tuning=dict(solid_tiles=True), **BB) as x:
        with pytest.raises(RuntimeError, match=r"\(-4\).*LBM_FLAG_SOLID_TILES"):
            x.set_buoyancy(0.0, 1e-4, 0.5)
    C, Rd = (ny - 1) / 2.0, 4.3
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    disc = np.hypot(xs - (C + 3.0), ys - C) < Rd
    q = solid.disc_fractions(disc, C + 3.0, C, Rd)
    with CavitySolver(nx, ny, RE, solid=disc, **BB) as x:
        x.set_shape(q)
        x.begin_scalar(0.1, 0.5)
        with pytest.raises(RuntimeError, match=r"\(-4\).*a shape is set"):
            x.set_buoyancy(0.0, 1e-4, 0.5)
        assert x.buoyancy is None
        x.set_shape(None)
        x.set_buoyancy(0.0, 1e-4, 0.5)
        with pytest.raises(RuntimeError, match=r"\(-4\).*buoyancy is set"):
            x.set_shape(q)
        assert x.buoyancy == (0.0, 1e-4, 0.5)
        x.set_shape(None)                                # (clearing a shape that is not there is no refusal)
        x.step(3)
        assert np.isfinite(x.get_fields()[0]).all()


def test_physics_fp64():
    """The heated cavity at Ra = 1e4 and the hydrostatic layer on the device in fp64 strict: the bounds of tests/test_buoyancy_cpu.py, and
    the reference's figures to the digits recorded."""
    r = P.check_cavity(CavitySolver, 1e4)
    P.same_as_record(r, 1e4)
    u = P.check_hydrostatic(CavitySolver)
    assert abs(u / P.RECORD["hydrostatic"] - 1.0) <= 5e-4, u
