"""GPU tests of the relaxation field of the obstacle lattices (CavitySolver.set_relaxation_field, set_viscosity, get_tau;
lbm_set_relaxation_field): strict arithmetic bit for bit against the NumPy reference tests/viscosity_ref.py -- fin, u, rho and the tau of
the next step -- with a seeded random omega in [0.55, 1.95], distinct in every cell (TRT: without and with a second random plane), on the
vector kernel (40 x 24), the one-cell route (37 x 24), across workgroup seams (1032 x 8, fp64 520 x 8), on the non-temporal route and in a
batch of three different fields, from the initial state and from a set_state; the scenarios of tests/subgrid_cases.py with a field, and
with a field and the closure; clearing; `fast` inside the budget of tests/cases.py against the long-double chain; the two-layer Poiseuille
flow; the checkpoint; every refusal."""
import numpy as np
import pytest

from cases import K
from checks import FAST_BOUND, perturbed, same_as_oracle, same_fields
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, periodic, solid, viscosity
from subgrid_cases import scenarios, setup
import viscosity_cases as VC
from viscosity_ref import ViscosityOracle, ViscositySolidOracle

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")
CS2 = 0.025
RE = 400.0
COLLS = ("SRT", "TRT", "MRT")
# (operator, with a second plane): TRT runs both ways
VARIANTS = (("SRT", False), ("TRT", False), ("TRT", True), ("MRT", False))
DTYPES = (np.float32, np.float64)


def _mask(nx, ny, seed=3):
    """Solid cells in the wall columns and beside them, in the lid row and beside it, on the bottom row, in the first and the last lane
    of a vector (fp32: x = 4 .. 7, fp64: 8 .. 9), a block, and a sprinkling of random cells."""
    m = np.random.default_rng(seed).random((nx, ny)) < 0.04
    for x, y in ((0, 10), (1, 15), (nx - 1, 5), (nx - 2, 17), (10, 0), (14, 1), (nx - 2, ny - 1), (4, 8), (7, 8), (8, 12), (9, 13), (11, 13)):
        m[x, y] = True
    m[20:24, 10:14] = True
    return m


def _planes(nx, ny, second, seed=21):
    return VC.random_rates((nx, ny), seed), (VC.random_rates((nx, ny), seed + 1) if second else None)


def _route(nx, dtype, kernel="auto"):
    return "k_step_solid" if kernel == "auto" and nx % (4 if dtype == np.float32 else 2) == 0 else "k_step_generic"


def _same_tau(s, o, what):
    tau, want = s.get_tau(), o.peek_tau()
    assert tau.dtype == want.dtype and np.array_equal(tau, want), f"{what}: tau differs in {np.count_nonzero(tau != want)} cells"
    return tau


def _walk(s, o, what, nx, ny, dtype, calls=(1, 6, 30)):
    """1, 7 and 37 steps from the initial state, then the same from a set_state; fin, u, rho and the tau of the next step each time."""
    for phase in range(2):
        if phase:
            st = perturbed(nx, ny, dtype, 11)
            o.set_state(st); s.set_state(st)
        _same_tau(s, o, f"{what} raw phase {phase}")
        for n in calls:
            s.step(n); o.step(n)
            tag = f"{what} phase {phase} after {o.nsteps}"
            same_as_oracle(s, o, tag)
            _same_tau(s, o, tag)


@pytest.mark.parametrize("nx", [40, 37])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("coll,second", VARIANTS)
def test_strict_bit_identical_to_reference(coll, second, dtype, nx):
    ny = 24
    m = _mask(nx, ny)
    w, wm = _planes(nx, ny, second)
    o = ViscositySolidOracle(nx, ny, RE, mask=m, collision=coll, dtype=dtype, omega_field=w, omegam_field=wm)
    with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, solid=m, **BB) as s:
        assert s.relaxation_field is None and "relax_field" not in s.describe()
        s.set_relaxation_field(w, wm)
        d = s.describe()
        assert d.get("relax_field+m" if second else "relax_field") is True and s.steps_done == 0 and d["kernel"] == _route(nx, dtype)
        gw, gwm = s.relaxation_field
        assert np.array_equal(gw, o.w_field.astype(np.float64)) and ((gwm is None) if not second else np.array_equal(gwm, o.wm_field.astype(np.float64)))
        _walk(s, o, f"{nx}x{ny} {coll}{'+m' if second else ''} {np.dtype(dtype).name}", nx, ny, dtype)
        tau = s.get_tau()
        assert np.all(tau[m] == o.lattice_tau0()) and np.unique(tau[~m]).size > 0.9 * np.count_nonzero(~m)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_strict_across_workgroup_seams_and_on_the_nt_route(dtype):
    """1032 x 8 (fp64: 520 x 8): two workgroups per row; then 40 x 24 with non-temporal accesses."""
    nx, ny = (1032, 8) if dtype == np.float32 else (520, 8)
    m = np.random.default_rng(5).random((nx, ny)) < 0.03
    for coll, second in VARIANTS:
        w, wm = _planes(nx, ny, second, seed=31)
        o = ViscositySolidOracle(nx, ny, RE, mask=m, collision=coll, dtype=dtype, omega_field=w, omegam_field=wm)
        with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, solid=m, **BB) as s:
            s.set_relaxation_field(w, wm)
            assert s.describe()["kernel"] == "k_step_solid"
            for n in (1, 6):
                s.step(n); o.step(n)
                same_as_oracle(s, o, f"seam {coll} after {o.nsteps}")
            _same_tau(s, o, f"seam {coll}")
    nx, ny = 40, 24
    m = _mask(nx, ny)
    for coll, second in VARIANTS:
        w, wm = _planes(nx, ny, second)
        o = ViscositySolidOracle(nx, ny, RE, mask=m, collision=coll, dtype=dtype, omega_field=w, omegam_field=wm)
        with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, solid=m, tuning=dict(nt=True), **BB) as s:
            s.set_relaxation_field(w, wm)
            d = s.describe()
            assert d["kernel"] == "k_step_solid" and d.get("nt") == 1, d
            for n in (1, 6, 30):
                s.step(n); o.step(n)
                same_as_oracle(s, o, f"nt {coll} after {o.nsteps}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("cs2", [0.0, CS2], ids=["field", "field+closure"])
def test_strict_with_the_closure_and_the_generic_route(cs2, dtype):
    """At rest with the closure on top of the field, vector kernel and both one-cell routes (by width, by request)."""
    ny = 24
    for nx, kernel in ((40, "auto"), (40, "generic"), (37, "auto")):
        m = _mask(nx, ny)
        for coll, second in VARIANTS:
            if cs2 == 0.0 and kernel == "auto":
                continue      # (test_strict_bit_identical_to_reference)
            w, wm = _planes(nx, ny, second)
            o = ViscositySolidOracle(nx, ny, RE, cs2=cs2, mask=m, collision=coll, dtype=dtype, omega_field=w, omegam_field=wm)
            with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, kernel=kernel, solid=m, **BB) as s:
                s.set_relaxation_field(w, wm)
                if cs2:
                    s.set_subgrid(cs2)
                assert s.describe()["kernel"] == _route(nx, dtype, kernel)
                _walk(s, o, f"{nx} {kernel} {coll}{'+m' if second else ''} cs2={cs2}", nx, ny, dtype, calls=(1, 6))


def _oracle(nx, ny, sc, coll, dtype, cs2, w, wm):
    tag, per, force, m, lab, nb, q, uw, mot, hold, f = sc
    return ViscosityOracle(nx, ny, RE, cs2=cs2, omega_field=w, omegam_field=wm, mask=m, labels=lab, centres=solid.centroids(m, lab, nb), periodic=per,
                           force=force, q=q, wall_velocity=uw, motion=mot, hold=hold, f=f, collision=coll, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("cs2", [0.0, CS2], ids=["field", "field+closure"])
@pytest.mark.parametrize("nx,kernel", [(72, "auto"), (69, "auto")])
def test_strict_with_the_other_rules(nx, kernel, cs2, dtype):
    """The scenarios of tests/subgrid_cases.py -- a motion with a wall velocity, a shape, hold cells, periodic sides, the force -- 72 wide
    (the vector kernel) and 69 wide (the one-cell route), with a field and with a field and the closure.  One variant per scenario at
    rest, all four with a motion or a shape."""
    ny = 40
    want = _route(nx, dtype, kernel)
    for i, sc in enumerate(scenarios(nx, ny)):
        tag, per, force, m, lab, nb, q, uw, mot, hold, f = sc
        for coll, second in (VARIANTS if (q is not None or mot is not None) else (VARIANTS[i % 4],)):
            w, wm = _planes(nx, ny, second, seed=41 + i)
            o = _oracle(nx, ny, sc, coll, dtype, cs2, w, wm)
            with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, kernel=kernel, solid=np.zeros((nx, ny), bool), **BB) as s:
                s.set_relaxation_field(w, wm)      # (before the geometry: the field survives the setters)
                setup(s, sc)
                if cs2:
                    s.set_subgrid(cs2)
                d = s.describe()
                assert d["kernel"] == want and ("relax_field+m" if second else "relax_field") in d and ("subgrid" in d) == bool(cs2)
                for phase in range(2):
                    if phase:
                        st = o.fin.copy()
                        o.set_state(st); s.set_state(st)
                    for n in (1, 6, 30):
                        s.step(n); o.step(n)
                        what = f"{nx}x{ny} {coll}{'+m' if second else ''} {np.dtype(dtype).name} cs2={cs2} {tag} phase {phase} after {o.nsteps}"
                        same_as_oracle(s, o, what)
                        tau = _same_tau(s, o, what)
                        if o.hold is not None:
                            assert np.all(tau[o.hold] == o.lattice_tau0()), what


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_batch_of_three_different_fields(dtype):
    nx, ny = 40, 24
    m = _mask(nx, ny)
    Res = [100.0, 400.0, 5000.0]
    w = np.stack([VC.random_rates((nx, ny), 50 + i) for i in range(3)])
    wm = np.stack([VC.random_rates((nx, ny), 60 + i) for i in range(3)])
    with CavityBatch(nx, ny, Res, RT="TRT", dtype=dtype, solid=np.stack([m] * 3), **BB) as b:
        b.set_relaxation_field(w, wm)
        b.step(1); b.step(36)
        u, rho, fin = b.get_fields(want_fin=True)
        tau = b.get_tau()
        gw, gwm = b.relaxation_field
    for i, Re in enumerate(Res):
        o = ViscositySolidOracle(nx, ny, Re, mask=m, collision="TRT", dtype=dtype, omega_field=w[i], omegam_field=wm[i]).step(37)
        assert np.array_equal(fin[i], o.fin) and np.array_equal(u[i], o.u) and np.array_equal(rho[i], o.rho), Re
        assert np.array_equal(tau[i], o.peek_tau()) and np.all(tau[i][m] == o.lattice_tau0()), Re      # (solid cells: each lattice its own tau0)
        assert np.array_equal(gw[i], o.w_field.astype(np.float64)) and np.array_equal(gwm[i], o.wm_field.astype(np.float64))
    # one [X, Y] field is broadcast over the batch
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=dtype, solid=np.stack([m] * 3), **BB) as b:
        b.set_viscosity(0.01 + 0.1 * (w[0] - VC.W_LO))
        b.step(7)
        fin = b.get_fields(want_fin=True)[2]
    for i, Re in enumerate(Res):
        o = ViscositySolidOracle(nx, ny, Re, mask=m, collision="MRT", dtype=dtype, omega_field=viscosity.rates(0.01 + 0.1 * (w[0] - VC.W_LO))[0]).step(7)
        assert np.array_equal(fin[i], o.fin), Re


@pytest.mark.parametrize("kernel", ["auto", "generic"])
def test_clearing_gives_the_bits_and_the_text_of_a_context_that_never_set_it(kernel):
    nx, ny = 40, 24
    m = _mask(nx, ny)
    w, wm = _planes(nx, ny, True)
    for dtype in DTYPES:
        with CavitySolver(nx, ny, RE, RT="TRT", dtype=dtype, kernel=kernel, solid=m, **BB) as plain, \
                CavitySolver(nx, ny, RE, RT="TRT", dtype=dtype, kernel=kernel, solid=m, **BB) as s:
            tau0 = plain.get_tau()
            s.set_relaxation_field(w, wm).set_relaxation_field(None)
            assert s.relaxation_field is None and s.describe() == plain.describe() and np.array_equal(s.get_tau(), tau0)
            s.set_viscosity(np.full((nx, ny), 0.05)).set_viscosity(None)
            assert s.relaxation_field is None
            for n in (1, 9):
                s.step(n); plain.step(n)
                same_fields(s, plain, f"cleared {kernel} after {s.steps_done}")
            # a field equal to the lattice's rates is the plain context bit for bit, through the other kernels
            s.set_relaxation_field(np.full((nx, ny), s.relax["omega"]), np.full((nx, ny), s.relax["omegam"]))
            s.step(7); plain.step(7)
            same_fields(s, plain, f"uniform field {kernel}")
            # the call restarts nothing: setting it mid-run continues from the state as it is
            o = ViscositySolidOracle(nx, ny, RE, mask=m, collision="TRT", dtype=dtype).step(17)
            s.set_relaxation_field(w, wm); o.set_relaxation_field(w, wm)
            assert s.steps_done == 17
            s.step(7); o.step(7)
            same_as_oracle(s, o, f"set mid-run {kernel}")
            # ... and it survives set_relaxation and set_solid
            s.set_relaxation(omegam=1.3)
            s.set_solid(m)
            assert s.relaxation_field is not None and "relax_field+m" in s.describe()


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    nx, ny = 40, 24
    m = _mask(nx, ny)
    w, wm = _planes(nx, ny, True)
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=m, **BB) as s:
        s.set_relaxation_field(w, wm)
        s.step(25)
        path = s.save_checkpoint(str(tmp_path / "field"))
        s.step(30)
        want = s.get_fields(want_fin=True)
        held = s.relaxation_field
    with np.load(path) as z:
        assert np.array_equal(z["relax_omega"], held[0]) and np.array_equal(z["relax_omegam"], held[1])
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=m, **BB) as r:
        r.begin_scalar(0.05, 1.0)
        r.set_buoyancy(0.0, 1e-4, 1.0)                         # (the file's field clears this solver's buoyancy)
        assert r.load_checkpoint(path) == 25 and r.buoyancy is None
        assert all(np.array_equal(a, b) for a, b in zip(r.relaxation_field, held))
        r.step(30)
        got = r.get_fields(want_fin=True)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
    with CavitySolver(nx, ny, RE, RT="TRT", dtype=np.float32, solid=m, **BB) as plain:      # files of other runs are unchanged
        plain.step(3)
        p2 = plain.save_checkpoint(str(tmp_path / "plain"))
        with np.load(p2) as z:
            assert "relax_omega" not in z.files and "relax_omegam" not in z.files
        plain.set_relaxation_field(w)
        plain.load_checkpoint(p2)                              # (a file without the arrays clears the field)
        assert plain.relaxation_field is None


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("coll,second", VARIANTS)
def test_fast_stays_within_the_budget(coll, second, dtype):
    """arith = fast with a field (and with a field and the closure) against the long-double chain: err(X) = max |X - X_ref| / max |X_ref|
    over the fluid cells for fin, u / uLB and rho after 1, 2, 5, 13 and 26 steps from an off-equilibrium state; err_fast <= 32 eps after
    one step and err_fast <= K max(err_strict, eps) after every call, K of tests/cases.py; and inside checks.FAST_BOUND."""
    nx, ny = 40, 24
    m = _mask(nx, ny)
    w, wm = _planes(nx, ny, second)
    eps = float(np.finfo(dtype).eps)
    st = perturbed(nx, ny, dtype, 13)
    worst = 0.0
    for cs2 in (0.0, CS2):
        ref = ViscositySolidOracle(nx, ny, RE, cs2=cs2, mask=m, collision=coll, dtype=np.longdouble, param_dtype=dtype, omega_field=w, omegam_field=wm)
        ref.set_state(st.astype(np.longdouble))
        with CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, solid=m, **BB) as a, \
                CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, arith="fast", solid=m, **BB) as f, \
                CavitySolver(nx, ny, RE, RT=coll, dtype=dtype, arith="fast", kernel="generic", solid=m, **BB) as g:
            for x in (a, f, g):
                x.set_relaxation_field(w, wm)
                if cs2:
                    x.set_subgrid(cs2)
                x.set_state(st)
            done = 0
            for n in (1, 1, 3, 8, 13):
                done += n
                ref.step(n)
                want = dict(fin=ref.fin[:, ~m], u=ref.u[:, ~m], rho=ref.rho[~m])
                errs = {}
                for name, x in (("strict", a), ("fast", f), ("generic", g)):
                    x.step(n)
                    u, rho, fin = x.get_fields(want_fin=True)
                    got = dict(fin=fin[:, ~m], u=u[:, ~m], rho=rho[~m])
                    errs[name] = {k: float(np.abs(got[k].astype(np.longdouble) - want[k]).max() / np.abs(want[k]).max()) for k in got}
                    errs[name]["u"] *= float(np.abs(want["u"]).max()) / 0.08
                same_fields(g, f, f"fast, both routes, after {done}")
                for k in ("fin", "u", "rho"):
                    es, ef = errs["strict"][k], errs["fast"][k]
                    ratio = ef / max(es, eps)
                    worst = max(worst, ratio)
                    print(f"{coll}{'+m' if second else ''} {np.dtype(dtype).name} cs2={cs2} after {done} {k}: strict {es / eps:.2f} eps, fast {ef / eps:.2f} eps, ratio {ratio:.2f}")
                    if done == 1:
                        assert ef <= 32 * eps, (k, ef / eps)
                    assert ef <= K * max(es, eps), (k, done, ratio)
                    assert ef < FAST_BOUND[dtype]
    print(f"largest ratio {worst:.2f}")


# ---- two-layer Poiseuille ---------------------------------------------------------------------------------------------------------------
# The CPU test's figures (tests/test_viscosity_cpu.py), and at 64 fluid rows what the same reference measured once.
TWO_LAYER_A = {16: 2.22e-11, 32: 1.58e-11, 64: 1.90e-11}      # (64 rows with the uniform omega-: 3.7369e-4, a ratio of 4.003 to 32 rows)
RATIO_16_32, FACTOR, RATIO_TOL = 5.9809e-3 / 1.49581e-3, 10.0, 0.15


def _two_layer_device(H, per_cell):
    c = VC.two_layer(H)
    with CavitySolver(c["nx"], c["ny"], c["Re"], RT="TRT", dtype=np.float64, solid=c["solid"], **BB) as s:
        s.set_relaxation(omegam=c["omegam_uniform"])
        s.set_periodic(*c["periodic"])
        s.set_driving_force(VC.FORCE, 0.0)
        s.set_viscosity(c["nu"], VC.MAGIC if per_cell else None)
        assert s.describe()["kernel"] == "k_step_solid"
        s.step(c["steps"])
        u, rho, fin = s.get_fields(want_fin=True)
    return u, rho, fin, c


def test_two_layer_poiseuille_on_the_device():
    """fp64 TRT, 18, 34 and 66 rows (16, 32, 64 fluid rows), 40 H^2 steps.  At 18 rows the state is the reference's bit for bit, with
    both rates per cell and with the uniform omega-.  With both rates per cell the profile error stays below 10 times what the reference
    measured; with the uniform omega- the error ratio between successive heights lies within 15 % of the reference's 16 / 32 ratio."""
    err = {}
    for per_cell in (True, False):
        o, _ = VC.two_layer_reference(16, per_cell)
        for H in (16, 32, 64):
            u, rho, fin, c = _two_layer_device(H, per_cell)
            err[H, per_cell] = VC.two_layer_error(u, rho, c)
            print(f"two-layer Poiseuille on the device, H = {H}, {'magic per cell' if per_cell else 'uniform omega-'}: {err[H, per_cell]:.4e}")
            if H == 16:
                assert np.array_equal(fin, o.fin) and np.array_equal(u, o.u) and np.array_equal(rho, o.rho), per_cell
    for H in (16, 32, 64):
        assert err[H, True] < FACTOR * TWO_LAYER_A[H], (H, err[H, True])
    for a, b in ((16, 32), (32, 64)):
        r = err[a, False] / err[b, False]
        print(f"uniform omega-: error ratio {a} / {b} rows = {r:.4f} (reference, 16 / 32: {RATIO_16_32:.4f})")
        assert abs(r / RATIO_16_32 - 1.0) < RATIO_TOL, (a, b, r)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    nx, ny = 40, 24
    m = _mask(nx, ny)
    INVALID, STATE = -1, -4
    w, wm = _planes(nx, ny, True)
    wp, wmp = w.ctypes.data, wm.ctypes.data
    with CavitySolver(nx, ny, 100.0, **BB) as plain:                   # another semantics
        with pytest.raises(RuntimeError, match="no solid mask"):
            plain.set_relaxation_field(w)
        assert plain.lib.lbm_set_relaxation_field(plain._h, wp, None) == STATE
        assert plain.lib.lbm_set_relaxation_field(plain._h, None, None) == 0 and plain.lib.lbm_get_relaxation_field(plain._h, None, None) == 0
    with CavitySolver(nx, ny, 100.0, semantics="mrt_gpu", turb=1) as wet:
        assert wet.lib.lbm_set_relaxation_field(wet._h, wp, None) == STATE
    for coll in ("SRT", "MRT"):                                        # omega- is TRT's
        with CavitySolver(nx, ny, 100.0, RT=coll, solid=m, **BB) as s:
            assert s.lib.lbm_set_relaxation_field(s._h, wp, wmp) == STATE and "not TRT" in s.lib.lbm_last_error(s._h).decode()
            assert s.relaxation_field is None
            s.set_relaxation_field(w)
    with CavitySolver(nx, ny, 100.0, RT="TRT", solid=m, **BB) as s:
        def refused(code, text, call):
            assert call() == code
            assert text in s.lib.lbm_last_error(s._h).decode(), s.lib.lbm_last_error(s._h)
        for v in (0.0, 2.0, -0.5, 2.5, np.nan, np.inf, -np.inf):
            bad = w.copy()
            bad[7, 5] = v
            bad[9, 3] = v                                              # (a later cell: the first one is named)
            refused(INVALID, "omega of lattice 0, cell (7, 5)", lambda: s.lib.lbm_set_relaxation_field(s._h, bad.ctypes.data, None))
            refused(INVALID, "omegam of lattice 0, cell (7, 5)", lambda: s.lib.lbm_set_relaxation_field(s._h, wp, bad.ctypes.data))
        bad = w.copy()
        sx, sy = np.argwhere(m)[0]
        bad[sx, sy] = 3.0                                              # (a solid cell is checked the same way)
        refused(INVALID, f"cell ({sx}, {sy})", lambda: s.lib.lbm_set_relaxation_field(s._h, bad.ctypes.data, None))
        assert s.relaxation_field is None
        refused(INVALID, "omegam without omega", lambda: s.lib.lbm_set_relaxation_field(s._h, None, wmp))
        assert s.lib.lbm_set_relaxation_field(None, wp, None) == INVALID and s.lib.lbm_get_relaxation_field(None, None, None) == INVALID
        with pytest.raises(ValueError, match="must have shape"):
            s.set_relaxation_field(w[:, 1:])
        # a passive scalar is allowed and keeps its own diffusivity; buoyancy and the field refuse each other
        s.begin_scalar(0.05, 1.0)
        s.set_relaxation_field(w, wm)
        s.step(3)
        assert s.scalar_active["D"] == 0.05
        refused(STATE, "a relaxation field is set", lambda: s.lib.lbm_set_buoyancy(s._h, 0.0, 1e-4, 1.0))
        assert s.buoyancy is None
        s.set_relaxation_field(None).set_buoyancy(0.0, 1e-4, 1.0)
        refused(STATE, "buoyancy is set", lambda: s.lib.lbm_set_relaxation_field(s._h, wp, None))
        assert s.relaxation_field is None
        s.set_buoyancy(0.0, 0.0)
        s.set_relaxation_field(w)
    with CavitySolver(128, 128, 100.0, solid=np.zeros((128, 128), bool), tuning=dict(solid_tiles=True), **BB) as t:      # the tile kernel
        with pytest.raises(RuntimeError, match="tile kernel"):
            t.set_relaxation_field(np.full((128, 128), 1.0))
        t.set_relaxation_field(None)                            # (clearing: nothing to refuse)
