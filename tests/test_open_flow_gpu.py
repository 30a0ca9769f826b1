"""GPU tests of the open boundaries (CavitySolver.set_open_cells, set_wall_velocity; lbm_set_open_cells, lbm_set_wall_velocity): strict
arithmetic bit for bit against the NumPy reference tests/open_flow_ref.py on the vector kernel (k_step_solid, all three wall modes) and
the generic route, over the hold-cell layouts a lane, a seam, the lid row or a neighbouring solid cell can get wrong; clearing gives the
bits of a context that never set them; `fast` arithmetic; a batch; the samplers; the force with the cell term; the checkpoint; a new mask;
every error path; and a free stream on the device."""
import math
import warnings

import numpy as np
import pytest

from checks import FAST_BOUND, HostStats, check_topology, same_as_oracle, same_fields, same_monitor_record, same_residual_record, same_stats
from curved_wall_ref import circle_fractions
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, channel, solid
from open_flow_ref import OpenFlowOracle, feq

pytestmark = pytest.mark.gpu
BB = dict(semantics="bounce_back")


def _held(nx, ny, seed):
    """Populations for the hold cells, different in every cell: the equilibrium of a random state near rho = 1 (a few per mille: at
    Re 100 on an 8-row lattice tau is 0.519, and hold cells scattered through a porous bed force it hard)."""
    r = np.random.default_rng(seed)
    return feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny)), 0.005 * r.standard_normal((nx, ny)))


def _layouts(nx, ny):
    """name -> (mask, labels, nbodies, hold, disc): where a hold cell can go wrong.  Rows are placed relative to ny (8-row lattices)."""
    ya, yb = max(1, ny // 4), min(ny - 2, ny // 4 + 3)
    z = lambda: (np.zeros((nx, ny), bool), np.zeros((nx, ny), np.int32), np.zeros((nx, ny), bool))  # noqa: E731
    out = {}
    m, lab, h = z()                                  # every lane position x mod 4 (fp64: mod 2), one per row, and a whole 16-byte vector
    for i in range(4):
        h[16 + i, ya + (i % (yb - ya + 1))] = True
    h[24:28, ya] = True
    h[32:34, yb] = True
    m[40:43, ya:yb + 1] = True
    out["lanes"] = (m, lab, 1, h, None)
    m, lab, h = z()                                  # column 0, column nx - 1, and across the seams between two workgroups' cells
    h[0, ya:yb + 1] = True
    h[nx - 1, 1:ny - 1] = True
    for seam in (512, 1024):
        if nx > seam + 4:
            h[seam - 2:seam + 2, ya] = True
            h[seam, yb] = True
    m[20:23, ya:yb + 1] = True
    out["edges"] = (m, lab, 1, h, None)
    m, lab, h = z()                                  # the lid row and all four corners
    h[5:11, 0] = True
    h[0, 0] = h[nx - 1, 0] = h[0, ny - 1] = h[nx - 1, ny - 1] = True
    m[30:33, 0:2] = True
    out["lid_corners"] = (m, lab, 1, h, None)
    m, lab, h = z()                                  # next to solid cells, orthogonally and diagonally; two bodies
    m[20:24, ya:yb] = True
    m[30:33, ya:yb] = True; lab[30:33, ya:yb] = 1
    h[19, ya] = h[24, ya + 1] = True                 # orthogonal
    h[19, yb] = h[24, yb] = h[29, yb] = True         # diagonal (the row below the blocks)
    h[21, yb] = True                                 # under the block
    h[26:28, ya] = True                              # between the two bodies, two cells from either
    out["beside_solid"] = (m, lab, 2, h, None)
    m, lab, h = z()                                  # alone in the interior
    h[nx // 2 + 1, ny // 2] = True
    m[8:10, ya:yb] = True
    out["alone"] = (m, lab, 1, h, None)
    r = np.random.default_rng(17)                    # random 10 % beside random 20 % solid
    m = r.random((nx, ny)) < 0.2
    h = (r.random((nx, ny)) < 0.1) & ~m
    out["random"] = (m, r.integers(0, 3, (nx, ny)).astype(np.int32), 3, h, None)
    m, lab, h = z()                                  # a disc about (C, C) (its exact wall distances) with hold cells around it
    C, R = (ny - 1) / 2.0, min(4.3, (ny - 3) / 2.0)
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    m[np.hypot(xs - C, ys - C) < R] = True
    h[nx - 1, :] = True
    h[int(C + R) + 2, int(C)] = True                 # two cells behind the disc: the next fluid cell of no link
    h[int(C + R) + 1, int(C) + 1] = True             # ... and one that is the cell behind a link, or itself beside the disc
    out["disc"] = (m, lab, 1, h & ~m, (C, R))
    return out


def _uw(mask, seed):
    return np.where(mask[None], np.random.default_rng(seed).uniform(-0.01, 0.01, (2,) + mask.shape), 0.0)


def _motion(nb, seed):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(-0.01, 0.01, nb), r.uniform(-0.01, 0.01, nb), r.uniform(-0.001, 0.001, nb)], axis=1)


def _modes(name, m, lab, nb, disc, seed):
    """[(tag, q, uw, motion)], every wall mode on every layout: at rest; cell velocities alone; cell velocities plus a body motion; both of
    those with a shape -- the disc with its circle's fractions, the other layouts with q uniform in (0, 1], which puts hold cells behind
    near links."""
    uw, mot = _uw(m, seed), _motion(nb, seed + 1)
    if name == "random":                             # (bodies scattered over the whole lattice: at an arm of 500 cells a rotation is no small velocity)
        mot[:, 2] = 0.0
    q = circle_fractions(m, disc[0], [disc[1]]) if disc is not None else 1.0 - np.random.default_rng(seed + 2).random((8,) + m.shape)
    return [("rest", None, None, None), ("cells", None, uw, None), ("cells+motion", None, uw, mot), ("shape cells", q, uw, None),
            ("shape cells+motion", q, uw, mot)]


# Re of the strict test: at Re 100 an 8-row lattice has tau = 0.519, at which SRT does not survive hold cells scattered through a porous
# bed (the reference itself leaves rho > 0); at Re 20 tau = 0.596 there and every case stays a flow on the reference (|u| < 0.1, rho > 0.4)
RE_STRICT = 20.0
SHAPES = {np.float32: [(72, 40), (70, 66), (1032, 8)], np.float64: [(72, 40), (70, 66), (1032, 8), (520, 8)]}
CASES = [(c, d, s) for d in (np.float32, np.float64) for c in ("SRT", "TRT", "MRT") for s in SHAPES[d]]


@pytest.mark.parametrize("coll,dtype,shape", CASES, ids=lambda v: v if isinstance(v, str) else (f"{v[0]}x{v[1]}" if isinstance(v, tuple) else np.dtype(v).name))
def test_strict_bit_identical_to_reference(coll, dtype, shape):
    """fin, u and rho after 1, 2, 7 and 37 steps from the setter's state, then from a set_state of the developed one; the default route
    and kernel='generic' against the reference and against each other."""
    nx, ny = shape
    V = 4 if dtype == np.float32 else 2
    with CavitySolver(nx, ny, RE_STRICT, RT=coll, dtype=dtype, solid=np.zeros(shape, bool), **BB) as s, \
            CavitySolver(nx, ny, RE_STRICT, RT=coll, dtype=dtype, kernel="generic", solid=np.zeros(shape, bool), **BB) as g:
        for ci, (name, (m, lab, nb, hold, disc)) in enumerate(_layouts(nx, ny).items()):
            cen = solid.centroids(m, lab, nb)
            f = _held(nx, ny, 40 + ci)
            for tag, q, uw, mot in _modes(name, m, lab, nb, disc, 60 + ci):
                o = OpenFlowOracle(nx, ny, RE_STRICT, mask=m, labels=lab, centres=cen, motion=mot, q=q, hold=hold, f=f, wall_velocity=uw,
                                   collision=coll, dtype=dtype)
                for x in (s, g):
                    x.set_solid(m).set_bodies(lab, cen)
                    assert x.open_cells is None and "open_cells" not in x.describe()
                    x.set_open_cells(hold, f)
                    d = x.describe()
                    assert d["open_cells"] == 1 and x.steps_done == 0 and np.array_equal(x.open_cells[0], hold)
                    assert np.array_equal(x.open_cells[1][:, hold], f[:, hold]) and not x.open_cells[1][:, ~hold].any()
                    if q is not None:
                        x.set_shape(q)
                        assert np.array_equal(x.shape, o.q_eff), (name, tag)
                    if uw is not None:
                        x.set_wall_velocity(uw)
                        assert x.describe()["wall_velocity"] == 1 and np.array_equal(x.wall_velocity, uw)
                    if mot is not None:
                        x.set_body_motion(mot)
                    d = x.describe()
                    assert ("wall_motion" in d) == (mot is not None) and ("wall_shape" in d) == (q is not None) and ("wall_velocity" in d) == (uw is not None)
                assert s.describe()["kernel"] == ("k_step_solid" if nx % V == 0 else "k_step_generic")
                for phase in range(2):
                    if phase:
                        st = o.fin.copy()
                        st[:, hold] = 0.25                      # (host values on hold cells are ignored)
                        o.set_state(st)
                        s.set_state(st); g.set_state(st)
                    for n in (1, 1, 5, 30):
                        s.step(n); g.step(n); o.step(n)
                        what = f"{nx}x{ny} {coll} {np.dtype(dtype).name} layout {name} mode {tag} phase {phase} after {o.nsteps}"
                        _, _, fin = same_as_oracle(s, o, what)
                        same_fields(g, s, what + " generic")
                        assert np.array_equal(fin[:, hold], f[:, hold].astype(dtype)), what + ": hold cells"
                for x in (s, g):                                # (geometry comes first: back to rest before the next layout)
                    x.set_body_motion(None).set_wall_velocity(None).set_shape(None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clearing_gives_the_bits_of_a_context_that_never_set_them(dtype):
    nx, ny = 72, 40
    m, lab, nb, hold, _ = _layouts(nx, ny)["beside_solid"]
    mot = _motion(nb, 3)
    for kernel in ("auto", "generic"):
        with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, kernel=kernel, solid=m, bodies=lab, **BB) as plain, \
                CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, kernel=kernel, solid=m, bodies=lab, **BB) as s:
            s.set_open_cells(hold, _held(nx, ny, 1))
            s.set_wall_velocity(_uw(m, 2))
            s.step(5)
            s.set_wall_velocity(np.zeros((2, nx, ny)))
            if kernel == "auto":
                s.set_open_cells(None)
            else:                                                # (an all-zero mask clears as NULL does, and needs no populations)
                assert s.lib.lbm_set_open_cells(s._h, np.zeros((nx, ny), np.uint8).ctypes.data, None) == 0
            assert s.steps_done == 0 and s.open_cells is None and not s.wall_velocity.any() and s.describe() == plain.describe()
            for n in (1, 6):
                s.step(n); plain.step(n)
                same_fields(s, plain, f"cleared {kernel} after {s.steps_done}")
            s.set_body_motion(mot); plain.set_body_motion(mot)
            s.set_wall_velocity(None)
            assert s.describe() == plain.describe() and s.describe()["wall_motion"] == 1
            s.step(4); plain.step(4)
            same_fields(s, plain, f"cleared {kernel}, with a motion")
            Fs, Fp = s.body_force(), plain.body_force()
            assert all(np.array_equal(Fs[k], Fp[k]) for k in Fp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_arithmetic(dtype):
    """The configuration of test_solid_gpu.test_fast_arithmetic (128 x 96, Re 1000, 2000 steps) with the geometry of channel() and a
    disc: the two routes agree bit for bit, and the distance from the strict fp64 run stays inside checks.FAST_BOUND.  A long-run smoke
    check (MRT, the default rates, against the device's own strict run): the bound on `fast` with hold cells and a wall velocity, for the
    three operators against a long-double reference, is tests/test_arith_error_budget_rules_gpu.py."""
    nx, ny = 128, 96
    g = channel.channel(nx, ny, 0.08, disc=(40, 47.5, 9.0))

    def run(**kw):
        with CavitySolver(nx, ny, 1000.0, RT="MRT", solid=g["solid"], bodies=g["labels"], **kw, **BB) as s:
            s.set_open_cells(g["hold"], g["f"]).set_wall_velocity(g["wall_velocity"])
            s.step(2000)
            return s.get_fields(want_fin=True, out_dtype=np.float64)[2], s.describe()["kernel"]
    f_ref, _ = run(dtype=np.float64)
    a, ka = run(dtype=dtype, arith="fast")
    b, kb = run(dtype=dtype, arith="fast", kernel="generic")
    assert (ka, kb) == ("k_step_solid", "k_step_generic") and np.array_equal(a, b), "fast arithmetic differs between the routes"
    err = float(np.abs(a - f_ref).max() / np.abs(f_ref).max())
    print(f"fast open flow MRT {np.dtype(dtype).name}: {err:.3e} (bound {FAST_BOUND[dtype]:.1e})")
    assert np.isfinite(a).all() and err < FAST_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_of_three_geometries_equals_the_lone_runs(dtype):
    nx, ny = 72, 40
    L = _layouts(nx, ny)
    names, Res = ("edges", "beside_solid", "random"), [100.0, 400.0, 1000.0]
    masks = np.stack([L[n][0] for n in names])
    holds = np.stack([L[n][3] for n in names])
    fs = np.stack([_held(nx, ny, 70 + i) for i in range(3)])
    uws = np.stack([_uw(masks[i], 80 + i) for i in range(3)])
    with CavityBatch(nx, ny, Res, RT="MRT", dtype=dtype, solid=masks, **BB) as b:
        b.set_open_cells(holds, fs).set_wall_velocity(uws)
        assert np.array_equal(b.open_cells[0], holds) and np.array_equal(b.wall_velocity, uws)
        b.step(1); b.step(22)
        u, rho, fin = b.get_fields(want_fin=True)
        F = b.solid_force()
    for i, Re in enumerate(Res):
        with CavitySolver(nx, ny, Re, RT="MRT", dtype=dtype, solid=masks[i], **BB) as s:
            s.set_open_cells(holds[i], fs[i]).set_wall_velocity(uws[i])
            s.step(23)
            u1, r1, f1 = s.get_fields(want_fin=True)
            F1 = s.solid_force()
        assert np.array_equal(fin[i], f1) and np.array_equal(u[i], u1) and np.array_equal(rho[i], r1), Re
        assert {k: F[k][i] for k in F} == F1, Re


def test_samplers_see_the_held_values():
    """monitor, residual, statistics and topology on a lattice with hold cells against their host restatements applied to get_fields of
    the same context: on a hold cell u and rho are the moments of the held values."""
    nx, ny = 72, 40
    m, lab, nb, hold, _ = _layouts(nx, ny)["beside_solid"]
    hold = hold.copy(); hold[nx - 1, 1:ny - 1] = True
    f = _held(nx, ny, 9)
    for dtype in (np.float32, np.float64):
        with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, solid=m, bodies=lab, **BB) as s:
            s.set_open_cells(hold, f).set_wall_velocity(_uw(m, 10))
            s.step(30)
            u, rho, fin = s.get_fields(want_fin=True)
            fh = f[:, hold].astype(dtype)
            r_h = ((((((((fh[0] + fh[1]) + fh[2]) + fh[3]) + fh[4]) + fh[5]) + fh[6]) + fh[7]) + fh[8])
            assert np.array_equal(fin[:, hold], fh) and np.array_equal(rho[hold], r_h)
            assert np.array_equal(u[0][hold], (((((fh[1] - fh[3]) + fh[5]) - fh[6]) - fh[7]) + fh[8]) / r_h)
            probes = ((19, ny // 4), (3, 3))
            rec = s.monitor(probes=probes)
            assert rec["nonfinite"] == 0
            same_monitor_record(rec, u, rho, s.uLB, "monitor", probes=probes)
            host = HostStats()
            s.begin_statistics(); s.begin_residual(); s.begin_monitor(every=0, capacity=4, probes=probes)
            samples = []
            for n in (0, 3, 4):
                s.step(n)
                s.sample_statistics(); s.sample_residual(); s.sample_monitor()
                uu, rr = s.get_fields()
                host.add(uu, rr)
                samples.append((s.steps_done, uu, rr))
            same_stats(s, host, "statistics")
            mon = s.monitor_series()
            assert mon["count"] == 3 and mon["dropped"] == 0
            for i, (step, uu, rr) in enumerate(samples):          # the monitor's series: every sample against the fields of its step
                r = {k: mon[k][i] for k in mon if k not in ("count", "dropped")}
                assert r["step"] == step and r["nonfinite"] == 0
                same_monitor_record(r, uu, rr, s.uLB, f"monitor series {i}", probes=probes)
            got = s.residual_series()
            assert got["count"] == 2 and got["dropped"] == 0
            for i in range(2):
                r = {k: got[k][i] for k in got if k not in ("count", "dropped")}
                assert r["nonfinite"] == 0 and r["cells"] == nx * ny
                same_residual_record(r, samples[i], samples[i + 1], f"residual {i}")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                check_topology(s, "topology", (dtype,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_force_uses_the_delta_with_the_cell_term(dtype):
    """body_force, solid_force and the force series against the reference's exactly rounded sums: links exactly; fx, fy, tz within
    links * 2^-52 * sum |terms|, the worst case of a double sum of that many terms; no link starts at a hold cell."""
    nx, ny = 72, 40
    L = _layouts(nx, ny)
    for name in ("beside_solid", "disc", "random"):
        m, lab, nb, hold, disc = L[name]
        cen, f, uw, mot = solid.centroids(m, lab, nb), _held(nx, ny, 21), _uw(m, 22), _motion(nb, 23)
        for q in ((None,) if disc is None else (None, circle_fractions(m, disc[0], [disc[1]]))):
            o = OpenFlowOracle(nx, ny, 100.0, mask=m, labels=lab, centres=cen, motion=mot, q=q, hold=hold, f=f, wall_velocity=uw,
                               collision="MRT", dtype=dtype).step(23)
            with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=dtype, solid=m, bodies=lab, centres=cen, **BB) as s:
                s.set_open_cells(hold, f)
                if q is not None:
                    s.set_shape(q)
                s.set_wall_velocity(uw).set_body_motion(mot)
                s.step(22)
                s.begin_force(every=1, capacity=4)
                s.step(1)
                F, T, series = s.body_force(), s.solid_force(), s.force_series()
            want, wt = o.body_force(), o.force()
            plain_links = len(solid.body_links(m, lab))
            assert F["links"].tolist() == want["links"].tolist() and T["links"] == wt["links"] == len(o.links) < plain_links, (name, q is None)
            for k, a in (("fx", "abs_x"), ("fy", "abs_y"), ("tz", "abs_z")):
                bound = want["links"] * 2.0 ** -52 * want[a]
                print(f"{name} shape {q is not None} {np.dtype(dtype).name} {k}: device {F[k]!r} reference {want[k]!r} bound {bound!r}")
                assert np.all(np.abs(F[k] - want[k]) <= bound), (name, k)
                assert series["count"] == 1 and np.array_equal(series[k][0], F[k]), (name, k)
            for k, a in (("fx", "abs_x"), ("fy", "abs_y")):
                assert abs(T[k] - wt[k]) <= wt["links"] * 2.0 ** -52 * wt[a], (name, k)
            if q is None:                                        # the public restatement: the same delta, hence the same terms
                t = solid.host_open_tables(m, lab, cen, mot, uw, hold, dtype=dtype)
                assert [tuple(r) for r in t["links"].tolist()] == o.links
                assert np.array_equal(t["delta"], [float(o.delta[k, x, y]) for x, y, k, _ in o.links])
                rest = OpenFlowOracle(nx, ny, 100.0, mask=m, labels=lab, centres=cen, motion=mot, hold=hold, f=f, collision="MRT", dtype=dtype)
                assert np.any(rest.delta != o.delta)            # (the cell term is in it)


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    nx, ny = 72, 40
    m, lab, nb, hold, disc = _layouts(nx, ny)["disc"]
    f, uw, mot, q = _held(nx, ny, 31), _uw(m, 32), _motion(nb, 33), circle_fractions(m, disc[0], [disc[1]])
    for shaped in (False, True):
        with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, bodies=lab, **BB) as s:
            s.set_open_cells(hold, f)
            if shaped:
                s.set_shape(q)
            s.set_wall_velocity(uw).set_body_motion(mot)
            s.step(25)
            path = s.save_checkpoint(str(tmp_path / f"open{int(shaped)}"))
            s.step(30)
            want = s.get_fields(want_fin=True)
        with np.load(path) as z:
            assert np.array_equal(z["open_hold"], hold) and np.array_equal(z["open_f"][:, hold], f[:, hold]) and np.array_equal(z["wall_velocity"], uw)
        with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, **BB) as r:
            assert r.load_checkpoint(path) == 25
            assert np.array_equal(r.open_cells[0], hold) and np.array_equal(r.wall_velocity, uw) and (r.shape is not None) == shaped
            r.step(30)
            got = r.get_fields(want_fin=True)
        assert all(np.array_equal(a, b) for a, b in zip(want, got)), shaped
    with CavitySolver(nx, ny, 400.0, RT="MRT", dtype=np.float32, solid=m, **BB) as plain:      # files of other runs are unchanged
        plain.step(3)
        with np.load(plain.save_checkpoint(str(tmp_path / "plain"))) as z:
            assert not {"open_hold", "open_f", "wall_velocity"} & set(z.files)


def test_a_new_mask_resets_hold_cells_and_velocities():
    nx, ny = 72, 40
    m, lab, nb, hold, _ = _layouts(nx, ny)["beside_solid"]
    with CavitySolver(nx, ny, 100.0, RT="MRT", dtype=np.float32, solid=m, bodies=lab, **BB) as s, \
            CavitySolver(nx, ny, 100.0, RT="MRT", dtype=np.float32, solid=m, **BB) as plain:
        s.set_open_cells(hold, _held(nx, ny, 5)).set_wall_velocity(_uw(m, 6))
        s.step(4)
        s.set_bodies(np.zeros((nx, ny), np.int32))                  # new bodies keep both
        assert s.describe()["open_cells"] == 1 and s.describe()["wall_velocity"] == 1 and s.wall_velocity.any()
        s.set_solid(m)
        assert s.open_cells is None and not s.wall_velocity.any() and s.steps_done == 0 and s.describe() == plain.describe()
        hb = np.zeros((nx, ny), np.uint8)
        assert s.lib.lbm_get_open_cells(s._h, hb.ctypes.data, None) == 0 and not hb.any()
        s.step(7); plain.step(7)
        same_fields(s, plain, "after the new mask")


def test_error_paths():
    nx, ny = 72, 40
    m, lab, nb, hold, _ = _layouts(nx, ny)["beside_solid"]
    f, uw = _held(nx, ny, 1), _uw(m, 2)
    INVALID, STATE = -1, -4
    with CavitySolver(nx, ny, 100.0, **BB) as plain:                   # another semantics
        with pytest.raises(RuntimeError, match="no solid mask"):
            plain.set_open_cells(hold, f)
        h8 = hold.astype(np.uint8)
        assert plain.lib.lbm_set_open_cells(plain._h, h8.ctypes.data, f.ctypes.data) == STATE
        assert plain.lib.lbm_get_open_cells(plain._h, h8.ctypes.data, None) == STATE
        assert plain.lib.lbm_set_wall_velocity(plain._h, uw.ctypes.data) == STATE and plain.lib.lbm_get_wall_velocity(plain._h, uw.ctypes.data) == STATE
        assert plain.open_cells is None and plain.wall_velocity is None
    with CavitySolver(nx, ny, 100.0, solid=m, bodies=lab, **BB) as s:
        def refused(code, text, hold_, f_):
            h8_ = np.ascontiguousarray(hold_, dtype=np.uint8)
            f_ = np.ascontiguousarray(f_)
            assert s.lib.lbm_set_open_cells(s._h, h8_.ctypes.data, f_.ctypes.data) == code
            assert text in s.lib.lbm_last_error(s._h).decode(), s.lib.lbm_last_error(s._h)
        bad = hold.copy(); bad[21, max(1, ny // 4)] = True
        refused(INVALID, "is a solid cell", bad, f)
        for v in (np.nan, np.inf, -1e-9):
            fb = f.copy(); fb[3][np.nonzero(hold)[0][0], np.nonzero(hold)[1][0]] = v
            refused(INVALID, "not finite or is negative", hold, fb)
        fb = f.copy(); fb[:, ~hold] = np.nan                            # (read on hold cells only)
        s.set_open_cells(hold, fb)
        refused(INVALID, "without a fluid cell", ~m, f)
        assert s.lib.lbm_set_open_cells(s._h, hold.astype(np.uint8).ctypes.data, None) == INVALID
        with pytest.raises(ValueError, match="shape"):
            s.set_open_cells(hold, f[:8])
        with pytest.raises(ValueError, match="shape"):
            s.set_wall_velocity(uw[0])
        assert np.array_equal(s.open_cells[0], hold)                    # (the refused calls left the context as it was)
        # geometry comes first
        s.set_shape(np.full((8, nx, ny), 0.5))
        refused(STATE, "geometry comes first", hold, f)
        s.set_wall_velocity(uw)
        with pytest.raises(RuntimeError, match="the shape first"):
            s.set_shape(None)
        s.set_wall_velocity(None).set_shape(None)
        s.set_wall_velocity(uw)
        refused(STATE, "geometry comes first", hold, f)
        s.set_wall_velocity(None).set_body_motion(_motion(nb, 4))
        refused(STATE, "geometry comes first", hold, f)
        s.set_body_motion(None)
        bad_uw = uw.copy(); bad_uw[1][m] = np.inf
        with pytest.raises(RuntimeError, match="not finite"):
            s.set_wall_velocity(bad_uw)
        off = uw.copy(); off[:, ~m] = np.nan                            # (read on solid cells only)
        s.set_wall_velocity(off)
        assert np.array_equal(s.wall_velocity, uw)
    # a closed lattice: the flux check holds, with the cell terms inside S and A
    inlet = np.zeros((nx, ny), bool); inlet[0, :] = True
    push = np.zeros((2, nx, ny)); push[0, 0, :] = 0.03
    with CavitySolver(nx, ny, 100.0, solid=inlet, **BB) as s:
        o = OpenFlowOracle(nx, ny, 100.0, mask=inlet, wall_velocity=push)
        with pytest.raises(RuntimeError, match="lbm_set_wall_velocity: lattice 0: the motion has a net flux") as e:
            s.set_wall_velocity(push)
        assert f"{o.S:.6g}" in str(e.value) and f"{o.A:.6g}" in str(e.value) and f"{len(o.links)} links" in str(e.value)
        assert not s.wall_velocity.any() and "wall_velocity" not in s.describe()
        belt = np.zeros((2, nx, ny)); belt[1, 0, :] = 0.04               # tangential: passes
        s.set_wall_velocity(belt)
        with pytest.raises(RuntimeError, match="lbm_set_body_motion: lattice 0"):
            s.set_body_motion([[0.02, 0.0, 0.0]])
        out = np.zeros((nx, ny), bool); out[nx - 1, 5] = True
        s.set_wall_velocity(None)
        s.set_open_cells(out, _held(nx, ny, 3))                          # one hold cell opens the lattice
        s.set_wall_velocity(push).set_body_motion([[0.02, 0.0, 0.0]])
        s.step(3)
        assert np.isfinite(s.get_fields(want_fin=True)[2]).all()
    with CavitySolver(128, 128, 100.0, solid=np.zeros((128, 128), bool), tuning=dict(solid_tiles=True), **BB) as t:      # the tile kernel never sees bit 9
        h = np.zeros((128, 128), bool); h[127, 5:100] = True
        with pytest.raises(RuntimeError, match="tile kernel"):
            t.set_open_cells(h, _held(128, 128, 1))
        t.set_solid(np.pad(np.ones((4, 4), bool), ((20, 104), (20, 104))))
        w = np.zeros((2, 128, 128)); w[1, 20:24, 20:24] = 0.01
        with pytest.raises(RuntimeError, match="tile kernel"):
            t.set_wall_velocity(w)
        t.set_wall_velocity(np.zeros((2, 128, 128)))      # (all zero: nothing to refuse)
        assert t.lib.lbm_set_open_cells(t._h, None, None) == STATE


def test_free_stream_on_the_device():
    """The free stream of tests/test_open_flow_cpu.py on the device, fp64 strict: the reference's bits after 500 steps."""
    nx, ny, U = 40, 24, 0.05
    g = channel.channel(nx, ny, U, profile="plug", walls="stream")
    o = OpenFlowOracle(nx, ny, 100.0, uLB=U, mask=g["solid"], hold=g["hold"], f=g["f"], wall_velocity=g["wall_velocity"], collision="TRT",
                       dtype=np.float64).step(500)
    with CavitySolver(nx, ny, 100.0, RT="TRT", uLB=U, dtype=np.float64, solid=g["solid"], **BB) as s:
        s.set_open_cells(g["hold"], g["f"]).set_wall_velocity(g["wall_velocity"])
        s.step(500)
        u, _, _ = same_as_oracle(s, o, "free stream after 500")
    fl = o.fluid()
    assert float(np.abs(u[0][fl] - U).max() / U) < 0.02 and math.isfinite(float(u.sum()))
