"""The case grids and case tables that more than one test file uses: the route grid of the sampler tests, the windows of the topology
readers, the masks and tile shapes of the solid-obstacle tests, and the constants, masks, bodies and helpers of the arithmetic error
budgets, the cases of the obstacle rules (shape, hold cells, periodic sides, scalar, buoyancy) among them.  Nothing here needs a device: the GPU files and the CPU files that check their cases by dry runs both read them from here.
The comparisons are in tests/checks.py, the labelled bodies and the Taylor-Couette case in tests/body_cases.py."""
import itertools

import numpy as np

from latticeboltzmannsimulations_amd import launch_plan
from oracle.lbm_fast import mrt_fast, srt_trt_fast


# ---- the route grid of the monitor, residual, statistics and topology GPU tests ------------------------------------------------------
def route_valid(cfg, size):
    """lbm_plan accepts the configuration (a dry run).  size: (nx, ny), or kernel -> (nx, ny)."""
    kernel, dtype, coll, turb, sem, arith = cfg
    nx, ny = size[kernel] if isinstance(size, dict) else size
    try:
        launch_plan(nx, ny, 1000.0, RT=coll, dtype=dtype, turb=turb, semantics=sem, kernel=kernel, arith=arith)
        return True
    except (RuntimeError, ValueError):
        return False


def route_id(c):
    return f"{c[0]}-{np.dtype(c[1]).name}-{c[2]}-t{c[3]}-{c[4]}-{c[5]}"


def route_cases(routes, ariths, size_of, seed=None, sample=0, extras=()):
    """(kernel, dtype, operator, closure, semantics, arithmetic) cases: of the product of `routes` x fp32 / fp64 x SRT / TRT / MRT x
    closure off / on x the three wall semantics x `ariths` that lbm_plan accepts at `size_of`, the first per (route, semantics,
    arithmetic) in product order, then `sample` of the rest drawn with `seed` (in product order), then those of `extras` not yet there.
    Without a sample, nothing past a key's first valid case is planned."""
    pick, others = {}, []
    for c in itertools.product(routes, [np.float32, np.float64], ["SRT", "TRT", "MRT"], [0, 1], ["mrt_gpu", "mrt_py", "bounce_back"], ariths):
        key = (c[0], c[4], c[5])
        if key not in pick:
            if route_valid(c, size_of):
                pick[key] = c
        elif sample and route_valid(c, size_of):
            others.append(c)
    out = list(pick.values())
    if sample:
        rng = np.random.default_rng(seed)
        out += [others[i] for i in sorted(rng.choice(len(others), size=min(sample, len(others)), replace=False))]
    return out + [c for c in extras if c not in out]


def windows(nx, ny):
    """Four windows, one of them empty: the interior, one that straddles the first block boundary (where there is one), one cell
    column at the right wall, nothing."""
    return ((1, nx - 1, 1, ny - 1), (min(60, nx // 2), min(70, nx), 0, ny // 2 + 1), (nx - 1, nx, ny // 3, ny), (nx // 2, nx // 2, 0, ny))


# ---- solid obstacles: masks and the tile kernel's geometry ---------------------------------------------------------------------------
def _masks(nx, ny, seed=11):
    """name -> mask: the cases the kernel can get wrong.  Block edges fall at x = 3 and x = 0 (mod 4) -- the last and the first cell of
    a thread's four (two) -- and, on the wide lattices, straddle the seams between two workgroups' cells at x = 511 | 512 and 1023 | 1024."""
    z = lambda: np.zeros((nx, ny), dtype=bool)  # noqa: E731
    out = {"fluid": z()}
    m = z(); m[nx // 2, ny // 2] = True
    out["cell"] = m
    m = z()
    y0, y1 = max(1, ny // 4), min(ny - 1, ny // 4 + 6)
    m[19:25, y0:y1] = True                       # columns 19 .. 24
    for seam in (512, 1024):
        if nx > seam + 4:
            m[seam - 5:seam + 5, y0:y1] = True   # columns seam - 5 (= 3 mod 4) .. seam + 4 (= 0 mod 4)
    out["block"] = m
    m = z()
    for i in range(min(nx, ny) - 3):             # a diagonal staircase: solid cells that touch at corners only
        m[2 + i, 1 + i] = True
    out["stairs"] = m
    m = z()                                      # cells on each wall, in each corner and in the lid row
    m[0, ny // 2] = m[nx - 1, ny // 3] = m[nx // 2, ny - 1] = True
    m[0, 0] = m[nx - 1, 0] = m[0, ny - 1] = m[nx - 1, ny - 1] = True
    m[nx // 3:nx // 3 + 5, 0] = True
    m[7, 0:2] = True
    out["walls"] = m
    out["random"] = np.random.default_rng(seed).random((nx, ny)) < 0.2
    return out


def _tile(dtype, S):
    """(F, TX, TY) of the tile kernel for S steps per launch (k_stepS_deep)."""
    V = 4 if np.dtype(dtype) == np.float32 else 2
    RV = (S - 1 + V - 1) // V
    return (4 if S == 3 else 8), (16 - 2 * RV) * V, 32 - 2 * (S - 1)


def _tile_shape(dtype, S):
    """The smallest lattice with two full tiles and a clipped third per axis (derived in tests/test_solid_tiles_gpu.py)."""
    if np.dtype(dtype) == np.float64:
        return 72, 72
    return (128, 72) if S == 3 else (136, 80)


# ---- the arithmetic error budgets (tests/test_arith_error_budget*_gpu.py; the *_cpu.py files check these cases without a device) ----
NX, NY, RE, ULB = 96, 80, 1000.0, 0.08
CALLS = (1, 1, 3, 8, 13)
DISTINCT = dict(omega_e=1.13, omega_eps=1.41, omega_q=1.67, omegam=1.31)
RATIO_MAX = 2.31       # measured on an MI355X over the whole matrix (see the docstring of tests/test_arith_error_budget_gpu.py)
K = min(16.0, 4 * RATIO_MAX)
FAM_CALLS = (1, 2, 7, 20)
BATCH_RATES = [dict(Re=400.0, omega_e=1.13, omega_eps=1.41, omega_q=1.67, omegam=1.31),
               dict(Re=1000.0, omega_e=0.9, omega_eps=1.55, omega_q=1.25, omegam=1.7),
               dict(Re=5000.0, omega_e=1.3, omega_eps=1.05, omega_q=1.8, omegam=1.1)]
# MRT.py's walls and bounce-back: the kernels lbm_plan accepts for them, each with the kernel and the steps per launch that describe()
# must report (tests/test_arith_error_budget_walls_cpu.py confirms every entry by a dry run).  vec, the streaming kernels with the walls
# inside and, under bounce-back, the push scheme know only MRT_GPU.py's walls.
WALL_FAMILIES = {
    "mrt_py": [("generic", 0, {}, "none", 1), ("push", 0, {}, "none", 1),
               ("tb", 2, {}, "k_step2_deep", 2), ("tb", 3, {}, "k_stepS_deep", 3), ("tb", 4, {}, "k_stepS_deep", 4), ("tb", 5, {}, "k_stepS_deep", 5),
               ("stream", 3, dict(stream_walls=False), "k_stream", 3), ("stream", 8, dict(stream_walls=False), "k_stream", 8)],
    "bounce_back": [("generic", 0, {}, "none", 1),
                    ("tb", 2, {}, "k_step2_deep", 2), ("tb", 3, {}, "k_stepS_deep", 3), ("tb", 4, {}, "k_stepS_deep", 4), ("tb", 5, {}, "k_stepS_deep", 5),
                    ("stream", 3, dict(stream_walls=False), "k_stream", 3), ("stream", 8, dict(stream_walls=False), "k_stream", 8)]}


def _family_shape(kernel):
    """The lattice a kernel family runs on: the streaming lattice is two strips wide, the second partly outside the lattice."""
    return (264, 150) if kernel == "stream" else (96, 80)


def _err(x, ref):
    return float(np.abs(np.asarray(x, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


def _errs(got, ref):
    e = {k: _err(got[k], ref[k]) for k in got}
    e["u"] *= float(np.abs(ref["u"]).max()) / ULB       # u / uLB
    return e


def _fields(s, turb):
    u, rho, fin = s.get_fields(want_fin=True)
    out = dict(fin=fin, u=u, rho=rho)
    if turb:
        out["tau"] = s.get_tau()
    return out


def _stepped(s, f0, calls):
    s.set_state(f0)
    out = []
    for n in calls:
        s.step(n)
        out.append(_fields(s, s.turb))
    return out


def _same_calls(a, b, what):
    """Two lists of field dicts, one per call (_stepped), hold the same bits."""
    for i, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, "call", i, k, np.abs(x[k] - y[k]).max())


def _assert_budget(m, tag0, dtype, rates):
    eps = float(np.finfo(dtype).eps)
    for a in m:
        if a == "strict":
            continue
        for (steps, e, at), (_, es, _) in zip(m[a], m["strict"]):
            tag = (a, np.dtype(dtype).name) + tag0 + ("distinct" if rates else "default", steps)
            if steps == 1 and a == "fast":
                for k, v in e.items():
                    assert v <= 32 * eps, (tag, k, v / eps, "eps after one step; largest fin error at (k, x, y) =", at)
            for k, v in e.items():
                bound = K * max(es[k], eps)
                assert v <= bound, (tag, k, v, "ratio", v / max(es[k], eps), "largest fin error at (k, x, y) =", at)


class _FastStep:
    """The oracle's step with collide() replaced by the restatements of the device's fast operators, fed the rho, ux, uy of the
    semantics' own macros(): on row 0 the overridden density and u = (uLB, 0) under MRT.py's and MRT_GPU.py's walls (where
    lbm_device.hpp passes lid = true to the factored MRT operator), the plain sums everywhere under bounce-back.  (The library
    compiles the fast operators for MRT_GPU.py's walls and for bounce-back; under MRT.py's walls arith = fast runs the strict ones,
    include/lbm.h, so that column of the checks of tests/test_arith_error_budget_walls_cpu.py is about the algebra alone.)"""
    meq_density = "rho"

    def macros(self, f):
        rho, ux, uy = super().macros(f)
        self._u = (ux, uy)
        return rho, ux, uy

    def collide(self, f, rho, feq, w_nu=None):
        if w_nu is None:
            w_nu = self.par(self.relax["omega"])
        if self.coll == "MRT":
            ov = self.omega_vec
            return np.array(mrt_fast(f, rho, ov[1], ov[2], ov[4], w_nu, meq_density=self.meq_density))
        ux, uy = self._u
        return np.array(srt_trt_fast(self.coll, f, rho, ux, uy, w_nu, self.par(self.relax["omegam"])))


# ---- the budget with solid obstacles and moving bodies: masks, bodies and routes (tests/test_arith_error_budget_solid_cpu.py checks
# all of them without a device) ---------------------------------------------------------------------------------------------------------
BB = dict(semantics="bounce_back")
TILES = dict(solid_tiles=True)
REST_STATES = ("S0", "S1", "S2", "S3")
MOVE_STATES = ("S0", "S2", "S3")
BATCH_STEPS = 29
SMALLEST = ((6, 6), (13, 9))


def budget_mask(nx, ny, dtype, S, seed=2026):
    """One mask with what a solid kernel can get wrong, for the tile kernel's geometry at S steps per launch (F, TX, TY of _tile):
    a 6 x 6 block with its edges on x = 3 and x = 0 (mod 4); three cells that touch at corners only; five
    lid-row cells and a column from the lid two cells down; a cell on each side wall, one on the bottom row, the corner (0, 0); a
    2 x 2 block across the first tile seam in x and y; single cells on the frame / tile boundary F - 1 | F; and seeded random 5 % of
    the interior (kept one cell clear of the staircase, so that it stays one)."""
    F, TX, TY = _tile(dtype, S)
    m = np.zeros((nx, ny), dtype=bool)
    m[1:-1, 1:-1] = np.random.default_rng(seed).random((nx - 2, ny - 2)) < 0.05
    sx, sy = nx // 2 - 6, ny // 2 + 6
    m[sx - 1:sx + 4, sy - 1:sy + 4] = False
    for i in range(3):
        m[sx + i, sy + i] = True
    by = ny // 4 + 2
    m[19:25, by:by + 6] = True                                   # columns 19 (= 3 mod 4) .. 24 (= 0 mod 4)
    m[nx // 2:nx // 2 + 5, 0] = True
    m[nx // 3, 0:3] = True
    m[0, ny // 2] = m[nx - 1, ny // 3] = m[nx // 2 + 7, ny - 1] = m[0, 0] = True
    xs, ys = F + TX, F + TY
    if xs < nx - F and ys < ny - F:
        m[xs - 1:xs + 1, ys - 1:ys + 1] = True
    for a, b in ((F - 1, 12), (F, 15)):
        if a < nx - 1 and b < ny - 1:
            m[a, b] = True
    for a, b in ((14, F - 1), (17, F)):
        if a < nx - 1 and b < ny - 1:
            m[a, b] = True
    assert not m.all()
    return m


def motion_case(nx, ny, shift=0):
    """(mask, labels, motion[6, 3]): bodies clear of the walls and of each other, so that every rigid motion passes the flux check.
    Body 0: a 6 x 6 block (edges on x = 3 and 0 mod 4 for shift = 0) that translates and rotates; 1: a single cell that does the same;
    2, 3: two 3 x 6 blocks one fluid column apart with different motions (a fluid cell linked to both, the `between` case of
    tests/test_body_motion_gpu.py); 4, 5: two 2 x 2 blocks three fluid cells apart, with different motions as well.  The speeds are
    half those of that file: at Re 1000 the SRT populations in the one-column gap between bodies 2 and 3 pass 1 within 21 steps otherwise."""
    m, lab = np.zeros((nx, ny), dtype=bool), np.zeros((nx, ny), dtype=np.int32)
    y = ny // 4
    boxes = [(19, 25, y, y + 6), (nx // 2 + 5, nx // 2 + 6, ny // 2, ny // 2 + 1), (32, 35, y + 9, y + 15), (36, 39, y + 9, y + 15),
             (44, 46, y, y + 2), (49, 51, y + 1, y + 3)]
    for b, (x0, x1, y0, y1) in enumerate(boxes):
        m[x0 + shift:x1 + shift, y0:y1] = True
        lab[x0 + shift:x1 + shift, y0:y1] = b
    mot = [[0.005, 0.01, 0.01 / nx], [0.01, -0.005, 0.015], [0.015, 0.0, 0.005], [-0.01, 0.005, -0.01], [0.0, -0.01, 0.0075], [0.0075, 0.005, -0.005]]
    return m, lab, np.asarray(mot)


def solid_routes(dtype):
    """[(shape, kernel, tuning, S of the mask, kernel name, steps per launch)] of the routes at rest: what describe() must report.  The
    first entry of a shape is the one the others of that shape are compared with.  k_step_generic runs on 96 x 80 against
    k_step_solid in both types; on 70 x 66 `auto` is k_step_solid in fp64 (a second real comparison) and k_step_generic itself in
    fp32 (70 is no multiple of 4: there the fast comparison is of the kernel with itself, and only the strict half says something)."""
    auto_70 = "k_step_generic" if np.dtype(dtype) == np.float32 else "k_step_solid"
    out = [((NX, NY), "auto", {}, 5, "k_step_solid", 1), ((NX, NY), "generic", {}, 5, "k_step_generic", 1),
           ((70, 66), "auto", {}, 5, auto_70, 1), ((70, 66), "generic", {}, 5, "k_step_generic", 1)]
    for S in (3, 4, 5):
        out.append((_tile_shape(dtype, S), "auto", dict(TILES, tb_steps=S), S, "k_stepS_deep", S))
    for S in (3, 5):
        for extra in (dict(frame_lds=False), dict(frame_fused=False)):
            out.append((_tile_shape(dtype, S), "auto", dict(TILES, tb_steps=S, **extra), S, "k_stepS_deep", S))
    return out


def budget_tile_steps(dtype):
    """Steps per launch of the tile route on the budget's lattice (a dry run)."""
    return launch_plan(NX, NY, RE, steps=13, dtype=dtype, tuning=TILES, solid=True, **BB)["steps_per_launch"]


def batch_cases(dtype, moving):
    """(masks, labels, motions) of the three lattices of the batch test, lattice i with BATCH_RATES[i]: at rest budget_mask with its own
    seed (labels and motions None); moving: motion_case shifted by 5 i cells with its speeds scaled by 1 - i / 4."""
    if not moving:
        return [budget_mask(NX, NY, dtype, budget_tile_steps(dtype), seed=2026 + i) for i in range(3)], None, None
    cases = [motion_case(NX, NY, shift=5 * i) for i in range(3)]
    return [c[0] for c in cases], np.stack([c[1] for c in cases]), np.stack([c[2] * (1.0 - 0.25 * i) for i, c in enumerate(cases)])


def smallest_mask(nx, ny):
    mask = np.zeros((nx, ny), dtype=bool)
    mask[nx // 2, ny // 2] = True
    return mask


# ---- the budget under the obstacle rules: a shape, hold cells with a wall velocity per cell, periodic sides with a driving force, the
# passive scalar and its buoyancy (tests/test_arith_error_budget_rules_gpu.py; tests/test_arith_error_budget_rules_cpu.py checks the
# cases, the references and the routes without a device) --------------------------------------------------------------------------------
RULE_NX, RULE_NY = 72, 40      # both vector widths divide 72: `auto` is the vector route, kernel="generic" the one-cell route
RULE_RE = 500.0                # on 40 rows the relaxation rates of the 96 x 80 lattice at Re 1000 (nu = uLB ny / Re: 80 / 1000 = 40 / 500)
RULE_D = 0.07
RULE_FORCE = (2e-5, -1e-5)
RULE_BUOY = (3e-5, 6e-5, 0.5)
RULE_STATES = ("S0", "S2")
RULE_DISC_R = 6.3
RULE_ROUTES = (("auto", None, "k_step_solid", 0), ("generic", None, "k_step_generic", 0), ("auto", dict(nt=True), "k_step_solid", 1))


def rule_disc(nx, ny):
    """(mask, labels, q, (x0, y0)): a disc of radius 6.3 about a point off the cell centres (body 0) with the exact fractions of
    solid.disc_fractions, and one more solid cell (body 1) directly behind the first fluid cell whose link to the disc along a lattice
    axis has q < 0.4: that link has no fluid cell behind it and falls back to q = 1/2, and the links of the extra cell, which cross no
    circle, carry q = 1/2 exactly (a == 1)."""
    from latticeboltzmannsimulations_amd import solid
    x0, y0 = nx / 2.0 + 0.37, ny / 2.0 + 0.21
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    m = np.hypot(xs - x0, ys - y0) < RULE_DISC_R
    q = solid.disc_fractions(m, x0, y0, RULE_DISC_R)
    lab = np.zeros((nx, ny), dtype=np.int32)
    for x, y, k, _ in solid.body_links(m, lab):
        if k <= 4 and q[k - 1, x, y] < 0.4:
            bx, by = int(x + (1, 0, -1, 0)[k - 1]), int(y - (0, 1, 0, -1)[k - 1])      # N = (x + cx_k, y - cy_k)
            m[bx, by] = True
            lab[bx, by] = 1
            break
    else:
        raise AssertionError("no axis link with q < 0.4")
    return m, lab, solid.disc_fractions(m, x0, y0, RULE_DISC_R), (x0, y0)


def rule_cases(nx=RULE_NX, ny=RULE_NY):
    """The cases of the rules' budget, each a dict like those of tests/test_buoyancy_gpu._scenarios (tag, mask, labels, nbodies,
    wall_value, c0, per, force, hold, f, hold_value, uw, motion) with three more keys: q (the shape, or None), scalar (a passive scalar
    runs) and buoy (its buoyancy, or None); rule_setup and rule_oracles serve them all.

      shaped            the disc of rule_disc at rest: near and far links, q = 1/2 exactly, a fallback link
      shaped moving     the same, the disc translating and rotating
      shaped scalar     the same at rest with a passive scalar, the half x < x0 of the disc Dirichlet at 1: k_scalar_step<.., SHAPED>
      open              an inlet column with a wall velocity per cell, an outlet hold column, single hold cells at the four lane
                        positions x mod 4 = 0 .. 3, a staircase of four cells that touch at corners
      periodic forced   "motion + wall velocity xy" as tests/test_buoyancy_gpu._scenarios builds it, without its scalar: both sides
                        periodic, a driving force, 10 % random solid in three bodies with a motion and a wall velocity
      buoyant hold      "hold cells" as that list builds it (an inlet wall at 0.25, an outlet hold column and two single hold cells with
                        their own hold values), with its scalar and the buoyancy: WALL_REST_BUOY
      buoyant periodic  "periodic forced" with its scalar, half of the solid cells Dirichlet, and the buoyancy: WALL_MOVE_BUOY
      rest scalar       "open" with every wall at rest, the driving force and a passive scalar, the inlet Dirichlet at 0.25, the hold cells
                        with hold values of their own: the mode at rest (WALL_REST) beside hold cells, which the one-cell route launches
                        for the force alone, and k_scalar_step<.., SHAPED = false> without buoyancy

    (The two scenarios are built here again, on a generator of this function's own, so that they exist at any lattice size; the list of
    tests/test_buoyancy_gpu.py needs 52 columns.)"""
    from latticeboltzmannsimulations_amd import periodic
    from open_flow_ref import feq
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    c0 = 0.5 + 0.4 * np.sin(2 * np.pi * xs / nx) * np.cos(2 * np.pi * ys / ny)
    base = dict(wall_value=None, c0=c0, per=(0, 0), force=(0.0, 0.0), hold=None, f=None, hold_value=None, uw=None, motion=None, q=None,
                scalar=False, buoy=None)
    out = []
    m, lab, q, (x0, y0) = rule_disc(nx, ny)
    disc = dict(base, mask=m, labels=lab, nbodies=2, q=q)
    out.append(dict(disc, tag="shaped"))
    out.append(dict(disc, tag="shaped moving", motion=np.array([[0.01, -0.005, 0.002], [0.0, 0.0, 0.0]])))
    out.append(dict(disc, tag="shaped scalar", scalar=True, wall_value=np.where(m & (lab == 0) & (xs < x0), 1.0, np.nan)))
    r = np.random.default_rng(29)
    m, lab, hold = np.zeros((nx, ny), bool), np.zeros((nx, ny), np.int32), np.zeros((nx, ny), bool)
    m[0, :] = True                                                   # the inlet: a solid column whose cells push
    for i in range(4):                                               # a staircase (body 1, at rest) and the four lane positions
        m[nx // 2 - 4 + i, ny // 2 + i] = True
        lab[nx // 2 - 4 + i, ny // 2 + i] = 1
        hold[8 + 5 * i, ny // 4 + i] = True
    hold[nx - 2, 1:ny - 1] = True                                    # the outlet
    uw = np.zeros((2, nx, ny))
    uw[0, 0, :] = 0.01 + 0.002 * np.sin(np.arange(ny))
    uw[1, 0, :] = 0.001 * np.cos(np.arange(ny))
    f = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 + 0.002 * r.standard_normal((nx, ny)), 0.002 * r.standard_normal((nx, ny)))
    opened = dict(base, mask=m, labels=lab, nbodies=2, hold=hold, f=f)
    out.append(dict(opened, tag="open", uw=uw))
    m = periodic.wrap(r.random((nx, ny)) < 0.1, 1, 1)
    lab = periodic.wrap(r.integers(0, 3, (nx, ny)).astype(np.int32), 1, 1)
    uw = periodic.wrap(np.where(m[None], r.uniform(-0.01, 0.01, (2, nx, ny)), 0.0), 1, 1)
    mot = np.stack([r.uniform(-0.01, 0.01, 3), r.uniform(-0.01, 0.01, 3), np.zeros(3)], axis=1)
    wv = periodic.wrap(np.where(m & (r.random((nx, ny)) < 0.5), r.uniform(0.0, 2.0, (nx, ny)), np.nan), 1, 1)
    forced = dict(base, mask=m, labels=lab, nbodies=3, per=(1, 1), force=RULE_FORCE, uw=uw, motion=mot, c0=periodic.wrap(c0, 1, 1))
    out.append(dict(forced, tag="periodic forced"))
    hold = np.zeros((nx, ny), bool)
    hold[nx - 2, 1:ny - 1] = True
    hold[5, 1] = hold[9, ny // 2] = True
    f = feq(1.0 + 0.002 * r.standard_normal((nx, ny)), 0.01 + 0.002 * r.standard_normal((nx, ny)), 0.002 * r.standard_normal((nx, ny)))
    inlet = np.zeros((nx, ny), bool)
    inlet[0, :] = True
    out.append(dict(base, tag="buoyant hold", mask=inlet, labels=np.zeros((nx, ny), np.int32), nbodies=1, wall_value=np.where(inlet, 0.25, np.nan),
                    hold=hold, f=f, hold_value=r.uniform(0.0, 1.0, (nx, ny)), scalar=True, buoy=RULE_BUOY))
    out.append(dict(forced, tag="buoyant periodic", wall_value=wv, scalar=True, buoy=RULE_BUOY))
    out.append(dict(opened, tag="rest scalar", force=RULE_FORCE, scalar=True, wall_value=np.where(opened["mask"] & (opened["labels"] == 0), 0.25, np.nan),
                    hold_value=r.uniform(0.0, 1.0, (nx, ny))))
    return out


def rule_setup(x, sc, rates=None):
    """A solver of sc's lattice brought to the case, in the order the library wants its geometry (mask and bodies, periodic sides, hold
    cells, shape, velocities, force, scalar, buoyancy), then the rates."""
    from latticeboltzmannsimulations_amd import solid
    x.set_driving_force(0.0, 0.0)
    x.set_body_motion(None).set_wall_velocity(None).set_shape(None)
    x.set_solid(sc["mask"]).set_bodies(sc["labels"], solid.centroids(sc["mask"], sc["labels"], sc["nbodies"]))
    x.set_periodic(*sc["per"])
    if sc["hold"] is not None:
        x.set_open_cells(sc["hold"], sc["f"])
    if sc["q"] is not None:
        x.set_shape(sc["q"])
    if sc["uw"] is not None:
        x.set_wall_velocity(sc["uw"])
    if sc["motion"] is not None:
        x.set_body_motion(sc["motion"])
    x.set_driving_force(*sc["force"])
    if sc["scalar"]:
        x.begin_scalar(RULE_D, sc["c0"], wall_value=sc["wall_value"], hold_value=sc["hold_value"])
    if sc["buoy"] is not None:
        x.set_buoyancy(*sc["buoy"])
    if rates:
        x.set_relaxation(0, **rates)
    return x


def rule_oracles(sc, coll, dtype, rates=None, long_double=False, Re=RULE_RE, flow_cls=None):
    """(flow, scalar or None): tests/buoyancy_ref.BuoyantOracle (the whole chain of rules) and tests/scalar_ref.ScalarOracle of a case, in
    the lattice type, or in long double with every parameter and table rounded to the lattice type first."""
    from buoyancy_ref import BuoyantOracle
    from scalar_ref import ScalarOracle
    from latticeboltzmannsimulations_amd import solid
    nx, ny = sc["mask"].shape
    kw = dict(dtype=np.longdouble, param_dtype=dtype) if long_double else dict(dtype=dtype)
    o = (flow_cls or BuoyantOracle)(nx, ny, Re, mask=sc["mask"], labels=sc["labels"], centres=solid.centroids(sc["mask"], sc["labels"], sc["nbodies"]),
                                    periodic=sc["per"], force=sc["force"], q=sc["q"], wall_velocity=sc["uw"], motion=sc["motion"], hold=sc["hold"],
                                    f=sc["f"], collision=coll, buoyancy=sc["buoy"], **(rates or {}), **kw)
    s = None
    if sc["scalar"]:
        s = ScalarOracle(sc["mask"], RULE_D, sc["c0"], wall_value=sc["wall_value"], hold=sc["hold"], hold_f=sc["f"], hold_value=sc["hold_value"],
                         periodic=sc["per"], **kw)
    return o, s


def rule_step(o, s, n=1):
    """n steps of a pair of rule_oracles as lbm_step runs them (buoyancy_ref.Coupled), or of the flow alone."""
    if s is None:
        return o.step(n)
    from buoyancy_ref import Coupled
    Coupled(o, s).step(n)
    return o
