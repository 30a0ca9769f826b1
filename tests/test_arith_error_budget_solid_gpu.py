"""Error budget of arith="fast" with solid obstacles (LBM_SEM_BOUNCE_BACK_SOLID) and moving bodies against a long-double reference,
at distinct relaxation rates and from off-equilibrium states.

The budget of tests/test_arith_error_budget_gpu.py (err(X) = max|X - X_ref| / max|X_ref| for fin, u / uLB and rho; the states S0..S3 of
oracle/states.py; the default rates and DISTINCT; 96 x 80; read-outs after 1, 2, 5, 13 and 26 steps) carried to the solid kernels.  The
reference is tests/solid_ref.SolidOracle -- with motion tests/moving_wall_ref.MovingWallOracle -- in np.longdouble, the rates, uLB and
every link's delta rounded to the lattice type first; the same class in the lattice type is what strict must equal bit for bit, and its
error is the budget's denominator.  err is taken over FLUID cells; solid cells must hold w_k exactly.

a. at rest (budget_mask: block, staircase, lid row, walls, corner, tile seams, frame boundary, 5 % scatter): strict (k_step_solid),
   fast, and fast on the tile route (solid_tiles) and on kernel="generic" (k_step_generic): the same bits as fast, so inside the
   same budget;
b. with motion (motion_case: a block and a single cell that translate and rotate, two bodies one fluid column apart with different
   motions, two more three cells apart): strict and fast on `auto` (k_step_solid + the store-side delta) and on kernel="generic";
c. from S2 at the distinct rates every solid route gives the oracle's bits (strict) and one set of bits (fast): solid_routes(), the
   moving twins, batches of three lattices with their own masks, rates and motions, and the smallest lattices.

* strict is np.array_equal to the lattice-type oracle at the same rates;
* after 1 step err_fast <= 32 eps of the lattice type;
* after every call err_fast <= K max(err_strict, eps), K of tests/test_arith_error_budget_gpu.py.

Measured on an MI355X (maxima over the states, both rate sets and the five read-outs; ratios err_fast / max(err_strict, eps) over
fin, u and rho).  The tile route (solid_tiles: one single step, then units of 5, 4 and 3 steps) gives the bits of the one-step route in
all 240 read-outs, so its row is the `rest` row:

| route | lattice | operator | err after 1 step, in eps: strict / fast | fin err after 26 steps: strict / fast | largest ratio: fast |
|---|---|---|---|---|---|
| rest = tile | fp32 | SRT | 4.4 / 4.9 | 1.7e-6 / 1.5e-6 | 1.27 |
| rest = tile | fp32 | TRT | 4.4 / 4.9 | 2.1e-6 / 2.0e-6 | 1.28 |
| rest = tile | fp32 | MRT | 2.6 / 2.4 | 7.1e-7 / 6.7e-7 | 1.89 |
| rest = tile | fp64 | SRT | 4.6 / 4.7 | 4.4e-15 / 4.3e-15 | 1.35 |
| rest = tile | fp64 | TRT | 4.6 / 4.7 | 4.9e-15 / 5.6e-15 | 1.24 |
| rest = tile | fp64 | MRT | 2.7 / 2.7 | 2.1e-15 / 2.0e-15 | 1.29 |
| moving | fp32 | SRT | 4.4 / 4.9 | 1.4e-6 / 1.3e-6 | 1.37 |
| moving | fp32 | TRT | 4.4 / 4.9 | 2.3e-6 / 2.0e-6 | 1.56 |
| moving | fp32 | MRT | 2.6 / 2.4 | 7.0e-7 / 5.8e-7 | 2.66 |
| moving | fp64 | SRT | 4.2 / 4.7 | 3.7e-15 / 3.8e-15 | 1.28 |
| moving | fp64 | TRT | 4.2 / 4.7 | 4.7e-15 / 5.1e-15 | 1.31 |
| moving | fp64 | MRT | 2.7 / 2.3 | 1.8e-15 / 1.8e-15 | 1.52 |

K: every one of the 1260 ratios lies inside K = 4 x 2.31 = 9.24, so K stays and the solid tests set no RATIO_MAX of their own.  The
largest, 2.66, is u after 2 steps from S0 at the default rates (moving, fp32 MRT), where err_strict is 1.07 eps -- the figure and the
place of plain bounce-back's largest ratio; the next are 1.89 (rest, fp32 MRT, u after 2 steps from S0, err_strict 1.59 eps) and 1.57.
The median fin ratio is 0.97 (59 % of the read-outs below 1).  The largest fin error of fast sits on a link cell (a fluid cell with a
solid source) in 81 of the 240 read-outs at rest (strict: 92) and in 22 of the 180 with motion (strict: 14), with fin ratios <= 1.29
and <= 1.31 there, and on the lid row in 19 and 9: no link cell, no lid-row cell next to a solid one and no route stands out.  Nothing
was found: strict is the oracle's bits at the distinct rates from every state on every route, fast is one set of bits across the
routes, and no bug showed in gather_a<..., SEM_SOLID>, the tile kernel's SOLID path or the moving twins.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.states import state  # noqa: E402
from moving_wall_ref import MovingWallOracle  # noqa: E402
from solid_ref import SolidOracle  # noqa: E402
from test_arith_error_budget_gpu import (BATCH_RATES, CALLS, DISTINCT, FAM_CALLS, K, _assert_budget, _err, _errs,  # noqa: E402,F401
                                         _same_bits, _stepped)
from test_solid_tiles_gpu import _shape as _tile_shape  # noqa: E402
from test_solid_tiles_gpu import _tile  # noqa: E402
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, launch_plan, solid  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
NX, NY, RE, ULB = 96, 80, 1000.0, 0.08
BB = dict(semantics="bounce_back")
TILES = dict(solid_tiles=True)
REST_STATES = ("S0", "S1", "S2", "S3")
MOVE_STATES = ("S0", "S2", "S3")
COLLS = ("SRT", "TRT", "MRT")


# ---- masks, bodies and routes (tests/test_arith_error_budget_solid_cpu.py checks all of them without a device) -------------------
def budget_mask(nx, ny, dtype, S, seed=2026):
    """One mask with what a solid kernel can get wrong, for the tile kernel's geometry at S steps per launch (F, TX, TY of
    test_solid_tiles_gpu._tile): a 6 x 6 block with its edges on x = 3 and x = 0 (mod 4); three cells that touch at corners only; five
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


BATCH_STEPS = 29
SMALLEST = ((6, 6), (13, 9))


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


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _open(nx, ny, coll, dtype, arith, mask, rates, kernel="auto", tune=None, bodies=None, Re=RE):
    s = CavitySolver(nx, ny, Re, RT=coll, dtype=dtype, arith=arith, kernel=kernel, solid=mask, tuning=tune or None, **BB)
    try:
        if rates:
            s.set_relaxation(0, **rates)
        if bodies is not None:
            lab, mot = bodies
            s.set_bodies(lab).set_body_motion(mot)
            assert s.describe()["wall_motion"] == 1
    except Exception:
        s.close()
        raise
    return s


def _oracle(nx, ny, coll, dtype, mask, rates, bodies=None, long_double=False, Re=RE):
    kw = dict(collision=coll, **{k: v for k, v in rates.items() if k != "Re"})
    kw.update(dict(dtype=LD, param_dtype=dtype) if long_double else dict(dtype=dtype))
    Re = rates.get("Re", Re)
    if bodies is None:
        return SolidOracle(nx, ny, Re, mask=mask, **kw)
    return MovingWallOracle(nx, ny, Re, mask=mask, labels=bodies[0], motion=bodies[1], **kw)


def _fields(s):
    u, rho, fin = s.get_fields(want_fin=True)
    return dict(fin=fin, u=u, rho=rho)


def _fluid(d, fl):
    return dict(fin=d["fin"][:, fl], u=d["u"][:, fl], rho=d["rho"][fl])


def _where(got, ref, fl, links):
    """The fluid cell of the largest fin error: dict(k, x, y, link)."""
    d = np.abs(np.asarray(got["fin"], dtype=LD) - ref["fin"]) * fl[None]
    k, x, y = (int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))
    return dict(k=k, x=x, y=y, link=bool(links[x, y]))


def measure(dtype, coll, st, rates, motion=False):
    """err over the fluid cells after every call: {"strict" | "fast": [(steps, {field: err}, where_fin)]}.  Asserts on the way that every
    strict solver is the lattice-type oracle's bits, that the fast solvers (at rest: one step per launch, the tile route and
    kernel="generic"; with motion: `auto` and kernel="generic") are the same bits, and that solid cells hold w_k.  Also the measurement that set K."""
    if motion:
        mask, lab, mot = motion_case(NX, NY)
        bodies = (lab, mot)
        plans = dict(strict=("strict", "auto", None), strict_generic=("strict", "generic", None), fast=("fast", "auto", None),
                     fast_generic=("fast", "generic", None))
    else:
        mask, bodies = budget_mask(NX, NY, dtype, budget_tile_steps(dtype)), None
        plans = dict(strict=("strict", "auto", None), fast=("fast", "auto", None), fast_tiles=("fast", "auto", TILES),
                     fast_generic=("fast", "generic", None))
    solvers = {}
    try:
        for name, (arith, kernel, tune) in plans.items():
            solvers[name] = _open(NX, NY, coll, dtype, arith, mask, rates, kernel, tune, bodies)
        assert solvers["strict"].describe()["kernel"] == "k_step_solid"
        assert solvers["fast_generic"].describe()["kernel"] == "k_step_generic"
        if not motion:
            assert solvers["fast_tiles"].describe()["kernel"] == "k_stepS_deep"
        f0 = solvers["strict"].get_fields(want_fin=True)[2] if st == "S0" else state(st, NX, NY, dtype)
        for s in solvers.values():
            s.set_state(f0)
        C = _oracle(NX, NY, coll, dtype, mask, rates, bodies)
        L = _oracle(NX, NY, coll, dtype, mask, rates, bodies, long_double=True)
        C.set_state(f0)
        L.set_state(f0.astype(LD))
        fl = ~mask
        links = np.any(np.array(L.link_sets()), axis=0)
        wk = np.broadcast_to(C.t[:, None], (9, int(mask.sum())))
        out = dict(strict=[], fast=[])
        for n in CALLS:
            L.step(n); C.step(n)
            ref = dict(fin=L.fin, u=L.u, rho=L.rho)
            got = {}
            for name, s in solvers.items():
                s.step(n)
                got[name] = _fields(s)
                tag = (name, coll, np.dtype(dtype).name, st, "distinct" if rates else "default", L.nsteps)
                assert np.array_equal(got[name]["fin"][:, mask], wk), (tag, "solid cells do not hold w_k")
                if name.startswith("strict"):
                    assert all(np.array_equal(got[name][k], getattr(C, k)) for k in ("fin", "u", "rho")), (tag, "differs from the oracle")
                elif name != "fast":
                    assert all(np.array_equal(got[name][k], got["fast"][k]) for k in ("fin", "u", "rho")), (tag, "differs from fast")
            for a in out:
                out[a].append((L.nsteps, _errs(_fluid(got[a], fl), _fluid(ref, fl)), _where(got[a], ref, fl, links)))
        return out
    finally:
        for s in solvers.values():
            s.close()


def _report(m, tag, dtype):
    eps = float(np.finfo(dtype).eps)
    for (steps, e, at), (_, es, _) in zip(m["fast"], m["strict"]):
        print(tag, "steps", steps, " ".join(f"{k} {es[k] / eps:.2f}/{e[k] / eps:.2f} eps ratio {e[k] / max(es[k], eps):.2f}" for k in e), "fin at", at)


# ---- a. and b.: the budget -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", REST_STATES)
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_stays_within_the_budget_with_obstacles_at_rest(dtype, coll, st):
    for rates in ({}, DISTINCT):
        m = measure(dtype, coll, st, rates)
        _report(m, ("rest", coll, np.dtype(dtype).name, st, "distinct" if rates else "default"), dtype)
        _assert_budget(m, ("solid", coll, st), dtype, rates)


@pytest.mark.parametrize("st", MOVE_STATES)
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_stays_within_the_budget_with_moving_bodies(dtype, coll, st):
    for rates in ({}, DISTINCT):
        m = measure(dtype, coll, st, rates, motion=True)
        _report(m, ("moving", coll, np.dtype(dtype).name, st, "distinct" if rates else "default"), dtype)
        _assert_budget(m, ("moving", coll, st), dtype, rates)


# ---- c. every solid route, the same bits at distinct rates from S2 ------------------------------------------------------------------
def _strict_walk(s, o, f0, what):
    s.set_state(f0); o.set_state(f0)
    for n in FAM_CALLS:
        s.step(n); o.step(n)
        got = _fields(s)
        for k in got:
            assert np.array_equal(got[k], getattr(o, k)), (what, "strict differs from the oracle after", o.nsteps, k)


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_route_at_rest_gives_the_same_bits_at_distinct_rates(dtype, coll):
    """solid_routes(dtype) from S2 at the distinct rates, after 1, 3, 10 and 30 steps: strict is the oracle's bits on every route; fast
    is, per lattice shape, the bits of the first one-step route of that shape: k_step_solid -- with which k_step_generic is compared
    on 96 x 80 in both types and on 70 x 66 in fp64 --, or, on 70 x 66 in fp32, k_step_generic, where `auto` against "generic" is
    the kernel against itself."""
    base = {}
    for (nx, ny), kernel, tune, S, name, spl in solid_routes(dtype):
        mask, f0 = budget_mask(nx, ny, dtype, S), state("S2", nx, ny, dtype)
        what = ((nx, ny), kernel, tune)
        with _open(nx, ny, coll, dtype, "strict", mask, DISTINCT, kernel, tune) as s:
            d = s.describe()
            assert (d["kernel"], d["steps_per_launch"]) == (name, spl), (what, d["kernel"], d["steps_per_launch"])
            _strict_walk(s, _oracle(nx, ny, coll, dtype, mask, DISTINCT), f0, what)
        with _open(nx, ny, coll, dtype, "fast", mask, DISTINCT, kernel, tune) as s:
            d = s.describe()
            assert (d["kernel"], d["steps_per_launch"]) == (name, spl), (what, d["kernel"], d["steps_per_launch"])
            got = _stepped(s, f0, FAM_CALLS)
        key = (nx, ny, S)
        if key not in base:
            if spl == 1:
                base[key] = got
                continue
            with _open(nx, ny, coll, dtype, "fast", mask, DISTINCT) as g:
                base[key] = _stepped(g, f0, FAM_CALLS)
        _same_bits(base[key], got, what)


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_moving_twins_give_the_same_bits_at_distinct_rates(dtype, coll):
    """k_step_solid_move (96 x 80) and k_step_generic_move (96 x 80 with kernel="generic"; 70 x 66 under `auto` in fp32) from S2 at the
    distinct rates: strict is MovingWallOracle's bits, fast one set of bits per shape.  (On 70 x 66 in fp32 `auto` and "generic" are
    the same kernel and the fast comparison is trivial; 96 x 80 in both types and 70 x 66 in fp64 compare the two twins.)"""
    V = 4 if dtype == np.float32 else 2
    for nx, ny in ((NX, NY), (70, 66)):
        mask, lab, mot = motion_case(nx, ny)
        f0 = state("S2", nx, ny, dtype)
        fast = []
        for kernel in ("auto", "generic"):
            with _open(nx, ny, coll, dtype, "strict", mask, DISTINCT, kernel, bodies=(lab, mot)) as s:
                want = "k_step_generic" if kernel == "generic" or nx % V else "k_step_solid"
                assert s.describe()["kernel"] == want, (nx, ny, kernel)
                _strict_walk(s, _oracle(nx, ny, coll, dtype, mask, DISTINCT, (lab, mot)), f0, ((nx, ny), kernel, "moving"))
            with _open(nx, ny, coll, dtype, "fast", mask, DISTINCT, kernel, bodies=(lab, mot)) as s:
                fast.append(_stepped(s, f0, FAM_CALLS))
        _same_bits(fast[0], fast[1], ((nx, ny), "moving, auto against generic"))


@pytest.mark.parametrize("moving", [False, True], ids=["rest", "moving"])
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_batch_with_its_own_masks_and_rates_equals_the_lattices_alone(dtype, coll, moving):
    """Three lattices side by side from S2, each with its own mask and its own BATCH_RATES entry (at rest also on the tile route; moving:
    a motion on every lattice, the bodies shifted from lattice to lattice): after 29 steps every lattice is the lattice run alone,
    strict and fast."""
    f0 = state("S2", NX, NY, dtype)
    masks, labels, mots = batch_cases(dtype, moving)
    if moving:
        cen = np.stack([solid.centroids(masks[i], labels[i], 6) for i in range(3)])
    for arith in ("strict", "fast"):
        alone = []
        for i, r in enumerate(BATCH_RATES):
            with _open(NX, NY, coll, dtype, arith, masks[i], r, bodies=(labels[i], mots[i]) if moving else None) as s:
                alone.append(_stepped(s, f0, (BATCH_STEPS,))[0])
        for tune in ((None,) if moving else (None, TILES)):
            with CavityBatch(NX, NY, [r["Re"] for r in BATCH_RATES], RT=coll, dtype=dtype, arith=arith, solid=np.stack(masks), tuning=tune, **BB) as b:
                for i, r in enumerate(BATCH_RATES):
                    b.set_relaxation(i, **r)
                if moving:
                    b.set_bodies(labels, cen).set_body_motion(mots)
                    assert b.describe()["wall_motion"] == 1
                b.set_state(np.ascontiguousarray(np.stack([f0] * 3)))
                b.step(BATCH_STEPS)
                u, rho, fin = b.get_fields(want_fin=True)
            for i in range(3):
                _same_bits([alone[i]], [dict(fin=fin[i], u=u[i], rho=rho[i])], ("batch", arith, tune, "lattice", i))


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_smallest_lattices_with_one_solid_cell(dtype, coll):
    """6 x 6 and 13 x 9 with one solid cell under `auto`, from S2 at the distinct rates: strict is the oracle's bits, fast the bits of
    kernel="generic".  (Only 6 x 6 in fp64 runs k_step_solid under `auto`; 13 x 9 in both types and 6 x 6 in fp32 run
    k_step_generic either way, so their fast comparison is trivial and the strict one is what they add.)"""
    for nx, ny in SMALLEST:
        mask = smallest_mask(nx, ny)
        f0 = state("S2", nx, ny, dtype)
        with _open(nx, ny, coll, dtype, "strict", mask, DISTINCT) as s:
            _strict_walk(s, _oracle(nx, ny, coll, dtype, mask, DISTINCT), f0, (nx, ny))
        with _open(nx, ny, coll, dtype, "fast", mask, DISTINCT) as a, _open(nx, ny, coll, dtype, "fast", mask, DISTINCT, "generic") as g:
            _same_bits(_stepped(g, f0, FAM_CALLS), _stepped(a, f0, FAM_CALLS), (nx, ny))
