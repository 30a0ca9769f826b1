"""Error budget of arith="fast" with solid obstacles (LBM_SEM_BOUNCE_BACK_SOLID) and moving bodies against a long-double reference,
at distinct relaxation rates and from off-equilibrium states.

The budget of tests/test_arith_error_budget_gpu.py (err(X) = max|X - X_ref| / max|X_ref| for fin, u / uLB and rho; the states S0..S3 of
oracle/states.py; the default rates and DISTINCT; 96 x 80; read-outs after 1, 2, 5, 13 and 26 steps) carried to the solid kernels.  The
reference is tests/solid_ref.SolidOracle -- with motion tests/moving_wall_ref.MovingWallOracle -- in np.longdouble, the rates, uLB and
every link's delta rounded to the lattice type first; the same class in the lattice type is what strict must equal bit for bit, and its
error is the budget's denominator.  err is taken over FLUID cells; solid cells must hold w_k exactly.

a. at rest (cases.budget_mask: block, staircase, lid row, walls, corner, tile seams, frame boundary, 5 % scatter): strict (k_step_solid),
   fast, and fast on the tile route (solid_tiles) and on kernel="generic" (k_step_generic): the same bits as fast, so inside the
   same budget;
b. with motion (motion_case: a block and a single cell that translate and rotate, two bodies one fluid column apart with different
   motions, two more three cells apart): strict and fast on `auto` (k_step_solid + the store-side delta) and on kernel="generic";
c. from S2 at the distinct rates every solid route gives the oracle's bits (strict) and one set of bits (fast): solid_routes(), the
   moving twins, batches of three lattices with their own masks, rates and motions, and the smallest lattices.

* strict is np.array_equal to the lattice-type oracle at the same rates;
* after 1 step err_fast <= 32 eps of the lattice type;
* after every call err_fast <= K max(err_strict, eps), K of tests/cases.py (derived in tests/test_arith_error_budget_gpu.py).

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
import numpy as np
import pytest

from cases import (BATCH_RATES, BATCH_STEPS, BB, CALLS, DISTINCT, FAM_CALLS, MOVE_STATES, NX, NY, RE, REST_STATES, SMALLEST, TILES,
                   _assert_budget, _errs, _stepped, batch_cases, budget_mask, budget_tile_steps, motion_case, smallest_mask, solid_routes)
from cases import _same_calls as _same_bits
from oracle.states import state
from moving_wall_ref import MovingWallOracle
from solid_ref import SolidOracle
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver, solid

pytestmark = pytest.mark.gpu

LD = np.longdouble
COLLS = ("SRT", "TRT", "MRT")


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
    """k_step_solid<.., WALL_MOVE> (96 x 80) and k_step_generic_wall<.., WALL_MOVE> (96 x 80 with kernel="generic"; 70 x 66 under `auto` in fp32) from S2 at the
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
