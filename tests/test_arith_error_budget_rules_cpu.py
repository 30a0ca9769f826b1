"""CPU side of the arithmetic error budget under the obstacle rules -- a shape, hold cells with a wall velocity per cell, periodic sides
with a driving force, the passive scalar and its buoyancy (the GPU side: tests/test_arith_error_budget_rules_gpu.py):

* in the long-double forms of the whole chain of references (tests/curved_wall_ref.py, open_flow_ref.py, periodic_ref.py, buoyancy_ref.py
  and scalar_ref.py) every table value is the lattice type's value widened, LD(P(x)), as the device's tables hold it: a and d of a shaped
  link, delta, the hold constants, F_k, B_k, c_ref, and the scalar's w+, w-, Dirichlet table, held values and initial c0;
* the long-double forms agree with their own fp64 forms to fp64 rounding after 100 steps on a 32 x 24 version of every case, and are
  not the same bits;
* a whole step built on the arith="fast" operators (cases._FastStep on oracle/lbm_fast.py) plus each rule's store side and read side
  is the dense long-double step on every fluid cell; deliberately wrong restatements of the rules fail that check, on the cells they
  touch and on no other;
* the cases of the GPU file hold what they claim, their long-double references stay finite with max|fin| <= 1 for every (case, state,
  rates) it runs, and its routes are what lbm_plan accepts and names, by a dry run."""
import itertools

import numpy as np
import pytest

from buoyancy_ref import BuoyantOracle
from cases import (CALLS, DISTINCT, RULE_BUOY, RULE_D, RULE_FORCE, RULE_NX, RULE_NY, RULE_RE, RULE_ROUTES, RULE_STATES, _FastStep, rule_cases,
                   rule_oracles, rule_step)
from oracle.states import state
from periodic_ref import drive_terms
from scalar_ref import WEIGHT, ScalarOracle, hold_values, rates as scalar_rates
from latticeboltzmannsimulations_amd import launch_plan

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
NX, NY = 32, 24
RE_SMALL = 300.0          # on 24 rows the relaxation rates of the GPU file's 72 x 40 lattice at Re 500 (nu = uLB ny / Re: 40 / 500 = 24 / 300)
COLLS = ("SRT", "TRT", "MRT")
TAGS = [sc["tag"] for sc in rule_cases(NX, NY)]


def _case(tag, nx=NX, ny=NY):
    return next(sc for sc in rule_cases(nx, ny) if sc["tag"] == tag)


def _start(o, s, st, dtype):
    """Both references of a pair at the state st: S0 is what the setters left, in the lattice type."""
    nx, ny = o.nx, o.ny
    if st != "S0":
        o.set_state(state(st, nx, ny, dtype).astype(o.dtype))
    return o, s


# ---- the cases hold what they claim ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(RULE_NX, RULE_NY), (NX, NY)], ids=["72x40", "32x24"])
def test_the_cases_hold_what_they_claim(shape):
    nx, ny = shape
    cs = {sc["tag"]: sc for sc in rule_cases(nx, ny)}
    assert list(cs) == ["shaped", "shaped moving", "shaped scalar", "open", "periodic forced", "buoyant hold", "buoyant periodic", "rest scalar"]
    # the disc: near links, far links, q = 1/2 exactly (a == 1) and a fallback link, all four
    sc = cs["shaped"]
    o, _ = rule_oracles(sc, "TRT", np.float64, Re=RE_SMALL)
    a, q_in = o.l_a, sc["q"][o.lk - 1, o.lx, o.ly]
    near, far = o.l_near, ~o.l_near & (o.l_q > 0.5)
    fallback = (q_in < 0.5) & ~o.l_near
    assert near.sum() >= 8 and far.sum() >= 8 and (q_in == 0.5).sum() >= 1 and fallback.sum() >= 1, (near.sum(), far.sum(), (q_in == 0.5).sum(), fallback.sum())
    assert np.all(a[q_in == 0.5] == 1.0) and np.all(a[fallback] == 1.0) and np.all(o.l_q[fallback] == 0.5)
    assert np.all(a[near] < 1.0) and np.all(a[far] < 1.0) and np.all(a[near] > 0.0)
    assert sc["mask"][sc["labels"] == 1].sum() == 1 and not np.any(cs["shaped"]["mask"] != cs["shaped moving"]["mask"])
    assert np.any(cs["shaped moving"]["motion"][0] != 0) and cs["shaped moving"]["motion"][0][2] != 0
    wv = cs["shaped scalar"]["wall_value"]
    d = ~np.isnan(wv)
    assert cs["shaped scalar"]["scalar"] and d.sum() >= 20 and (sc["mask"] & ~d).sum() >= 20 and not (d & ~sc["mask"]).any(), "half of the disc is Dirichlet"
    # open: the inlet pushes with a velocity of its own per cell, the outlet holds, a hold cell at every lane position, a staircase
    sc = cs["open"]
    assert sc["mask"][0].all() and len(set(sc["uw"][0, 0].tolist())) == ny and sc["hold"][nx - 2, 1:ny - 1].all()
    singles = sc["hold"].copy(); singles[nx - 2] = False
    assert sorted(int(x) % 4 for x in np.nonzero(singles)[0]) == [0, 1, 2, 3]
    stairs = np.argwhere(sc["mask"] & (sc["labels"] == 1))
    assert len(stairs) == 4 and np.all(np.diff(stairs, axis=0) == 1), "four cells that touch at corners only"
    # periodic xy with a force, a motion and a wall velocity; the buoyant twins at rest (hold cells) and with the motion
    for tag in ("periodic forced", "buoyant periodic"):
        sc = cs[tag]
        assert tuple(sc["per"]) == (1, 1) and sc["force"] == RULE_FORCE and np.any(sc["motion"]) and np.any(sc["uw"]) and 0.05 < sc["mask"].mean() < 0.15
        assert rule_oracles(sc, "TRT", np.float64, Re=RE_SMALL)[0].closed(), "the library's flux check"
    assert not cs["periodic forced"]["scalar"] and cs["periodic forced"]["buoy"] is None
    for tag in ("buoyant hold", "buoyant periodic"):
        assert cs[tag]["scalar"] and cs[tag]["buoy"] == RULE_BUOY and cs[tag]["q"] is None
    sc = cs["buoyant hold"]
    assert sc["hold"].sum() == ny - 2 + 2 and sc["motion"] is None and sc["uw"] is None and (~np.isnan(sc["wall_value"])).sum() == ny
    assert (~np.isnan(cs["buoyant periodic"]["wall_value"])).sum() >= 10
    for tag in ("shaped moving", "open"):
        assert rule_oracles(cs[tag], "TRT", np.float64, Re=RE_SMALL)[0].closed()
    # the open lattice at rest with the driving force and a passive scalar
    sc = cs["rest scalar"]
    assert np.array_equal(sc["mask"], cs["open"]["mask"]) and np.array_equal(sc["hold"], cs["open"]["hold"]) and sc["uw"] is None and sc["motion"] is None
    assert sc["scalar"] and sc["buoy"] is None and sc["q"] is None and sc["force"] == RULE_FORCE and (~np.isnan(sc["wall_value"])).sum() == ny
    assert not rule_oracles(sc, "TRT", np.float64, Re=RE_SMALL)[0].moving


# ---- every table value as the device holds it --------------------------------------------------------------------------------------------
def test_long_double_references_take_every_table_value_as_the_device_holds_it():
    cs = {sc["tag"]: sc for sc in rule_cases(NX, NY)}
    seen = {}
    for P in (np.float32, np.float64):
        W = lambda v: LD(P(v))  # noqa: E731
        # a and d of the shaped links (with the motion: d != 0)
        o, _ = rule_oracles(cs["shaped moving"], "MRT", P, long_double=True, Re=RE_SMALL)
        assert o.l_a.dtype == LD and o.l_d.dtype == LD and len(o.figs) > 40 and np.any(o.l_d != 0)
        for i, f in enumerate(o.figs):
            assert o.l_a[i] == W(f["a"]) and o.l_d[i] == W(f["d"]), (P, i)
        seen[P] = o.l_a.copy()
        # the hold constants and delta with the cell term
        sc = cs["open"]
        o, _ = rule_oracles(sc, "MRT", P, long_double=True, Re=RE_SMALL)
        assert o.held.dtype == LD and np.array_equal(o.held, np.asarray(sc["f"])[:, sc["hold"]].astype(P).astype(LD))
        assert o.delta.dtype == LD and np.any(o.delta[:, 1, :] != 0), "the inlet's cell term"
        for (x, y, k, _), d in zip(o.links, o.delta64):
            assert o.delta[k, x, y] == W(d), (P, x, y, k)
        # F_k, B_k, c_ref; the scalar's rates, Dirichlet table, held values and c0
        for tag in ("buoyant hold", "buoyant periodic"):
            sc = cs[tag]
            o, s = rule_oracles(sc, "MRT", P, long_double=True, Re=RE_SMALL)
            if sc["force"] != (0.0, 0.0):
                assert [v for v in o.drive] == [W(v) for v in drive_terms(*sc["force"])] and any(v != 0 for v in o.drive)
            assert [v for v in o.B] == [W(v) for v in drive_terms(*RULE_BUOY[:2])] and o.c_ref == W(RULE_BUOY[2])
            wp, wm = scalar_rates(RULE_D, 0.25)
            assert s.wp == W(wp) and s.wm == W(wm) and s.wp.dtype == LD
            wv = np.asarray(sc["wall_value"])
            n = 0
            for k in range(1, 9):
                assert s.t[k].dtype == LD
                for x, y in zip(*np.nonzero(s.dlink[k])):
                    sx, sy = (x - (0, 1, 0, -1, 0, 1, -1, -1, 1)[k]) % NX, (y + (0, 0, 1, 0, -1, 1, 1, -1, -1)[k]) % NY
                    assert s.t[k][x, y] == W((2.0 * WEIGHT[k]) * wv[sx, sy]), (P, k, x, y)
                    n += 1
                assert not s.t[k][~s.dlink[k]].any()
            assert n > 8
            for x, y in zip(*np.nonzero(s.uhold)):
                want = [W(v) for v in hold_values(np.asarray(sc["f"], dtype=np.float64)[:, x, y], sc["hold_value"][x, y])]
                assert s.held[:, x, y].tolist() == want, (P, x, y)
            free = ~s.mask & ~s.hold
            for k in range(9):
                assert np.array_equal(s.s[k][free], LD(WEIGHT[k]) * sc["c0"].astype(P).astype(LD)[free])
            # the lattice-type oracle is unchanged: its tables, widened, are the long-double oracle's
            _, sl = rule_oracles(sc, "MRT", P, Re=RE_SMALL)
            assert sl.wp.dtype == np.dtype(P) and LD(sl.wp) == s.wp and LD(sl.wm) == s.wm and np.array_equal(sl.held.astype(LD), s.held)
            assert all(np.array_equal(sl.t[k].astype(LD), s.t[k]) for k in range(1, 9))
            seen[(P, tag)] = (s.wp, s.held.copy())
    assert not np.array_equal(seen[np.float32], seen[np.float64]) and seen[(np.float32, "buoyant hold")][0] != seen[(np.float64, "buoyant hold")][0]
    # the default parameter type of a long-double oracle is float64
    sc = cs["buoyant hold"]
    s = ScalarOracle(sc["mask"], RULE_D, sc["c0"], LD, wall_value=sc["wall_value"], hold=sc["hold"], hold_f=sc["f"], hold_value=sc["hold_value"])
    assert s.wp == seen[(np.float64, "buoyant hold")][0] and np.array_equal(s.held, seen[(np.float64, "buoyant hold")][1])


# ---- the long-double references against their fp64 forms -------------------------------------------------------------------------------
LD_VS_FP64_MEASURED = 6.78e-14     # the largest distance over the 96 runs below (fin, u / uLB, rho, the scalar's populations and C): u / uLB of
                                   # "buoyant hold"; per case 1.7e-14 .. 6.8e-14 (shaped 1.7, moving 2.0, open 5.6, periodic 3.2, buoyant 6.8 and 1.5, rest scalar 6.6)


def _distances(N, sN, L, sL):
    fl = L.fluid()
    ref = np.abs(L.fin[:, fl]).max()
    e = dict(fin=float(np.abs(N.fin - L.fin)[:, fl].max() / ref), u=float(np.abs(N.u - L.u)[:, fl].max()) / 0.08, rho=float(np.abs(N.rho - L.rho)[fl].max()))
    if sL is not None:
        g, gl = sN.populations(), sL.populations()
        e["g"] = float(np.abs(g - gl)[:, fl].max() / np.abs(gl[:, fl]).max())
        e["C"] = float(np.abs(sN.conc() - sL.conc())[fl].max() / np.abs(sL.conc()[fl]).max())
    return e


@pytest.mark.parametrize("tag", TAGS)
def test_long_double_rule_references_agree_with_their_fp64_forms(tag):
    """32 x 24 at Re 300 (the rates of the GPU file's lattice), every case, the three operators, from S0 and S2 at the default and at the
    distinct rates, 1 + 99 steps: the long-double pair against the fp64 pair of the same classes on the fluid cells that are not held --
    fin (relative to max|fin|), u / uLB, rho, and where a scalar runs its arriving populations and C (relative to their maxima) -- within
    4 x the largest distance measured over all 96 runs, LD_VS_FP64_MEASURED; not the same bits; max|fin| <= 1 at the read-outs."""
    sc = _case(tag)
    worst = 0.0
    for coll, st, rates in itertools.product(COLLS, RULE_STATES, ({}, DISTINCT)):
        N, sN = _start(*rule_oracles(sc, coll, np.float64, rates, Re=RE_SMALL), st, np.float64)
        L, sL = _start(*rule_oracles(sc, coll, np.float64, rates, long_double=True, Re=RE_SMALL), st, np.float64)
        assert L.fin.dtype == LD and (sL is None or sL.s.dtype == LD)
        for n in (1, 99):
            rule_step(N, sN, n); rule_step(L, sL, n)
            assert L.fin.dtype == LD and np.isfinite(L.fin).all() and float(np.abs(L.fin).max()) <= 1.0, (coll, st, rates)
        e = _distances(N, sN, L, sL)
        worst = max(worst, max(e.values()))
        print(f"{tag} long double vs fp64 {coll} {st} {'distinct' if rates else 'default'}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= 4 * LD_VS_FP64_MEASURED, (coll, st, rates, e)
        assert not np.array_equal(N.fin, L.fin.astype(np.float64)), "the reference really is another precision"
    print(f"{tag}: largest {worst:.3e}")


# ---- a whole step on the fast operators, per rule -----------------------------------------------------------------------------------------
class FastRules(BuoyantOracle):
    """The chain of references with the collision of cases._FastStep -- the restatements of the device's fast operators (oracle/lbm_fast.py),
    fed the plain-sum macros -- followed by what the rules add on the store side as lbm_solid.hpp spells it for every arithmetic: on the
    cells that are neither solid nor held fpost_k + (F_k + B_k (Cp - c_ref)) with buoyancy, fpost_k + F_k with a driving force alone.
    The read side (the shape, the hold cells, the image cells, delta) is the chain's own stream_bb."""
    meq_density = "rho"

    def macros(self, f):
        rho, ux, uy = super().macros(f)
        self._u = (ux, uy)
        return rho, ux, uy

    def operator(self, f, rho, feq, w_nu):
        return _FastStep.collide(self, f, rho, feq, w_nu)

    def hold_cells_too(self):
        return False

    def collide(self, f, rho, feq, w_nu=None):
        out = self.operator(f, rho, feq, w_nu)
        fl = ~self.mask if self.hold_cells_too() else self.fluid()
        F = self.drive if self.drive is not None else [self.R(0.0)] * 9
        if self.buoy is not None:
            t = self.Cp[fl] - self.c_ref
            for k in range(1, 9):
                out[k][fl] = out[k][fl] + (F[k] + self.B[k] * t)
        elif self.drive is not None:
            for k in range(1, 9):
                out[k][fl] = out[k][fl] + F[k]
        return out


class ForceOnHoldCells(FastRules):
    """WRONG on purpose: a hold cell adds the force (with buoyancy d_k) to the values it holds, so its neighbours pull held_k + d_k."""
    def stream_bb(self, fpost, rho):
        held = self.held
        d = np.zeros_like(held)
        F = self.drive if self.drive is not None else [self.R(0.0)] * 9
        for k in range(1, 9):
            d[k] = F[k] if self.buoy is None else F[k] + self.B[k] * (self.Cp[self.hold] - self.c_ref)
        self.held = held + d
        try:
            return super().stream_bb(fpost, rho)
        finally:
            self.held = held


class ReferenceValueUnrounded(FastRules):
    """WRONG on purpose: B_k (Cp - c_ref) with c_ref as given in double, not as rounded to the lattice type."""
    def set_buoyancy(self, ax=0.0, ay=0.0, c_ref=0.0):
        super().set_buoyancy(ax, ay, c_ref)
        self.c_ref = self.R(c_ref)
        return self


class RatesSwapped(FastRules):
    """WRONG on purpose: the MRT rates omega_eps and omega_q change places."""
    def operator(self, f, rho, feq, w_nu):
        ov = self.omega_vec
        keep = list(ov)
        ov[2], ov[4], ov[6] = keep[4], keep[2], keep[2]
        try:
            return super().operator(f, rho, feq, w_nu)
        finally:
            self.omega_vec = keep


class InterpolationFromOwn(BuoyantOracle):
    """The interpolation of a shaped link written as own + (1 - a) (other - own): the same algebra as a own + (1 - a) other, other
    roundings."""
    def stream_bb(self, fpost, rho):
        fin = super().stream_bb(fpost, rho)
        own = fpost[self.lo, self.lx, self.ly]
        other = np.where(self.l_near, fpost[self.lo, self.lnx, self.lny], fpost[self.lk, self.lx, self.ly])
        a, d = self.l_a, self.l_d
        fin[self.lk, self.lx, self.ly] = np.where(a == self.R(1.0), own + d, (own + (self.R(1.0) - a) * (other - own)) + d)
        return fin


class FastInterpolationFromOwn(InterpolationFromOwn, FastRules):
    pass


def _pair(sc, dense, fast, coll, st, P=np.float64, rates=DISTINCT):
    """(dense, its scalar, fast, its scalar) in long double from the state st, one Cp for both."""
    d, sd = _start(*rule_oracles(sc, coll, P, rates, long_double=True, Re=RE_SMALL, flow_cls=dense), st, P)
    q, sq = _start(*rule_oracles(sc, coll, P, rates, long_double=True, Re=RE_SMALL, flow_cls=fast), st, P)
    return d, sd, q, sq


def _cell_errors(q, d):
    """Per cell: fin (relative to max|fin| over the fluid cells), and u / uLB and rho as the next step will form them from fin."""
    fl = d.fluid()
    (rq, xq, yq), (rd, xd, yd) = q.macros(q.fin), d.macros(d.fin)
    return dict(fin=(np.abs(q.fin - d.fin) / np.abs(d.fin[:, fl]).max()).max(axis=0), u=np.maximum(np.abs(xq - xd), np.abs(yq - yd)) / LD(0.08),
                rho=np.abs(rq - rd))


ONE_STEP_TOL = 32 * EPS_LD      # the budget's bound after one step, in the eps of the type the two steps run in
ONE_STEP_MEASURED = 12.1        # eps of long double: the largest per-cell difference after one step over the matrix below (per case 8.8 .. 12.1)


@pytest.mark.parametrize("tag", TAGS)
def test_a_step_on_the_fast_operators_is_the_dense_step_under_every_rule(tag):
    """FastRules against the dense long-double chain on the 32 x 24 version of every case, the three operators, from S0 and S2 at the
    default and at the distinct rates: after one step fin (relative to max|fin| over the fluid cells) and the u / uLB and rho the next
    step forms from it agree on every cell that is neither solid nor held within 32 long-double eps (measured: ONE_STEP_MEASURED);
    solid cells hold w_k, hold cells and image cells what they hold, in both."""
    sc = _case(tag)
    worst = 0.0
    for coll, st, rates in itertools.product(COLLS, RULE_STATES, ({}, DISTINCT)):
        d, sd, q, sq = _pair(sc, BuoyantOracle, FastRules, coll, st, rates=rates)
        fl = d.fluid()
        rule_step(d, sd, 1); rule_step(q, sq, 1)
        assert q.fin.dtype == LD
        pinned = d.mask | (d._uhold if getattr(d, "_uhold", None) is not None else False)      # (an image cell holds its partner's values)
        assert np.array_equal(q.fin[:, pinned], d.fin[:, pinned]), "solid cells and the user's hold cells hold the same in both"
        for k, v in _cell_errors(q, d).items():
            v = np.where(fl, v, 0)
            worst = max(worst, float(v.max()))
            assert float(v.max()) <= ONE_STEP_TOL, (coll, st, rates, k, float(v.max()) / EPS_LD, "eps at", np.unravel_index(int(np.argmax(v)), v.shape))
    print(f"{tag}: fast step vs dense, largest after one step {worst / EPS_LD:.1f} eps")


def _pulls_from(sel):
    """Cells with a slot whose source lies in sel (no wrap)."""
    from scalar_ref import CX, CY
    out = np.zeros_like(sel)
    X, Y = sel.shape
    for k in range(1, 9):
        for x, y in zip(*np.nonzero(sel)):
            tx, ty = x + CX[k], y - CY[k]
            if 0 <= tx < X and 0 <= ty < Y:
                out[tx, ty] = True
    return out


@pytest.mark.parametrize("coll", COLLS)
def test_the_step_check_sees_a_wrong_rule_on_the_cells_it_touches(coll):
    """One step from S2 at the distinct rates, each wrong restatement against the dense chain:
    * the force added to hold cells ("rest scalar": F_k; "buoyant hold": d_k): fin is off by more than 1e3 tolerances on fluid cells that pull from a hold cell
      whose d_k is not zero, within the tolerance on every other cell;
    * c_ref before its rounding (c_ref = 0.3 in an fp32 lattice, "buoyant periodic"): every fluid cell is off, by B_k times the rounding
      of c_ref, more than 1e3 tolerances;
    * omega_eps and omega_q swapped (MRT, "shaped moving" and "buoyant hold"): every fluid cell is off."""
    for tag in ("rest scalar", "buoyant hold"):      # (the driving force alone; the buoyancy's d_k)
        d, sd, q, sq = _pair(_case(tag), BuoyantOracle, ForceOnHoldCells, coll, "S2")
        rule_step(d, sd, 1); rule_step(q, sq, 1)
        fl = d.fluid()
        err = np.where(fl, _cell_errors(q, d)["fin"], 0)
        beside = _pulls_from(d.hold) & fl
        bad = err > ONE_STEP_TOL
        assert bad.any() and not (bad & ~beside).any() and float(err[beside].max()) > 1e3 * ONE_STEP_TOL, tag
        assert bad.sum() >= beside.sum() // 2, (tag, bad.sum(), beside.sum())

    sc = dict(_case("buoyant periodic"), buoy=(RULE_BUOY[0], RULE_BUOY[1], 0.3))
    assert LD(np.float32(0.3)) != LD(0.3)
    d, sd, q, sq = _pair(sc, BuoyantOracle, ReferenceValueUnrounded, coll, "S2", P=np.float32)
    assert d.c_ref == LD(np.float32(0.3)) and q.c_ref == LD(0.3)
    rule_step(d, sd, 1); rule_step(q, sq, 1)
    fl = d.fluid()
    err = np.where(fl, _cell_errors(q, d)["fin"], 0)
    assert (err[fl] > 1e3 * ONE_STEP_TOL).all()
    d, sd, q, sq = _pair(sc, BuoyantOracle, FastRules, coll, "S2", P=np.float32)      # (rounded as the device rounds it: inside the bound)
    rule_step(d, sd, 1); rule_step(q, sq, 1)
    assert float(np.where(fl, _cell_errors(q, d)["fin"], 0).max()) <= ONE_STEP_TOL

    if coll == "MRT":
        for tag in ("shaped moving", "buoyant hold"):
            d, sd, q, sq = _pair(_case(tag), BuoyantOracle, RatesSwapped, coll, "S2")
            rule_step(d, sd, 1); rule_step(q, sq, 1)
            fl = d.fluid()
            err = np.where(fl, _cell_errors(q, d)["fin"], 0)
            assert (err[fl] > 1e3 * ONE_STEP_TOL).all(), tag
            d, sd, q, sq = _pair(_case(tag), BuoyantOracle, RatesSwapped, coll, "S2", rates={})
            rule_step(d, sd, 1); rule_step(q, sq, 1)                                   # (at the default rates the two are equal: nothing to see)
            assert float(np.where(fl, _cell_errors(q, d)["fin"], 0).max()) <= ONE_STEP_TOL, tag


@pytest.mark.parametrize("coll", COLLS)
def test_the_interpolation_written_from_own_is_seen_by_the_bits_and_not_by_the_bound(coll):
    """own + (1 - a) (other - own) is a own + (1 - a) other in exact arithmetic, so no bound on the error can tell the two apart: in long
    double the fast step with it stays within the one-step tolerance of the dense step.  What tells them apart is the bit identity the
    GPU file asserts of strict: in the lattice type, one step from S2, the populations differ from the reference's on shaped links with
    a != 1 (23 to 26 of the 120 in fp32, where the two roundings often meet; at least a tenth is asserted) and on no other cell."""
    sc = _case("shaped moving")
    d, sd, q, sq = _pair(sc, BuoyantOracle, FastInterpolationFromOwn, coll, "S2")
    rule_step(d, sd, 1); rule_step(q, sq, 1)
    fl = d.fluid()
    assert float(np.where(fl, _cell_errors(q, d)["fin"], 0).max()) <= ONE_STEP_TOL
    for P in (np.float32, np.float64):
        f0 = state("S2", NX, NY, P)
        a, _ = rule_oracles(sc, coll, P, DISTINCT, Re=RE_SMALL)
        b, _ = rule_oracles(sc, coll, P, DISTINCT, Re=RE_SMALL, flow_cls=InterpolationFromOwn)
        a.set_state(f0); b.set_state(f0)
        a.step(1); b.step(1)
        differs = a.fin != b.fin
        touched = np.zeros_like(differs)
        sel = a.l_a != a.R(1.0)
        touched[a.lk[sel], a.lx[sel], a.ly[sel]] = True
        assert differs.any() and not (differs & ~touched).any() and differs.sum() >= touched.sum() // 10, (P, differs.sum(), touched.sum())


# ---- what the GPU file runs: finite references and the routes -----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_the_long_double_reference_stays_finite_on_every_case_state_and_rate_set_of_the_gpu_tests(tag):
    """72 x 40 at Re 500, in long double with the parameters of each lattice type, the three operators, S0 and S2, the default and the
    distinct rates: finite with max|fin| <= 1 after each of the 26 steps, and the scalar finite.  No combination is left out."""
    sc = _case(tag, RULE_NX, RULE_NY)
    for dtype, coll, st, rates in itertools.product((np.float32, np.float64), COLLS, RULE_STATES, ({}, DISTINCT)):
        o, s = _start(*rule_oracles(sc, coll, dtype, rates, long_double=True), st, dtype)
        assert o.relax["omega"] == pytest.approx(2.0 / (6.0 * 0.08 * RULE_NY / RULE_RE + 1.0))
        for _ in range(sum(CALLS)):
            rule_step(o, s, 1)
            assert np.isfinite(o.fin).all() and float(np.abs(o.fin).max()) <= 1.0, (tag, dtype, coll, st, rates, o.nsteps, float(np.abs(o.fin).max()))
        assert s is None or np.isfinite(s.populations()).all()


@pytest.mark.parametrize("arith", ["strict", "fast"])
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_gpu_tests_rule_routes_are_what_the_plan_accepts(dtype, coll, arith):
    """RULE_ROUTES on 72 x 40: `auto` plans the vector kernel k_step_solid (both vector widths divide 72), kernel="generic" the one-cell
    route, and tuning nt=True the vector kernel with nt == 1 -- one step per launch each."""
    assert RULE_NX % 4 == 0 and RULE_NX % 2 == 0
    for kernel, tune, name, nt in RULE_ROUTES:
        p = launch_plan(RULE_NX, RULE_NY, RULE_RE, steps=sum(CALLS), kernel=kernel, tuning=tune, RT=coll, semantics="bounce_back", solid=True, dtype=dtype,
                        arith=arith)
        assert (p["kernel"], p["nt"], p["steps_per_launch"], p["semantics"]) == (name, nt, 1, "bounce_back_solid"), (kernel, tune, p)
        assert p["vec"] == (1 if name == "k_step_solid" else 0) and p["units"] == [1] * sum(CALLS)
