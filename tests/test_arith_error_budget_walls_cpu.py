"""CPU side of the arithmetic error budgets under MRT.py's walls and the half-way bounce-back walls (the GPU side:
tests/test_arith_error_budget_gpu.py):

* the long-double form of the bounce-back reference (tests/bounce_back_ref.BounceBackOracle with dtype=np.longdouble) agrees with
  its own fp64 form to fp64 rounding after 100 steps, and keeps the total mass to long-double rounding: it is pinned without a device;
* a whole step built on the arith="fast" operators (oracle/lbm_fast.py, given the rho, ux, uy that each semantics' own macros()
  produces) is the oracle's dense step in long double in every cell, wall cells included, for MRT_GPU.py's walls, MRT.py's walls
  and bounce-back; the density that m_eq[1], m_eq[2] took before the lid-row fix is seen on row 0 under MRT.py's walls too;
* the kernel families that the GPU test runs under these two semantics are the ones lbm_plan accepts, by a dry run."""
import numpy as np
import pytest

from bounce_back_ref import BounceBackOracle
from cases import CALLS, DISTINCT, WALL_FAMILIES, _FastStep
from cases import _family_shape as _shape
from oracle.lbm_numpy import CavityOracle
from oracle.states import state
from latticeboltzmannsimulations_amd import launch_plan
from latticeboltzmannsimulations_amd.slab import partition_rows

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
NX, NY = 32, 24


# ---- the bounce-back reference in long double ------------------------------------------------------------------------------------
MASS_MEASURED = 25.3    # eps of long double: the largest relative change of sum fin over the 18 runs below


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_long_double_bounce_back_reference_agrees_with_its_fp64_form_and_keeps_the_mass(coll):
    """32 x 24, Re 1000, from S0, S2 and S3 at the default and at distinct rates, 1 + 99 steps.  Against the fp64 form of the same
    class: <= 1e-13 on fin (relative to max|fin|), u / uLB and rho (measured over the 18 runs: fin 1.2e-14, u / uLB 3.7e-14, rho
    2.1e-14), and not the same bits.  Independently of any other code: the wall rule moves +t to slot 8 and -t to slot 7 of the same
    cell and bounces every other population back, and the collision keeps m0, so sum fin changes by rounding only: measured <= 25.3
    long-double eps relative after 100 steps (10.7 - 13.3 for MRT, 21.3 - 25.3 for SRT and TRT; sum in long double); bound 4 x that."""
    for st in ("S0", "S2", "S3"):
        for rates in ({}, DISTINCT):
            f = state(st, NX, NY, np.float64)
            L = BounceBackOracle(NX, NY, 1000.0, collision=coll, dtype=LD, **rates)
            N = BounceBackOracle(NX, NY, 1000.0, collision=coll, dtype=np.float64, **rates)
            N.set_state(f)
            L.set_state(f.astype(LD))
            assert L.fin.dtype == LD and L.t.dtype == LD
            m0 = np.sum(L.fin, dtype=LD)
            for n in (1, 99):
                L.step(n); N.step(n)
                assert L.fin.dtype == LD and L.rho.dtype == LD and L.u.dtype == LD
                assert np.isfinite(L.fin).all() and float(np.abs(L.fin).max()) <= 0.85, (st, rates)
            ref = np.abs(L.fin).max()
            e = (float(np.abs(N.fin - L.fin).max() / ref), float(np.abs(N.u - L.u).max()) / 0.08, float(np.abs(N.rho - L.rho).max()))
            drift = float(abs(np.sum(L.fin, dtype=LD) - m0) / m0) / EPS_LD
            print(f"bounce-back long double vs fp64 {coll} {st} {'distinct' if rates else 'default'}: fin {e[0]:.2e} u/uLB {e[1]:.2e} "
                  f"rho {e[2]:.2e}; mass drift {drift:.1f} eps")
            assert max(e) <= 1e-13, (st, rates, e)
            assert not np.array_equal(N.fin, L.fin.astype(np.float64)), "the reference really is another precision"
            assert drift <= 4 * MASS_MEASURED, (st, rates, drift)


def test_long_double_bounce_back_reference_takes_the_parameters_as_the_device_holds_them():
    o32 = BounceBackOracle(8, 6, 1000.0, collision="MRT", dtype=LD, param_dtype=np.float32, **DISTINCT)
    o64 = BounceBackOracle(8, 6, 1000.0, collision="MRT", dtype=LD, **DISTINCT)
    for o, P in ((o32, np.float32), (o64, np.float64)):
        assert o.omega_vec[1] == LD(P(1.13)) and o.omega_vec[2] == LD(P(1.41)) and o.omega_vec[4] == LD(P(1.67))
        assert o.omega_vec[7] == LD(P(o.relax["omega"])) and o.par(o.relax["omegam"]) == LD(P(1.31)) and o.par(o.uLB) == LD(P(0.08))
    assert o32.omega_vec[1] != o64.omega_vec[1]
    assert o64.relax["omega_eps"] == 1.41 and BounceBackOracle(8, 6, 1000.0).relax["omega_eps"] == 1.2


# ---- a whole step on the fast operators (_FastStep of tests/cases.py), per wall semantics ------------------------------------------
class FastCavity(_FastStep, CavityOracle):
    pass


class FastBounceBack(_FastStep, BounceBackOracle):
    pass


def _pair(sem, coll, st, **kw):
    """(dense, fast) long-double oracles of one semantics from the same state at the distinct rates."""
    f = state(st, NX, NY, np.float64).astype(LD)
    if sem == "bounce_back":
        d, q = (c(NX, NY, 1000.0, collision=coll, dtype=LD, **DISTINCT) for c in (BounceBackOracle, FastBounceBack))
    else:
        d, q = (c(NX, NY, 1000.0, semantics=sem, collision=coll, dtype=LD, **DISTINCT) for c in (CavityOracle, FastCavity))
    for k, v in kw.items():
        setattr(q, k, v)
    d.set_state(f); q.set_state(f)
    return d, q


STEP_MEASURED = 72.8     # eps of long double: the largest per-cell difference over the matrix below
STEP_TOL = 4 * STEP_MEASURED * EPS_LD


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("sem", ["mrt_gpu", "mrt_py", "bounce_back"])
def test_a_step_on_the_fast_operators_is_the_dense_step_in_long_double(sem, coll):
    """From S2 and S3 at the distinct rates, after 1, 2, 5, 13 and 26 steps: fin (relative to max|fin|), u / uLB and rho of the
    fast step against the dense long-double oracle, in every cell.  Measured (32 x 24, Re 1000): at most 72.8 long-double eps over the
    read-outs (SRT 69.5 - 72.8, TRT 56.2 - 67.8, MRT 26.6 - 28.9 per semantics; after one step at most 2.9); the tolerance is 4 x
    that, 3.2e-17 -- a seventh of an fp64 eps, so an algebraic difference on any cell is far outside it."""
    worst = 0.0
    for st in ("S2", "S3"):
        d, q = _pair(sem, coll, st)
        for n in CALLS:
            d.step(n); q.step(n)
            assert q.fin.dtype == LD
            e = dict(fin=np.abs(q.fin - d.fin) / np.abs(d.fin).max(), u=np.abs(q.u - d.u) / LD(0.08), rho=np.abs(q.rho - d.rho))
            for k, v in e.items():
                worst = max(worst, float(v.max()))
                assert float(v.max()) <= STEP_TOL, (st, d.nsteps, k, float(v.max()) / EPS_LD, "eps at",
                                                    np.unravel_index(int(np.argmax(v)), v.shape))
            if d.nsteps == 1:
                print(f"fast step vs dense {sem} {coll} {st}: one step {max(float(v.max()) for v in e.values()) / EPS_LD:.1f} eps")
    print(f"fast step vs dense {sem} {coll}: largest {worst / EPS_LD:.1f} eps")


@pytest.mark.parametrize("sem", ["mrt_gpu", "mrt_py"])
def test_the_step_check_sees_the_population_sum_in_m_eq_on_the_lid_row(sem):
    """m_eq[1], m_eq[2] from the population sum, as the factored form built them before its fix: one step from S2 and S3 leaves the
    post-collision populations of row 0, and of no other row, off by more than 1e-7 in every column (MRT.py's walls override the
    lid row's density exactly as MRT_GPU.py's do, MRT.py:337); the step check above fails on it after one step.  Under bounce-back
    no density is overridden, and the same choice changes nothing beyond rounding."""
    for st in ("S2", "S3"):
        d, q = _pair(sem, "MRT", st, meq_density="r")
        d.step(1); q.step(1)
        err = np.abs(q.fpost - d.fpost).max(axis=0)
        assert err[:, 1:].max() <= STEP_TOL * np.abs(d.fpost).max(), st
        assert err[:, 0].min() > 1e-7, (st, float(err[:, 0].min()))
        assert float(np.abs(q.fin - d.fin).max() / np.abs(d.fin).max()) > 1e3 * STEP_TOL
    d, q = _pair("bounce_back", "MRT", "S3", meq_density="r")
    d.step(5); q.step(5)
    assert float(np.abs(q.fin - d.fin).max() / np.abs(d.fin).max()) <= STEP_TOL


# ---- the kernel families of the GPU test, by a dry run ---------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["strict", "fast"])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sem", ["mrt_py", "bounce_back"])
def test_the_gpu_tests_kernel_families_are_what_the_plan_accepts(sem, dtype, coll, arith):
    """Every entry of WALL_FAMILIES plans the kernel and the steps per launch it names, the streaming entries with the wall frame;
    the 96 x 80 lattice of the budget takes the multi-step tile kernel with its frame under `auto`, and its three slabs agree on
    one plan; vec is refused for both semantics, and the push scheme and the streaming kernels with the walls inside for bounce-back
    (under MRT.py's walls a request for the latter plans the kernel with the frame)."""
    kw = dict(RT=coll, semantics=sem, dtype=dtype, arith=arith)
    for kernel, tbs, tune, name, steps in WALL_FAMILIES[sem]:
        p = launch_plan(*_shape(kernel), 1000.0, steps=20, kernel=kernel, tuning=dict(tb_steps=tbs, **tune), **kw)
        assert (p["kernel"], p["steps_per_launch"]) == (name, steps), (kernel, tbs, p)
        assert (p["frame"] > 0) == (steps > 1) and p["stream"] == (kernel == "stream") and max(p["units"]) == steps, (kernel, tbs, p)
    whole = launch_plan(96, 80, 1000.0, steps=13, **kw)
    assert whole["kernel"] == "k_stepS_deep" and whole["frame"] > 0 and max(whole["units"]) >= 4
    slabs = [launch_plan(96, 80, 1000.0, steps=29, rows=rows, **kw) for rows in partition_rows(80, 3)]
    assert len({(p["kernel"], p["steps_per_launch"], p["frame"], p["deep_halo"], tuple(p["units"])) for p in slabs}) == 1, slabs
    refused = [("vec", {})] + ([("push", {}), ("stream", dict(stream_walls=True)), ("stream", dict(stream_pairs=True))]
                               if sem == "bounce_back" else [])
    for kernel, tune in refused:
        with pytest.raises(RuntimeError, match="lbm_plan"):
            launch_plan(*_shape(kernel), 1000.0, kernel=kernel, tuning=tune, **kw)
    if sem == "mrt_py":
        for tune in (dict(stream_walls=True), dict(stream_pairs=True)):
            assert launch_plan(264, 150, 1000.0, kernel="stream", tuning=dict(tb_steps=5, **tune), **kw)["kernel"] == "k_stream"
