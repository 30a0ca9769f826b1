"""CPU side of the arithmetic error budgets (tests/test_arith_error_budget_gpu.py):

* the long-double reference (oracle.lbm_numpy.CavityOracle with dtype=np.longdouble) is what the budgets measure against: it
  agrees with the fp64 NumPy and C oracles to fp64 rounding after 100 steps, for every operator, with and without the closure,
  both semantics, from rest and from off-equilibrium states, at the default and at distinct relaxation rates;
* the algebra of the arith="fast" operators (oracle/lbm_fast.py restates them as lbm_device.hpp writes them) is that of the
  oracle's dense operators: in long double the two agree to long-double rounding on random off-equilibrium states, the lid row
  included."""
import numpy as np
import pytest

from oracle.lbm_fast import history_fast, mrt_fast, srt_trt_fast
from oracle.lbm_numpy import CX, CY, M_GS, M_GS_INV, CavityOracle, equ, m_gs_inv, weights
from oracle.lbm_ref import CavityOracleC
from oracle.states import state

LD = np.longdouble
DISTINCT = dict(omega_e=1.13, omega_eps=1.41, omega_q=1.67, omegam=1.31)
EPS_LD = float(np.finfo(LD).eps)


def test_long_double_is_extended():
    assert np.finfo(LD).nmant >= 63
    t = weights(LD)
    assert t.dtype == LD and t[0] == LD(4) / 9 and t[1] == LD(1) / 9 and t[5] == LD(1) / 36
    assert abs(t.sum() - 1) <= 4 * EPS_LD
    assert t[1] != LD(1.0 / 9.0)                                    # not the fp64 literal
    mi = m_gs_inv(LD)
    assert np.abs(mi @ M_GS.astype(LD) - np.eye(9, dtype=LD)).max() <= 16 * EPS_LD
    assert np.array_equal(m_gs_inv(np.float64), M_GS_INV) and np.array_equal(m_gs_inv(np.float32), M_GS_INV.astype(np.float32))


def test_long_double_reference_takes_the_parameters_as_the_device_holds_them():
    o32 = CavityOracle(8, 6, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=LD, param_dtype=np.float32, **DISTINCT)
    o64 = CavityOracle(8, 6, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=LD, **DISTINCT)
    for o, P in ((o32, np.float32), (o64, np.float64)):
        assert o.omega_vec[1] == LD(P(1.13)) and o.omega_vec[2] == LD(P(1.41)) and o.omega_vec[4] == LD(P(1.67))
        assert o.omega_vec[7] == LD(P(o.relax["omega"])) and o.par(o.relax["omegam"]) == LD(P(1.31))
        assert o.fin.dtype == LD and o.fin[1, 0, 0] == (LD(1) / 9) * (1 + 3 * LD(P(0.08)) + LD(4.5) * LD(P(0.08)) ** 2
                                                                       - LD(1.5) * LD(P(0.08)) ** 2)
    assert o32.omega_vec[1] != o64.omega_vec[1]


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("sem,turb", [("mrt_gpu", 0), ("mrt_gpu", 1), ("mrt_py", 0)])
def test_long_double_reference_agrees_with_the_fp64_oracles(coll, sem, turb):
    """<= 1e-13 relative after 100 steps (measured: 5e-15 to 1.3e-14 on 40 x 30, Re 1000), from rest and from S2 / S3, at the
    default and at distinct rates; the fp64 NumPy and C oracles stay bit-identical to each other at the distinct rates.
    (MRT.py's windows with TRT do not survive S3's density contrast -- populations grow to 1e8 in 100 steps in every precision --
    so mrt_py runs from S0 and S2.)"""
    nx, ny = 32, 24
    for st in ("S0", "S2") + (("S3",) if sem == "mrt_gpu" else ()):
        for rates in ({}, DISTINCT):
            f = state(st, nx, ny, np.float64)
            kw = dict(semantics=sem, collision=coll, turb=turb, **rates)
            L = CavityOracle(nx, ny, 1000.0, dtype=LD, **kw)
            N = CavityOracle(nx, ny, 1000.0, dtype=np.float64, **kw)
            C = CavityOracleC(nx, ny, 1000.0, dtype=np.float64, **kw)
            for o in (N, C):
                o.set_state(f)
            L.set_state(f.astype(LD))
            for n in (1, 99):
                L.step(n); N.step(n); C.step(n)
                assert np.array_equal(N.fin, C.fin) and np.array_equal(N.u, C.u) and np.array_equal(N.rho, C.rho), (st, rates)
            ref = np.abs(L.fin).max()
            assert float(np.abs(N.fin - L.fin).max() / ref) <= 1e-13, (st, rates)
            assert float(np.abs(N.u - L.u).max()) / 0.08 <= 1e-13 and float(np.abs(N.rho - L.rho).max()) <= 1e-13, (st, rates)
            assert not np.array_equal(N.fin, L.fin.astype(np.float64)), "the reference really is another precision"


def _off_equilibrium_cells(nx=48, ny=36, seed=11):
    """Random off-equilibrium populations (rho in [0.6, 1.6], |u| <= 0.15, 2 % independent noise) and the macroscopic fields
    the oracle's macros() gives them -- row 0 is the lid: rho_l = f0 + f1 + f3 + 2 (f2 + f5 + f6), u = (uLB, 0)."""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.6, 1.6, (nx, ny))
    ux, uy = rng.uniform(-0.1, 0.1, (nx, ny)), rng.uniform(-0.1, 0.1, (nx, ny))
    f = equ(rho, ux, uy, weights(np.float64)) * (1 + 0.02 * rng.uniform(-1, 1, (9, nx, ny)))
    o = CavityOracle(nx, ny, 1000.0, semantics="mrt_gpu", collision="MRT", dtype=LD, **DISTINCT)
    f = f.astype(LD)
    r, u, v = o.macros(f)
    assert np.abs(r[:, 0] - f.sum(axis=0)[:, 0]).min() > 1e-4                 # the lid's density is not m0 there
    return o, f, r, u, v


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("w_nu", [1.0, 1.37, 1.93])
def test_factored_mrt_is_the_dense_operator_in_long_double(w_nu):
    """The factored MRT operator (lbm_device.hpp collide<T, C_MRT_FAST>) against the oracle's dense M / M^-1 products with the
    reference's m_eq polynomial: equal to long-double rounding in every cell.  The pre-fix form, m_eq[1], m_eq[2] built from
    the population sum instead of rho, is off by O(1e-3) on the lid row and nowhere else -- this test is what catches it."""
    o, f, rho, ux, uy = _off_equilibrium_cells()
    dense = o.collide(f, rho, None, LD(w_nu))
    ov = o.omega_vec
    fast = np.array(mrt_fast(f, rho, ov[1], ov[2], ov[4], LD(w_nu)))
    assert _rel(fast, dense) <= 64 * EPS_LD, _rel(fast, dense)
    old = np.array(mrt_fast(f, rho, ov[1], ov[2], ov[4], LD(w_nu), meq_density="r"))
    err = np.abs(old - dense).max(axis=0)
    assert err[:, 1:].max() <= 64 * EPS_LD * np.abs(dense).max()
    assert err[:, 0].min() > 1e-7


@pytest.mark.parametrize("coll", ["SRT", "TRT"])
def test_fused_srt_trt_are_the_dense_operators_in_long_double(coll):
    o, f, rho, ux, uy = _off_equilibrium_cells()
    o.coll = coll
    for w_nu in (LD(1.0), LD(1.37), LD(1.93)):
        dense = o.collide(f, rho, equ(rho, ux, uy, o.t), w_nu)
        fast = np.array(srt_trt_fast(coll, f, rho, ux, uy, w_nu, o.par(o.relax["omegam"])))
        assert _rel(fast, dense) <= 64 * EPS_LD, (coll, w_nu, _rel(fast, dense))


def test_closure_history_is_rho_ux_uy_in_long_double():
    """sum_k cx cy feq_k = rho ux uy (the fast forms' closure history), in long double, lid and walls included."""
    o, f, rho, ux, uy = _off_equilibrium_cells()
    fe = equ(rho, ux, uy, o.t)
    q = -fe[8] + (fe[7] + (-fe[6] + fe[5]))
    assert all(int(CX[k]) * int(CY[k]) in (0, 1, -1) for k in range(9))
    assert float(np.abs(q - history_fast(rho, ux, uy)).max()) <= 16 * EPS_LD * float(np.abs(fe).max())
