"""The shared comparators, states and case grid (tests/checks.py, tests/cases.py) themselves, on stand-ins: a comparator that wrongly
passes would weaken every test that relies on it."""
import numpy as np
import pytest

from cases import route_cases, route_id, route_valid
from checks import nan_equal, perturbed, reordered_sum_bound, rest, same_as_oracle, same_bits, same_fields


class _Solver:
    """What same_as_oracle and same_fields ask of a solver: get_fields(want_fin=True) -> (u [2, 5, 4], rho [5, 4], fin [9, 5, 4])."""

    def __init__(self, u, rho, fin):
        self.fields = (u, rho, fin)

    def get_fields(self, want_fin=False):
        assert want_fin
        return tuple(a.copy() for a in self.fields)


class _Oracle:
    def __init__(self, u, rho, fin):
        self.u, self.rho, self.fin = u.copy(), rho.copy(), fin.copy()


def _fields(dtype=np.float32):
    rng = np.random.default_rng(3)
    return rng.random((2, 5, 4)).astype(dtype), (1.0 + rng.random((5, 4))).astype(dtype), rng.random((9, 5, 4)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_same_as_oracle_sees_one_ulp_in_every_field(dtype):
    u, rho, fin = _fields(dtype)
    got = same_as_oracle(_Solver(u, rho, fin), _Oracle(u, rho, fin), "equal")
    assert all(np.array_equal(a, b) for a, b in zip(got, (u, rho, fin)))
    for i, at in enumerate(((1, 4, 3), (0, 2), (8, 0, 1))):
        off = [a.copy() for a in (u, rho, fin)]
        off[i][at] = np.nextafter(off[i][at], dtype(2.0))
        assert off[i][at] != (u, rho, fin)[i][at]
        with pytest.raises(AssertionError, match=("u", "rho", "fin")[i] + " differs"):
            same_as_oracle(_Solver(*off), _Oracle(u, rho, fin), "one ulp")
        with pytest.raises(AssertionError, match=("u", "rho", "fin")[i] + " differs"):
            same_fields(_Solver(*off), _Solver(u, rho, fin), "one ulp")
        with pytest.raises(AssertionError, match=("u", "rho", "fin")[i] + " differs"):
            same_fields(tuple(off), (u, rho, fin), "one ulp, tuples")
    same_fields(_Solver(u, rho, fin), _Solver(u, rho, fin), "equal")
    same_fields((u, rho, fin), (u, rho, fin), "equal, tuples")


def test_same_as_oracle_refuses_equal_fields_that_are_not_finite():
    for i, at in enumerate(((0, 0, 0), (4, 3), (5, 2, 2))):
        for bad in (np.inf, np.nan):
            f = [a.copy() for a in _fields()]
            f[i][at] = bad
            with pytest.raises(AssertionError, match="not finite"):
                same_as_oracle(_Solver(*f), _Oracle(*f), "not finite")
            with pytest.raises(AssertionError, match="not finite"):
                same_fields(_Solver(*f), _Solver(*f), "not finite")
    f = [a.copy() for a in _fields()]
    f[2][5, 2, 2] = np.inf
    same_as_oracle(_Solver(*f), _Oracle(*f), "the same inf", finite=False)
    g = [a.copy() for a in f]
    g[2][5, 2, 2] = -np.inf
    with pytest.raises(AssertionError, match="fin differs"):
        same_as_oracle(_Solver(*g), _Oracle(*f), "another inf", finite=False)


def test_same_bits_takes_nan_for_nan_and_names_the_key_that_differs():
    a = dict(step=7, sum_ux=0.25, probe=np.array([[1.0, np.nan, 3.0]]), spare=1)
    b = dict(step=7, sum_ux=0.25, probe=np.array([[1.0, np.nan, 3.0]]), spare=2)
    same_bits(a, b, ("step", "sum_ux", "probe"), "equal")
    with pytest.raises(AssertionError, match="spare differs"):
        same_bits(a, b, ("step", "spare"), "a key outside the first set")
    b["probe"] = np.array([[1.0, 2.0, 3.0]])
    with pytest.raises(AssertionError, match="probe differs"):
        same_bits(a, b, ("step", "sum_ux", "probe"), "NaN against a number")
    b["probe"], b["sum_ux"] = a["probe"], np.nextafter(0.25, 1.0)
    with pytest.raises(AssertionError, match="sum_ux differs"):
        same_bits(a, b, ("step", "sum_ux", "probe"), "one ulp")


def test_reordered_sum_bound_is_two_gamma_n_over_the_finite_terms():
    g3 = 3 * 2.0 ** -53 / (1.0 - 3 * 2.0 ** -53)
    assert reordered_sum_bound([1.5, np.nan, -2.25, 0.125]) == 2.0 * g3 * 3.875
    assert reordered_sum_bound(np.array([[1.5, -2.25], [0.125, np.inf]])) == 2.0 * g3 * 3.875
    assert reordered_sum_bound([]) == 0.0 and reordered_sum_bound([np.nan]) == 0.0
    x = np.random.default_rng(1).standard_normal(1000)
    assert abs(float(np.sum(x)) - float(np.sum(x[::-1]))) <= reordered_sum_bound(x) < 1e-9


def test_nan_equal():
    nan = float("nan")
    assert nan_equal(1.5, 1.5) and nan_equal(nan, np.float32("nan"))
    assert not nan_equal(1.5, 2.5) and not nan_equal(nan, 1.5) and not nan_equal(1.5, nan)
    assert nan_equal(np.inf, np.inf) and not nan_equal(np.inf, -np.inf) and nan_equal(-1, -1)


def test_states():
    for dtype in (np.float32, np.float64):
        a, b = perturbed(7, 5, dtype, 11), perturbed(7, 5, dtype, 11)
        assert a.dtype == dtype and a.shape == (9, 7, 5) and a.tobytes() == b.tobytes()
        assert a.tobytes() != perturbed(7, 5, dtype, 12).tobytes()
        assert 0.0 < np.abs(a.sum(axis=0) - 1.0).max() < 0.2
        r = rest(7, 5, dtype)
        assert r.dtype == dtype and r.shape == (9, 7, 5) and r.flags["C_CONTIGUOUS"] and r.flags["WRITEABLE"]
        assert np.abs(r.astype(np.float64).sum(axis=0) - 1.0).max() <= 4 * np.finfo(dtype).eps
        assert (r == r[:, :1, :1]).all() and r[0, 0, 0] == dtype(4 / 9) and r[8, 6, 4] == dtype(1 / 36)
    assert np.array_equal(perturbed(7, 5, np.float32, 11), perturbed(7, 5, np.float64, 11).astype(np.float32))


def test_route_cases():
    ariths = ["strict", "fast", "promoted"]
    extras = [("generic", np.float64, "MRT", 1, "mrt_gpu", "strict"), ("generic", np.float32, "SRT", 0, "mrt_gpu", "strict")]
    first = route_cases(["generic"], ariths, (97, 80))
    assert first and all(route_valid(c, (97, 80)) for c in first)
    assert {c[5] for c in first} == {a for a in ariths if any(route_valid(("generic", d, "MRT", 0, "mrt_gpu", a), (97, 80))
                                                               for d in (np.float32, np.float64))}
    assert len({(c[0], c[4], c[5]) for c in first}) == len(first), "one case per (route, semantics, arithmetic)"
    assert ("generic", np.float32, "SRT", 0, "mrt_gpu", "strict") in first, "the first of the product"
    for size in ((97, 80), {"generic": (97, 80)}):
        cases = route_cases(["generic"], ariths, size, seed=5, sample=4, extras=extras)
        assert cases[:len(first)] == first and len(cases) in (len(first) + 4, len(first) + 5)
        assert all(cases.count(c) == 1 for c in cases + extras), "every case once; an extra that is already there is not repeated"
        assert all(route_valid(c, size) for c in cases)
        assert cases == route_cases(["generic"], ariths, size, seed=5, sample=4, extras=extras)
        assert len({route_id(c) for c in cases}) == len(cases)
    assert cases != route_cases(["generic"], ariths, (97, 80), seed=6, sample=4, extras=extras)
    one = route_cases(["generic"], ["strict"], (97, 80), seed=1, sample=10 ** 6)
    assert len(set(one)) == len(one) and {c[4] for c in one} == {"mrt_gpu", "mrt_py", "bounce_back"}, "a sample larger than the rest takes all"
    assert route_id(("tb", np.float64, "MRT", 1, "mrt_py", "fast")) == "tb-float64-MRT-t1-mrt_py-fast"
