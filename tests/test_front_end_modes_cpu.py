"""CPU tests of what the two front ends share and of their modes run together, with the stand-ins of tests/front_end_standin.py: the
mean-u stop rule of run_cavity against the reference's expression evaluated by hand, datagen's per-lattice loop under both stop rules
against each lattice run alone, and the order of calls, prints and files of run_cavity when several modes are on at once
(tests/golden/front_end_transcripts.json)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_front_end_transcripts as FT  # noqa: E402
from front_end_standin import BatchStandIn, standin  # noqa: E402
from latticeboltzmannsimulations_amd.datagen import generate  # noqa: E402
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity  # noqa: E402


# -- the mean-u rule of run_cavity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_run_cavity_stops_at_the_sixth_hit_of_the_reference_expression(form, tmp_path, monkeypatch):
    """MRT_GPU.py:883-889 as run_cavity evaluates it: a check after iteration 0, 400, 800, ...; the host form on NumPy's float32 means of
    the downloaded u, from u_past = 0, the device form on mean_u(), from 0.0; a hit counts whether or not it is consecutive, the sixth
    one ends the run.  Both sides compute the same floats in one process: the stop iteration is equal, not close."""
    monkeypatch.chdir(tmp_path)
    uLB, P = 0.08, 400
    s = standin()(16, 16, 100.0, RT="MRT", uLB=uLB, dtype=np.float64, turb=0)
    hits, It = 0, 0
    u_past, mean_past = np.zeros((2, 16, 16), dtype=np.float32), 0.0
    while hits < 6:
        s.step(It + 1 - s.steps_done)
        if form == "host":
            u = s.get_fields(out_dtype=np.float32)[0]
            hits += bool(abs(np.mean(u) - np.mean(u_past)) / uLB < 1e-8)
            u_past = u
        else:
            m = s.mean_u()
            hits += bool(abs(m - mean_past) / uLB < 1e-8)
            mean_past = m
        It += P
    want = s.steps_done
    assert P * 6 < want < 10 ** 6                                  # (not the first six checks: the rule waited for the flow)
    r = run_cavity(maxIt=10 ** 7, Re=100.0, RT="MRT", turb=0, xsize=16, ysize=16, uLB=uLB, Pinterval=P, SavePlot=False, SaveVTK=True,
                   dtype=np.float64, solver_factory=standin(), convergence=form, quiet=True)
    assert r.converged and r.iterations == want


# -- datagen's loop ----------------------------------------------------------------------------------------------------------------
SWEEP = dict(xsize=24, ysize=24, Pinterval=100, save=False, quiet=True)


def test_datagen_records_each_lattice_where_the_mean_u_rule_stops_it_alone():
    """The loop of tests/test_gpu_parity.py::test_reynolds_sweep_datagen (MRT_GPU_datagen.py:862-871), run on one oracle alone, against
    generate() on a batch of four and one: the iteration, the populations and the velocity of every lattice, host and device form."""
    from oracle.lbm_ref import CavityOracleC
    Re, maxIt, tol = np.array([100, 150, 400, 1000, 2500]), 3000, 2e-3
    means = dict(host=lambda o: float(np.mean(o.u)),                               # NumPy's float32 mean of the downloaded field
                 device=lambda o: float(np.mean(o.u.astype(np.float64))))          # lbm_mean_u: accumulated in double
    for form in ("host", "device"):
        its, f, u = [], [], []
        for re in Re:
            o = CavityOracleC(24, 24, float(re), semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1)
            count, past, It = 0, 0.0, 0
            while True:
                o.step(It + 1 - o.nsteps)
                m = means[form](o)
                count += abs(m - past) / 0.08 < tol
                past = m
                if count > 5:
                    break
                if It + 100 > maxIt - 1:
                    o.step(maxIt - o.nsteps)
                    break
                It += 100
            its.append(o.nsteps)
            f.append(o.fin.copy())
            u.append(o.u.copy())
        print("stop iterations alone,", form, "form:", its)
        assert len(set(its)) > 1 and min(its) < maxIt              # (the tolerance separates the lattices, and not by running out)
        _, f2, u2, _, its2 = generate(Re, maxIt=maxIt, tolerance=tol, concurrent=4, convergence=form, batch_factory=BatchStandIn, **SWEEP)
        assert np.array_equal(its2, its), form
        assert np.array_equal(f2, np.stack(f)) and np.array_equal(u2, np.stack(u)), form


def test_datagen_stops_each_lattice_where_the_residual_rule_stops_run_cavity():
    """criterion='residual': every lattice of a batch stops at the check run_cavity stops the lone stand-in at, with that run's last
    residual value, exactly."""
    from latticeboltzmannsimulations_amd import residual
    Re = np.array([100.0, 400.0, 1000.0])
    kw = dict(RT="SRT", turb=1, xsize=24, ysize=24, Pinterval=100, SavePlot=False, quiet=True, criterion="residual",
              solver_factory=standin())
    free = [FT.residual_values(run_cavity(maxIt=1201, Re=float(re), residual_tol=1e-30, **kw)) for re in Re]
    print("residuals alone:", free)
    # between the fourth and the fifth value of the middle lattice: the lattices cross it at different checks or not at all
    tol = float(np.sqrt(free[1][3] * free[1][4]))
    alone = [run_cavity(maxIt=1201, Re=float(re), residual_tol=tol, **kw) for re in Re]
    assert len({r.iterations for r in alone}) > 1 and alone[1].converged
    for v in free:
        assert all(abs(x - tol) > 0.01 * tol for x in v)            # (no stop sits on a rounding tie)
    out = generate(Re, maxIt=1201, concurrent=3, criterion="residual", residual_tol=tol, batch_factory=BatchStandIn, **SWEEP)
    _, f2, u2, _, its2, last = out
    for i, r in enumerate(alone):
        assert its2[i] == r.iterations, (i, its2[i], r.iterations)
        assert np.array_equal(u2[i], r.u)
        assert last[i] == residual.norms(r.residuals[-1][1], 0.08)["rel_l2_per_step"]


# -- run_cavity's modes together ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single():
    """The single-mode runs the combined ones are compared with, and the residual tolerance of the cases."""
    runs = {name: FT.run(kw)[0] for name, kw in FT.SINGLE.items()}
    v = FT.residual_values(runs["residual"])
    assert len(v) == 4 and all(a > b for a, b in zip(v, v[1:]))    # falling: one check is the first below the tolerance
    assert v[1] - v[2] > 0.01 * v[1]                               # (more than 1 % apart: no stop sits on a rounding tie)
    return runs, FT.tolerance(runs["residual"])


@pytest.fixture(scope="module")
def recorded():
    with open(FT.PATH) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(FT.CASES)


@pytest.mark.parametrize("case", list(FT.CASES))
def test_modes_together_follow_the_recorded_transcript(case, single, recorded):
    runs, tol = single
    r, got = FT.run(FT.CASES[case], tol)
    want = recorded[case]
    for part in ("result", "files", "journal", "lines"):
        assert got[part] == want[part], part
    # the numbers of a combined run are those of the single-mode runs at the same iterations
    at = lambda rows: {row[0]: row[1:] for row in rows}             # noqa: E731
    assert r.regression and all(at(runs["device"].regression)[it] == v for it, v in at(r.regression).items())
    assert all(at(runs["device"].vortices)[it] == v for it, v in at(r.vortices).items())
    assert all(at(runs["table"].vortex_tables)[it] == v for it, v in at(r.vortex_tables).items())
    assert all(at(runs["average"].regression_mean)[it] == v for it, v in at(r.regression_mean).items())
    assert all(at(runs["residual"].residuals)[it] == v for it, v in at(r.residuals).items())
    kw = FT.CASES[case]
    assert len(r.vortices) == (len(r.regression) if kw.get("monitor") == "device" else 0)
    assert len(r.vortex_tables) == (len(r.regression) if kw.get("vortex_table") else 0)
    assert bool(r.residuals) == (kw.get("criterion") == "residual")
    assert bool(r.regression_mean) == ("AverageFrom" in kw and not r.diverged)


def test_the_solver_is_closed_on_every_exit_path(tmp_path, monkeypatch):
    """An exception inside a check, and the refusal of a solver without a residual sampler, leave no open context behind."""
    monkeypatch.chdir(tmp_path)

    class Failing(standin()):
        def lines(self, **kw):
            raise RuntimeError("lost the device")
    with pytest.raises(RuntimeError, match="lost the device"):
        run_cavity(solver_factory=Failing, monitor="device", quiet=True, **FT.BASE)
    assert Failing.journal[-1] == ("close",) and Failing.journal.count(("close",)) == 1
    plain = standin(without=("residual",))
    with pytest.raises(TypeError, match="sample_residual"):
        run_cavity(solver_factory=plain, criterion="residual", residual_tol=1e-6, quiet=True, **FT.BASE)
    assert plain.journal == [("close",)]
    done = standin()
    run_cavity(solver_factory=done, quiet=True, **FT.BASE)
    assert done.journal[-1] == ("close",) and done.journal.count(("close",)) == 1
