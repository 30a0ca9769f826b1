"""CPU tests of the time statistics (lbm_stats_*): the C ABI is declared, bound and exported and refuses a null context, and
run_cavity's averaging bookkeeping -- when statistics begin, what is printed, which files are written, what the result
carries -- runs through a stand-in stepper that implements the statistics contract in NumPy.  With averaging off the driver's
stdout, calls and results are those of a run without the new arguments."""
import os
import re

import numpy as np
import pytest

from front_end_standin import standin
from latticeboltzmannsimulations_amd import _lib, ghia, mrt_gpu
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lbm_stats_begin", "lbm_stats_sample", "lbm_stats_get", "lbm_stats_end")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbm.h")).read(), flags=re.S)
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(L, n), n


def test_null_context_is_rejected():
    L = _lib.lib()
    assert L.lbm_stats_begin(None, 0) == -1
    assert L.lbm_stats_begin(None, 10) == -1
    assert L.lbm_stats_sample(None) == -1
    assert L.lbm_stats_get(None, None, None, None, None) == -1
    assert L.lbm_stats_end(None) == -1


StatsStepper = standin(source="synthetic")      # the fields after n steps are a fixed function of n (SyntheticFields)


def _mean_of(st, ns):
    u = np.zeros((2, st.nx, st.ny))
    for n in ns:
        u += st.o.fields(n)[0].astype(np.float64)
    return u / len(ns)


def test_averaging_schedule_lines_files_and_result(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    made = []

    def factory(*a, **kw):
        made.append(StatsStepper(*a, **kw))
        return made[-1]
    r = run_cavity(maxIt=451, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=True,
                   solver_factory=factory, AverageFrom=150, AverageEvery=40)
    st = made[0]
    # the enqueue that crosses iteration 150 is split there, statistics begin after exactly 150 steps
    assert StatsStepper.calls == [1, 100, 49, 51, 100, 100, 50] and StatsStepper.begins == [(150, 40)]
    assert st.sampled == [190, 230, 270, 310, 350, 390, 430]
    out = capsys.readouterr().out
    assert out.count("current regression value of the time-mean is ") == 3
    assert [it for it, _ in r.regression_mean] == [200, 300, 400]
    # the value at an output iteration is the regression of the mean over the samples taken up to it
    for (it, val), ns in zip(r.regression_mean, ([190], [190, 230, 270], [190, 230, 270, 310, 350, 390])):
        assert val == pytest.approx(float(ghia.r2_value(_mean_of(st, ns), 100.0, 0.08)), rel=1e-12, abs=1e-12)
    for i in range(5):
        assert os.path.exists(tmp_path / "output" / f"ldc.{i:05d}.vtr")
        assert os.path.exists(tmp_path / "output" / f"ldc_mean.{i:05d}.vtr") == (i >= 2)
    assert r.samples == 7 and r.iterations == 451
    ns = st.sampled
    U = np.stack([st.o.fields(n)[0].astype(np.float64) for n in ns])
    R = np.stack([st.o.fields(n)[1].astype(np.float64) for n in ns])
    assert np.allclose(r.u_mean, U.mean(0), rtol=0, atol=1e-15) and np.allclose(r.rho_mean, R.mean(0), rtol=0, atol=1e-15)
    assert np.allclose(r.uu, U[:, 0].var(0), rtol=1e-6, atol=1e-15)
    assert np.allclose(r.vv, U[:, 1].var(0), rtol=1e-6, atol=1e-15)
    assert np.allclose(r.uv, (U[:, 0] * U[:, 1]).mean(0) - U[:, 0].mean(0) * U[:, 1].mean(0), rtol=1e-6, atol=1e-15)
    assert r.u_mean.dtype == np.float64 and r.u_mean.shape == (2, 32, 32) and r.uu.shape == (32, 32)


def test_averaging_from_the_first_iteration_and_without_ghia_column(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=201, Re=250.0, RT="SRT", turb=0, xsize=16, ysize=16, Pinterval=100, SavePlot=False, SaveVTK=False,
                   solver_factory=StatsStepper, AverageFrom=0, AverageEvery=25, quiet=True)
    assert StatsStepper.begins == [(0, 25)] and StatsStepper.calls == [201]   # (no output files: one enqueue)
    assert r.samples == 8 and r.regression_mean == [] and r.regression == []   # (no Ghia column at Re 250)


def _normalised(out):
    return [ln for ln in out.splitlines() if "elapsed" not in ln]   # (wall-clock times differ from run to run)


def test_averaging_off_changes_nothing(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    kw = dict(maxIt=251, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=False, SaveVTK=True,
              solver_factory=StatsStepper)
    a = run_cavity(**kw)
    calls_a, out_a = list(StatsStepper.calls), capsys.readouterr().out
    b = run_cavity(AverageFrom=None, AverageEvery=7, **kw)
    calls_b, out_b = list(StatsStepper.calls), capsys.readouterr().out
    assert calls_a == calls_b == [1, 100, 100, 50] and StatsStepper.begins == []
    assert _normalised(out_a) == _normalised(out_b) and "time-mean" not in out_b
    assert not any("_mean" in f for f in os.listdir(tmp_path / "output"))
    assert a.regression == b.regression and np.array_equal(a.u, b.u)
    assert b.u_mean is None and b.rho_mean is None and b.uu is None and b.samples == 0 and b.regression_mean == []


def test_averaging_arguments_are_checked_and_reach_the_cli(monkeypatch):
    with pytest.raises(ValueError):
        run_cavity(maxIt=1, AverageFrom=-1, solver_factory=StatsStepper, quiet=True)
    with pytest.raises(ValueError):
        run_cavity(maxIt=1, AverageFrom=0, AverageEvery=0, solver_factory=StatsStepper, quiet=True)
    seen = {}

    class R:
        mlups = 0.0
    monkeypatch.setattr(mrt_gpu, "run_cavity", lambda **kw: (seen.update(kw), R())[1])
    mrt_gpu.main(["--average-from", "5000", "--average-every", "50", "--no-plot"])
    assert seen["AverageFrom"] == 5000 and seen["AverageEvery"] == 50
    mrt_gpu.main(["--no-plot"])
    assert seen["AverageFrom"] is None and seen["AverageEvery"] == 100
