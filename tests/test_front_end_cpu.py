"""CPU test of the drop-in front end's HOST logic (mrt_gpu.run_cavity: which iterations produce output, the
reference's metric and prints, PNG / VTK files, convergence stop) with a stand-in stepper backed by the oracle.
The product has no CPU stepper; the stand-in lives in tests/front_end_standin.py."""
import os

import numpy as np
import pytest

from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity
from front_end_standin import standin
from oracle.lbm_ref import CavityOracleC


OracleStepper = standin()


def test_output_iterations_batches_and_files(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=251, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=True, SaveVTK=True,
                   solver_factory=OracleStepper)
    # iteration 0 alone, then batches up to every multiple of Pinterval, then the remainder (no output after it)
    assert OracleStepper.calls == [1, 100, 100, 50]
    assert r.iterations == 251 and [it for it, _ in r.regression] == [0, 100, 200]
    for i in range(3):
        assert os.path.exists(tmp_path / "output" / f"ldc_{i:05d}.png")
        assert os.path.exists(tmp_path / "output" / f"ldc.{i:05d}.vtr")
    out = capsys.readouterr().out
    for line in ("the value of uLB is  0.08", "xsize value is  32", "RT chosen is  SRT", "Turbulence is on",
                 "current iteration : 200", "current regression value is ", "time elapsed is ", "TOTAL time elapsed is "):
        assert line in out
    assert "max iterations reached" not in out          # 250 is not an output iteration
    o = CavityOracleC(32, 32, 100.0, semantics="mrt_gpu", collision="SRT", dtype=np.float32, turb=1).step(251)
    assert np.array_equal(r.u, o.u) and r.u.dtype == np.float32


def test_convergence_stop(tmp_path, monkeypatch, capsys):
    """MRT_GPU.py:883-889: |mean(u) - mean(u_past)| / uLB < 1e-8 on more than five output iterations ends the run."""
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=10 ** 7, Re=100.0, RT="MRT", turb=0, xsize=16, ysize=16, Pinterval=400, SavePlot=False, SaveVTK=True,
                   dtype=np.float64, solver_factory=OracleStepper)
    assert r.converged and r.iterations < 10 ** 6
    assert "breaking out of loop because of convergence" in capsys.readouterr().out


def test_convergence_on_the_device_mean_stops_within_one_check_of_the_host_criterion(tmp_path, monkeypatch):
    """convergence='device': the same test on lbm_mean_u (reduced in double on the GPU) instead of NumPy's float32 mean of the
    downloaded field.  The two means differ in the last bits of a float, so the six hits may complete one check apart."""
    monkeypatch.chdir(tmp_path)
    kw = dict(maxIt=10 ** 7, Re=100.0, RT="MRT", turb=0, xsize=16, ysize=16, Pinterval=400, SavePlot=False, SaveVTK=True,
              dtype=np.float64, solver_factory=OracleStepper, quiet=True)
    host = run_cavity(**kw)
    dev = run_cavity(convergence="device", **kw)
    assert host.converged and dev.converged and OracleStepper.mean_calls >= 6
    assert abs(dev.iterations - host.iterations) <= 400
    with pytest.raises(ValueError):
        run_cavity(convergence="gpu", **kw)


def test_dashboard_carries_the_reference_legend_and_closure_lines(tmp_path, monkeypatch):
    """MRT_GPU.py:846-847 (two legend lines) and 862-866 (Smagorinsky constant, mean relaxation time from taus_g)."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot
    texts = []
    real = pyplot.figtext
    monkeypatch.setattr(pyplot, "figtext", lambda x, y, s, **kw: (texts.append((round(x, 2), round(y, 2), s)), real(x, y, s, **kw))[1])
    monkeypatch.chdir(tmp_path)
    run_cavity(maxIt=1, Re=100.0, RT="SRT", turb=1, xsize=32, ysize=32, Pinterval=100, SavePlot=True, SaveVTK=False,
               solver_factory=OracleStepper, quiet=True)
    assert (0.65, 0.45, "Square dots in above figure represent vortex locations from Ghia data") in texts
    assert (0.65, 0.43, "Circular dots represent vortex locations of current simulation") in texts
    assert any(t[:2] == (0.65, 0.17) and t[2].startswith("Smagorinsky constant, Cs = 0.1581 at wall to 0.16 at bulk") for t in texts)
    assert any(t[:2] == (0.65, 0.15) and t[2].startswith("Mean relaxation time, tau+tau_turbulent, is  ") for t in texts)
    texts.clear()
    run_cavity(maxIt=1, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=True, SaveVTK=False,
               solver_factory=OracleStepper, quiet=True)
    assert not any(t[1] in (0.17, 0.15) for t in texts)                    # closure off: no closure lines
    assert any(t[2].startswith("omega_nu, omega_e, omega_eps, omega_q") for t in texts)


def test_no_output_flags_means_one_batch(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=37, Re=400.0, RT="TRT", turb=0, xsize=16, ysize=16, Pinterval=10, SavePlot=False, SaveVTK=False,
                   quiet=True, solver_factory=OracleStepper)
    assert OracleStepper.calls == [37] and r.regression == [] and not os.path.exists(tmp_path / "output")


def test_unknown_reynolds_number_has_no_ghia_column(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = run_cavity(maxIt=11, Re=250.0, RT="SRT", turb=0, xsize=16, ysize=16, Pinterval=5, SavePlot=True, SaveVTK=False,
                   quiet=True, solver_factory=OracleStepper)
    assert r.regression == [] and r.iterations == 11
