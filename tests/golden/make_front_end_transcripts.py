#!/usr/bin/env python3
"""Generate tests/golden/front_end_transcripts.json: what mrt_gpu.run_cavity does, in order, when several of its modes run together.

Each case of CASES is one run at 32 x 32, Re 100, Pinterval 100, maxIt 451 with the stand-in solver of tests/front_end_standin.py.  Its
transcript holds the order and the control flow, which no single-mode test pins:

* ``journal`` -- the stand-in's ordered call log;
* ``lines``   -- the printed lines without the wall-clock ones; a token that reads as a number and is not an integer literal (one
  with '.', an exponent, nan or inf) is replaced by '#': the values are pinned mode by mode by the tests of each mode;
* ``files``   -- the names of the files written;
* ``result``  -- the integer side of the CavityResult: iterations, converged, diverged, samples and the iteration column of
  regression, regression_mean, vortices, vortex_tables and residuals.

tests/test_front_end_modes_cpu.py compares run_cavity with this file; the script is run by hand when the front end's behaviour is
meant to change.  It needs no GPU and no reference."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from front_end_standin import standin  # noqa: E402
from latticeboltzmannsimulations_amd import residual  # noqa: E402
from latticeboltzmannsimulations_amd.mrt_gpu import run_cavity  # noqa: E402

PATH = os.path.join(HERE, "front_end_transcripts.json")
BASE = dict(maxIt=451, Re=100.0, RT="MRT", turb=0, xsize=32, ysize=32, Pinterval=100, SavePlot=False)
AVERAGE = dict(AverageFrom=150, AverageEvery=40)
ALL = dict(monitor="device", MonitorEvery=10, criterion="residual", vortex_table=True, **AVERAGE)
CASES = {"device+vtk": dict(monitor="device", SaveVTK=True),
         "device+table": dict(monitor="device", vortex_table=True),
         "device+average+vtk": dict(monitor="device", SaveVTK=True, **AVERAGE),
         "device+residual2": dict(monitor="device", criterion="residual", residual_hits=2),
         "host+table+residual": dict(vortex_table=True, criterion="residual"),
         "all": ALL,
         "all+blow-up": dict(ALL, blow_up_at=150)}
SINGLE = {"device": dict(monitor="device"), "table": dict(vortex_table=True), "average": dict(SaveVTK=True, **AVERAGE),
          "residual": dict(criterion="residual", residual_tol=1e-30)}       # (never below: the whole sequence of records)


def residual_values(r, uLB=0.08):
    return [residual.norms(rec, uLB)["rel_l2_per_step"] for _, rec in r.residuals]


def mask(line):
    out = []
    for tok in line.split(" "):
        core = tok.strip("()[],;:")
        try:
            float(core)
            out.append(tok if core.lstrip("+-").isdigit() else tok.replace(core, "#"))
        except ValueError:
            out.append(tok)
    return " ".join(out)


def run(kw, tol=None):
    """(CavityResult, transcript) of run_cavity(**BASE, **kw) in a directory of its own; tol: the residual_tol of a case that has none."""
    kw = dict(kw)
    cls = standin(blow_up_at=kw.pop("blow_up_at", None))
    if kw.get("criterion") == "residual":
        kw.setdefault("residual_tol", tol)
    out, cwd = io.StringIO(), os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(out):
                r = run_cavity(solver_factory=cls, **BASE, **kw)
            files = sorted(os.listdir("output")) if os.path.isdir("output") else []
        finally:
            os.chdir(cwd)
    column = lambda rows: [int(row[0]) for row in rows]       # noqa: E731
    result = dict(iterations=int(r.iterations), converged=bool(r.converged), diverged=bool(r.diverged), samples=int(r.samples),
                  **{k: column(getattr(r, k)) for k in ("regression", "regression_mean", "vortices", "vortex_tables", "residuals")})
    lines = [mask(ln) for ln in out.getvalue().splitlines() if "elapsed" not in ln]
    return r, json.loads(json.dumps(dict(journal=cls.journal, lines=lines, files=files, result=result)))


def tolerance(free):
    """The residual tolerance of the cases: the geometric mean of the free run's values at iterations 200 and 300, so the first check
    below it is the one at iteration 300."""
    v = residual_values(free)
    return float(np.sqrt(v[1] * v[2]))


if __name__ == "__main__":
    tol = tolerance(run(SINGLE["residual"])[0])
    with open(PATH, "w") as f:
        json.dump({name: run(kw, tol)[1] for name, kw in CASES.items()}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(PATH, os.path.getsize(PATH), "bytes")
