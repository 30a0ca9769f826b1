"""What tests/test_mrt_gpu_text_cpu.py and tests/test_mrt_gpu_text_gpu.py share: the committed digests of MRT_GPU.py's compiled
kernel text (tests/golden/mrt_gpu_text.json, written by tests/golden/make_mrt_gpu_text.py), the digest itself, and the closure's
tau from an oracle's state.  The case table is oracle.reftext.CASES; nothing here reads the reference."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("fin", "u", "rho", "taus")


def digest(a):
    """SHA-256 of the little-endian C-contiguous float32 bytes of an array in the project's layout ([k, X, Y] / [X, Y])."""
    a = np.asarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").tobytes()).hexdigest()


def golden():
    with open(os.path.join(GOLDEN, "mrt_gpu_text.json")) as f:
        return json.load(f)


def promoted_tau(o, omega):
    """taus_g of MRT_GPU.py:385 from the state an iteration starts from, as tests/test_arith_promoted_gpu.py::test_get_tau computes
    it: float tau0*tau0 and |q|, the rest in double, one rounding."""
    f, fe = o.fin, o.feq
    q = (-f[8] + (f[7] + (-f[6] + f[5]))) - (-fe[8] + (fe[7] + (-fe[6] + fe[5])))       # float32 throughout
    tau0 = np.float32(1.0) / np.float32(omega)
    tt, aq = tau0 * tau0, np.abs(q)
    t = 0.5 * (np.float64(tau0) + np.sqrt(np.float64(tt) + ((18 * 1.4142) * np.float64(np.float32(0.025))) * aq.astype(np.float64)
                                          / o.rho.astype(np.float64)))
    return t.astype(np.float32)


def oracle_checkpoints(o, case, checkpoints):
    """Step an oracle (C or NumPy, promote or not) through the checkpoints; yields (n, {fin, u, rho, taus, feq}).  taus is what the
    text leaves in taus_g: the closure's tau of the LAST iteration (computed from the state that iteration started from) with
    turb = 1, and the initial zeros otherwise -- the text never writes it then."""
    taus = np.zeros((case.nx, case.ny), dtype=np.float32)
    for n in checkpoints:
        o.step(n - 1 - o.nsteps)
        if case.turb:
            taus = promoted_tau(o, o.relax["omega"])
        o.step(1)
        yield n, dict(fin=o.fin, u=o.u, rho=o.rho, taus=taus, feq=o.feq)


def first_difference(got, want):
    """'max |diff| ..., first differing cell ...' for a failure message (arrays of the same shape)."""
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if bad.size == 0:
        return "equal values (signed zeros differ)" if got.tobytes() != want.tobytes() else "equal"
    i = tuple(int(v) for v in bad[0])
    return "max |diff| %.3e in %d cells, first at %s: got %r, want %r" % (
        np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64))), len(bad), i, float(got[i]), float(want[i]))
