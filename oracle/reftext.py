"""The reference's own CUDA kernel text as a host library.  TEST INFRASTRUCTURE ONLY.

MRT_GPU.py keeps its hot path in four string literals: `funRT` for SRT, TRT and MRT, and `funBC`.  This module reads the script
AS TEXT (it is never imported or executed), cuts those literals out, substitutes the constants with the script's own `%`
formatting, and compiles the result as host C++ between reftext_shim.hpp and reftext_driver.inc, without multiply-add contraction.
That library is what `arith="promoted"` and the oracles with promote=True claim to reproduce; tests/test_mrt_gpu_text_*.py
compare them with it bit for bit.

Everything generated goes to oracle/_ref/ (git-ignored): no committed file holds any of the extracted text; the regular
expressions below are all that names it.  Constants are baked into the text, so there is one library per (operator, turb, Re, ny).
Without the reference directory build_all() does nothing; the committed digests (tests/golden/mrt_gpu_text.json) still hold.
"""
import ctypes
import os
import re
import subprocess
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "_ref")
SHIM, DRIVER = "reftext_shim.hpp", "reftext_driver.inc"
CXX = os.environ.get("CXX", "g++")
FLAGS = ["-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"]
ULB = 0.08                                   # MRT_GPU.py:58
ORDERS = (0, 1, 1982)                        # ascending, descending, a seeded shuffle of (block, thread)
CHECKPOINTS = (1, 2, 7, 20, 37)

OPS = [("SRT", 0), ("SRT", 1), ("TRT", 0), ("TRT", 1), ("MRT", 0), ("MRT", 1)]
# (nx, ny, Re): each side is <= 32 or a multiple of 32 (the text derives xsize from blockDim*gridDim); 160 x 160 at Re 10000 is
# the script's default.  The second row holds the shapes the device routes need (tests/test_mrt_gpu_text_gpu.py): tile kernels,
# the streaming kernel with a partial second strip (288 x 160) and with several row segments (128 x 320).
SHAPES = [(16, 16, 100.0), (32, 32, 1000.0), (64, 32, 10000.0), (16, 96, 100.0), (96, 64, 1000.0), (160, 160, 10000.0),
          (64, 64, 1000.0), (96, 128, 100.0), (288, 160, 10000.0), (128, 320, 1000.0)]
BATCH_RE = (100.0, 1000.0, 10000.0)          # the batch test: SRT + closure, 96 x 64, one lattice per Reynolds number


class Case(namedtuple("Case", "coll turb Re nx ny")):
    @property
    def id(self):
        return "%s-t%d-Re%g-%dx%d" % self

    @property
    def lib(self):
        return "reftext_%s_t%d_Re%g_ny%d" % (self.coll, self.turb, self.Re, self.ny)


def case(coll, turb, Re, nx, ny):
    return Case(coll, int(turb), float(Re), int(nx), int(ny))


CASES = [case(c, t, Re, nx, ny) for nx, ny, Re in SHAPES for c, t in OPS]
CASES += [case("SRT", 1, Re, 96, 64) for Re in BATCH_RE if Re != 1000.0]
assert len({c.id for c in CASES}) == len(CASES)


def reference_dir():
    """LBM_REFERENCE_DIR, else the directory tests/golden/make_golden.py reads."""
    env = os.environ.get("LBM_REFERENCE_DIR")
    if env:
        return env
    text = open(os.path.join(os.path.dirname(_HERE), "tests", "golden", "make_golden.py")).read()
    return re.search(r'^REF = "([^"]+)"', text, re.M).group(1)


def valid_shape(nx, ny):
    return all(n >= 1 and (n <= 32 or n % 32 == 0) for n in (nx, ny))


def extract(script):
    """The kernel literals of a script, in file order: ([SRT, TRT, MRT], BC)."""
    text = open(script).read()
    rt = re.findall(r'funRT\s*=\s*"""(.*?)"""', text, re.S)
    bc = re.findall(r'funBC\s*=\s*"""(.*?)"""', text, re.S)
    if len(rt) != 3 or len(bc) != 1:
        raise RuntimeError("%s: expected three funRT literals and one funBC, found %d and %d" % (script, len(rt), len(bc)))
    return rt, bc[0]


def _unindented(text):
    return "\n".join(line.strip() for line in text.splitlines())


def datagen_comparison(ref=None):
    """MRT_GPU_datagen.py carries the same four literals: "identical" when they equal MRT_GPU.py's after stripping leading (and
    trailing) blanks of every line, else the names of those that differ."""
    ref = ref or reference_dir()
    a, abc = extract(os.path.join(ref, "MRT_GPU.py"))
    b, bbc = extract(os.path.join(ref, "MRT_GPU_datagen.py"))
    diff = [n for n, x, y in zip(("SRT", "TRT", "MRT", "BC"), a + [abc], b + [bbc]) if _unindented(x) != _unindented(y)]
    return "identical" if not diff else "differ: " + ",".join(diff)


def substituted(c, literals):
    """The kernel of a case with the script's own substitution (MRT_GPU.py:422,531,662): Python's %s of the same doubles."""
    from .lbm_numpy import relaxation
    r = relaxation(c.Re, c.ny, ULB, 1.2, 1.2)                 # MRT_GPU.py:63-90, ysize = ny
    args = {"SRT": (ULB, r["omega"], c.turb),
            "TRT": (ULB, r["omega"], r["omegam"], c.turb),
            "MRT": (ULB, r["omega"], 1.0, 1.2, 1.2, c.turb)}[c.coll]
    return literals[("SRT", "TRT", "MRT").index(c.coll)] % args


def _source(c, rt, bc):
    return ('// generated by oracle/reftext.py from the reference; never committed\n#include "%s"\n%s\n%s\n#include "%s"\n'
            % (SHIM, substituted(c, rt), bc, DRIVER))


def _compile(src, so, extra=()):
    cmd = [CXX] + FLAGS + list(extra) + ["-I", _HERE, src, "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "narrowing" in r.stderr:       # the brace initialisers of the MRT matrices
        r = subprocess.run(cmd[:1] + ["-Wno-narrowing"] + cmd[1:], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))


def build_case(c, rt, bc, out=OUT, extra=(), force=False):
    """One library; up to date when the generated source is unchanged and the library is newer than it, the shim and the driver."""
    os.makedirs(out, exist_ok=True)
    src, so = os.path.join(out, c.lib + ".cpp"), os.path.join(out, c.lib + ".so")
    text = _source(c, rt, bc)
    if not force and os.path.exists(src) and os.path.exists(so) and open(src).read() == text:
        if os.path.getmtime(so) >= max(os.path.getmtime(p) for p in (src, os.path.join(_HERE, SHIM), os.path.join(_HERE, DRIVER))):
            return so, False
    with open(src, "w") as f:
        f.write(text)
    _compile(src, so, extra)
    return so, True


def build_all(cases=None, out=OUT, extra=(), force=False, verbose=False):
    """Build the library of every case (default: the case table) into oracle/_ref/.  Returns the number compiled, or None when
    the reference is absent (then nothing is done; libraries that travelled with the tree stay as they are)."""
    ref = reference_dir()
    script = os.path.join(ref, "MRT_GPU.py")
    if not os.path.exists(script):
        if verbose:
            print("reftext: no reference at %s; nothing built" % ref)
        return None
    rt, bc = extract(script)
    todo = list({c.lib: c for c in (CASES if cases is None else cases)}.values())
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        built = sum(b for _, b in pool.map(lambda c: build_case(c, rt, bc, out, extra, force), todo))
    if verbose:
        print("reftext: %d libraries in %s (%d compiled); datagen literals: %s" % (len(todo), out, built, datagen_comparison(ref)))
    return built


def available(cases=None, out=OUT):
    return all(os.path.exists(os.path.join(out, c.lib + ".so")) for c in (CASES if cases is None else cases))


class RefTextCavity:
    """The compiled text behind the oracles' interface: fin[9, X, Y], u[2, X, Y], rho, feq, taus in the project's layout.

    Starts as MRT_GPU.py:309-328 does: fin from the host's equilibrium (here: the oracle's promoted initial state -- the host-side
    initialisation is not part of the text), ftemp = feq = fin, rho = 1, u = 0; taus = 0."""

    def __init__(self, nx, ny, Re, collision="SRT", turb=0, order=0, out=OUT):
        from .lbm_ref import CavityOracleC
        if not valid_shape(nx, ny):
            raise ValueError("the kernel text is defined only where each side is <= 32 or a multiple of 32: %d x %d" % (nx, ny))
        self.case = case(collision, turb, Re, nx, ny)
        self.nx, self.ny, self.order = int(nx), int(ny), int(order)
        so = os.path.join(out, self.case.lib + ".so")
        if not os.path.exists(so):
            raise FileNotFoundError(so)
        self._step = ctypes.CDLL(so).step
        p = ctypes.POINTER(ctypes.c_float)
        self._step.restype = ctypes.c_int
        self._step.argtypes = [p] * 6 + [ctypes.c_int] * 4
        fin = CavityOracleC(nx, ny, Re, semantics="mrt_gpu", collision=collision, dtype=np.float32, turb=turb, promote=True).fin
        self._fin = np.ascontiguousarray(fin.transpose(0, 2, 1))       # the script's post-transpose layout: i = x + y*xsize
        self._ftemp, self._feq = self._fin.copy(), self._fin.copy()
        self._rho = np.ones((ny, nx), dtype=np.float32)
        self._u = np.zeros((2, ny, nx), dtype=np.float32)
        self._taus = np.zeros((ny, nx), dtype=np.float32)
        self.nsteps = 0

    def step(self, n=1):
        a = [x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for x in (self._fin, self._ftemp, self._feq, self._rho, self._u, self._taus)]
        if self._step(*a, self.nx, self.ny, int(n), self.order) != 0:
            raise RuntimeError("the library refused %d x %d" % (self.nx, self.ny))
        self.nsteps += n
        return self

    fin = property(lambda s: np.ascontiguousarray(s._fin.transpose(0, 2, 1)))
    feq = property(lambda s: np.ascontiguousarray(s._feq.transpose(0, 2, 1)))
    u = property(lambda s: np.ascontiguousarray(s._u.transpose(0, 2, 1)))
    rho = property(lambda s: np.ascontiguousarray(s._rho.T))
    taus = property(lambda s: np.ascontiguousarray(s._taus.T))


if __name__ == "__main__":
    build_all(verbose=True)
