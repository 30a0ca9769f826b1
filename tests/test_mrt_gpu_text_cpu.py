"""The promoted oracles against MRT_GPU.py's own kernel text (oracle/reftext.py: the four CUDA literals of the script, cut out as
text and compiled as host C++ without multiply-add contraction into oracle/_ref/).  This is the one checker here that the
project's authors did not write: CavityOracleC(promote=True) and the NumPy oracle with promotion must equal it bit for bit on
fin, u, rho (feq and taus with the closure) for SRT / TRT / MRT, with and without the closure, at every checkpoint of every case
of oracle.reftext.CASES.

Tests that need the libraries skip only when oracle/_ref/ does not hold them (no reference on that machine); the committed
digests (tests/golden/mrt_gpu_text.json) are asserted against the oracle everywhere."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import reftext
from oracle.lbm_numpy import CavityOracle
from oracle.lbm_ref import CavityOracleC
from mrt_gpu_text_ref import GOLDEN, digest, first_difference, golden, oracle_checkpoints

reftext.build_all()          # cheap when up to date; nothing without the reference

CASES = reftext.CASES
CHECKPOINTS = reftext.CHECKPOINTS
IDS = [c.id for c in CASES]
needs_text = pytest.mark.skipif(not reftext.available(), reason="oracle/_ref holds no libraries: no reference on this machine")


def _oracle(cls, c, promote=True):
    return cls(c.nx, c.ny, c.Re, semantics="mrt_gpu", collision=c.coll, dtype=np.float32, turb=c.turb, promote=promote)


def _text(c, order=0, out=reftext.OUT):
    return reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb, order=order, out=out)


def _compare(c, states, t, n):
    names = ("fin", "u", "rho") + (("feq", "taus") if c.turb else ())
    for name in names:
        got, want = states[name], getattr(t, name)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), "%s after %d steps, %s: oracle vs text: %s" % (c.id, n, name, first_difference(got, want))


@needs_text
@pytest.mark.parametrize("cls", [CavityOracleC, CavityOracle], ids=["c", "numpy"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_promoted_oracle_equals_the_text(c, cls):
    t = _text(c)
    for n, states in oracle_checkpoints(_oracle(cls, c), c, CHECKPOINTS):
        t.step(n - t.nsteps)
        _compare(c, states, t, n)
    if not c.turb:
        assert not t.taus.any()          # the text writes taus_g inside `if (turb==1)` only


@needs_text
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_thread_order_does_not_matter(c):
    """Ascending, descending and shuffled (block, thread) give the same bits in every array the kernels touch: the text is per-thread
    code, so the sequential run states the CUDA program.  A failure names the array, not an order that would be 'right'."""
    runs = [_text(c, order) for order in reftext.ORDERS]
    for n in CHECKPOINTS:
        for t in runs:
            t.step(n - t.nsteps)
        for name in ("_fin", "_ftemp", "_feq", "_rho", "_u", "_taus"):
            ref = getattr(runs[0], name)
            for t in runs[1:]:
                assert getattr(t, name).tobytes() == ref.tobytes(), "%s after %d steps: %s depends on the thread order" % (c.id, n, name[1:])


@needs_text
@pytest.mark.parametrize("c", [c for c in CASES if (c.coll, c.turb) in (("MRT", 0), ("SRT", 1))], ids=lambda c: c.id)
def test_strict_oracle_is_not_the_text(c):
    """The comparison can tell the two arithmetics apart: plain fp32 evaluation differs from the text after 37 steps (the pair of
    operators of test_promoted_is_not_strict)."""
    n = CHECKPOINTS[-1]
    assert not np.array_equal(_oracle(CavityOracleC, c, promote=False).step(n).fin, _text(c).step(n).fin)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_digests_equal_the_committed_ones(c):
    """(a) Runs everywhere: the C oracle reproduces what the text gave where the fixtures were generated."""
    want = golden()["digests"][c.id]
    assert sorted(want, key=int) == [str(n) for n in CHECKPOINTS]
    for n, states in oracle_checkpoints(_oracle(CavityOracleC, c), c, CHECKPOINTS):
        assert set(want[str(n)]) == {"fin", "u", "rho"} | ({"taus"} if c.turb else set())
        for name, d in want[str(n)].items():
            assert digest(states[name]) == d, (c.id, n, name)


def _generator():
    spec = importlib.util.spec_from_file_location("make_mrt_gpu_text", os.path.join(GOLDEN, "make_mrt_gpu_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GENERATOR = _generator()


@needs_text
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_regenerated_digests_equal_the_committed_ones(c):
    """(b) The committed digests are what the libraries under oracle/_ref give now."""
    want = golden()["digests"]
    assert list(want) == IDS
    got = {str(n): {k: digest(getattr(t, k)) for k in GENERATOR.fields(c)} for n, t in GENERATOR.text_checkpoints(c)}
    assert got == want[c.id]


@needs_text
def test_regenerated_settings_and_values_equal_the_committed_ones():
    """(b) for the rest of the fixtures: the flags, the checkpoints, the value fixture, and (where the reference itself is present)
    the outcome of the comparison with MRT_GPU_datagen.py's literals."""
    want = golden()
    assert want["compile_flags"] == reftext.FLAGS and "-ffp-contract=off" in reftext.FLAGS
    assert want["checkpoints"] == list(CHECKPOINTS)
    if os.path.exists(os.path.join(reftext.reference_dir(), "MRT_GPU_datagen.py")):
        assert reftext.datagen_comparison() == want["datagen_literals"] == "identical"
    (c, n), z = GENERATOR.VALUES, np.load(os.path.join(GOLDEN, "mrt_gpu_text_16x16.npz"))
    t = _text(c).step(n)
    for name in ("fin", "u", "rho", "taus"):
        assert z[name].tobytes() == getattr(t, name).tobytes(), name


def test_value_fixture_equals_both_oracles():
    """The recorded values (MRT + closure, 16 x 16, 20 steps), not only their digests: a difference shows where and by how much."""
    z = np.load(os.path.join(GOLDEN, "mrt_gpu_text_16x16.npz"))
    c = [c for c in CASES if c.id == str(z["case"])][0]
    n = int(z["steps"])
    assert (c.coll, c.turb, c.nx, c.ny, n) == ("MRT", 1, 16, 16, 20)
    for cls in (CavityOracleC, CavityOracle):
        (m, states), = oracle_checkpoints(_oracle(cls, c), c, (n,))
        for name in ("fin", "u", "rho", "taus"):
            assert states[name].tobytes() == z[name].tobytes(), "%s %s: %s" % (cls.__name__, name, first_difference(states[name], z[name]))
            assert digest(z[name]) == golden()["digests"][c.id][str(n)][name]


def test_case_table():
    """Six operators on every shape; the issue's shapes, Reynolds numbers and checkpoints are all there; every shape is one the
    text is defined on, and the wrapper refuses the others."""
    assert CHECKPOINTS == (1, 2, 7, 20, 37)
    for nx, ny in ((16, 16), (32, 32), (64, 32), (16, 96), (96, 64), (160, 160)):
        assert {(c.coll, c.turb) for c in CASES if (c.nx, c.ny) == (nx, ny)} == set(reftext.OPS)
    assert {c.Re for c in CASES} == {100.0, 1000.0, 10000.0}
    assert reftext.case("SRT", 1, 10000.0, 160, 160) in CASES            # the script's defaults
    assert all(reftext.valid_shape(c.nx, c.ny) for c in CASES)
    for nx, ny in ((48, 32), (32, 33), (100, 64), (0, 16)):
        assert not reftext.valid_shape(nx, ny)
        with pytest.raises(ValueError, match="multiple of 32"):
            reftext.RefTextCavity(nx, ny, 1000.0, "SRT", 0)


def test_build_all_without_the_reference_is_a_no_op(tmp_path, monkeypatch):
    monkeypatch.setenv("LBM_REFERENCE_DIR", str(tmp_path))
    assert reftext.build_all(out=str(tmp_path / "out")) is None
    assert not (tmp_path / "out").exists()


@needs_text
def test_text_under_address_and_ub_sanitizers(tmp_path):
    """The three operators + funBC with the closure, built with -fsanitize=address,undefined into a temporary directory, at 32 x 32
    and 64 x 32: the text's u_g[xsize/2 + xsize] read and its neighbour stores are where it could leave an array.  No report, and
    the same bits as the plain libraries.  (Host build only; following test_c_oracle_under_address_and_ub_sanitizers.)"""
    import shutil
    if shutil.which(reftext.CXX) is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(reftext.reference_dir(), "MRT_GPU.py")):
        pytest.skip("the sanitized libraries are built from the reference, which is not on this machine")
    asan = subprocess.run([reftext.CXX, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("libasan not installed")
    cases = [c for c in CASES if c.turb == 1 and (c.nx, c.ny) in ((32, 32), (64, 32))]
    assert len(cases) == 6
    out = str(tmp_path / "san")
    # -O0: the dead Van Driest read of u_g stays in the program, so AddressSanitizer sees it
    assert reftext.build_all(cases, out=out, extra=["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]) == 6
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import reftext
n = 0
for c in reftext.CASES:
    if c.turb == 1 and (c.nx, c.ny) in ((32, 32), (64, 32)):
        for order in reftext.ORDERS:
            a = reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb, order=order, out=%r).step(5)
            b = reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb).step(5)
            assert all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("_fin", "_ftemp", "_feq", "_rho", "_u", "_taus")), c.id
            n += 1
print("sanitized cases ok:", n)
""" % (ROOT, out)
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sanitized cases ok: 18" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
