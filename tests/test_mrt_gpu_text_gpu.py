"""arith='promoted' on the device against MRT_GPU.py's own kernel text: fin, u, rho (and get_tau with the closure) of
CavitySolver(dtype=float32, arith="promoted") have the committed digests of the compiled text (tests/golden/mrt_gpu_text.json,
tests/golden/make_mrt_gpu_text.py) for SRT / TRT / MRT with and without the closure on every kernel route, at the smallest shapes
that are valid for the text (each side <= 32 or a multiple of 32) and still reach the route.  Where the libraries under oracle/_ref
travelled with the tree the fields are compared with them directly as well, so a failure names the size of the difference and the
first differing cell.  Nothing here reads the reference."""
import functools

import numpy as np
import pytest

from oracle import reftext
from latticeboltzmannsimulations_amd import CavityBatch, CavitySolver
from latticeboltzmannsimulations_amd.solver import launch_plan
from mrt_gpu_text_ref import digest, first_difference, golden

pytestmark = pytest.mark.gpu

reftext.build_all()          # nothing without the reference (the GPU box): the libraries travel with the tree or are absent

OPS = reftext.OPS
COUNTS = (1, 7, 20, 37)
RE = {(nx, ny): Re for nx, ny, Re in reftext.SHAPES}
HAVE_TEXT = reftext.available()
GOLDEN = golden()["digests"]


@functools.lru_cache(maxsize=None)
def _text(c):
    """{n: fields} of the compiled text, computed once per case and shared (read-only) by the routes."""
    t = reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb)
    out = {}
    for n in COUNTS:
        t.step(n - t.nsteps)
        out[n] = dict(fin=t.fin, u=t.u, rho=t.rho, taus=t.taus)
        for a in out[n].values():
            a.flags.writeable = False
    return out


def _check(c, n, got):
    want = GOLDEN[c.id][str(n)]
    assert set(got) == set(want)
    if HAVE_TEXT:
        for name, a in got.items():
            b = _text(c)[n][name]
            assert a.dtype == b.dtype and a.shape == b.shape
            assert a.tobytes() == b.tobytes(), "%s after %d steps, %s: device vs text: %s" % (c.id, n, name, first_difference(a, b))
    for name, a in got.items():
        assert digest(a) == want[name], "%s after %d steps: digest of %s" % (c.id, n, name)


def _run(nx, ny, coll, turb, **kw):
    c = reftext.case(coll, turb, RE[nx, ny], nx, ny)
    with CavitySolver(nx, ny, c.Re, RT=coll, dtype=np.float32, turb=turb, arith="promoted", **kw) as s:
        for n in COUNTS:
            s.step(n - s.steps_done)
            u, rho, fin = s.get_fields(want_fin=True)
            got = dict(fin=fin, u=u, rho=rho)
            if turb:
                got["taus"] = s.get_tau()
            _check(c, n, got)
        return s.describe()


@pytest.mark.parametrize("coll,turb", OPS)
@pytest.mark.parametrize("nx,ny", [(32, 32), (64, 32)])
@pytest.mark.parametrize("kernel", ["generic", "vec"])
def test_single_step_kernels(kernel, nx, ny, coll, turb):
    _run(nx, ny, coll, turb, kernel=kernel)


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
@pytest.mark.parametrize("nx,ny", [(32, 32), (64, 32)])
def test_push_kernel(nx, ny, coll):
    _run(nx, ny, coll, 0, kernel="push")


@pytest.mark.parametrize("coll,turb", OPS)
@pytest.mark.parametrize("nx,ny", [(64, 64), (96, 128)])
@pytest.mark.parametrize("tb_steps", [2, 5])
def test_tile_kernels(tb_steps, nx, ny, coll, turb):
    d = _run(nx, ny, coll, turb, kernel="tb", tuning=dict(tb_steps=tb_steps))
    assert d["kernel"] == ("k_step2_deep" if tb_steps == 2 else "k_stepS_deep") and d["steps_per_launch"] == tb_steps


@pytest.mark.parametrize("coll,turb", OPS)
@pytest.mark.parametrize("nx,ny", [(64, 64), (288, 160), (128, 320)])
@pytest.mark.parametrize("mode", ["frame3", "frame8", "walls"])
def test_streaming_kernels(mode, nx, ny, coll, turb):
    # 288 x 160: a partial second strip; 128 x 320: several row segments; the checkpoints leave tail units and single steps
    tune = dict(stream_walls=True) if mode == "walls" else dict(stream_walls=False, tb_steps=3 if mode == "frame3" else 8)
    d = _run(nx, ny, coll, turb, kernel="stream", tuning=tune)
    assert d["kernel"] == ("k_stream_walls" if mode == "walls" else "k_stream")
    assert d["steps_per_launch"] == (3 if mode == "frame3" else 8)


@pytest.mark.parametrize("coll,turb", OPS)
def test_auto_route_at_the_scripts_default_shape(coll, turb):
    """160 x 160 at Re 10000: MRT_GPU.py's own defaults, on whatever the library chooses."""
    d = _run(160, 160, coll, turb)
    want = launch_plan(160, 160, RE[160, 160], RT=coll, turb=turb, arith="promoted")
    assert d["kernel"] == want["kernel"] and d["steps_per_launch"] == want["steps_per_launch"]


def test_batch_of_three_reynolds_numbers():
    """SRT + closure, 96 x 64: each lattice of a batch equals the text compiled for its own Reynolds number."""
    Re = list(reftext.BATCH_RE)
    with CavityBatch(96, 64, Re, RT="SRT", dtype=np.float32, turb=1, arith="promoted") as b:
        for n in COUNTS:
            b.step(n - b.steps_done)
            u, rho, fin = b.get_fields(want_fin=True)
            tau = b.get_tau()
            for i, r in enumerate(Re):
                _check(reftext.case("SRT", 1, r, 96, 64), n, dict(fin=fin[i], u=u[i], rho=rho[i], taus=tau[i]))
