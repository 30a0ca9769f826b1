"""CPU tests of the launch planning (lbm_plan, the device-free dry run of lbm_create's plan and lbm_step's units) against the
fixture tests/golden/launch_plans.txt.gz, recorded by tests/golden/make_launch_plans.py.  Two classes of entries differ from the
fixture on purpose; every other plan and unit sequence must be the same."""
import ctypes
import os
import sys

import numpy as np

from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import launch_plan
from latticeboltzmannsimulations_amd.solver import _params, relaxation

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_launch_plans as gen  # noqa: E402


def _fields(text):
    return dict(kv.split("=", 1) for kv in text.split())


def _walls_slab_two_steps(text):
    """A slab planned with the walls inside and two steps per launch: its two-step units ran the frame passes on the second
    stream while the walls kernel wrote the same columns on the first.  Now planned with the frame variant (k_stream)."""
    f = _fields(text) if text.startswith("kernel=") else {}
    return f.get("kernel") == "k_stream_walls" and f.get("slab") == "1" and f.get("steps_per_launch") == "2"


def _frame_beside(text):
    """frame_beside: the segment length lbm_create sets from the CU count is now part of the plan, so the dry run reports it."""
    return text.startswith("kernel=") and _fields(text).get("frame_beside") == "1"


def test_launch_plans_equal_the_fixture():
    old = gen.read()
    cur = gen.entries()
    assert set(cur) == set(old)
    changed = {k for k, (p, _) in old.items() if _walls_slab_two_steps(p) or _frame_beside(p)}
    assert len([k for k in changed if _frame_beside(old[k][0])]) == 72
    assert len([k for k in changed if _walls_slab_two_steps(old[k][0])]) == 314
    grid = dict(gen.grid())
    for k in sorted(set(old) - changed):
        assert cur[k] == old[k], k
    for k in sorted(changed):
        (p_old, u_old), (p_new, u_new) = old[k], cur[k]
        assert u_new == u_old, k
        f_old, f_new = _fields(p_old), _fields(p_new)
        if _walls_slab_two_steps(p_old):
            # the plan of the same parameters with the walls kernel switched off
            nx, ny, y0, nyl, mn, dt, rt, sem, turb, arith, kernel, batch, layout, ncu, tuning = grid[k]
            off = gen.plan(nx, ny, y0, nyl, mn, dt, rt, sem, turb, arith, kernel, batch, layout, ncu, dict(tuning, stream_walls=False), 0)
            assert f_new["kernel"] == "k_stream" and p_new == off, k
        else:
            nx, ny, y0, nyl, mn, ncu = grid[k][:5] + (grid[k][13],)
            per = 2 * nx + 2 * ((mn or nyl) - 2 * int(f_old["frame"]))
            cu = ncu or 256
            assert int(f_new["frame_seg"]) == max(64, ((per + cu - 1) // cu + 7) // 8 * 8), k
            assert {n: v for n, v in f_new.items() if n != "frame_seg"} == {n: v for n, v in f_old.items() if n != "frame_seg"}, k


def test_two_step_slab_keeps_the_wall_frame():
    d = launch_plan(320, 600, 100.0, rows=(200, 200), kernel="stream", tuning=dict(tb_steps=2))
    assert d["kernel"] == "k_stream" and d["steps_per_launch"] == 2 and d["frame"] == 4
    assert launch_plan(320, 600, 100.0, rows=(200, 200), kernel="stream", tuning=dict(tb_steps=3))["kernel"] == "k_stream_walls"


def test_frame_beside_segment_in_the_dry_run():
    kw = dict(dtype=np.float64, RT="TRT", tuning=dict(frame_beside=True))
    assert launch_plan(8192, 8192, 1000.0, **kw)["frame_seg"] == 128
    assert launch_plan(8192, 8192, 1000.0, ncu=80, **kw)["frame_seg"] == 416


def test_long_calls_list_every_unit():
    d = launch_plan(4096, 4096, 1000.0, steps=20000)
    assert sum(d["units"]) == 20000 and d["units"][0] == 1
    d = launch_plan(64, 64, 1000.0, steps=20000, kernel="generic")
    assert d["units"] == [1] * 20000


def test_buffer_too_small_is_an_error():
    p = _params(4096, 4096, 0, 4096, np.float32, "MRT", "mrt_gpu", "auto", 0, 0, "auto", 1, "strict", None, None, 0.08,
                relaxation(1000.0, 4096, 0.08, 1.2, 1.2))
    big = ctypes.create_string_buffer(4096)
    n = L.lib().lbm_plan(ctypes.byref(p), 0, 37, big, len(big))
    assert n > 0 and len(big.value) == n
    for size in (n, 40, 1):
        buf = ctypes.create_string_buffer(size)
        assert L.lib().lbm_plan(ctypes.byref(p), 0, 37, buf, len(buf)) == -1   # LBM_ERR_INVALID
        assert buf.value.decode() == "error: buffer too small"[:size - 1]
    buf = ctypes.create_string_buffer(n + 1)
    assert L.lib().lbm_plan(ctypes.byref(p), 0, 37, buf, len(buf)) == n and buf.value == big.value
