"""Record the dry-run launch plans (lbm_plan) of a fixed grid of parameters into tests/golden/launch_plans.txt.gz.

    python tests/golden/make_launch_plans.py            # writes the fixture from the library built in the tree
    python tests/golden/make_launch_plans.py --check    # compares instead (exit 1 and the differing keys on a mismatch)

The grid covers, on both sides of every threshold, what the launch planning branches on: lattice shapes around the tile and
streaming kernels' limits and the 512^2 / 768^2 / 1024^2 / 1, 2, 4, 8 Mi cell / 3072^2 marks, both dtypes, the three collision
operators, both semantics, the closure, both arithmetics, every kernel value, batches, first / middle / last slabs with and
without ny_local_min, tb_steps 0 and 2 .. 10, every flag alone, and step counts that reach every branch of the unit sequence.
Parameter errors are recorded with their messages.

Per entry: lbm_plan's text for steps = 0 (or the error text) and the units for each of STEPS (";"-separated comma lists), one
line per entry (see write(); `zcat` shows the text).  Keys name the parameters (see key())."""
import ctypes
import gzip
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from latticeboltzmannsimulations_amd import _lib as L  # noqa: E402
from latticeboltzmannsimulations_amd.solver import _params, relaxation  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_plans.txt.gz")
STEPS = tuple(range(1, 12)) + (20, 37)

# (nx, ny): the tile kernel's 32 / 64 limits and vector width, the 512^2 / 768^2 / 1024^2 frame-segment and crossover marks,
# 2048 / 4096 columns, the 1 / 2 / 4 / 8 Mi cell marks of the streaming kernel, 3072^2
SHAPES = [(28, 40), (32, 32), (34, 64), (36, 32), (64, 31), (60, 64), (64, 64), (64, 63), (96, 96), (160, 160), (512, 512),
          (512, 516), (768, 768), (768, 764), (1024, 1024), (1024, 1028), (1020, 1024), (1536, 1536), (2048, 512), (2048, 508),
          (2048, 1024), (2048, 2048), (2048, 2044), (2044, 2048), (4096, 512), (4096, 508), (4096, 1024), (4096, 1020),
          (4096, 2048), (2048, 4096), (3072, 3072), (3068, 3072), (3072, 3064), (8192, 1024), (4096, 4096), (320, 600)]
KERNELS = ("auto", "generic", "vec", "tb", "push", "stream")
FLAG_SWITCHES = [dict(deep_halo=False), dict(frame_fused=False), dict(frame_fused_batch=True), dict(frame_lds=False), dict(nt=True),
                 dict(nt=False), dict(comm_priority=False), dict(eager_lag=True), dict(frame_beside=True), dict(frame_beside=False),
                 dict(frame_wide=False), dict(edge_first=False), dict(edge_reserve=False), dict(xcd_bands=False), dict(tail_tiles=False),
                 dict(stream_walls=True), dict(stream_walls=False), dict(stream_pairs=True), dict(frame_seg=8), dict(frame_seg=24),
                 dict(frame_seg=4)]


def slabs(ny):
    """(y0, ny_local, ny_local_min) of a lone lattice and of first / middle / last slabs, with and without ny_local_min."""
    h, q = ny // 2, ny // 4
    return [(0, ny, 0), (0, h, 0), (q, h, 0), (ny - h, h, 0), (q, h, h - 8), (0, ny - q, q)]


def key(nx, ny, y0, nyl, mn, dt, rt, sem, turb, arith, kernel, batch, layout, ncu, tuning):
    """nx x ny, rows y0 + ny_local, dtype, collision, semantics, arithmetic, kernel, then whatever differs from the defaults."""
    k = f"{nx}x{ny} {y0}+{nyl} {np.dtype(dt).name[5:]} {rt} {sem[4:]} {arith} {kernel}"
    extra = dict(min=mn, turb=turb, batch=None if batch == 1 else batch, layout=None if layout == "auto" else layout, ncu=ncu, **tuning)
    return k + "".join(f" {n}={int(v) if isinstance(v, bool) else v}" for n, v in extra.items()
                       if not (v is None or type(v) is int and v == 0))


def plan(nx, ny, y0, nyl, mn, dt, rt, sem, turb, arith, kernel, batch, layout, ncu, tuning, steps):
    relax = relaxation(1000.0, ny, 0.08, 1.0 if sem == "mrt_py" else 1.2, 1.2)
    try:
        p = _params(nx, ny, y0, nyl, dt, rt, sem, kernel, turb, 0, layout, batch, arith, mn or None, tuning, 0.08, relax)
    except ValueError as e:
        return "python error: " + str(e)
    buf = ctypes.create_string_buffer(1 << 16)
    rc = L.lib().lbm_plan(ctypes.byref(p), int(ncu), int(steps), buf, len(buf))
    text = buf.value.decode()
    return text if rc >= 0 else f"rc={rc} {text}"


def grid():
    """Parameter tuples (deduplicated, in a fixed order)."""
    base = dict(dt=np.float32, rt="MRT", sem="mrt_gpu", turb=0, arith="strict", kernel="auto", batch=1, layout="auto", ncu=0,
                tuning={})
    out = []

    def add(nx, ny, y0, nyl, mn, **kw):
        d = dict(base, **kw)
        out.append((nx, ny, y0, nyl, mn, d["dt"], d["rt"], d["sem"], d["turb"], d["arith"], d["kernel"], d["batch"], d["layout"],
                    d["ncu"], d["tuning"]))

    # every shape x slab position x dtype x semantics under the multi-step kernels; the one-step kernels on a lone lattice and a slab
    for (nx, ny) in SHAPES:
        for (y0, nyl, mn), kernel, dt, sem in itertools.product(slabs(ny), KERNELS, (np.float32, np.float64), ("mrt_gpu", "mrt_py")):
            if kernel in ("auto", "tb", "stream") or (y0, nyl, mn) in slabs(ny)[2:3] or y0 == 0 and nyl == ny:
                add(nx, ny, y0, nyl, mn, kernel=kernel, dt=dt, sem=sem)
    # operator variants (collision x closure x arithmetic) on the shapes where the AUTO choices and steps per launch differ
    for (nx, ny) in [(160, 160), (1024, 1024), (2048, 2048), (4096, 1024), (4096, 4096), (8192, 1024)]:
        for (y0, nyl, mn) in slabs(ny)[:3]:
            for dt, rt, sem, turb, arith in itertools.product((np.float32, np.float64), ("SRT", "TRT", "MRT"), ("mrt_gpu", "mrt_py"),
                                                              (0, 1), ("strict", "fast")):
                if sem == "mrt_py" and turb:
                    continue
                for kernel in ("auto", "stream"):
                    add(nx, ny, y0, nyl, mn, dt=dt, rt=rt, sem=sem, turb=turb, arith=arith, kernel=kernel)
    add(64, 64, 0, 64, 0, turb=1, sem="mrt_py")
    # batches, layouts, compute units
    for (nx, ny), batch, dt, kernel in itertools.product([(64, 64), (160, 160), (384, 384), (768, 768), (1024, 1024)], (0, 2, 8, 64),
                                                         (np.float32, np.float64), ("auto", "tb", "stream", "vec")):
        add(nx, ny, 0, ny, 0, batch=batch, dt=dt, kernel=kernel)
        add(nx, ny, 0, ny, 0, batch=batch, dt=dt, kernel=kernel, tuning=dict(frame_fused=False))
    for (nx, ny), layout, (y0, nyl, mn) in itertools.product([(160, 160), (4096, 1024), (4096, 4096)], ("planes", "rows"),
                                                            slabs(1024)[:4]):
        add(nx, ny, y0 * ny // 1024, nyl * ny // 1024, 0, layout=layout)
    for (nx, ny), ncu, (y0, nyl, mn), dt in itertools.product([(4096, 1536), (4096, 3072), (8192, 4096), (16384, 6144)], (0, 80, 304),
                                                             slabs(1024)[:4], (np.float32, np.float64)):
        add(nx, ny, y0 * ny // 1024, nyl * ny // 1024, 0, ncu=ncu, dt=dt, arith="fast")
        add(nx, ny, y0 * ny // 1024, nyl * ny // 1024, 0, ncu=ncu, dt=dt, arith="fast", tuning=dict(frame_beside=True))
    # the wall frame beside the streaming kernel (lone lattices whose operator variant keeps the frame)
    for (nx, ny), ncu, dt, (rt, sem, sw) in itertools.product([(2048, 2048), (4096, 4096), (8192, 8192), (8192, 1024)], (0, 80, 304),
                                                              (np.float32, np.float64), [("TRT", "mrt_gpu", {}), ("MRT", "mrt_py", {}),
                                                                                         ("MRT", "mrt_gpu", dict(stream_walls=False))]):
        for fb in (True, False, None):
            add(nx, ny, 0, ny, 0, ncu=ncu, dt=dt, rt=rt, sem=sem, kernel="stream", tuning=dict(sw, frame_beside=fb))
    add(320, 600, 200, 200, 0, kernel="stream", tuning=dict(tb_steps=2))
    add(320, 600, 200, 200, 0, kernel="stream", tuning=dict(tb_steps=2, stream_walls=True))
    # tb_steps 0, 2 .. 10 (and the rejected 1, 11) under the kernel values that take it
    for (nx, ny), tb, kernel, dt in itertools.product([(36, 40), (64, 64), (160, 160), (1024, 1024), (4096, 1024), (4096, 4096)],
                                                     (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11), ("auto", "tb", "stream", "generic"),
                                                     (np.float32, np.float64)):
        for (y0, nyl, mn) in slabs(ny)[:3]:
            add(nx, ny, y0, nyl, mn, kernel=kernel, dt=dt, tuning=dict(tb_steps=tb))
        add(nx, ny, 0, ny, 0, kernel=kernel, dt=dt, sem="mrt_py", tuning=dict(tb_steps=tb))
        add(nx, ny, 0, ny, 0, kernel=kernel, dt=dt, tuning=dict(tb_steps=tb, stream_pairs=True))
    # every flag alone (and with two steps per launch)
    for (nx, ny), sw, kernel, dt in itertools.product([(160, 160), (1024, 1024), (4096, 1024), (4096, 4096), (8192, 1024)],
                                                      FLAG_SWITCHES, ("auto", "tb", "stream"), (np.float32, np.float64)):
        for (y0, nyl, mn) in slabs(ny)[:3]:
            add(nx, ny, y0, nyl, mn, kernel=kernel, dt=dt, tuning=sw)
        add(nx, ny, 0, ny, 0, kernel=kernel, dt=dt, tuning=dict(sw, tb_steps=2))
        add(nx, ny, ny // 4, ny // 2, 0, kernel=kernel, dt=dt, tuning=dict(sw, tb_steps=2))
    # parameter errors
    add(3, 64, 0, 64, 0)
    add(64, 64, 0, 1, 0)
    add(64, 64, 60, 8, 0)
    add(64, 100000, 0, 100000, 0)
    add(64, 64, 0, 32, 0, batch=2)
    add(64, 64, 0, 64, 0, batch=70000)
    add(64, 64, 0, 32, 40)
    add(64, 64, 0, 32, 0, kernel="push")
    add(64, 64, 0, 64, 0, kernel="push", turb=1)
    add(64, 64, 0, 64, 0, tuning=dict(nt=True, frame_seg=0))
    seen, uniq = set(), []
    for g in out:
        k = key(*g)
        if k not in seen:
            seen.add(k)
            uniq.append((k, g))
    return uniq


def entries():
    """{key: (plan text, units text)} for the whole grid."""
    res = {}
    for k, g in grid():
        text = plan(*g, 0)
        units = "" if text.startswith(("rc=", "python")) else ";".join(plan(*g, s).rsplit("units=", 1)[1] for s in STEPS)
        res[k] = (text, units)
    return res


def write(res, path=FIXTURE):
    """One line "<key>\t<plan>\t<units>" per entry, gzip-compressed with no name and no time stamp (the same bytes on every run)."""
    text = "".join(f"{k}\t{p}\t{u}\n" for k, (p, u) in res.items()).encode()
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, compresslevel=9, mtime=0) as z:
        z.write(text)


def read(path=FIXTURE):
    """{key: (plan text, units text)} of the fixture."""
    with gzip.open(path, "rt") as f:
        return {k: (p, u) for k, p, u in (line.rstrip("\n").split("\t") for line in f)}


def main():
    cur = entries()
    if "--check" in sys.argv[1:]:
        old = read()
        bad = sorted(k for k in set(old) | set(cur) if old.get(k) != cur.get(k))
        for k in bad:
            print(k, "\n  fixture:", old.get(k), "\n  library:", cur.get(k))
        print(f"{len(cur)} entries, {len(bad)} differ")
        return 1 if bad else 0
    write(cur)
    print(f"{len(cur)} entries -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
