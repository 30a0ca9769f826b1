"""bench.py end to end on an MI355X: the result line and --dump-outputs, whose arrays are checked against the C oracle run for the
same number of steps (strict arithmetic: bit for bit; fast arithmetic: to rounding)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench
from oracle.lbm_ref import CavityOracleC, max_threads, set_threads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arith", ["strict", "fast"])
def test_bench_dumps_what_its_timed_steps_computed(arith, tmp_path):
    steps, warmup, cfg = 21, 4, "c2"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--config", cfg, "--arith", arith, "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["steps"] == steps and res["warmup"] == warmup and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["dump_outputs"]["sample"] and res["dump_outputs"]["dtype"] == "float64"
    assert res["dump_outputs"]["steps_done"] == warmup + steps        # the state dumped is the one the last timed step left

    nx, ny, Re, dtype, RT, sem, _ = bench.CONFIGS[cfg]
    set_threads(max(1, min(16, max_threads())))
    try:
        o = CavityOracleC(nx, ny, Re, semantics=sem, collision=RT, dtype=np.dtype(dtype)).step(warmup + steps)
    finally:
        set_threads(1)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(nx * ny, bench.DUMP_CELLS, replace=False))
    want = {"u": o.u.reshape(2, -1)[:, idx], "rho": o.rho.reshape(-1)[idx], "fin": o.fin.reshape(9, -1)[:, idx]}
    for name, ref in want.items():
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == ref.dtype and got.shape == ref.shape, name
        if arith == "strict":
            assert np.array_equal(got, ref), name
        else:
            assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), name
