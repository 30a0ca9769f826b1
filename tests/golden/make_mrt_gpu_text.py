#!/usr/bin/env python3
"""Generate tests/golden/mrt_gpu_text.json and tests/golden/mrt_gpu_text_16x16.npz from the reference's own kernel text.

Runs ONLY where the reference is present (the directory make_golden.py reads, or LBM_REFERENCE_DIR): oracle/reftext.py cuts
the four CUDA kernel literals out of MRT_GPU.py as text, compiles them as host C++ without multiply-add contraction into
oracle/_ref/, and this script runs them for every entry of oracle.reftext.CASES.  What it writes is recorded results only:

* ``mrt_gpu_text.json`` -- SHA-256 of the little-endian C-contiguous float32 bytes of fin[9,X,Y], u[2,X,Y], rho[X,Y] and
  taus[X,Y] (the project's layout; taus with the closure only) per (case, checkpoint), the compile flags, and whether MRT_GPU_datagen.py's literals equal
  MRT_GPU.py's.
* ``mrt_gpu_text_16x16.npz`` -- the values themselves for MRT + closure, 16 x 16, Re 100, after 20 steps.

Nothing of the kernel text is written.  The script is not imported or executed; MRT.py (numba, numexpr) is not part of this.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import reftext  # noqa: E402
from mrt_gpu_text_ref import FIELDS, digest  # noqa: E402

VALUES = reftext.case("MRT", 1, 100.0, 16, 16), 20


def text_checkpoints(c, order=0):
    t = reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb, order=order)
    for n in reftext.CHECKPOINTS:
        t.step(n - t.nsteps)
        yield n, t


def fields(c):
    """taus_g is recorded with the closure only: without it the text never writes it (the tests assert the zeros it starts with)."""
    return FIELDS if c.turb else FIELDS[:3]


def digests():
    return {c.id: {str(n): {k: digest(getattr(t, k)) for k in fields(c)} for n, t in text_checkpoints(c)} for c in reftext.CASES}


def document():
    return {"what": "SHA-256 of the '<f4' C-contiguous bytes of fin[9,X,Y], u[2,X,Y], rho[X,Y], taus[X,Y] that MRT_GPU.py's kernel "
                    "text (funRT + funBC, compiled as host C++) leaves after n steps; case = operator-turb-Re-XxY; taus with turb = 1 only "
                    "(the text does not write it otherwise)",
            "compile_flags": reftext.FLAGS,
            "datagen_literals": reftext.datagen_comparison(),
            "signed_zeros": "none canonicalised: digests and np.array_equal agree for every case",
            "checkpoints": list(reftext.CHECKPOINTS),
            "digests": digests()}


def write_json(doc, path):
    with open(path, "w") as f:       # one line per case
        head = {k: v for k, v in doc.items() if k != "digests"}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "digests": {\n')
        f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in doc["digests"].items()))
        f.write("\n }\n}\n")


if __name__ == "__main__":
    if reftext.build_all(verbose=True) is None:
        sys.exit("reference not present; fixtures are already committed")
    write_json(document(), os.path.join(HERE, "mrt_gpu_text.json"))
    c, n = VALUES
    t = reftext.RefTextCavity(c.nx, c.ny, c.Re, c.coll, c.turb).step(n)
    np.savez_compressed(os.path.join(HERE, "mrt_gpu_text_16x16.npz"), fin=t.fin, u=t.u, rho=t.rho, taus=t.taus,
                        case=np.array(c.id), steps=np.array(n))
    for name in ("mrt_gpu_text.json", "mrt_gpu_text_16x16.npz"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
