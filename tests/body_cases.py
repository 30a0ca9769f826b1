"""Labelled solid masks for the tests of the per-body force (tests/test_body_force_cpu.py, tests/test_body_force_gpu.py), and the
Taylor-Couette case of the moving-body tests (tests/test_body_motion_cpu.py, tests/test_body_motion_gpu.py).

cases(nx, ny) -> name -> (mask bool [nx, ny], labels int32 [nx, ny] or None, nbodies): what the link list, the segments of the
reduction and the labels can get wrong.  Rows are placed relative to ny, so that the cases exist on the 8-row lattices too."""
import math

import numpy as np


def cases(nx, ny, seed=5):
    ya, yb = max(1, ny // 4), min(ny - 1, ny // 4 + 4)         # a band of up to four rows off the lid and the bottom wall
    out = {}

    def new():
        return np.zeros((nx, ny), dtype=bool), np.full((nx, ny), -7, dtype=np.int32)      # (-7: a label on a fluid cell is ignored)

    m, lab = new()                                              # 1. two separate blocks
    m[8:14, ya:yb] = True; lab[8:14, ya:yb] = 0
    m[30:33, ya + 1:yb] = True; lab[30:33, ya + 1:yb] = 1
    out["two_blocks"] = (m, lab, 2)

    m, lab = new()                                              # 2. two blocks that touch along an edge, a third at a corner
    m[10:16, ya:ya + 2] = True; lab[10:16, ya:ya + 2] = 0
    m[16:20, ya:ya + 2] = True; lab[16:20, ya:ya + 2] = 1
    m[20:24, ya + 2:yb] = True; lab[20:24, ya + 2:yb] = 2
    out["touching"] = (m, lab, 3)

    m, lab = new()                                              # 3. a body on a wall, one in a corner, one in the lid row
    m[0:3, ya:yb] = True; lab[0:3, ya:yb] = 0
    m[nx - 3:nx, ny - 2:ny] = True; lab[nx - 3:nx, ny - 2:ny] = 1
    m[nx // 3:nx // 3 + 5, 0] = True; lab[nx // 3:nx // 3 + 5, 0] = 2
    out["walls"] = (m, lab, 3)

    m, lab = new()                                              # 4. a one-cell body (beside a block)
    m[nx // 2, ya + 1] = True; lab[nx // 2, ya + 1] = 1
    m[5:9, ya:yb] = True; lab[5:9, ya:yb] = 0
    out["cell"] = (m, lab, 2)

    m, lab = new()                                              # 5. a ring that encloses fluid (inside it: a second body)
    m[30:38, ya - 1:ya + 5] = True
    m[31:37, ya:ya + 4] = False
    lab[m] = 0
    m[33:35, ya + 1:ya + 3] = True; lab[33:35, ya + 1:ya + 3] = 1
    out["ring"] = (m, lab, 2)

    m, lab = new()                                              # 6. a body wholly surrounded by another: no links
    m[40:45, ya:ya + 3] = True; lab[40:45, ya:ya + 3] = 0
    lab[41:44, ya + 1] = 1
    out["enclosed"] = (m, lab, 2)

    m, lab = new()                                              # 7. a label that no cell carries
    m[8:14, ya:yb] = True; lab[8:14, ya:yb] = 0
    m[30:33, ya:yb] = True; lab[30:33, ya:yb] = 2
    out["unused_label"] = (m, lab, 3)

    rng = np.random.default_rng(seed)                           # 8. random 20 % with 7 random labels
    m = rng.random((nx, ny)) < 0.2
    out["random"] = (m, rng.integers(0, 7, (nx, ny)).astype(np.int32), 7)

    m, _ = new()                                                # 9. the default: no labels given, every solid cell in one body
    m[19:25, ya:yb] = True
    m |= np.random.default_rng(seed + 1).random((nx, ny)) < 0.2      # (one body of several thousand links: more than one chunk)
    out["default"] = (m, None, 1)

    if nx >= 760:                                               # a w x h block far from the walls has 6 (w + h) - 4 links: exactly one chunk
        m, lab = new()                                          # of 2048 links (w + h = 342), and one link pair more (w + h = 343)
        m[20:358, 2:6] = True; lab[20:358, 2:6] = 0
        m[400:739, 2:6] = True; lab[400:739, 2:6] = 1
        out["chunk_edge"] = (m, lab, 2)
    return out


def labels_of(mask, labels):
    """The labels the library reports: `labels` on solid cells (0 for the default body), -1 on fluid cells."""
    lab = np.zeros(mask.shape, dtype=np.int32) if labels is None else labels
    return np.where(mask, lab, -1).astype(np.int32)


# ---- Taylor-Couette: the case and what the reference measured on it -------------------------------------------------------
TC_N, TC_C, TC_R1, TC_R2, TC_UW, TC_STEPS = 48, 23.5, 6.2, 20.6, 0.05, 6000
TC_RE = 0.08 * 48 * 6                       # nu = uLB nx / Re = 1/6: tau = 1
TC_TORQUE_ERR, TC_PROFILE_ERR = 0.0084836, 0.0152721      # |tz / closed form - 1| and max |u_theta - (A r + B / r)| / (Om R1), measured once
TC_FACTOR = 2.0                             # covers a later change of operator constants and nothing else


def tc_case():
    xs, ys = np.meshgrid(np.arange(TC_N), np.arange(TC_N), indexing="ij")
    r = np.hypot(xs - TC_C, ys - TC_C)
    mask = (r < TC_R1) | (r > TC_R2)
    labels = np.where(r < TC_R1, 0, 1).astype(np.int32)
    Om = TC_UW / TC_R1
    return dict(mask=mask, labels=labels, centres=[[TC_C, TC_C], [TC_C, TC_C]], motion=[[0.0, 0.0, Om], [0.0, 0.0, 0.0]], r=r, xs=xs, ys=ys, Om=Om)


def tc_errors(u, tz, case):
    """(torque errors of both bodies, profile error) against the closed form: tz = -+ 4 pi nu Om R1^2 R2^2 / (R2^2 - R1^2), nu = 1/6, and
    u_theta = A r + B / r for R1 + 1.5 < r < R2 - 1.5, as a fraction of the wall speed."""
    R1, R2, Om, r = TC_R1, TC_R2, case["Om"], case["r"]
    T = 4.0 * math.pi * (1.0 / 6.0) * Om * R1 ** 2 * R2 ** 2 / (R2 ** 2 - R1 ** 2)
    A, B = -Om * R1 ** 2 / (R2 ** 2 - R1 ** 2), Om * R1 ** 2 * R2 ** 2 / (R2 ** 2 - R1 ** 2)
    sel = (r > R1 + 1.5) & (r < R2 - 1.5)
    ut = ((case["ys"] - TC_C) * u[0] + (case["xs"] - TC_C) * u[1]) / r          # counter-clockwise with the lid on top
    return (abs(tz[0] / -T - 1.0), abs(tz[1] / T - 1.0)), float(np.abs(ut - (A * r + B / r))[sel].max() / TC_UW)
