"""Loader for liblbm_hip.so (the C ABI of include/lbm.h) -- ctypes only, no torch types.

The product path has NO CPU fallback: if the shared library is missing or cannot be
loaded, every entry point raises.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("LBM_LIB_PATH", os.path.join(_HERE, "liblbm_hip.so"))   # override: A/B builds of the kernels
HEADER = os.path.join(os.path.dirname(_HERE), "include", "lbm.h")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall"]
LINK_FLAGS = ["-ldl"]   # RCCL is bound lazily with dlopen inside the library

LBM_F32, LBM_F64 = 0, 1
LBM_SRT, LBM_TRT, LBM_MRT = 0, 1, 2
LBM_SEM_MRT_PY, LBM_SEM_MRT_GPU, LBM_SEM_BOUNCE_BACK, LBM_SEM_BOUNCE_BACK_SOLID = 0, 1, 2, 3
LBM_KERNEL_AUTO, LBM_KERNEL_GENERIC, LBM_KERNEL_VEC, LBM_KERNEL_TB, LBM_KERNEL_PUSH, LBM_KERNEL_STREAM = 0, 1, 2, 3, 4, 5
LBM_LAYOUT_AUTO, LBM_LAYOUT_PLANES, LBM_LAYOUT_ROWS = 0, 1, 2
LBM_SIDE_LOW, LBM_SIDE_HIGH = 0, 1
LBM_ARITH_STRICT, LBM_ARITH_FAST, LBM_ARITH_PROMOTED = 0, 1, 2
# lbm_params.flags (A/B switches of the launch plan; results never depend on them)
LBM_FLAG_NO_DEEP_HALO, LBM_FLAG_FRAME_UNFUSED, LBM_FLAG_FRAME_FUSED_BATCH, LBM_FLAG_NO_FRAME_LDS = 1, 2, 4, 8
LBM_FLAG_NT_ON, LBM_FLAG_NT_OFF, LBM_FLAG_COMM_PRIORITY_OFF, LBM_FLAG_EAGER_LAG = 16, 32, 64, 128
LBM_FLAG_FRAME_BESIDE_ON, LBM_FLAG_FRAME_BESIDE_OFF, LBM_FLAG_FRAME_NARROW, LBM_FLAG_NO_EDGE_FIRST = 512, 1024, 2048, 4096
LBM_FLAG_NO_EDGE_RESERVE, LBM_FLAG_NO_XCD_BANDS, LBM_FLAG_NO_TAIL_TILES, LBM_FLAG_STREAM_WALLS = 8192, 16384, 32768, 65536
LBM_FLAG_STREAM_PAIRS, LBM_FLAG_NO_STREAM_WALLS, LBM_FLAG_SOLID_TILES = 131072, 262144, 524288
ABI_VERSION = 4        # = LBM_ABI_VERSION of include/lbm.h (tests/test_abi.py keeps them equal)


class lbm_params(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("ny_local", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("collision", ctypes.c_int32), ("semantics", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("turb", ctypes.c_int32), ("device", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("arith", ctypes.c_int32), ("ny_local_min", ctypes.c_int32),
                ("tb_steps", ctypes.c_int32), ("frame_seg", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("uLB", ctypes.c_double), ("omega", ctypes.c_double), ("omegam", ctypes.c_double),
                ("omega_e", ctypes.c_double), ("omega_eps", ctypes.c_double), ("omega_q", ctypes.c_double)]


LBM_MONITOR_MAX_BOXES, LBM_MONITOR_MAX_PROBES = 4, 8


class lbm_monitor_spec(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("host_dtype", ctypes.c_int32), ("x_lo", ctypes.c_int32), ("x_hi", ctypes.c_int32),
                ("y_lo", ctypes.c_int32), ("y_hi", ctypes.c_int32), ("nboxes", ctypes.c_int32), ("nprobes", ctypes.c_int32),
                ("box", (ctypes.c_int32 * 4) * LBM_MONITOR_MAX_BOXES), ("probe", (ctypes.c_int32 * 2) * LBM_MONITOR_MAX_PROBES)]


class lbm_monitor_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "nonfinite", "sum_ux", "sum_uy", "sum_rho", "sum_q", "max_q", "min_q", "min_x",
                                               "min_y")] + [("probe", (ctypes.c_double * 3) * LBM_MONITOR_MAX_PROBES)]


class lbm_residual_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "step_prev", "cells", "nonfinite", "sum_du2", "sum_u2", "sum_drho2", "max_du2",
                                               "max_x", "max_y", "max_drho2")]


LBM_TOPOLOGY_MAX_WINDOWS, LBM_TOPOLOGY_BLOCK = 8, 64


class lbm_topology_spec(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("host_dtype", ctypes.c_int32), ("nwindows", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("window", (ctypes.c_int32 * 4) * LBM_TOPOLOGY_MAX_WINDOWS)]


class lbm_topology_extremum(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("psi", "x", "y", "omega")]


class _lbm_topology_window(ctypes.Structure):
    _fields_ = [("min", lbm_topology_extremum), ("max", lbm_topology_extremum)]


class lbm_topology_record(ctypes.Structure):
    _fields_ = [("step", ctypes.c_double), ("closure", ctypes.c_double), ("window", _lbm_topology_window * LBM_TOPOLOGY_MAX_WINDOWS)]


class lbm_solid_force_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "links", "fx", "fy")]


class lbm_body_force_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "body", "links", "fx", "fy", "tz")]


class lbm_scalar_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "cells", "sum", "min", "max")]


class lbm_scalar_flux_record(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("step", "links", "flux")]


def sources():
    return [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".hip", ".hpp"))] + [HEADER]


def build(force=False, verbose=False):
    """Compile csrc/*.hip for gfx950 into liblbm_hip.so next to this file (in-tree).  The translation units (eight of host code +
    C ABI: lbm_hip / lbm_plan / lbm_launch / lbm_comm / lbm_sampling / lbm_monitor / lbm_residual / lbm_topology / lbm_solid / lbm_bodies / lbm_body_motion / lbm_body_shape / lbm_scalar (with its kernels, from lbm_scalar.hpp); the explicit instantiations of the tile and
    streaming kernels, of the one-step kernels with a solid mask per mode of the wall rule, a base | feature bits -- lbm_solid{,_move,_shape} the bases,
    lbm_solid_buoy buoyancy, lbm_solid_sgs{,_move,_shape} the sub-grid closure, lbm_solid_relax{,_move,_shape} a relaxation field, lbm_solid_relax_sgs{,_move,_shape}
    both, lbm_solid_rheo{,_move,_shape} a rheology table, all from the one macro of lbm_solid.hpp -- and of the tile kernel with solid cells, for float and for double) are compiled in parallel into csrc/_obj/ and linked."""
    srcs = sources()
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    from concurrent.futures import ThreadPoolExecutor
    objdir = os.path.join(_CSRC, "_obj")
    os.makedirs(objdir, exist_ok=True)
    units = [s for s in srcs if s.endswith(".hip")]
    objs = [os.path.join(objdir, os.path.basename(u)[:-4] + ".o") for u in units]

    def compile_one(pair):
        cmd = [HIPCC] + cflags + ["-c", pair[0], "-o", pair[1]]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 4, 16)) as pool:   # (at most 16 compiles at once)
        list(pool.map(compile_one, zip(units, objs)))
    cmd = [HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + objs + LINK_FLAGS
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None

# name -> (restype, argtypes); exactly the entry points declared in include/lbm.h
_vp, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SIGNATURES = {
    "lbm_abi_version": (_i, []),
    "lbm_device_count": (_i, []),
    "lbm_create": (_vp, [ctypes.POINTER(lbm_params), ctypes.c_char_p, ctypes.c_size_t]),
    "lbm_destroy": (None, [_vp]),
    "lbm_last_error": (ctypes.c_char_p, [_vp]),
    "lbm_init_equilibrium": (_i, [_vp]),
    "lbm_set_state": (_i, [_vp, _vp, _i]),
    "lbm_set_relaxation": (_i, [_vp, _i, _d, _d, _d, _d, _d]),
    "lbm_step": (_i, [_vp, _i]),
    "lbm_sync": (_i, [_vp]),
    "lbm_time_steps": (_i, [_vp, _i, ctypes.POINTER(_d)]),
    "lbm_steps_done": (ctypes.c_longlong, [_vp]),
    "lbm_next_unit": (_i, [_vp, _i]),
    "lbm_describe": (_i, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "lbm_plan": (_i, [ctypes.POINTER(lbm_params), _i, _i, ctypes.c_char_p, ctypes.c_size_t]),
    "lbm_get_fields": (_i, [_vp, _vp, _vp, _vp, _i]),
    "lbm_mean_u": (_i, [_vp, ctypes.POINTER(_d)]),
    "lbm_get_tau": (_i, [_vp, _vp, _i]),
    "lbm_stats_begin": (_i, [_vp, _i]),
    "lbm_stats_sample": (_i, [_vp]),
    "lbm_stats_get": (_i, [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_longlong)]),
    "lbm_stats_end": (_i, [_vp]),
    "lbm_monitor": (_i, [_vp, ctypes.POINTER(lbm_monitor_spec), ctypes.POINTER(lbm_monitor_record)]),
    "lbm_monitor_begin": (_i, [_vp, ctypes.POINTER(lbm_monitor_spec), _i, _i]),
    "lbm_monitor_sample": (_i, [_vp]),
    "lbm_monitor_read": (_i, [_vp, ctypes.POINTER(lbm_monitor_record), _i, ctypes.POINTER(ctypes.c_longlong),
                              ctypes.POINTER(ctypes.c_longlong)]),
    "lbm_monitor_end": (_i, [_vp]),
    "lbm_get_lines": (_i, [_vp, _i, _i, _vp, _vp, _i]),
    "lbm_residual_begin": (_i, [_vp, _i, _i, _i]),
    "lbm_residual_sample": (_i, [_vp]),
    "lbm_residual_read": (_i, [_vp, ctypes.POINTER(lbm_residual_record), _i, ctypes.POINTER(ctypes.c_longlong),
                               ctypes.POINTER(ctypes.c_longlong)]),
    "lbm_residual_end": (_i, [_vp]),
    "lbm_topology": (_i, [_vp, ctypes.POINTER(lbm_topology_spec), ctypes.POINTER(lbm_topology_record)]),
    "lbm_get_stream_function": (_i, [_vp, _vp, _vp, _i]),
    "lbm_set_solid": (_i, [_vp, _vp]),
    "lbm_get_solid": (_i, [_vp, _vp]),
    "lbm_solid_force": (_i, [_vp, ctypes.POINTER(lbm_solid_force_record)]),
    "lbm_set_solid_bodies": (_i, [_vp, _vp, _i, _vp]),
    "lbm_get_solid_bodies": (_i, [_vp, _vp, _vp]),
    "lbm_solid_body_count": (_i, [_vp]),
    "lbm_body_force": (_i, [_vp, ctypes.POINTER(lbm_body_force_record)]),
    "lbm_force_begin": (_i, [_vp, _i, _i]),
    "lbm_force_sample": (_i, [_vp]),
    "lbm_force_read": (_i, [_vp, _vp, _i, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),   # (records: [samples][B][nbodies])
    "lbm_force_end": (_i, [_vp]),
    "lbm_set_body_motion": (_i, [_vp, _vp]),            # (motion: [B][nbodies][3] doubles, or NULL)
    "lbm_get_body_motion": (_i, [_vp, _vp]),
    "lbm_set_solid_shape": (_i, [_vp, _vp]),            # (q: [B][8][X][Y] doubles, or NULL)
    "lbm_get_solid_shape": (_i, [_vp, _vp]),
    "lbm_set_open_cells": (_i, [_vp, _vp, _vp]),        # (hold: [B][X][Y] uint8 or NULL; f: [B][9][X][Y] doubles)
    "lbm_get_open_cells": (_i, [_vp, _vp, _vp]),
    "lbm_set_wall_velocity": (_i, [_vp, _vp]),          # (uw: [B][2][X][Y] doubles, or NULL)
    "lbm_get_wall_velocity": (_i, [_vp, _vp]),
    "lbm_set_periodic": (_i, [_vp, _i, _i]),            # (px, py: 0 / 1)
    "lbm_get_periodic": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "lbm_set_driving_force": (_i, [_vp, _d, _d]),       # (fx, fy: force density per cell)
    "lbm_get_driving_force": (_i, [_vp, ctypes.POINTER(_d), ctypes.POINTER(_d)]),
    "lbm_scalar_begin": (_i, [_vp, _d, _d, _vp, _vp, _vp, _vp]),   # (D, magic; c0, dirichlet, wall_value, hold_value: [X][Y] or NULL)
    "lbm_scalar_end": (_i, [_vp]),
    "lbm_scalar_active": (_i, [_vp, ctypes.POINTER(_d), ctypes.POINTER(_d)]),
    "lbm_scalar_get": (_i, [_vp, _vp, _vp, _i]),
    "lbm_scalar_get_stored": (_i, [_vp, _vp, _i]),
    "lbm_scalar_set_state": (_i, [_vp, _vp, _i]),
    "lbm_scalar_totals": (_i, [_vp, ctypes.POINTER(lbm_scalar_record)]),
    "lbm_scalar_flux": (_i, [_vp, ctypes.POINTER(lbm_scalar_flux_record)]),
    "lbm_set_buoyancy": (_i, [_vp, _d, _d, _d]),        # (ax, ay: acceleration per unit of C; c_ref)
    "lbm_set_buoyancy_plane": (_i, [_vp, _vp, _i]),     # (conc: [X][Y], as lbm_scalar_get's conc_out)
    "lbm_get_buoyancy": (_i, [_vp, ctypes.POINTER(_d), ctypes.POINTER(_d), ctypes.POINTER(_d)]),
    "lbm_set_subgrid": (_i, [_vp, _d]),                 # (cs2: the sub-grid constant; 0 clears)
    "lbm_get_subgrid": (_i, [_vp, ctypes.POINTER(_d)]),
    "lbm_set_relaxation_field": (_i, [_vp, _vp, _vp]),  # (omega[B][nx][ny] doubles, omegam the same or NULL; both NULL clears)
    "lbm_get_relaxation_field": (_i, [_vp, _vp, _vp]),  # -> 1 if set, 0 if not
    "lbm_set_rheology": (_i, [_vp, _vp, _vp, _i, _d]),  # (omega[n] doubles, omegam[n] or NULL, n, g_max; omega NULL clears)
    "lbm_get_rheology": (_i, [_vp, _vp, _vp, ctypes.POINTER(_i), ctypes.POINTER(_d)]),  # -> 1 if set, 0 if not
    "lbm_get_shear": (_i, [_vp, _vp, _i]),
    "lbm_halo_elems": (_i, [_vp]),
    "lbm_halo_export": (_i, [_vp, _i, _vp]),
    "lbm_halo_import": (_i, [_vp, _i, _vp]),
    "lbm_step_edges": (_i, [_vp]),
    "lbm_step_interior": (_i, [_vp]),
    "lbm_step_finish": (_i, [_vp]),
    "lbm_halo_rows_elems": (ctypes.c_longlong, [_vp, _i]),
    "lbm_halo_export_rows": (_i, [_vp, _i, _i, _vp]),
    "lbm_halo_import_rows": (_i, [_vp, _i, _i, _vp]),
    "lbm_step_unit": (_i, [_vp, _i]),
    "lbm_comm_unique_id": (_i, [_vp]),
    "lbm_comm_init": (_i, [_vp, _i, _i, _vp]),
    "lbm_comm_loopback": (_i, [_vp]),
    "lbm_copy_bandwidth": (_i, [_vp, ctypes.c_size_t, _i, ctypes.POINTER(_d)]),
    "lbm_fma_rate": (_i, [_vp, _d, ctypes.POINTER(_d)]),
}


def _preload_torch_runtime(names=("libamdhip64.so",)):
    """One process can hold only ONE HIP runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64 / librccl (torch/lib); if liblbm_hip.so pulled in /opt/rocm's copies first, a
    later `import torch` would find no GPU (measured on the MI355X box).  So when torch is
    installed, load ITS runtime libraries by path first (without importing torch); the
    DT_NEEDED entries of liblbm_hip.so then resolve to them by SONAME, and torch.distributed
    (RCCL) and this library share one runtime whichever is imported first."""
    if os.environ.get("LBM_USE_SYSTEM_ROCM"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in names:
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def lib():
    """The loaded library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _preload_torch_runtime()
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if an exported symbol is missing
            f.restype, f.argtypes = res, args
        if L.lbm_abi_version() != ABI_VERSION:
            raise RuntimeError("liblbm_hip.so ABI version mismatch")
        _lib = L
    return _lib
