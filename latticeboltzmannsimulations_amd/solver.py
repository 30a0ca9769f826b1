"""Host side of the hot path: a thin ctypes wrapper over liblbm_hip.so that mirrors how the
reference script drives PyCUDA (MRT_GPU.py:23-30,309-328,701-760): create device state,
upload / initialise populations, advance N steps, read u / rho / fin back in the reference's
host layout ([k, x, y], y fastest, y = 0 the lid)."""
import ctypes

import numpy as np

from . import _lib as L
from . import monitor as M
from . import residual as RS
from . import solid as S
from . import topology as T

_DT = {np.dtype(np.float32): L.LBM_F32, np.dtype(np.float64): L.LBM_F64}
_COLL = {"SRT": L.LBM_SRT, "TRT": L.LBM_TRT, "MRT": L.LBM_MRT}
_SEM = {"mrt_py": L.LBM_SEM_MRT_PY, "mrt_gpu": L.LBM_SEM_MRT_GPU, "bounce_back": L.LBM_SEM_BOUNCE_BACK}
_SEM_SOLID = "bounce_back_solid"    # what semantics='bounce_back' becomes with solid=...: LBM_SEM_BOUNCE_BACK_SOLID
_KERNEL = {"auto": L.LBM_KERNEL_AUTO, "generic": L.LBM_KERNEL_GENERIC, "vec": L.LBM_KERNEL_VEC, "tb": L.LBM_KERNEL_TB,
           "push": L.LBM_KERNEL_PUSH, "stream": L.LBM_KERNEL_STREAM}
_ARITH = {"strict": L.LBM_ARITH_STRICT, "fast": L.LBM_ARITH_FAST, "promoted": L.LBM_ARITH_PROMOTED}
_LAYOUT = {"auto": L.LBM_LAYOUT_AUTO, "planes": L.LBM_LAYOUT_PLANES, "rows": L.LBM_LAYOUT_ROWS}


def relaxation(Re, ysize, uLB=0.08, omega_eps=1.2, omega_q=1.2):
    """Relaxation parameters exactly as the reference script derives them on the host
    (MRT_GPU.py:63-93): nuLB from the WHOLE lattice height, omega, TRT omegam with
    Lambda = 1/3.5, MRT vector (omega_e = 1, omega_eps = omega_q = 1.2)."""
    nuLB = uLB * ysize / Re
    omega = 2.0 / (6. * nuLB + 1)
    delTRT = 1.0 / 3.5
    omegam = 1.0 / (0.5 + (delTRT / ((1 / omega) - 0.5)))
    return dict(omega=omega, omegam=omegam, omega_e=1.0, omega_eps=omega_eps, omega_q=omega_q)


def _tuning(t):
    """(tb_steps, frame_seg, flags) of lbm_params from a dict of A/B switches (see CavitySolver)."""
    t = dict(t or {})
    tb, seg, flags = int(t.pop("tb_steps", 0) or 0), int(t.pop("frame_seg", 0) or 0), 0
    off = {"deep_halo": L.LBM_FLAG_NO_DEEP_HALO, "frame_fused": L.LBM_FLAG_FRAME_UNFUSED, "frame_lds": L.LBM_FLAG_NO_FRAME_LDS,
           "comm_priority": L.LBM_FLAG_COMM_PRIORITY_OFF, "frame_wide": L.LBM_FLAG_FRAME_NARROW, "edge_first": L.LBM_FLAG_NO_EDGE_FIRST,
           "edge_reserve": L.LBM_FLAG_NO_EDGE_RESERVE, "xcd_bands": L.LBM_FLAG_NO_XCD_BANDS,
           "tail_tiles": L.LBM_FLAG_NO_TAIL_TILES}
    on = {"frame_fused_batch": L.LBM_FLAG_FRAME_FUSED_BATCH, "eager_lag": L.LBM_FLAG_EAGER_LAG, "stream_pairs": L.LBM_FLAG_STREAM_PAIRS,
          "solid_tiles": L.LBM_FLAG_SOLID_TILES}
    if "stream_walls" in t:     # (three states: True / False force it, absent = the library's choice per operator variant)
        flags |= L.LBM_FLAG_STREAM_WALLS if t.pop("stream_walls") else L.LBM_FLAG_NO_STREAM_WALLS
    for k, bit in off.items():
        if not t.pop(k, True):
            flags |= bit
    for k, bit in on.items():
        if t.pop(k, False):
            flags |= bit
    nt = t.pop("nt", None)
    if nt is not None:
        flags |= L.LBM_FLAG_NT_ON if nt else L.LBM_FLAG_NT_OFF
    fb = t.pop("frame_beside", None)
    if fb is not None:
        flags |= L.LBM_FLAG_FRAME_BESIDE_ON if fb else L.LBM_FLAG_FRAME_BESIDE_OFF
    if t:
        raise ValueError(f"unknown tuning switches {sorted(t)}")
    return tb, seg, flags


class CavitySolver:
    """One lattice (or one y-slab of it) resident on one MI355X.

    xsize, ysize : whole lattice (MRT_GPU.py:53-54)
    Re, uLB      : MRT_GPU.py:47,57
    RT           : 'SRT' | 'TRT' | 'MRT' (MRT_GPU.py:48)
    semantics    : 'mrt_gpu' (full streaming windows + NEBB on four walls, MRT_GPU.py:412,674-692)
                   or 'mrt_py' (the CPU script's windows and wall rules, MRT.py:404-453)
                   or 'bounce_back' (half-way bounce-back walls with Ladd's moving-lid term, the reference's 'BB' option,
                   MRT_GPU.py:281: every cell is a fluid cell, walls half a cell outside the lattice, mass conserved to rounding;
                   relaxation rates as 'mrt_gpu'; kernels 'auto' / 'generic' / 'tb' / 'stream', arith 'strict' / 'fast', turb=0)
    dtype        : float32 (what MRT_GPU.py stores, MRT_GPU.py:207) or float64 (what MRT.py computes in)
    rows         : (y0, ny_local) when this object holds only a slab
    kernel       : 'auto' | 'generic' (one thread per cell) | 'vec' (16 B per access, MRT_GPU.py semantics) |
                   'tb' (three to five steps per launch through LDS; what 'auto' picks when it applies) |
                   'push' (the reference's two-launch push scheme, for A/B only)
    layout       : device arrays 'planes' [k][y][x], 'rows' [y][k][x], 'auto' (= rows)
    arith        : 'strict' (default; the reference's operation order, bit-identical to the CPU restatement the tests check against), 'fast' (MRT operator
                   in factored form, about half the arithmetic, agrees to rounding; semantics='mrt_py' runs the strict form for it) or 'promoted' (MRT_GPU.py's CUDA text: the strict order, with
                   the sub-expressions its double literals make double -- equilibrium bracket, MRT m_eq sums, Smagorinsky tau -- evaluated in
                   double and rounded to float once; fp32 bit-identical to the oracles' promote=True, fp64 the same as 'strict';
                   semantics='mrt_gpu' only)
    min_rows     : slabs: the smallest ny_local of ALL slabs of the decomposition (lbm_params.ny_local_min) -- the launch plan is
                   derived from it, so that neighbours run the same exchange protocol
    solid        : None (default), or a mask [X, Y] (a CavityBatch: [B, X, Y], or [X, Y] for all lattices) whose nonzero cells are solid
                   obstacles at rest inside the cavity (semantics='bounce_back' only; the context is then LBM_SEM_BOUNCE_BACK_SOLID): a
                   source that is a solid cell bounces like a wall, solid cells hold the rest equilibrium (u = 0 in every export), one
                   step per launch (kernel 'auto' or 'generic'), no slabs.  See set_solid, solid, solid_force.  tuning=dict(solid_tiles=True):
                   three to five steps per launch on the tile kernel instead (kernel 'auto' or 'tb'; planned as plain 'bounce_back' with
                   kernel='tb' plans the same lattice; the same bits).
    bodies       : with solid=...: integer labels of the mask's shape that split the solid cells into bodies, and `centres`, the points
                   their torques refer to (None: the centroids).  See set_bodies, bodies, body_force, begin_force, force_series.
    tuning       : A/B switches of the launch plan, none of which changes a result: tb_steps (2..5 steps per launch; 2..8 with kernel='stream'),
                   frame_seg, and the boolean flags deep_halo, frame_fused, frame_fused_batch, frame_lds, nt, comm_priority,
                   eager_lag, frame_beside, frame_wide, edge_first, edge_reserve, xcd_bands, tail_tiles, solid_tiles (lbm_params.tb_steps / frame_seg / flags)
    """

    def __init__(self, xsize, ysize, Re, RT="MRT", uLB=0.08, semantics="mrt_gpu", dtype=np.float32, turb=0,
                 device=0, rows=None, kernel="auto", layout="auto", omega_eps=None, omega_q=None, batch=1, arith="strict",
                 min_rows=None, tuning=None, solid=None, bodies=None, centres=None):
        self._h = None
        self.batch = int(batch)
        self._lead = getattr(self, "_lead", ())      # leading axes of the host arrays: (B,) for a CavityBatch
        self.lib = L.lib()
        self.nx, self.ny = int(xsize), int(ysize)
        self.dtype = np.dtype(dtype)
        if self.dtype not in _DT:
            raise ValueError("dtype must be float32 or float64")
        if RT not in _COLL:
            raise ValueError("RT must be 'SRT', 'TRT' or 'MRT'")
        if semantics not in _SEM:
            raise ValueError("semantics must be 'mrt_gpu', 'mrt_py' or 'bounce_back'")
        if omega_eps is None:
            omega_eps = 1.0 if semantics == "mrt_py" else 1.2      # MRT.py:72 vs MRT_GPU.py:90
        if omega_q is None:
            omega_q = 1.2
        self.Re, self.RT, self.uLB, self.semantics = float(Re), RT, float(uLB), semantics
        self._omega_eps, self._omega_q = omega_eps, omega_q
        self.relax = relaxation(self.Re, self.ny, self.uLB, omega_eps, omega_q)
        self.y0, self.ny_local = (0, self.ny) if rows is None else (int(rows[0]), int(rows[1]))
        self.turb = int(turb)
        self.arith = arith
        self.has_solid = solid is not None
        if self.has_solid and semantics != "bounce_back":
            raise ValueError("solid=... needs semantics='bounce_back'")
        if bodies is not None and not self.has_solid:
            raise ValueError("bodies=... labels the cells of a solid mask: it needs solid=...")
        p = _params(self.nx, self.ny, self.y0, self.ny_local, self.dtype, RT, _SEM_SOLID if self.has_solid else semantics, kernel, turb, device,
                    layout, self.batch, arith, min_rows, tuning, self.uLB, self.relax)
        err = ctypes.create_string_buffer(512)
        h = self.lib.lbm_create(ctypes.byref(p), err, len(err))
        if not h:
            raise RuntimeError("lbm_create: " + err.value.decode())
        self._h = ctypes.c_void_p(h)
        if self.has_solid:
            try:
                self.set_solid(solid)
                if bodies is not None:
                    self.set_bodies(bodies, centres)
            except Exception:
                self.close()
                raise

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.lbm_last_error(self._h).decode()}")

    def close(self):
        if self._h is not None:
            self.lib.lbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _host(self, a, shape, name):
        shape = self._lead + tuple(shape)
        a = np.asarray(a)
        if a.dtype not in _DT or a.shape != shape or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{name} must be a C-contiguous float32/float64 array of shape {shape}")
        return a

    # -- state in -----------------------------------------------------------------------
    def init_equilibrium(self):
        self._check(self.lib.lbm_init_equilibrium(self._h), "lbm_init_equilibrium")

    def set_state(self, fin):
        fin = self._host(fin, (9, self.nx, self.ny), "fin")
        self._check(self.lib.lbm_set_state(self._h, fin.ctypes.data, _DT[fin.dtype]), "lbm_set_state")

    def set_relaxation(self, index=0, Re=None, **rates):
        """Relaxation rates of lattice `index` for all later steps: from a Reynolds number (as the reference derives them,
        MRT_GPU.py:63-93) and / or explicit omega, omegam, omega_e, omega_eps, omega_q."""
        r = dict(self.relax if Re is None else relaxation(float(Re), self.ny, self.uLB, self._omega_eps, self._omega_q))
        unknown = set(rates) - set(r)
        if unknown:
            raise ValueError(f"unknown relaxation rates {sorted(unknown)}")
        r.update(rates)
        self._check(self.lib.lbm_set_relaxation(self._h, int(index), r["omega"], r["omegam"], r["omega_e"], r["omega_eps"],
                                                r["omega_q"]), "lbm_set_relaxation")
        return r

    # -- time loop ----------------------------------------------------------------------
    def step(self, nsteps=1):
        self._check(self.lib.lbm_step(self._h, int(nsteps)), "lbm_step")
        return self

    def sync(self):
        self._check(self.lib.lbm_sync(self._h), "lbm_sync")

    def time_steps(self, nsteps):
        ms = ctypes.c_double(0.0)
        self._check(self.lib.lbm_time_steps(self._h, int(nsteps), ctypes.byref(ms)), "lbm_time_steps")
        return ms.value

    @property
    def steps_done(self):
        return int(self.lib.lbm_steps_done(self._h))

    def describe(self):
        """The launch plan as a dict (lbm_describe): kernel of the multi-step units, steps per launch, frame width, ..."""
        buf = ctypes.create_string_buffer(512)
        if self.lib.lbm_describe(self._h, buf, len(buf)) < 0:
            raise RuntimeError("lbm_describe failed")
        out = {}
        for kv in buf.value.decode().split():
            if "=" not in kv:      # (a bare word: `relax_field`, `relax_field+m`)
                out[kv] = True
                continue
            k, v = kv.split("=", 1)
            if k == "rheology":      # (`rheology=<n>` or `rheology=<n>+m`: the entries, and whether the table carries TRT's odd rate)
                out[k], out["rheology_m"] = int(v.split("+")[0]), v.endswith("+m")
                continue
            out[k] = int(v) if v.lstrip("-").isdigit() else v
        return out

    def next_unit(self, steps_left):
        """Time steps the next launch unit of step() advances when `steps_left` remain (1 = a single step)."""
        n = int(self.lib.lbm_next_unit(self._h, int(steps_left)))
        if n < 0:
            raise RuntimeError("lbm_next_unit failed")
        return n

    # -- state out ----------------------------------------------------------------------
    def get_fields(self, want_fin=False, out_dtype=None, u=None, rho=None, fin=None):
        """Returns (u[2,X,Y], rho[X,Y]) (and fin[9,X,Y]).  Arrays are whole-lattice shaped;
        a slab writes only its rows y0:y0+ny_local."""
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        lead = self._lead
        u = np.zeros(lead + (2, self.nx, self.ny), dtype=dt) if u is None else self._host(u, (2, self.nx, self.ny), "u")
        rho = np.zeros(lead + (self.nx, self.ny), dtype=dt) if rho is None else self._host(rho, (self.nx, self.ny), "rho")
        if want_fin and fin is None:
            fin = np.zeros(lead + (9, self.nx, self.ny), dtype=dt)
        if fin is not None:
            fin = self._host(fin, (9, self.nx, self.ny), "fin")
        self._check(self.lib.lbm_get_fields(self._h, u.ctypes.data, rho.ctypes.data,
                                            fin.ctypes.data if fin is not None else None, _DT[u.dtype]),
                    "lbm_get_fields")
        return (u, rho, fin) if fin is not None else (u, rho)

    def mean_u(self):
        """mean(u) of the fields get_fields() would return, reduced on the device in double (lbm_mean_u): one float per
        lattice crosses PCIe instead of the field.  A batch returns an array [B]."""
        out = (ctypes.c_double * self.batch)()
        self._check(self.lib.lbm_mean_u(self._h, out), "lbm_mean_u")
        return np.array(out[:]) if self._lead else float(out[0])

    def get_tau(self, out_dtype=None):
        """tau + tau_turbulent per cell of the last iteration (taus_g, MRT_GPU.py:387); 1 / omega everywhere when turb = 0.  With a
        sub-grid constant (set_subgrid): the tau of the step that starts from the current state, solid and hold cells at 1 / omega.
        With a rheology table (set_rheology) likewise: 1 / omega of the rate the table gives each cell's shear."""
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        tau = np.zeros(self._lead + (self.nx, self.ny), dtype=dt)
        self._check(self.lib.lbm_get_tau(self._h, tau.ctypes.data, _DT[tau.dtype]), "lbm_get_tau")
        return tau

    # -- time statistics (lbm_stats_*) -------------------------------------------------------
    def begin_statistics(self, every=0):
        """Start (or restart from zero) the time statistics of u and rho on the device (lbm_stats_begin).  every > 0: step()
        samples by itself at steps_done + every, + 2 every, ...; every = 0: samples only through sample_statistics().  A sample is
        exactly what get_fields() would return after that step.  Not on a slab with every > 0 (sample by hand there)."""
        self._check(self.lib.lbm_stats_begin(self._h, int(every)), "lbm_stats_begin")
        return self

    def sample_statistics(self):
        """Add the fields get_fields() would return now to the statistics (lbm_stats_sample)."""
        self._check(self.lib.lbm_stats_sample(self._h), "lbm_stats_sample")
        return self

    def end_statistics(self):
        """Stop sampling and free the device sums (lbm_stats_end)."""
        self._check(self.lib.lbm_stats_end(self._h), "lbm_stats_end")

    def statistics(self):
        """The time statistics so far, float64, whole-lattice shaped (a slab fills its own rows): u [2,X,Y] and rho [X,Y], the
        means; uu, vv, uv [X,Y], the central moments E[ab] - E[a] E[b] (computed here from the device's means of the products);
        samples, the number of samples.  With no sample yet the arrays are None.  A batch carries a leading [B]."""
        lead = self._lead
        mu = np.zeros(lead + (2, self.nx, self.ny))
        mrho = np.zeros(lead + (self.nx, self.ny))
        sec = np.zeros(lead + (3, self.nx, self.ny))
        n = ctypes.c_longlong(0)
        self._check(self.lib.lbm_stats_get(self._h, mu.ctypes.data, mrho.ctypes.data, sec.ctypes.data, ctypes.byref(n)), "lbm_stats_get")
        if n.value == 0:
            return dict(u=None, rho=None, uu=None, vv=None, uv=None, samples=0)
        ux, uy = mu[..., 0, :, :], mu[..., 1, :, :]
        return dict(u=mu, rho=mrho, uu=sec[..., 0, :, :] - ux * ux, vv=sec[..., 1, :, :] - uy * uy, uv=sec[..., 2, :, :] - ux * uy,
                    samples=int(n.value))

    # -- run monitor (lbm_monitor*, lbm_get_lines) ------------------------------------------------
    def _out_code(self, out_dtype):
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        if dt not in _DT:
            raise ValueError("out_dtype must be float32 or float64")
        return dt, _DT[dt]

    def monitor(self, window=None, exclude=(), probes=(), out_dtype=None):
        """One pass over the lattice on the device (lbm_monitor): the record monitor.host_monitor(*get_fields(out_dtype=...)) would
        give, as a dict -- step, nonfinite, sum_ux, sum_uy, sum_rho, sum_q, max_q, min_q, min_x, min_y and probe [len(probes), 3] --
        without downloading a field.  window (x_lo, x_hi, y_lo, y_hi), half open, global rows (None: the whole lattice); exclude: up
        to 4 boxes in the same form; probes: up to 8 cells (x, y).  A slab reports its own rows (slab.LocalSlabs.monitor combines
        them); a batch returns arrays with a leading [B]."""
        _, code = self._out_code(out_dtype)
        spec = M.make_spec(self.nx, self.ny, code, window, exclude, probes)
        rec = (L.lbm_monitor_record * self.batch)()
        self._check(self.lib.lbm_monitor(self._h, ctypes.byref(spec), rec), "lbm_monitor")
        out = M.records_to_dict(rec, (self.batch,), spec.nprobes)
        return out if self._lead else {k: v[0] for k, v in out.items()}

    def lines(self, x=None, y=None, out_dtype=None):
        """(column, row): ux, uy, rho of column x, [3, Y], and of global row y, [3, X] -- the same bits as get_fields(out_dtype=...)
        [.., x, :] and [.., :, y] (lbm_get_lines).  Defaults: the middle column and row of the reference's centre-line plots,
        int(X / 2) and int(Y / 2).  A slab fills its own rows of the column and returns row = None when it does not own row y; a batch
        carries a leading [B]."""
        dt, code = self._out_code(out_dtype)
        x = int(self.nx / 2) if x is None else int(x)
        y = int(self.ny / 2) if y is None else int(y)
        col = np.zeros(self._lead + (3, self.ny), dtype=dt)
        row = np.zeros(self._lead + (3, self.nx), dtype=dt)
        owns = self.y0 <= y < self.y0 + self.ny_local
        self._check(self.lib.lbm_get_lines(self._h, x, y, col.ctypes.data, row.ctypes.data, code), "lbm_get_lines")
        return col, (row if owns else None)

    def locate_vortices(self, out_dtype=np.float32, first=None):
        """ghia.locate_vortices(get_fields(out_dtype=...)[0], uLB) from two monitor passes: ((x1, y1), (x2, y2)); a batch returns a
        list of such pairs.  first: a record monitor(window=monitor.vortex_window(X, Y)[1], out_dtype=out_dtype) has just returned for
        the same step -- its minimum is the first vortex, and that pass is not repeated."""
        off, win = M.vortex_window(self.nx, self.ny)
        a = self.monitor(window=win, out_dtype=out_dtype) if first is None else first
        if not self._lead:
            loc1 = (int(a["min_x"]), int(a["min_y"]))
            b = self.monitor(window=win, exclude=(M.vortex_box(loc1, off),), out_dtype=out_dtype)
            return loc1, (int(b["min_x"]), int(b["min_y"]))
        out = []
        for i in range(self.batch):   # (the box differs from lattice to lattice: one pass per lattice, each reads its own entry)
            loc1 = (int(a["min_x"][i]), int(a["min_y"][i]))
            b = self.monitor(window=win, exclude=(M.vortex_box(loc1, off),), out_dtype=out_dtype)
            out.append((loc1, (int(b["min_x"][i]), int(b["min_y"][i]))))
        return out

    def begin_monitor(self, every=0, capacity=1024, window=None, exclude=(), probes=(), out_dtype=None):
        """Start (or restart) a series of monitor records on the device (lbm_monitor_begin) with room for `capacity` samples.
        every > 0: step() samples by itself at steps_done + every, + 2 every, ... -- nothing returns to the host before
        monitor_series(); every = 0: samples through sample_monitor() only.  Samples beyond the capacity are dropped and counted.
        Not on a slab with every > 0."""
        _, code = self._out_code(out_dtype)
        spec = M.make_spec(self.nx, self.ny, code, window, exclude, probes)
        self._check(self.lib.lbm_monitor_begin(self._h, ctypes.byref(spec), int(every), int(capacity)), "lbm_monitor_begin")
        self._mon = (int(capacity), spec.nprobes)
        return self

    def sample_monitor(self):
        """Append the record of the fields get_fields() would return now to the series (lbm_monitor_sample)."""
        self._check(self.lib.lbm_monitor_sample(self._h), "lbm_monitor_sample")
        return self

    def _series(self, read, record, to_dict):
        """A record series (lbm_monitor_read / lbm_residual_read) in two calls, the count and then the records: to_dict(records,
        (count, B)) without the [B] axis of a lone lattice, plus count and dropped."""
        n, dropped = ctypes.c_longlong(0), ctypes.c_longlong(0)
        self._check(read(self._h, None, 0, ctypes.byref(n), ctypes.byref(dropped)), read.__name__)
        count = int(n.value)
        rec = (record * (count * self.batch))()
        if count:
            self._check(read(self._h, rec, count, ctypes.byref(n), ctypes.byref(dropped)), read.__name__)
        out = to_dict(rec, (count, self.batch))
        if not self._lead:
            out = {k: v[:, 0] for k, v in out.items()}
        out["count"], out["dropped"] = count, int(dropped.value)
        return out

    def monitor_series(self):
        """The series so far (lbm_monitor_read): the keys of monitor() as arrays [count] (a batch: [count, B]; probe: [count(, B),
        len(probes), 3]), plus count and dropped."""
        _, nprobes = getattr(self, "_mon", (0, 0))
        return self._series(self.lib.lbm_monitor_read, L.lbm_monitor_record, lambda rec, shape: M.records_to_dict(rec, shape, nprobes))

    def end_monitor(self):
        """Stop the series and free its device buffer (lbm_monitor_end)."""
        self._check(self.lib.lbm_monitor_end(self._h), "lbm_monitor_end")

    # -- field residual (lbm_residual_*) --------------------------------------------------------------
    def begin_residual(self, every=0, capacity=1024, out_dtype=None):
        """Start (or restart) the field residual on the device (lbm_residual_begin): every sample is compared with the previous one,
        which stays on the device, and leaves one record -- residual.host_residual of the two get_fields(out_dtype=...) results -- in a
        buffer with room for `capacity` records.  The first sample only fills the snapshot.  every > 0: step() samples by itself at
        steps_done + every, + 2 every, ...; every = 0: samples through sample_residual() only.  Records beyond the capacity are dropped
        and counted; the snapshot is refreshed all the same.  Not on a slab with every > 0 (sample by hand there, and combine the
        slabs' records with residual.combine)."""
        _, code = self._out_code(out_dtype)
        self._check(self.lib.lbm_residual_begin(self._h, code, int(every), int(capacity)), "lbm_residual_begin")
        return self

    def sample_residual(self):
        """Compare the fields get_fields() would return now with the previous sample and keep them as the next one
        (lbm_residual_sample)."""
        self._check(self.lib.lbm_residual_sample(self._h), "lbm_residual_sample")
        return self

    def residual_series(self):
        """The records so far (lbm_residual_read): step, step_prev, cells, nonfinite, sum_du2, sum_u2, sum_drho2, max_du2, max_x, max_y,
        max_drho2 as arrays [count] (a batch: [count, B]), plus count and dropped.  residual.norms() turns them into the usual norms."""
        return self._series(self.lib.lbm_residual_read, L.lbm_residual_record, RS.records_to_dict)

    def end_residual(self):
        """Stop the residual and free its snapshot and records (lbm_residual_end)."""
        self._check(self.lib.lbm_residual_end(self._h), "lbm_residual_end")

    # -- flow topology (lbm_topology, lbm_get_stream_function) -------------------------------------
    def topology(self, windows=(), out_dtype=None):
        """The extrema of the stream function inside up to 8 windows (x_lo, x_hi, y_lo, y_hi), reduced on the device (lbm_topology):
        the record topology.host_topology(get_fields(out_dtype=...)[0], uLB, windows) would give, every bit -- step, closure and per
        window dict(min=..., max=...), each extremum a dict(psi, x, y, omega) -- without downloading a field.  omega is counter-clockwise
        positive (Ghia's table lists -omega).  A batch returns a list of records (the windows are common); not on a slab."""
        _, code = self._out_code(out_dtype)
        spec = T.make_spec(self.nx, self.ny, code, windows)
        rec = (L.lbm_topology_record * self.batch)()
        self._check(self.lib.lbm_topology(self._h, ctypes.byref(spec), rec), "lbm_topology")
        out = T.records_to_dict(rec, spec.nwindows)
        return out if self._lead else out[0]

    def stream_function(self, out_dtype=None):
        """(psi, omega), float64 [X, Y], of the fields get_fields(out_dtype=...) would return, computed on the device
        (lbm_get_stream_function): topology.host_stream_function of those fields, every bit; the extrema topology() reports are
        extrema of this psi.  A batch carries a leading [B]; not on a slab."""
        _, code = self._out_code(out_dtype)
        psi = np.zeros(self._lead + (self.nx, self.ny))
        omega = np.zeros(self._lead + (self.nx, self.ny))
        self._check(self.lib.lbm_get_stream_function(self._h, psi.ctypes.data, omega.ctypes.data, code), "lbm_get_stream_function")
        return psi, omega

    def vortex_table(self, out_dtype=np.float32):
        """Ghia's named vortices from one device record of four windows (topology.vortex_windows, topology.vortex_table): dict
        'Primary' | 'Top' | 'BL1' | 'BR1' -> dict(x, y, psi, omega), or None where the vortex is absent.  A batch returns a list."""
        rec = self.topology(T.vortex_windows(self.nx, self.ny), out_dtype=out_dtype)
        if self._lead:
            return [T.vortex_table(r, self.nx, self.ny) for r in rec]
        return T.vortex_table(rec, self.nx, self.ny)

    # -- solid obstacles (lbm_set_solid, lbm_get_solid, lbm_solid_force) ---------------------------------
    def _mask(self, mask):
        """A mask as the library takes it: uint8 0 / 1, C order, [X, Y] (a batch: [B, X, Y]; one [X, Y] mask serves every lattice)."""
        m = np.asarray(mask) != 0
        if self._lead and m.shape == (self.nx, self.ny):
            m = np.broadcast_to(m, self._lead + m.shape)
        if m.shape != self._lead + (self.nx, self.ny):
            raise ValueError(f"solid mask must have shape {self._lead + (self.nx, self.ny)}")
        return np.ascontiguousarray(m, dtype=np.uint8)

    def _need_solid(self):
        if not self.has_solid:
            raise RuntimeError("this solver has no solid mask: create it with semantics='bounce_back', solid=mask")

    def set_solid(self, mask):
        """A new solid mask (lbm_set_solid): ends every sampler and restarts the lattice from the initial equilibrium, solid cells at
        the rest equilibrium.  Every lattice needs at least one fluid cell."""
        self._need_solid()
        m = self._mask(mask)
        self._check(self.lib.lbm_set_solid(self._h, m.ctypes.data), "lbm_set_solid")
        self._bodies_given = self._motion_given = self._shape_given = False
        return self

    @property
    def solid(self):
        """A copy of the solid mask, bool [X, Y] (a batch: [B, X, Y]); None without solid=..."""
        if not self.has_solid:
            return None
        m = np.zeros(self._lead + (self.nx, self.ny), dtype=np.uint8)
        self._check(self.lib.lbm_get_solid(self._h, m.ctypes.data), "lbm_get_solid")
        return m.astype(bool)

    def solid_force(self):
        """The momentum-exchange force of the fluid on the solid cells, reduced on the device (lbm_solid_force): dict(step, links, fx,
        fy) -- solid.host_force(get_fields(want_fin=True)[2], mask) to the rounding of a double sum; fy > 0 points to the lid, as u[1].
        A batch returns arrays [B].  Not before the first step."""
        self._need_solid()
        rec = (L.lbm_solid_force_record * self.batch)()
        self._check(self.lib.lbm_solid_force(self._h, rec), "lbm_solid_force")
        out = {k: np.array([getattr(r, k) for r in rec]) for k in ("step", "links", "fx", "fy")}
        out["step"], out["links"] = out["step"].astype(np.int64), out["links"].astype(np.int64)
        return out if self._lead else {k: v[0].item() for k, v in out.items()}

    # -- the bodies of the mask (lbm_set_solid_bodies, lbm_get_solid_bodies, lbm_body_force, lbm_force_*) ---------
    def set_bodies(self, labels, centres=None):
        """Split the solid cells into bodies (lbm_set_solid_bodies): labels is an integer array of the mask's shape (one [X, Y] array
        serves every lattice of a batch) with a value in [0, nbodies) on every solid cell, nbodies = the largest label on a solid cell
        + 1 -- or the number of centres where they are given: [nbodies, 2] (a batch: [B, nbodies, 2]) of (x0, y0) in index
        coordinates, the points the torques refer to; None takes each body's centroid.  Ends a running force series; the lattice and
        the step count stay.  set_solid returns to one body that holds every solid cell."""
        self._need_solid()
        lab = np.asarray(labels)
        if self._lead and lab.shape == (self.nx, self.ny):
            lab = np.broadcast_to(lab, self._lead + lab.shape)
        if lab.shape != self._lead + (self.nx, self.ny) or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"body labels must be an integer array of shape {self._lead + (self.nx, self.ny)}")
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        if centres is None:
            on = lab[self.solid]
            n, cen = (int(on.max()) + 1 if on.size else 1), None
        else:
            cen = np.asarray(centres, dtype=np.float64)
            if self._lead and cen.ndim == 2:
                cen = np.broadcast_to(cen, self._lead + cen.shape)
            if cen.ndim != len(self._lead) + 2 or cen.shape[:-2] != self._lead or cen.shape[-1] != 2:
                raise ValueError(f"centres must have shape {self._lead + ('nbodies', 2)}")
            n, cen = cen.shape[-2], np.ascontiguousarray(cen)
        self._check(self.lib.lbm_set_solid_bodies(self._h, lab.ctypes.data, n, None if cen is None else cen.ctypes.data), "lbm_set_solid_bodies")
        self._bodies_given, self._motion_given = True, False      # (a checkpoint then carries them; every body is at rest again)
        return self

    @property
    def nbodies(self):
        """The number of bodies (1 until set_bodies); 0 without solid=..."""
        return int(self.lib.lbm_solid_body_count(self._h))

    @property
    def bodies(self):
        """(labels, centres): copies of the labels, int32 [X, Y] with -1 on fluid cells, and of the centres, float64 [nbodies, 2] (a
        batch: [B, X, Y] and [B, nbodies, 2]); None without solid=..."""
        if not self.has_solid:
            return None
        lab = np.zeros(self._lead + (self.nx, self.ny), dtype=np.int32)
        cen = np.zeros(self._lead + (self.nbodies, 2))
        self._check(self.lib.lbm_get_solid_bodies(self._h, lab.ctypes.data, cen.ctypes.data), "lbm_get_solid_bodies")
        return lab, cen

    def _force_dict(self, rec, shape):
        a = np.frombuffer(rec, dtype=np.float64).reshape(tuple(shape) + (6,)) if len(rec) else np.zeros(tuple(shape) + (6,))
        out = {k: a[..., i].copy() for i, k in enumerate(("step", "body", "links", "fx", "fy", "tz"))}
        for k in ("step", "body", "links"):
            out[k] = out[k].astype(np.int64)
        return out

    def body_force(self):
        """The momentum-exchange force and torque of the fluid on every body, reduced on the device from the link list
        (lbm_body_force): dict(step, body, links, fx, fy, tz) of arrays [nbodies] (a batch: [B, nbodies]) --
        solid.host_body_force(get_fields(want_fin=True)[2], mask, labels, centres) to the rounding of a double sum.  fy > 0 points to
        the lid; tz > 0 turns counter-clockwise in the picture with the lid on top.  Not before the first step."""
        self._need_solid()
        nb = self.nbodies
        rec = (L.lbm_body_force_record * (self.batch * nb))()
        self._check(self.lib.lbm_body_force(self._h, rec), "lbm_body_force")
        out = self._force_dict(rec, (self.batch, nb))
        return out if self._lead else {k: v[0] for k, v in out.items()}

    def begin_force(self, every=0, capacity=1024):
        """Start (or restart) a series of body_force() records on the device (lbm_force_begin) with room for `capacity` samples.
        every > 0: step() samples by itself at steps_done + every, + 2 every, ... -- each record is what body_force() returns at that
        step count, every bit, and nothing returns to the host before force_series(); every = 0: samples through sample_force() only.
        Samples beyond the capacity are dropped and counted.  Not before the first step."""
        self._need_solid()
        self._check(self.lib.lbm_force_begin(self._h, int(every), int(capacity)), "lbm_force_begin")
        return self

    def sample_force(self):
        """Append the record body_force() would return now to the series (lbm_force_sample)."""
        self._check(self.lib.lbm_force_sample(self._h), "lbm_force_sample")
        return self

    def force_series(self):
        """The series so far (lbm_force_read): the keys of body_force() as arrays [count, nbodies] (a batch: [count, B, nbodies]), plus
        count and dropped."""
        nb = self.nbodies
        sample = L.lbm_body_force_record * nb      # one sample of a lattice
        return self._series(self.lib.lbm_force_read, sample, lambda rec, shape: self._force_dict(rec, shape + (nb,)))

    def end_force(self):
        """Stop the series and free its device buffer (lbm_force_end)."""
        self._check(self.lib.lbm_force_end(self._h), "lbm_force_end")

    # -- moving bodies (lbm_set_body_motion, lbm_get_body_motion) --------------------------------------
    def set_body_motion(self, motion):
        """Give the surface of every body a wall velocity (lbm_set_body_motion): motion is [nbodies, 3] (a batch: [B, nbodies, 3], or
        [nbodies, 3] for every lattice) of (Ux, Uy, Om) -- Ux, Uy in the components of u, Om in radians per step, counter-clockwise
        positive in the picture with the lid on top, about the body's centre (set_bodies).  None, or all zero: every body at rest, the
        kernels and the bits of obstacles at rest.  The bodies keep their cells; every link carries Ladd's moving-wall term from the next
        step on.  The lattice, the step count and the samplers stay.  A motion that would pump mass through a wall, or between two touching
        bodies, is refused.  set_solid and set_bodies return every body to rest."""
        self._need_solid()
        if motion is None:
            self._check(self.lib.lbm_set_body_motion(self._h, None), "lbm_set_body_motion")
            self._motion_given = False
            return self
        m = np.asarray(motion, dtype=np.float64)
        nb = self.nbodies
        if self._lead and m.shape == (nb, 3):
            m = np.broadcast_to(m, self._lead + m.shape)
        if m.shape != self._lead + (nb, 3):
            raise ValueError(f"body motion must have shape {self._lead + (nb, 3)}: (Ux, Uy, Om) of every body")
        m = np.ascontiguousarray(m)
        self._check(self.lib.lbm_set_body_motion(self._h, m.ctypes.data), "lbm_set_body_motion")
        self._motion_given = bool(np.any(m))      # (a checkpoint then carries it)
        return self

    @property
    def body_motion(self):
        """A copy of the motion of the bodies, float64 [nbodies, 3] (a batch: [B, nbodies, 3]), all zero at rest; None without solid=..."""
        if not self.has_solid:
            return None
        m = np.zeros(self._lead + (self.nbodies, 3))
        self._check(self.lib.lbm_get_body_motion(self._h, m.ctypes.data), "lbm_get_body_motion")
        return m

    # -- curved surfaces (lbm_set_solid_shape, lbm_get_solid_shape) --------------------------------------
    def set_shape(self, q):
        """Give every link of the mask a wall distance (lbm_set_solid_shape): q is [8, X, Y] (a batch: [B, 8, X, Y], or [8, X, Y] for
        every lattice), plane k - 1 for slot k, on every link the fraction 0 < q <= 1 of the link from the fluid cell to the wall
        (solid.disc_fractions, solid.fractions_from_distance); values off the links are ignored.  The links then bounce by linear
        interpolation, second order for curved walls, instead of half-way -- at the price of the lattice's mass, which a shape does not
        conserve.  None clears the shape.  Only while every body is at rest: the shape first, then set_body_motion.  The lattice, the
        step count and the samplers stay; set_solid drops the shape, set_bodies keeps it."""
        self._need_solid()
        if q is None:
            self._check(self.lib.lbm_set_solid_shape(self._h, None), "lbm_set_solid_shape")
            self._shape_given = False
            return self
        a = np.asarray(q, dtype=np.float64)
        if self._lead and a.shape == (8, self.nx, self.ny):
            a = np.broadcast_to(a, self._lead + a.shape)
        if a.shape != self._lead + (8, self.nx, self.ny):
            raise ValueError(f"the shape must have shape {self._lead + (8, self.nx, self.ny)}: q of slot k in plane k - 1")
        a = np.ascontiguousarray(a)
        self._check(self.lib.lbm_set_solid_shape(self._h, a.ctypes.data), "lbm_set_solid_shape")
        self._shape_given = True      # (a checkpoint then carries it)
        return self

    @property
    def shape(self):
        """A copy of the effective q, float64 [8, X, Y] (a batch: [B, 8, X, Y]): on the links the q in force (1/2 where a link with
        q < 1/2 has no fluid cell behind it), 0 elsewhere; None without a shape."""
        if not self.has_solid or not getattr(self, "_shape_given", False):
            return None
        a = np.zeros(self._lead + (8, self.nx, self.ny))
        self._check(self.lib.lbm_get_solid_shape(self._h, a.ctypes.data), "lbm_get_solid_shape")
        return a

    # -- open boundaries (lbm_set_open_cells, lbm_get_open_cells, lbm_set_wall_velocity, lbm_get_wall_velocity) ---------
    def set_open_cells(self, hold, f=None):
        """Hold cells (lbm_set_open_cells): hold is a mask of the solid mask's shape (one [X, Y] array serves every lattice of a
        batch), f is [9, X, Y] (a batch: [B, 9, X, Y], or [9, X, Y] for every lattice), read on the hold cells only -- for a stream of
        density rho and velocity (ux, uy), solid.equilibrium(rho, ux, uy).  A hold cell is never updated and keeps f_k; it is no wall:
        its neighbours pull from it as from a fluid cell.  It serves as a pressure or far-field outlet, or as a reservoir.  Ends every
        sampler and restarts the lattice from the initial equilibrium, as set_solid does.  None clears.  Geometry comes first: before
        set_shape, set_body_motion and set_wall_velocity.  set_solid drops the hold cells, set_bodies keeps them."""
        self._need_solid()
        if hold is None:
            self._check(self.lib.lbm_set_open_cells(self._h, None, None), "lbm_set_open_cells")
            return self
        h = self._mask(hold)
        a = np.asarray(f, dtype=np.float64)
        if self._lead and a.shape == (9, self.nx, self.ny):
            a = np.broadcast_to(a, self._lead + a.shape)
        if a.shape != self._lead + (9, self.nx, self.ny):
            raise ValueError(f"the held populations must have shape {self._lead + (9, self.nx, self.ny)}")
        a = np.ascontiguousarray(a)
        self._check(self.lib.lbm_set_open_cells(self._h, h.ctypes.data, a.ctypes.data), "lbm_set_open_cells")
        return self

    @property
    def open_cells(self):
        """(hold, f): copies of the hold cells, bool [X, Y], and of their populations, float64 [9, X, Y], zero elsewhere (a batch:
        [B, X, Y] and [B, 9, X, Y]); None without hold cells."""
        if not self.has_solid or self._h is None:
            return None
        h = np.zeros(self._lead + (self.nx, self.ny), dtype=np.uint8)
        self._check(self.lib.lbm_get_open_cells(self._h, h.ctypes.data, None), "lbm_get_open_cells")      # (the library's answer, as wall_velocity)
        if not h.any():
            return None
        f = np.zeros(self._lead + (9, self.nx, self.ny))
        self._check(self.lib.lbm_get_open_cells(self._h, None, f.ctypes.data), "lbm_get_open_cells")
        return h.astype(bool), f

    def set_wall_velocity(self, uw):
        """Give single solid cells a wall velocity (lbm_set_wall_velocity): uw is [2, X, Y] (a batch: [B, 2, X, Y], or [2, X, Y] for
        every lattice), components as u, read on solid cells only.  Every link adds Ladd's term of its source cell's velocity to that of
        its body's motion (set_body_motion), in either order of the two calls: a velocity bounce-back inlet with any profile, a sliding
        side wall.  None, or all zero: no term.  The lattice, the step count and the samplers stay.  On a lattice without hold cells a
        velocity with a net flux is refused, as a motion is; a lattice with hold cells (set_open_cells) is open.  The shape first, then
        velocities.  set_solid resets it, set_bodies keeps it."""
        self._need_solid()
        if uw is None:
            self._check(self.lib.lbm_set_wall_velocity(self._h, None), "lbm_set_wall_velocity")
            return self
        a = np.asarray(uw, dtype=np.float64)
        if self._lead and a.shape == (2, self.nx, self.ny):
            a = np.broadcast_to(a, self._lead + a.shape)
        if a.shape != self._lead + (2, self.nx, self.ny):
            raise ValueError(f"the wall velocity must have shape {self._lead + (2, self.nx, self.ny)}")
        a = np.ascontiguousarray(a)
        self._check(self.lib.lbm_set_wall_velocity(self._h, a.ctypes.data), "lbm_set_wall_velocity")
        return self

    @property
    def wall_velocity(self):
        """A copy of the wall velocity of the solid cells, float64 [2, X, Y] (a batch: [B, 2, X, Y]), zero on every other cell and all
        zero when none is set; None without solid=..."""
        if not self.has_solid:
            return None
        a = np.zeros(self._lead + (2, self.nx, self.ny))
        self._check(self.lib.lbm_get_wall_velocity(self._h, a.ctypes.data), "lbm_get_wall_velocity")
        return a

    # -- periodic sides and the driving force (lbm_set_periodic, lbm_get_periodic, lbm_set_driving_force, lbm_get_driving_force) ---------
    def set_periodic(self, x=False, y=False):
        """Periodic sides (lbm_set_periodic): with x, columns 0 and nx - 1 become images of columns nx - 2 and 1 and the periodic domain is
        columns 1 .. nx - 2; with y the same for rows 0 and ny - 1.  The mask and the body labels must equal their own wrap on the image
        cells (periodic.wrap fills them).  Geometry: it ends every sampler and restarts the lattice from the initial equilibrium, and comes
        before set_shape, set_body_motion and set_wall_velocity.  The exported arrays include the image cells (periodic.interior cuts them
        off).  set_solid clears it; set_open_cells and set_bodies keep it.  set_periodic() restores the closed box."""
        self._need_solid()
        self._check(self.lib.lbm_set_periodic(self._h, int(bool(x)), int(bool(y))), "lbm_set_periodic")
        return self

    @property
    def periodic(self):
        """(x, y): which sides are periodic; None without solid=..."""
        if not self.has_solid or self._h is None:
            return None
        px, py = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self.lib.lbm_get_periodic(self._h, ctypes.byref(px), ctypes.byref(py)), "lbm_get_periodic")
        return bool(px.value), bool(py.value)

    def set_driving_force(self, fx, fy):
        """A uniform driving force (lbm_set_driving_force): (fx, fy) is the force density per cell, components as u.  Every collision of
        a cell that is neither solid nor held adds (3 w_k) (cx_k fx + cy_k fy) to its post-collision population of direction k.  The
        lattice, the step count and the samplers stay; every lattice of a batch takes the same force.  The exported u is the bare moment:
        the physical velocity is periodic.velocity(u, rho, (fx, fy)).  (0, 0): no force."""
        self._check(self.lib.lbm_set_driving_force(self._h, float(fx), float(fy)), "lbm_set_driving_force")
        return self

    @property
    def driving_force(self):
        """(fx, fy) as set; (0.0, 0.0) without a force."""
        fx, fy = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self.lib.lbm_get_driving_force(self._h, ctypes.byref(fx), ctypes.byref(fy)), "lbm_get_driving_force")
        return fx.value, fy.value

    # -- sub-grid viscosity (lbm_set_subgrid, lbm_get_subgrid) ------------------------------------------------------------------
    def set_subgrid(self, cs2=0.025):
        """The local Smagorinsky closure of an obstacle lattice (lbm_set_subgrid; solid=..., one step per launch): every collision of a
        cell that is neither solid nor held takes the rate 1 / tau, tau = (tau0 + sqrt(tau0^2 + 18 sqrt(2) cs2 |P| / rho)) / 2, |P| the
        norm of the cell's whole non-equilibrium momentum flux -- nu_t = cs2 |S|.  No history: the lattice, the step count and the
        samplers stay; every lattice of a batch takes the same constant with its own tau0.  A passive scalar keeps its molecular
        diffusivity; with buoyancy the call is refused.  get_tau() returns the field.  0: no closure."""
        self._check(self.lib.lbm_set_subgrid(self._h, float(cs2)), "lbm_set_subgrid")
        return self

    @property
    def subgrid(self):
        """The sub-grid constant as set; 0.0 without the closure."""
        cs2 = ctypes.c_double(0.0)
        self._check(self.lib.lbm_get_subgrid(self._h, ctypes.byref(cs2)), "lbm_get_subgrid")
        return cs2.value

    # -- per-cell relaxation rates: a viscosity field (lbm_set_relaxation_field, lbm_get_relaxation_field) -----------------------
    def _rate_cells(self, a, name):
        a = np.asarray(a, dtype=np.float64)
        if self._lead and a.shape == (self.nx, self.ny):
            a = np.broadcast_to(a, self._lead + a.shape)
        if a.shape != self._lead + (self.nx, self.ny):
            raise ValueError(f"{name} must have shape {self._lead + (self.nx, self.ny)}")
        return np.ascontiguousarray(a)

    def set_relaxation_field(self, omega, omegam=None):
        """Per-cell relaxation rates of an obstacle lattice (lbm_set_relaxation_field; solid=..., one step per launch): omega[X, Y]
        ([B, X, Y], or [X, Y] for every lattice of a batch) is the viscous rate of each cell -- SRT's omega, TRT's omega+, MRT's
        omega_nu -- and omegam, the same shape, TRT's omega- (None: the lattice's; a TRT solver only).  Every value in (0, 2).  The
        lattice, the step count and the samplers stay; the field survives set_solid, set_relaxation and the other setters.  With
        set_subgrid the closure's tau0 is 1 / omega of the cell.  A passive scalar keeps its own diffusivity; with buoyancy the call
        is refused.  omega=None clears the field: the kernels and the bits of a solver without one."""
        if omega is None:
            if omegam is not None:
                raise ValueError("omegam without omega")
            self._check(self.lib.lbm_set_relaxation_field(self._h, None, None), "lbm_set_relaxation_field")
            return self
        w = self._rate_cells(omega, "omega")
        wm = None if omegam is None else self._rate_cells(omegam, "omegam")
        self._check(self.lib.lbm_set_relaxation_field(self._h, w.ctypes.data, None if wm is None else wm.ctypes.data), "lbm_set_relaxation_field")
        return self

    @property
    def relaxation_field(self):
        """(omega, omegam) as the device holds them (rounded to the lattice type), omegam None without that plane; None without a field."""
        if self._h is None:
            return None
        w = np.zeros(self._lead + (self.nx, self.ny))
        wm = np.full(self._lead + (self.nx, self.ny), np.nan)
        rc = self.lib.lbm_get_relaxation_field(self._h, w.ctypes.data, wm.ctypes.data)
        if rc == 0:
            return None
        if rc != 1:
            self._check(rc, "lbm_get_relaxation_field")
        return w, (None if np.isnan(wm).all() else wm)

    def set_viscosity(self, nu, magic=None):
        """The viscosity of each cell in lattice units, nu[X, Y] or [B, X, Y] ([X, Y] is broadcast over a batch): omega = 1 / (3 nu +
        1/2) (viscosity.rates).  magic=L on a TRT solver: omega- = 1 / (1/2 + L / (3 nu)) per cell as well, so that the magic parameter
        (1/omega+ - 1/2)(1/omega- - 1/2) = L holds in every cell.  None clears the field."""
        if nu is None:
            return self.set_relaxation_field(None)
        from .viscosity import rates
        return self.set_relaxation_field(*rates(nu, magic))

    # -- shear-dependent viscosity: a rheology table (lbm_set_rheology, lbm_get_rheology, lbm_get_shear) ---------------------------
    def set_rheology(self, omega, omegam=None, g_max=None):
        """A generalised Newtonian fluid on an obstacle lattice (lbm_set_rheology; solid=..., one step per launch): omega[n], 2 <= n <=
        65536, is the viscous rate -- SRT's omega, TRT's omega+, MRT's omega_nu -- at the shears g_i = i g_max / (n - 1), g = |deviatoric
        non-equilibrium momentum flux| / rho of a cell (get_shear), and omegam[n] TRT's omega- there (None: the lattice's; a TRT solver
        only).  Every value in (0, 2); between entries the rates are interpolated linearly, beyond g_max the table holds its last entry.
        rheology.table builds both arrays from a law nu(gdot).  One table for every lattice of a batch.  The lattice, the step count and
        the samplers stay; the table survives set_solid and the other setters.  With buoyancy, set_subgrid or a relaxation field the call
        is refused, and they refuse while a table is set.  omega=None clears the table: the kernels and the bits of a solver without one."""
        if omega is None:
            if omegam is not None:
                raise ValueError("omegam without omega")
            self._check(self.lib.lbm_set_rheology(self._h, None, None, 0, 0.0), "lbm_set_rheology")
            return self
        if g_max is None:
            raise ValueError("set_rheology needs g_max, the shear of the table's last entry")
        w = np.ascontiguousarray(omega, dtype=np.float64)
        wm = None if omegam is None else np.ascontiguousarray(omegam, dtype=np.float64)
        if w.ndim != 1 or (wm is not None and wm.shape != w.shape):
            raise ValueError("omega (and omegam) must be one-dimensional arrays of one length")
        self._check(self.lib.lbm_set_rheology(self._h, w.ctypes.data, None if wm is None else wm.ctypes.data, int(w.size), float(g_max)),
                    "lbm_set_rheology")
        return self

    @property
    def rheology(self):
        """(omega, omegam, g_max) as the device holds the table (rounded to the lattice type), omegam None without it; None without a
        table."""
        if self._h is None:
            return None
        n, g_max = ctypes.c_int(0), ctypes.c_double(0.0)
        rc = self.lib.lbm_get_rheology(self._h, None, None, ctypes.byref(n), ctypes.byref(g_max))
        if rc == 0:
            return None
        if rc != 1:
            self._check(rc, "lbm_get_rheology")
        w, wm = np.zeros(n.value), np.full(n.value, np.nan)
        self._check(self.lib.lbm_get_rheology(self._h, w.ctypes.data, wm.ctypes.data, None, None) - 1, "lbm_get_rheology")
        return w, (None if np.isnan(wm).all() else wm), g_max.value

    def get_shear(self, out_dtype=None):
        """g[X, Y] ([B, X, Y]) of the current state (lbm_get_shear): the Frobenius norm of the deviatoric non-equilibrium momentum flux
        over rho, what a rheology table is indexed with; 0 on solid and hold cells.  Works without a table too (solid=... only).  The
        shear rate is rheology.shear_rate(g, tau)."""
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        g = np.zeros(self._lead + (self.nx, self.ny), dtype=dt)
        self._check(self.lib.lbm_get_shear(self._h, g.ctypes.data, _DT[g.dtype]), "lbm_get_shear")
        return g

    # -- a passive scalar: temperature or dye (lbm_scalar_*) ---------------------------------------------------------------
    def _cells(self, a, name, fill=None):
        """A float64 [X, Y] array as the scalar calls take it; a number fills the lattice."""
        a = np.asarray(fill if a is None else a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((self.nx, self.ny), float(a))
        if a.shape != (self.nx, self.ny):
            raise ValueError(f"{name} must be a number or an array of shape {(self.nx, self.ny)}")
        return np.ascontiguousarray(a)

    def begin_scalar(self, D, c0=0.0, magic=0.25, wall_value=None, hold_value=None):
        """Start a passive scalar C (lbm_scalar_begin) that every later flow step carries along: advected by the exported velocity,
        diffusing with the diffusivity D (lattice units; TRT with the product `magic`, BGK is magic = (3 D)**2).  c0: the initial values,
        a number or [X, Y].  wall_value: [X, Y] with the value a solid cell holds (Dirichlet, anti-bounce-back) and NaN on adiabatic
        cells; None: every wall is adiabatic, as the box edges and the lid always are.  hold_value: a number or [X, Y], what the user's
        hold cells (set_open_cells) hold; None: their initial values.  One lattice with solid=..., one step per launch.  set_solid,
        set_open_cells and set_periodic end the scalar; set_state and init_equilibrium keep it.  Replaces an active scalar."""
        self._need_solid()
        if self._lead:
            raise RuntimeError("the scalar knows no batches")
        c0 = self._cells(c0, "c0")
        flag = value = None
        if wall_value is not None:
            wv = self._cells(wall_value, "wall_value")
            flag = np.ascontiguousarray(~np.isnan(wv), dtype=np.uint8)
            value = np.ascontiguousarray(np.where(flag != 0, wv, 0.0))
        hv = None if hold_value is None else self._cells(hold_value, "hold_value")
        self._check(self.lib.lbm_scalar_begin(self._h, float(D), float(magic), c0.ctypes.data, None if flag is None else flag.ctypes.data,
                                              None if value is None else value.ctypes.data, None if hv is None else hv.ctypes.data),
                    "lbm_scalar_begin")
        self._scalar_given = dict(scalar_c0=c0, **({} if wall_value is None else dict(scalar_wall_value=wv)),
                                  **({} if hv is None else dict(scalar_hold_value=hv)))
        return self

    def end_scalar(self):
        """End the scalar (lbm_scalar_end): the flow steps, and describe(), are then those of a solver that never had one."""
        self._check(self.lib.lbm_scalar_end(self._h), "lbm_scalar_end")
        self._scalar_given = None
        return self

    @property
    def scalar_active(self):
        """None, or dict(D, magic) of the active scalar."""
        if self._h is None:
            return None
        D, m = ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = self.lib.lbm_scalar_active(self._h, ctypes.byref(D), ctypes.byref(m))
        if rc < 0:
            self._check(rc, "lbm_scalar_active")
        return dict(D=D.value, magic=m.value) if rc else None

    def scalar(self, out_dtype=None):
        """C[X, Y] of the state the last scalar step started from (the one-step lag of get_fields: C and u of one moment belong to the
        same iteration); zero on solid cells.  Image cells of periodic sides included (scalar.interior cuts them off)."""
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        C = np.zeros((self.nx, self.ny), dtype=dt)
        self._check(self.lib.lbm_scalar_get(self._h, C.ctypes.data, None, _DT[dt]), "lbm_scalar_get")
        return C

    def scalar_populations(self, stored=False, out_dtype=None):
        """g[9, X, Y]: the arriving populations of the current state (what the next scalar step gathers; set_scalar_state of them continues
        the run bit for bit), or, stored=True, the post-collision populations as the lattice holds them."""
        dt = self.dtype if out_dtype is None else np.dtype(out_dtype)
        g = np.zeros((9, self.nx, self.ny), dtype=dt)
        if stored:
            self._check(self.lib.lbm_scalar_get_stored(self._h, g.ctypes.data, _DT[dt]), "lbm_scalar_get_stored")
        else:
            self._check(self.lib.lbm_scalar_get(self._h, None, g.ctypes.data, _DT[dt]), "lbm_scalar_get")
        return g

    def set_scalar_state(self, g):
        """Upload plain scalar populations g[9, X, Y] (lbm_scalar_set_state); the next scalar step is raw, as the flow's after set_state."""
        g = self._host(g, (9, self.nx, self.ny), "g")
        self._check(self.lib.lbm_scalar_set_state(self._h, g.ctypes.data, _DT[g.dtype]), "lbm_scalar_set_state")
        return self

    def scalar_totals(self):
        """dict(step, cells, sum, min, max) of scalar() over the cells that are neither solid nor images, reduced on the device in double."""
        rec = L.lbm_scalar_record()
        self._check(self.lib.lbm_scalar_totals(self._h, ctypes.byref(rec)), "lbm_scalar_totals")
        return dict(step=int(rec.step), cells=int(rec.cells), sum=rec.sum, min=rec.min, max=rec.max)

    def scalar_flux(self):
        """The scalar that enters the fluid per step from each body (lbm_scalar_flux): dict(step, links, flux) of arrays [nbodies]; zero on
        adiabatic bodies.  Not before the first scalar step."""
        self._need_solid()
        rec = (L.lbm_scalar_flux_record * self.nbodies)()
        self._check(self.lib.lbm_scalar_flux(self._h, rec), "lbm_scalar_flux")
        return dict(step=np.array([int(r.step) for r in rec]), links=np.array([int(r.links) for r in rec]), flux=np.array([r.flux for r in rec]))

    # -- Boussinesq buoyancy: the scalar acts on the flow (lbm_set_buoyancy, lbm_get_buoyancy) ------------------------------------
    def set_buoyancy(self, ax, ay, c_ref=0.0):
        """Let the scalar act on the flow (lbm_set_buoyancy): (ax, ay) is the acceleration per unit of C, components as u -- hot fluid
        rising toward the lid row y = 0 is ay > 0.  Every collision of a cell that is neither solid nor held adds
        F_k + B_k (C - c_ref), B_k = (3 w_k) (cx_k ax + cy_k ay), to its post-collision population of direction k; C is what scalar()
        returns at that moment.  Needs an active scalar; no shape.  The lattices, the step counts and the samplers stay.  The exported u is
        the bare moment: the physical velocity is convection.velocity(u, rho, C, (ax, ay), c_ref).  (0, 0): no buoyancy."""
        self._check(self.lib.lbm_set_buoyancy(self._h, float(ax), float(ay), float(c_ref)), "lbm_set_buoyancy")
        return self

    @property
    def buoyancy(self):
        """None, or (ax, ay, c_ref) as set."""
        if self._h is None:
            return None
        ax, ay, cr = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = self.lib.lbm_get_buoyancy(self._h, ctypes.byref(ax), ctypes.byref(ay), ctypes.byref(cr))
        if rc < 0:
            self._check(rc, "lbm_get_buoyancy")
        return (ax.value, ay.value, cr.value) if rc else None

    def _scalar_entry(self):
        """What a checkpoint says of the scalar: nothing without one (the file of such a run is what it was), else its parameters, the
        arrays begin_scalar took and the arriving populations; with buoyancy its three numbers and the plane (scalar(): the C the next
        flow step reads)."""
        act = self.scalar_active if self.has_solid and not self._lead else None
        if act is None:
            return {}
        by = self.buoyancy
        return dict(scalar_D=act["D"], scalar_magic=act["magic"], scalar_g=self.scalar_populations(), **(getattr(self, "_scalar_given", None) or {}),
                    **({} if by is None else dict(buoyancy=np.array(by), buoyancy_plane=self.scalar())))

    # -- checkpoint / restart (the reference has neither) -------------------
    def save_checkpoint(self, path):
        """Write the populations and the run parameters to `path` (.npz).  Restarting from it continues bit-identically
        (the state of the scheme is `fin`); with turb = 1 the one-step Smagorinsky history restarts from the state.  The time
        statistics (begin_statistics) are not part of a checkpoint, and load_checkpoint ends them."""
        u, rho, fin = self.get_fields(want_fin=True)
        path = _npz(path)
        np.savez(path, fin=fin, steps_done=self.steps_done, nx=self.nx, ny=self.ny, Re=self.Re, RT=self.RT, uLB=self.uLB,
                 semantics=self.semantics, dtype=self.dtype.name, rows=np.array([self.y0, self.ny_local]), turb=self.turb, u=u, rho=rho,
                 arith=self.arith, **(dict(solid=self.solid) if self.has_solid else {}),
                 **{**(dict(zip(("body_labels", "body_centres"), self.bodies)) if getattr(self, "_bodies_given", False) else {}),
                    **self._motion_entry(), **self._shape_entry(), **self._open_entry(), **self._scalar_entry()})
        return path

    def _open_entry(self):
        """What a checkpoint says of the open boundaries: nothing without them (the file of such a run is what it was), else the hold
        cells with their populations, and the wall velocity of the solid cells."""
        out = {}
        oc = self.open_cells if self.has_solid else None
        if oc is not None:
            out.update(open_hold=oc[0], open_f=oc[1])
        uw = self.wall_velocity if self.has_solid and self._h is not None else None
        if uw is not None and uw.any():
            out.update(wall_velocity=uw)
        per = self.periodic
        if per is not None and any(per):
            out.update(periodic=np.array(per))
        if self._h is not None and any(self.driving_force):
            out.update(driving_force=np.array(self.driving_force))
        if self._h is not None and self.subgrid > 0.0:
            out.update(subgrid=np.float64(self.subgrid))
        rf = self.relaxation_field if self.has_solid else None
        if rf is not None:
            out.update(relax_omega=rf[0], **({} if rf[1] is None else dict(relax_omegam=rf[1])))
        rh = self.rheology if self.has_solid else None
        if rh is not None:
            out.update(rheology_omega=rh[0], rheology_gmax=np.float64(rh[2]), **({} if rh[1] is None else dict(rheology_omegam=rh[1])))
        return out

    def _shape_entry(self):
        """What a checkpoint says of the shape: nothing without one (the file of such a run is what it was), else the effective q."""
        q = self.shape if self.has_solid else None
        return {} if q is None else dict(solid_shape=q)

    def _motion_entry(self):
        """What a checkpoint says of the bodies' motion: nothing at rest (the file of a run without it is what it was), else the
        motion with the labels and centres it refers to."""
        if not getattr(self, "_motion_given", False):
            return {}
        m = self.body_motion
        lab, cen = self.bodies
        return dict(body_motion=m, body_labels=lab, body_centres=cen)

    def load_checkpoint(self, path, strict=True):
        """Upload the populations of a checkpoint written by save_checkpoint; returns the number of steps the checkpointed
        run had done.  The lattice size must match; with `strict` (default) so must dtype, semantics, collision operator,
        closure and Reynolds number -- a continuation is bit-identical only then -- and, where either side is 'promoted', the
        arithmetic (strict and fast states mix as before; a checkpoint without the key counts as strict) and the solid mask (none on either
        side, or the same cells; without `strict` the populations are uploaded under this solver's own mask).  The array is the whole lattice, so a slab
        may restart from a checkpoint of the undivided lattice (each context reads its own rows) but not from another slab's.
        A file that carries a sub-grid constant sets it and clears a buoyancy this solver had set (the two refuse each other); a file
        without one clears the constant.  A relaxation field (set_relaxation_field) likewise: a file with one sets both arrays and clears
        this solver's buoyancy, a file without one clears the field.  A rheology table (set_rheology) likewise: a file with one sets it
        (and clears this solver's buoyancy), a file without one clears the table."""
        with np.load(_npz(path), allow_pickle=False) as z:
            if int(z["nx"]) != self.nx or int(z["ny"]) != self.ny:
                raise ValueError("checkpoint lattice size differs")
            rows = tuple(int(v) for v in z["rows"]) if "rows" in z else (0, self.ny)
            if rows != (0, self.ny) and rows != (self.y0, self.ny_local):
                raise ValueError(f"checkpoint holds rows {rows} only, this context needs {(self.y0, self.ny_local)}")
            if strict:
                have = dict(dtype=str(z["dtype"]), semantics=str(z["semantics"]), RT=str(z["RT"]), Re=float(z["Re"]), uLB=float(z["uLB"]),
                            turb=int(z["turb"]) if "turb" in z else self.turb)
                want = dict(dtype=self.dtype.name, semantics=self.semantics, RT=self.RT, Re=self.Re, uLB=self.uLB, turb=self.turb)
                diff = {k: (have[k], want[k]) for k in want if have[k] != want[k]}
                arith = str(z["arith"]) if "arith" in z else "strict"
                if "promoted" in (arith, self.arith) and arith != self.arith:
                    diff["arith"] = (arith, self.arith)
                mask = np.asarray(z["solid"], dtype=bool) if "solid" in z else None
                if (mask is None) != (not self.has_solid) or (mask is not None and not np.array_equal(mask, self.solid)):
                    diff["solid"] = ("none" if mask is None else f"{int(mask.sum())} solid cells",
                                     f"{int(self.solid.sum())} solid cells" if self.has_solid else "none")
                if diff:
                    raise ValueError(f"checkpoint was written by a different run (checkpoint, this solver): {diff}")
            same_mask = self.has_solid and "solid" in z and np.array_equal(np.asarray(z["solid"], dtype=bool), self.solid)
            if same_mask and self._h is not None and self.wall_velocity.any():     # (this solver's own velocity goes first: it would stand in the
                self.set_wall_velocity(None)                                      # flux check of every call below)
            per = tuple(bool(v) for v in z["periodic"]) if same_mask and "periodic" in z else (False, False)
            if same_mask and self.periodic is not None and per != self.periodic:      # (geometry first, as the hold cells: the periodic sides)
                self.set_body_motion(None)
                self.set_shape(None)
                if not any(per):
                    self.set_periodic()
                else:
                    self.set_open_cells(None)                                       # (a hold cell of this solver's may sit on an image cell)
                    self.set_periodic(*per)
            if same_mask and ("open_hold" in z or self.open_cells is not None):     # (geometry first: it restarts the lattice, so before the state)
                self.set_body_motion(None)
                self.set_shape(None)
                self.set_open_cells(*((np.asarray(z["open_hold"]), np.asarray(z["open_f"])) if "open_hold" in z else (None,)))
            self.set_state(np.ascontiguousarray(z["fin"]))
            if same_mask and ("solid_shape" in z or self.shape is not None):     # (the shape first, then the motion)
                self.set_body_motion(None)
                self.set_shape(np.where(np.asarray(z["solid_shape"]) > 0.0, z["solid_shape"], 0.5) if "solid_shape" in z else None)
            uw = np.asarray(z["wall_velocity"]) if same_mask and "wall_velocity" in z else None
            if "body_labels" in z and self.has_solid and np.array_equal(np.asarray(z["solid"], dtype=bool), self.solid):
                self.set_bodies(np.asarray(z["body_labels"]), np.asarray(z["body_centres"]))     # (files without them: the bodies stay)
                if "body_motion" in z:
                    # The two halves of the wall velocity are two calls, each with the flux check of a closed lattice: the motion
                    # first, and where it is refused on its own, the cells' velocity first.  A pair of which neither half is closed
                    # alone (only their sum is) cannot be set by two calls and is refused here as it was when it was first set.
                    try:
                        self.set_body_motion(np.asarray(z["body_motion"]))
                    except RuntimeError:
                        if uw is None:
                            raise
                        self.set_wall_velocity(uw)
                        self.set_body_motion(np.asarray(z["body_motion"]))
                        uw = None
            if uw is not None:
                self.set_wall_velocity(uw)
            if "driving_force" in z or (self._h is not None and any(self.driving_force)):      # (the force last: it is no geometry)
                self.set_driving_force(*(np.asarray(z["driving_force"]) if "driving_force" in z else (0.0, 0.0)))
            if "rheology_omega" not in z and self.has_solid and self.rheology is not None:      # (first: the table would refuse the two below)
                self.set_rheology(None)
            cs2 = float(z["subgrid"]) if "subgrid" in z else 0.0      # (the sub-grid constant: no geometry, no history)
            if cs2 > 0.0 or (self._h is not None and self.subgrid > 0.0):
                if cs2 > 0.0 and self.buoyancy is not None:      # (this solver's own buoyancy would refuse the constant)
                    self.set_buoyancy(0.0, 0.0)
                self.set_subgrid(cs2)
            if "relax_omega" in z:      # (the relaxation field: no geometry, no history)
                if self.buoyancy is not None:
                    self.set_buoyancy(0.0, 0.0)
                self.set_relaxation_field(np.asarray(z["relax_omega"]), np.asarray(z["relax_omegam"]) if "relax_omegam" in z else None)
            elif self.has_solid and self.relaxation_field is not None:
                self.set_relaxation_field(None)
            if "rheology_omega" in z:      # (the rheology table: no geometry, no history; a file carries it with neither of the two above)
                if self.buoyancy is not None:
                    self.set_buoyancy(0.0, 0.0)
                self.set_rheology(np.asarray(z["rheology_omega"]), np.asarray(z["rheology_omegam"]) if "rheology_omegam" in z else None,
                                  float(z["rheology_gmax"]))
            if same_mask and "scalar_g" in z:      # (the scalar last: the geometry calls above end one; a file without it leaves this solver's as it is)
                self.begin_scalar(float(z["scalar_D"]), np.asarray(z["scalar_c0"]), float(z["scalar_magic"]),
                                  np.asarray(z["scalar_wall_value"]) if "scalar_wall_value" in z else None,
                                  np.asarray(z["scalar_hold_value"]) if "scalar_hold_value" in z else None)
                self.set_scalar_state(np.ascontiguousarray(z["scalar_g"]))
                if "buoyancy" in z:      # (after the state: the plane is the C the checkpointed run would have read next)
                    self.set_buoyancy(*np.asarray(z["buoyancy"]))
                    plane = np.ascontiguousarray(z["buoyancy_plane"])
                    self._check(self.lib.lbm_set_buoyancy_plane(self._h, plane.ctypes.data, _DT[plane.dtype]), "lbm_set_buoyancy_plane")
                elif self.buoyancy is not None:
                    self.set_buoyancy(0.0, 0.0)
            return int(z["steps_done"])

    # -- slab exchange primitives ---------------------------------------------------------
    def halo_elems(self):
        return int(self.lib.lbm_halo_elems(self._h))

    def halo_export(self, side, ptr):
        self._check(self.lib.lbm_halo_export(self._h, int(side), ctypes.c_void_p(ptr)), "lbm_halo_export")

    def halo_import(self, side, ptr):
        self._check(self.lib.lbm_halo_import(self._h, int(side), ctypes.c_void_p(ptr)), "lbm_halo_import")

    def step_edges(self):
        self._check(self.lib.lbm_step_edges(self._h), "lbm_step_edges")

    def step_interior(self):
        self._check(self.lib.lbm_step_interior(self._h), "lbm_step_interior")

    def step_finish(self):
        self._check(self.lib.lbm_step_finish(self._h), "lbm_step_finish")

    # multi-step launch units between slabs: S complete rows per side before the unit, no communication inside it
    def halo_rows_elems(self, nrows):
        return int(self.lib.lbm_halo_rows_elems(self._h, int(nrows)))

    def halo_export_rows(self, side, nrows, ptr):
        self._check(self.lib.lbm_halo_export_rows(self._h, int(side), int(nrows), ctypes.c_void_p(ptr)), "lbm_halo_export_rows")

    def halo_import_rows(self, side, nrows, ptr):
        self._check(self.lib.lbm_halo_import_rows(self._h, int(side), int(nrows), ctypes.c_void_p(ptr)), "lbm_halo_import_rows")

    def step_unit(self, unit_steps):
        self._check(self.lib.lbm_step_unit(self._h, int(unit_steps)), "lbm_step_unit")

    def comm_init(self, nranks, rank, uid_bytes):
        _one_rccl()
        buf = ctypes.create_string_buffer(bytes(uid_bytes), 128)
        self._check(self.lib.lbm_comm_init(self._h, int(nranks), int(rank), buf), "lbm_comm_init")

    def comm_loopback(self):
        """Diagnostic: run lbm_step's RCCL exchange path on one GPU (the slab is its own periodic neighbour)."""
        _one_rccl()
        self._check(self.lib.lbm_comm_loopback(self._h), "lbm_comm_loopback")

    def fma_rate(self, ms=20.0):
        """About `ms` milliseconds of packed fp32 FMAs on every CU; achieved TFLOP/s (lbm_fma_rate)."""
        g = ctypes.c_double(0.0)
        self._check(self.lib.lbm_fma_rate(self._h, float(ms), ctypes.byref(g)), "lbm_fma_rate")
        return g.value

    def copy_bandwidth(self, nbytes=1 << 30, iters=10):
        g = ctypes.c_double(0.0)
        self._check(self.lib.lbm_copy_bandwidth(self._h, int(nbytes), int(iters), ctypes.byref(g)), "lbm_copy_bandwidth")
        return g.value


class CavityBatch(CavitySolver):
    """B independent cavities of the same size and scheme, one per Reynolds number, advanced by the same launches -- the
    sweep MRT_GPU_datagen.py:55-57 runs one lattice after the other.  Host arrays carry a leading [B] axis:
    fin[B,9,X,Y], u[B,2,X,Y], rho[B,X,Y].  Every lattice evolves exactly as it would alone."""

    def __init__(self, xsize, ysize, Re_list, **kw):
        self.Re_list = [float(r) for r in Re_list]
        if not self.Re_list:
            raise ValueError("Re_list is empty")
        for bad in ("rows", "batch"):
            if kw.get(bad) is not None:
                raise ValueError(f"CavityBatch does not take `{bad}`")
        self._lead = (len(self.Re_list),)
        super().__init__(xsize, ysize, self.Re_list[0], batch=len(self.Re_list), **kw)
        self.relax_list = [self.set_relaxation(i, Re=r) for i, r in enumerate(self.Re_list)]

    def save_checkpoint(self, path):
        raise NotImplementedError("checkpoint the lattices of a batch one by one through get_fields / set_state")

    load_checkpoint = save_checkpoint


def _params(nx, ny, y0, ny_local, dtype, RT, semantics, kernel, turb, device, layout, batch, arith, min_rows, tuning, uLB, relax):
    """lbm_params of include/lbm.h from the Python-level arguments."""
    p = L.lbm_params()
    p.struct_size = ctypes.sizeof(L.lbm_params)
    p.nx, p.ny, p.y0, p.ny_local = int(nx), int(ny), int(y0), int(ny_local)
    p.dtype, p.collision = _DT[np.dtype(dtype)], _COLL[RT]
    p.semantics = L.LBM_SEM_BOUNCE_BACK_SOLID if semantics == _SEM_SOLID else _SEM[semantics]
    p.kernel, p.turb, p.device = _KERNEL[kernel], int(turb), int(device)
    p.layout = _LAYOUT[layout]
    p.batch = int(batch)
    if arith not in _ARITH:
        raise ValueError("arith must be 'strict', 'fast' or 'promoted'")
    p.arith = _ARITH[arith]
    p.ny_local_min = 0 if min_rows is None else int(min_rows)
    p.tb_steps, p.frame_seg, p.flags = _tuning(tuning)
    p.uLB = float(uLB)
    p.omega, p.omegam = relax["omega"], relax["omegam"]
    p.omega_e, p.omega_eps, p.omega_q = relax["omega_e"], relax["omega_eps"], relax["omega_q"]
    return p


def launch_plan(xsize, ysize, Re, steps=0, ncu=0, RT="MRT", uLB=0.08, semantics="mrt_gpu", dtype=np.float32, turb=0, rows=None,
                kernel="auto", layout="auto", batch=1, arith="strict", min_rows=None, tuning=None, solid=False):
    """Dry run (lbm_plan, NO GPU needed): the launch plan lbm_create would derive for these arguments -- the dict of
    CavitySolver.describe() -- plus `units`, the launch units step(steps) would run from a fresh lattice.  All ranks of a slab
    decomposition must agree on kernel / steps_per_launch / frame / deep_halo and on the units: a launcher (bench.py --gpus N) and
    the CPU tests check that before any rank touches a device.  solid=True: the plan of the same arguments with a solid mask (solid=... of
    CavitySolver; semantics='bounce_back' only)."""
    if solid:
        if semantics != "bounce_back":
            raise ValueError("solid=True needs semantics='bounce_back'")
        semantics = _SEM_SOLID
    ny = int(ysize)
    y0, nyl = (0, ny) if rows is None else (int(rows[0]), int(rows[1]))
    relax = relaxation(float(Re), ny, float(uLB), 1.0 if semantics == "mrt_py" else 1.2, 1.2)
    p = _params(xsize, ny, y0, nyl, dtype, RT, semantics, kernel, turb, 0, layout, batch, arith, min_rows, tuning, uLB, relax)
    buf = ctypes.create_string_buffer(1024 + 2 * max(int(steps), 0))   # (the plan, then at most "1," per step)
    rc = L.lib().lbm_plan(ctypes.byref(p), int(ncu), int(steps), buf, len(buf))
    text = buf.value.decode()
    if rc < 0:
        raise RuntimeError("lbm_plan: " + text)
    out = {}
    for kv in text.split():
        k, v = kv.split("=", 1)
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    out["units"] = [int(x) for x in str(out.get("units", "")).split(",") if x != ""]
    return out


def _npz(path):
    """np.savez appends '.npz' to a name without it; use one spelling for writing and reading."""
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


def _one_rccl():
    """PyTorch before RCCL -- belt and braces since r03.  r02: a process that created a communicator through the library and imported
    torch only AFTERWARDS aborted in exit() ("double free or corruption").  r03 found the cause and fixed it in the library
    (lbm_comm.hip, rccl()): RCCL had been opened RTLD_GLOBAL, which put its dependency librocm_smi64 into the global symbol scope, and a
    library mapped later that defines the same namespace-scope std::map<amd::smi::DevInfoTypes, const char*> (the wheel's librocm_smi64,
    /opt/rocm's libamd_smi.so) bound its initialiser and destructor to that one object: destroyed twice (backtraces
    profiles/r03_logs/rc134_gdb.log, rc134_gdb2.log; after the fix every order exits 0: rccl_order_r03.log).  RCCL is now opened
    RTLD_LOCAL and taken from the directory of the HIP runtime in use.  Importing torch first, where it is installed, costs nothing:
    processes that use this path exchange the communicator id through torch.distributed anyway."""
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def comm_unique_id():
    _one_rccl()
    buf = ctypes.create_string_buffer(128)
    if L.lib().lbm_comm_unique_id(buf) != 0:
        raise RuntimeError("lbm_comm_unique_id failed")
    return buf.raw
