"""CPU stand-ins for CavitySolver and CavityBatch as far as the front ends use them (TEST DOUBLES; the product has no CPU stepper).

FrontEndStandIn has CavitySolver's keyword signature and the whole surface mrt_gpu.run_cavity calls.  The fields come from a pluggable
source (SOURCES: the C oracle, the bounce-back reference of tests/bounce_back_ref.py, or fields that are a fixed function of the step
count); every mode is stated through the package's own host statement on those fields -- monitor.host_monitor, residual.host_residual,
topology.host_topology / vortex_table, float64 sums for the time statistics -- so one object can run any combination of modes.

Every call is appended to one ordered journal of (method, the arguments that matter); the journal belongs to the class and starts
afresh with every instance, and the counters the tests read (calls, mean_calls, log, begins on the class; sampled on the instance) are
read from it.  `made` collects the keyword arguments of every instance, `last` is the latest instance.  standin(...) returns a fresh
subclass -- with its own journal -- with another source, a blow-up step, or without a feature.

BatchStandIn is B such lattices side by side with the surface of CavityBatch that datagen._solve_batch calls."""
import numpy as np

from latticeboltzmannsimulations_amd import monitor as M
from latticeboltzmannsimulations_amd import relaxation
from latticeboltzmannsimulations_amd import residual as RS
from latticeboltzmannsimulations_amd import topology as T


def _oracle_c(X, Y, Re, kw):
    from oracle.lbm_ref import CavityOracleC
    return CavityOracleC(X, Y, Re, uLB=kw["uLB"], semantics=kw["semantics"], collision=kw["RT"], dtype=kw["dtype"], turb=kw["turb"],
                         promote=kw["arith"] == "promoted")


def _bounce_back(X, Y, Re, kw):
    from bounce_back_ref import BounceBackOracle
    return BounceBackOracle(X, Y, Re, uLB=kw["uLB"], collision=kw["RT"], dtype=np.float64)


class SyntheticFields:
    """Fields that are a fixed function of the step count n: what a sample at step n must have seen can be written down."""

    def __init__(self, X, Y, Re, kw):
        self.uLB, self.nsteps = kw["uLB"], 0
        x = np.arange(X)[:, None] / X
        y = np.arange(Y)[None, :] / Y
        self.base = np.stack([np.sin(np.pi * x) * (1 - y) ** 3 - 0.2 * np.sin(2 * np.pi * y) * np.sin(np.pi * x),
                              0.3 * np.sin(2 * np.pi * x) * np.sin(np.pi * y)])
        self.fin = np.zeros((9, X, Y), dtype=np.float32)
        self.u, self.rho = self.fields(0)

    def fields(self, n):
        u = (self.uLB * self.base * (1 + 0.1 * np.sin(n / 7.0))).astype(np.float32)
        rho = (1 + 1e-3 * np.cos(n / 3.0) * self.base[0]).astype(np.float32)
        return u, rho

    def step(self, n=1):
        self.nsteps += int(n)
        self.u, self.rho = self.fields(self.nsteps)
        return self


SOURCES = dict(oracle=_oracle_c, bounce_back=_bounce_back, synthetic=SyntheticFields)
FEATURES = dict(monitor=("monitor", "lines", "locate_vortices", "begin_monitor", "monitor_series"),
                residual=("begin_residual", "sample_residual", "residual_series"), topology=("topology", "vortex_table"),
                statistics=("begin_statistics", "sample_statistics", "statistics"), tau=("get_tau",), mean_u=("mean_u",))


def _entries(journal, method):
    return [e[1:] for e in journal if e[0] == method]


class _Counters(type):
    """The counters of the class, read from the journal of its latest instance."""
    calls = property(lambda cls: [n for n, in _entries(cls.journal, "step")])
    mean_calls = property(lambda cls: len(_entries(cls.journal, "mean_u")))
    begins = property(lambda cls: _entries(cls.journal, "begin_statistics"))
    log = property(lambda cls: dict(steps=cls.calls, downloads=len(_entries(cls.journal, "get_fields")),
                                    monitors=len(_entries(cls.journal, "monitor")), lines=len(_entries(cls.journal, "lines")),
                                    begin=([b for b, in _entries(cls.journal, "begin_monitor")] or [None])[-1]))


class FrontEndStandIn(metaclass=_Counters):
    source = "oracle"      # a key of SOURCES
    blow_up_at = None      # from the step after this one on, the fields every call sees hold two cells that are not finite
    journal = []
    made = []
    last = None

    def __init__(self, xsize, ysize, Re, RT="MRT", uLB=0.08, semantics="mrt_gpu", dtype=np.float32, turb=0, device=0, arith="strict"):
        kw = dict(RT=RT, uLB=uLB, semantics=semantics, dtype=dtype, turb=turb, device=device, arith=arith)
        cls = type(self)
        cls.journal, cls.last = [], self
        cls.made.append(kw)
        self.o = SOURCES[self.source](xsize, ysize, Re, kw)
        self.relax = relaxation(Re, ysize, uLB)
        self.nx, self.ny, self.uLB, self.dtype, self.steps_done = xsize, ysize, uLB, np.dtype(dtype), 0
        self._series = self._stats = self._res = None

    def _note(self, method, *args):
        self.journal.append((method,) + args)

    def _fields(self, dt=None):
        dt = self.o.u.dtype if dt is None else dt
        u, rho = self.o.u.astype(dt), self.o.rho.astype(dt)
        if self.blow_up_at is not None and self.steps_done > self.blow_up_at:
            u[0, 3, 4] = np.nan
            rho[5, 6] = np.inf
        return u, rho

    # -- life cycle and time loop -----------------------------------------------------------------
    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        self._note("close")

    def sync(self):
        self._note("sync")

    def step(self, n=1):
        """n steps, in pieces that end where a sampler with every > 0 is due (as lbm_step samples by itself)."""
        self._note("step", int(n))
        left = int(n)
        while left:
            due = [s["every"] - (self.steps_done - s["n0"]) % s["every"] for s in (self._series, self._stats) if s and s["every"]]
            k = min([left] + due)
            self.o.step(k)
            self.steps_done += k
            left -= k
            s = self._series
            if s and s["every"] and (self.steps_done - s["n0"]) % s["every"] == 0:
                if len(s["records"]) < s["capacity"]:
                    s["records"].append(M.host_monitor(*self._fields(s["out"]), self.uLB, step=self.steps_done, **s["spec"]))
                else:
                    s["dropped"] += 1
            s = self._stats
            if s and s["every"] and (self.steps_done - s["n0"]) % s["every"] == 0:
                self.sample_statistics()
        return self

    # -- state out --------------------------------------------------------------------------------
    def get_fields(self, want_fin=False, out_dtype=None, **kw):
        self._note("get_fields", bool(want_fin))
        u, rho = self._fields(out_dtype)
        return (u, rho, self.o.fin.astype(u.dtype)) if want_fin else (u, rho)

    def mean_u(self):          # lbm_mean_u: the mean accumulated in double
        self._note("mean_u")
        return float(np.mean(self.o.u.astype(np.float64)))

    def get_tau(self):
        self._note("get_tau")
        return np.full((self.nx, self.ny), 1.0 / self.relax["omega"] + 0.01)

    # -- time statistics: a sample at step count n is the fields after n steps, added in float64 ----------------------
    def begin_statistics(self, every=0):
        self._note("begin_statistics", self.steps_done, int(every))
        self._stats = dict(every=int(every), n0=self.steps_done, count=0,
                           S=[np.zeros((2, self.nx, self.ny)), np.zeros((self.nx, self.ny)), np.zeros((3, self.nx, self.ny))])
        return self

    def sample_statistics(self):
        self._note("sample_statistics", self.steps_done)
        u, rho = (a.astype(np.float64) for a in self._fields())
        S = self._stats["S"]
        S[0] += u
        S[1] += rho
        S[2] += np.stack([u[0] * u[0], u[1] * u[1], u[0] * u[1]])
        self._stats["count"] += 1
        return self

    @property
    def sampled(self):
        return [n for n, in _entries(self.journal, "sample_statistics")]

    def statistics(self):
        self._note("statistics")
        count = self._stats["count"]
        if count == 0:
            return dict(u=None, rho=None, uu=None, vv=None, uv=None, samples=0)
        mu, mrho, sec = (s / count for s in self._stats["S"])
        return dict(u=mu, rho=mrho, uu=sec[0] - mu[0] * mu[0], vv=sec[1] - mu[1] * mu[1], uv=sec[2] - mu[0] * mu[1], samples=count)

    # -- run monitor ------------------------------------------------------------------------------
    def monitor(self, window=None, exclude=(), probes=(), out_dtype=None):
        self._note("monitor", window, tuple(exclude))
        return M.host_monitor(*self._fields(out_dtype), self.uLB, window=window, exclude=exclude, probes=probes, step=self.steps_done)

    def lines(self, x=None, y=None, out_dtype=None):
        self._note("lines")
        u, rho = self._fields(out_dtype)
        x, y = int(self.nx / 2) if x is None else x, int(self.ny / 2) if y is None else y
        return np.stack([u[0, x, :], u[1, x, :], rho[x, :]]), np.stack([u[0, :, y], u[1, :, y], rho[:, y]])

    def locate_vortices(self, out_dtype=np.float32, first=None):
        self._note("locate_vortices", first is not None)
        off, win = M.vortex_window(self.nx, self.ny)
        a = self.monitor(window=win, out_dtype=out_dtype) if first is None else first
        loc1 = (a["min_x"], a["min_y"])
        b = self.monitor(window=win, exclude=(M.vortex_box(loc1, off),), out_dtype=out_dtype)
        return loc1, (b["min_x"], b["min_y"])

    def begin_monitor(self, every=0, capacity=1024, window=None, exclude=(), probes=(), out_dtype=None):
        self._note("begin_monitor", dict(every=every, capacity=capacity, probes=tuple(probes)))
        self._series = dict(n0=self.steps_done, every=int(every), capacity=int(capacity), out=out_dtype, records=[], dropped=0,
                            spec=dict(window=window, exclude=exclude, probes=tuple(probes)))
        return self

    def monitor_series(self):
        self._note("monitor_series")
        recs = self._series["records"]
        out = {k: np.array([r[k] for r in recs]) for k in M.SCALARS + ("probe",)}
        out["count"], out["dropped"] = len(recs), self._series["dropped"]
        return out

    # -- field residual -----------------------------------------------------------------------------
    def begin_residual(self, every=0, capacity=1024, out_dtype=None):
        assert every == 0
        self._note("begin_residual", int(capacity))
        self._res = dict(records=[], prev=None, capacity=int(capacity), out=out_dtype, dropped=0)
        return self

    def sample_residual(self):
        self._note("sample_residual", self.steps_done)
        s = self._res
        u, rho = self._fields(s["out"])
        if s["prev"] is not None:
            if len(s["records"]) < s["capacity"]:
                s["records"].append(RS.host_residual(s["prev"][1], s["prev"][2], u, rho, step=self.steps_done, step_prev=s["prev"][0]))
            else:
                s["dropped"] += 1
        s["prev"] = (self.steps_done, u, rho)
        return self

    def residual_series(self):
        self._note("residual_series")
        out = {k: np.array([r[k] for r in self._res["records"]]) for k in RS.FIELDS}
        out["count"], out["dropped"] = len(self._res["records"]), self._res["dropped"]
        return out

    # -- flow topology ------------------------------------------------------------------------------
    def topology(self, windows=(), out_dtype=None):
        self._note("topology", tuple(windows))
        return T.host_topology(self._fields(out_dtype)[0], self.uLB, windows, step=self.steps_done)

    def vortex_table(self, out_dtype=np.float32):
        self._note("vortex_table")
        return T.vortex_table(self.topology(T.vortex_windows(self.nx, self.ny), out_dtype=out_dtype), self.nx, self.ny)


def standin(without=(), **config):
    """A fresh subclass of FrontEndStandIn with its own journal and `made`: config sets source / blow_up_at; `without` names the
    FEATURES it lacks (their methods raise AttributeError, so hasattr is False)."""
    gone = {name: property() for f in without for name in FEATURES[f]}
    return _Counters("StandIn", (FrontEndStandIn,), dict(config, journal=[], made=[], **gone))


class BatchStandIn:
    """B lone stand-ins side by side: host arrays carry a leading [B] axis, mean_u returns an array, the residual series has shape
    [count, B].  The journal is the instance's."""
    source = "oracle"

    def __init__(self, xsize, ysize, Re_list, **kw):
        lone = standin(source=self.source)
        self.lattices = [lone(xsize, ysize, float(Re), **kw) for Re in Re_list]
        self.journal = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.journal.append(("close",))

    @property
    def steps_done(self):
        return self.lattices[0].steps_done

    def step(self, n=1):
        self.journal.append(("step", int(n)))
        for s in self.lattices:
            s.step(n)
        return self

    def get_fields(self, want_fin=False, out_dtype=None):
        self.journal.append(("get_fields", bool(want_fin)))
        return tuple(np.stack(a) for a in zip(*(s.get_fields(want_fin=want_fin, out_dtype=out_dtype) for s in self.lattices)))

    def mean_u(self):
        self.journal.append(("mean_u",))
        return np.array([s.mean_u() for s in self.lattices])

    def begin_residual(self, **kw):
        self.journal.append(("begin_residual", int(kw.get("capacity", 1024))))
        for s in self.lattices:
            s.begin_residual(**kw)
        return self

    def sample_residual(self):
        self.journal.append(("sample_residual", self.steps_done))
        for s in self.lattices:
            s.sample_residual()
        return self

    def residual_series(self):
        self.journal.append(("residual_series",))
        each = [s.residual_series() for s in self.lattices]
        out = {k: np.stack([e[k] for e in each], axis=-1) for k in RS.FIELDS}
        out["count"], out["dropped"] = each[0]["count"], each[0]["dropped"]
        return out
