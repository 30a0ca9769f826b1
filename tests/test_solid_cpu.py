"""CPU tests of solid obstacles in the bounce-back cavity: the properties of the reference tests/solid_ref.py (what the GPU tests
compare the device with), the host restatement latticeboltzmannsimulations_amd/solid.py against the reference's own link sets and
force, the dry-run plan of the new semantics with every refused combination, and the front ends -- argument checks, the command
lines' masks, the force lines of run_cavity, solid.npy of the sweep -- through the stand-ins of tests/front_end_standin.py."""

import numpy as np
import pytest


import front_end_standin as FS
from bounce_back_ref import BounceBackOracle
from solid_ref import SolidOracle
from latticeboltzmannsimulations_amd import _lib as L
from latticeboltzmannsimulations_amd import datagen, launch_plan, mrt_gpu, solid
from latticeboltzmannsimulations_amd.solver import CavitySolver

NX, NY = 48, 40


def _mask():
    """An 8 x 6 block, a 3 x 3 block in a bottom corner and one solid cell in the lid row."""
    m = np.zeros((NX, NY), dtype=bool)
    m[20:28, 14:20] = True
    m[0:3, NY - 3:NY] = True
    m[33, 0] = True
    return m


@pytest.fixture(scope="module")
def developed():
    """coll -> the fp64 reference after 2000 steps of the 48 x 40 lattice at Re 100 with _mask(), and its fluid mass at the start."""
    out = {}
    for coll in ("SRT", "TRT", "MRT"):
        o = SolidOracle(NX, NY, 100.0, mask=_mask(), collision=coll, dtype=np.float64)
        m0 = o.fluid_mass()
        out[coll] = (o.step(2000), m0)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_all_fluid_mask_is_the_bounce_back_reference(coll, dtype):
    a = BounceBackOracle(NX, NY, 100.0, collision=coll, dtype=dtype).step(37)
    b = SolidOracle(NX, NY, 100.0, collision=coll, dtype=dtype).step(37)
    assert np.array_equal(a.fin, b.fin) and np.array_equal(a.u, b.u) and np.array_equal(a.rho, b.rho)
    assert b.force() == dict(links=0, fx=0.0, fy=0.0, abs_x=0.0, abs_y=0.0)


@pytest.mark.parametrize("coll", ["SRT", "TRT", "MRT"])
def test_reference_conserves_fluid_mass_and_keeps_solid_cells(coll, developed):
    o, m0 = developed[coll]
    m = _mask()
    assert np.isfinite(o.fin).all()
    drift = abs(o.fluid_mass() - m0) / m0
    print(f"{coll}: fluid mass drift after 2000 steps {drift:.3e}")
    assert drift < 1e-11
    assert np.array_equal(o.fin[:, m], np.broadcast_to(o.t[:, None], (9, int(m.sum()))))
    assert not o.u[:, m].any() and np.all(o.rho[m] == o.rho[m][0])


@pytest.mark.parametrize("coll", ["SRT", "MRT"])
def test_host_restatement_agrees_with_the_reference(coll, developed):
    o, _ = developed[coll]
    m = _mask()
    for k, (a, b) in enumerate(zip(solid.links(m), o.link_sets())):
        assert np.array_equal(a, b), f"links of slot {k}"
    want, got = o.force(), solid.host_force(o.fin, m)
    assert got["links"] == want["links"] > 0
    assert got["fx"] == want["fx"] and got["fy"] == want["fy"]          # both are exactly rounded sums of the same terms
    tx, ty = solid.force_terms(o.fin, m)
    assert tx.size == ty.size == want["links"] and abs(got["fx"]) > 0.0
    # one cell in the middle: four axis links and four diagonal ones
    one = np.zeros((NX, NY), bool); one[10, 10] = True
    ls = solid.links(one)
    assert [int(l.sum()) for l in ls] == [0] + [1] * 8
    assert ls[1][11, 10] and ls[2][10, 9] and ls[5][11, 9]               # slot k pulls from (x - cx, y + cy)
    # a cell in a corner of the lid row: links only from inside the lattice
    one = np.zeros((NX, NY), bool); one[0, 0] = True
    assert sum(int(l.sum()) for l in solid.links(one)) == 3


def test_boxes_and_files_make_masks(tmp_path):
    m = solid.boxes_mask(NX, NY, [(20, 28, 14, 20), (0, 3, NY - 3, NY), (33, 34, 0, 1)])
    assert np.array_equal(m, _mask())
    for bad in ((5, 5, 0, 1), (0, NX + 1, 0, 1), (-1, 2, 0, 1), (0, 1, 3, 2)):
        with pytest.raises(ValueError, match="solid box"):
            solid.boxes_mask(NX, NY, [bad])
    assert solid.mask_from(NX, NY) is None
    path = str(tmp_path / "m.npy")
    np.save(path, _mask().astype(np.int32) * 5)
    assert np.array_equal(solid.mask_from(NX, NY, path=path), _mask())
    assert solid.mask_from(NX, NY, [(40, 42, 30, 31)], path)[41, 30] and solid.mask_from(NX, NY, [(40, 42, 30, 31)], path)[20, 14]
    with pytest.raises(ValueError, match="shape"):
        solid.mask_from(NX + 1, NY, path=path)


# ---- the dry-run plan --------------------------------------------------------------------------------------------------------------
def test_plan_names_its_kernel_and_steps_one_step_per_launch():
    kw = dict(semantics="bounce_back", solid=True)
    p = launch_plan(4096, 4096, 1000.0, steps=6, **kw)
    assert p["kernel"] == "k_step_solid" and p["semantics"] == "bounce_back_solid" and p["steps_per_launch"] == 1
    assert p["units"] == [1] * 6 and p["vec"] == 1 and p["nt"] == 1 and p["slab"] == 0
    plain = launch_plan(4096, 4096, 1000.0, steps=6, semantics="bounce_back")
    assert plain["semantics"] == "bounce_back" and plain["units"] != p["units"]
    assert p["lattice_bytes"] * 9 == plain["lattice_bytes"] * 10          # one more plane: the link words
    assert launch_plan(70, 66, 100.0, **kw)["kernel"] == "k_step_generic"                           # 70 % 4 != 0
    assert launch_plan(70, 66, 100.0, dtype=np.float64, **kw)["kernel"] == "k_step_solid"           # 70 % 2 == 0
    assert launch_plan(72, 40, 100.0, kernel="generic", **kw)["kernel"] == "k_step_generic"
    assert launch_plan(384, 384, 100.0, batch=64, arith="fast", steps=3, **kw)["units"] == [1, 1, 1]
    with pytest.raises(ValueError, match="bounce_back"):
        launch_plan(72, 40, 100.0, solid=True)


@pytest.mark.parametrize("kw,text", [
    (dict(rows=(0, 64)), "no slabs"),
    (dict(rows=(64, 64)), "no slabs"),
    (dict(kernel="tb"), "one step per launch"),
    (dict(kernel="stream"), "one step per launch"),
    (dict(kernel="vec"), "one step per launch"),
    (dict(kernel="push"), "one step per launch"),
    (dict(turb=1), "turb = 1"),
    (dict(arith="promoted"), "promoted"),
    (dict(tuning=dict(stream_walls=True)), "STREAM_WALLS"),
    (dict(tuning=dict(stream_pairs=True)), "STREAM_WALLS"),
])
def test_plan_refuses_with_a_reason(kw, text):
    with pytest.raises(RuntimeError, match=text):
        launch_plan(128, 128, 100.0, semantics="bounce_back", solid=True, **kw)


def test_abi_has_the_new_calls_and_keeps_lbm_params():
    import ctypes
    assert L.LBM_SEM_BOUNCE_BACK_SOLID == 3 and ctypes.sizeof(L.lbm_params) == 18 * 4 + 6 * 8
    assert ctypes.sizeof(L.lbm_solid_force_record) == 32
    lib = L.lib()
    for name in ("lbm_set_solid", "lbm_get_solid", "lbm_solid_force"):
        assert hasattr(lib, name)
    text = open(L.HEADER).read()
    assert "LBM_SEM_BOUNCE_BACK_SOLID = 3" in text and "int lbm_solid_force(lbm_ctx* c, lbm_solid_force_record* out);" in text


# ---- the front ends, through the stand-ins ------------------------------------------------------------------------------------------
def _solid_standin(base):
    """A stand-in with CavitySolver's solid=... and solid_force, stepping the reference of tests/solid_ref.py."""
    class S(base):
        source = "solid"
        masks = []

        def __init__(self, xsize, ysize, Re, solid=None, **kw):
            type(self).masks.append(None if solid is None else np.array(solid))
            FS.SOURCES["solid"] = lambda X, Y, R, k: SolidOracle(X, Y, R, mask=solid, uLB=k["uLB"], collision=k["RT"], dtype=np.float64)
            super().__init__(xsize, ysize, Re, **kw)

        def solid_force(self):
            self._note("solid_force", self.steps_done)
            F = self.o.force()
            return dict(step=self.steps_done, links=F["links"], fx=F["fx"], fy=F["fy"])
    return S


def test_run_cavity_prints_the_force_at_every_output_iteration(capsys):
    S = _solid_standin(FS.standin())
    r = mrt_gpu.run_cavity(maxIt=41, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=20, SavePlot=False, BC="BB", solid=_mask(),
                           solver_factory=S)
    out = capsys.readouterr().out
    assert S.made[-1]["semantics"] == "bounce_back" and np.array_equal(S.masks[-1], _mask())
    assert [it for it, _ in r.forces] == [0, 20, 40] and [n for n, in FS._entries(S.journal, "solid_force")] == [1, 21, 41]
    o = SolidOracle(NX, NY, 100.0, mask=_mask(), collision="MRT", dtype=np.float64).step(21)
    F = o.force()
    assert r.forces[1][1] == dict(step=21, links=F["links"], fx=F["fx"], fy=F["fy"])
    assert out.count("current force on the obstacles is (") == 3
    assert f"current force on the obstacles is ({F['fx']}, {F['fy']}) over {F['links']} links" in out
    assert not r.u[:, _mask()].any()
    # without solid=... nothing changes: no force line, no output iteration of its own
    P = FS.standin(source="bounce_back")
    r = mrt_gpu.run_cavity(maxIt=41, Re=100.0, RT="MRT", turb=0, xsize=NX, ysize=NY, Pinterval=20, SavePlot=False, BC="BB", solver_factory=P)
    assert r.forces == [] and "force" not in capsys.readouterr().out and P.calls == [41]


@pytest.mark.parametrize("kw,text", [
    (dict(), "BC='BB'"),
    (dict(BC="EB-NEBB "), "BC='BB'"),
    (dict(BC="BB", turb=1), "turb=0"),
    (dict(BC="BB", turb=0, semantics="mrt_py"), "bounce_back"),
])
def test_solid_needs_bounce_back_walls(kw, text):
    S = _solid_standin(FS.standin())
    kw = dict(dict(turb=0), **kw)
    with pytest.raises(ValueError, match=text):
        mrt_gpu.run_cavity(maxIt=5, xsize=NX, ysize=NY, SavePlot=False, quiet=True, solid=_mask(), solver_factory=S, **kw)
    assert S.made == []
    if "semantics" not in kw:      # (the sweep has no semantics argument)
        with pytest.raises(ValueError, match=text):
            datagen.generate([100.0], xsize=NX, ysize=NY, save=False, quiet=True, solid=_mask(), batch_factory=FS.BatchStandIn, **kw)


def test_command_line_builds_the_mask_and_checks_bc(tmp_path, monkeypatch, capsys):
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return mrt_gpu.CavityResult()
    monkeypatch.setattr(mrt_gpu, "run_cavity", fake)
    path = str(tmp_path / "mask.npy")
    one = np.zeros((NX, NY), np.uint8); one[33, 0] = 1
    np.save(path, one)
    size = ["--xsize", str(NX), "--ysize", str(NY), "--turb", "0"]
    boxes = ["--solid-box", "20", "28", "14", "20", "--solid-box", "0", "3", str(NY - 3), str(NY), "--solid-file", path]
    assert mrt_gpu.main(size + ["--BC", "BB"] + boxes) == 0
    assert np.array_equal(seen["solid"], _mask()) and seen["BC"] == "BB"
    seen.clear()
    assert mrt_gpu.main(size + ["--BC", "BB"]) == 0 and seen["solid"] is None
    for argv, text in ((size + boxes, "BC='BB'"), (size + ["--BC", "EB-NEBB"] + boxes, "BC='BB'"),
                       (["--xsize", str(NX), "--ysize", str(NY), "--BC", "BB"] + boxes, "turb=0"),
                       (size + ["--BC", "BB", "--solid-box", "0", "99", "0", "1"], "solid box"),
                       (size + ["--BC", "BB", "--solid-file", str(tmp_path / "none.npy")], "none.npy")):
        seen.clear()
        with pytest.raises(SystemExit) as e:
            mrt_gpu.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err and not seen


def test_sweep_takes_a_mask_per_lattice_and_saves_it(tmp_path, monkeypatch):
    made = []

    class B(FS.BatchStandIn):
        def __init__(self, xsize, ysize, Re_list, solid=None, **kw):
            made.append(np.array(solid))
            lone = _solid_standin(FS.standin())
            self.lattices = [lone(xsize, ysize, float(Re), solid=solid[i], **kw) for i, Re in enumerate(Re_list)]
            self.journal = []
    masks = np.stack([_mask(), np.zeros((NX, NY), bool), _mask()[::-1]])
    out = datagen.generate([100.0, 200.0, 300.0], xsize=NX, ysize=NY, RT="MRT", turb=0, maxIt=30, Pinterval=10, BC="BB", concurrent=2,
                           OutputFolder=str(tmp_path), quiet=True, solid=masks, batch_factory=B)
    assert [m.shape for m in made] == [(2, NX, NY), (1, NX, NY)] and np.array_equal(made[0], masks[:2]) and np.array_equal(made[1], masks[2:])
    assert np.array_equal(np.load(tmp_path / "solid.npy"), masks) and (tmp_path / "u_final.npy").exists()
    assert not out[2][0][:, _mask()].any() and out[2][1].any()
    o = SolidOracle(NX, NY, 300.0, mask=masks[2], collision="MRT", dtype=np.float64).step(30)
    assert np.array_equal(out[1][2], o.fin.astype(np.float32))
    # one mask for all lattices
    made.clear()
    datagen.generate([100.0, 200.0], xsize=NX, ysize=NY, RT="MRT", turb=0, maxIt=5, Pinterval=10, BC="BB", save=False, quiet=True,
                     solid=_mask(), batch_factory=B)
    assert made[0].shape == (2, NX, NY) and np.array_equal(made[0][1], _mask())
    with pytest.raises(ValueError, match="shape"):
        datagen.generate([100.0, 200.0], xsize=NX, ysize=NY, turb=0, BC="BB", save=False, quiet=True, solid=masks, batch_factory=B)
    seen = {}
    monkeypatch.setattr(datagen, "generate", lambda *a, **kw: seen.update(kw))
    assert datagen.main(["--size", str(NX), "--BC", "BB", "--solid-box", "1", "3", "2", "4"]) == 0
    assert seen["solid"][1:3, 2:4].all() and seen["solid"].sum() == 4 and seen["turb"] == 0
    with pytest.raises(SystemExit):
        datagen.main(["--size", str(NX), "--solid-box", "1", "3", "2", "4"])


def test_checkpoint_carries_the_mask(tmp_path, monkeypatch):
    """save_checkpoint / load_checkpoint around a context-free double of the solver's state calls: the mask travels in the file, and a
    mask that differs -- or is missing on one side -- is an error under strict."""
    class Double(CavitySolver):
        def __init__(self, mask):
            self._h, self._lead, self.batch = None, (), 1
            self.nx, self.ny, self.Re, self.RT, self.uLB, self.semantics = NX, NY, 100.0, "MRT", 0.08, "bounce_back"
            self.dtype, self.y0, self.ny_local, self.turb, self.arith = np.dtype(np.float64), 0, NY, 0, "strict"
            self.has_solid, self._m, self.steps, self.state = mask is not None, mask, 25, None

        solid = property(lambda self: None if self._m is None else self._m.copy())
        steps_done = property(lambda self: self.steps)

        def get_fields(self, want_fin=False, **kw):
            o = SolidOracle(NX, NY, 100.0, mask=self._m, dtype=np.float64).step(3)
            return o.u, o.rho, o.fin

        def set_state(self, fin):
            self.state = fin
    path = Double(_mask()).save_checkpoint(str(tmp_path / "c"))
    with np.load(path) as z:
        assert np.array_equal(z["solid"], _mask()) and z["solid"].dtype == bool
    same = Double(_mask())
    assert same.load_checkpoint(path) == 25 and same.state is not None
    for other in (Double(None), Double(np.zeros((NX, NY), bool)), Double(_mask()[::-1].copy())):
        with pytest.raises(ValueError, match="solid"):
            other.load_checkpoint(path)
        assert other.state is None
        assert other.load_checkpoint(path, strict=False) == 25 and other.state is not None
    plain = Double(None).save_checkpoint(str(tmp_path / "p"))
    with np.load(plain) as z:
        assert "solid" not in z
    with pytest.raises(ValueError, match="solid"):
        Double(_mask()).load_checkpoint(plain)
    assert Double(None).load_checkpoint(plain) == 25
