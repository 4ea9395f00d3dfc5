"""The reference's own PYTHON layer, run in-process -- TEST INFRASTRUCTURE ONLY.

``oracle/oracle.py`` and ``lightpycl_amd/{light_source,geo_optical_elements,
iterative_tracer,scenes}.py`` restate the reference's host code.  This module
runs the reference's host code itself, so that the restatements can be held
against it (``tests/test_ref_host.py``), and records what it computes as
fixtures (``tests/golden/ref_host/*.npz``) for machines without the reference.
``lightpycl_amd`` never imports it.

Recipe; everything derived from the reference goes to
``oracle/_ref/py/`` (git-ignored), nothing of it into the repository:

* ``light_source.py``, ``geo_optical_elements.py`` and ``iterative_tracer.py``
  are read from the reference directory (``/root/reference``; override with the
  environment variable ``LPC_REFERENCE_DIR`` or ``--reference DIR``), translated
  with ``lib2to3`` (they are Python 2) and their tabs expanded to 8 (they mix
  tabs and spaces);
* ``dxfwrite`` (a ``DXFEngine`` class) and ``triangle`` are empty stand-ins in
  ``sys.modules`` while the translated modules are imported;
* ``pyopencl`` / ``pyopencl.array`` are stand-ins too (:class:`_FakeCL`): only the
  surface the reference uses -- ``get_platforms`` and devices, ``Context``,
  ``CommandQueue``, ``mem_flags``, ``Program(ctx, src).build()``,
  ``cl_array.to_device`` / ``zeros``, array ``+ scalar``, ``.data``, ``.get()``,
  event ``.wait()``.  ``build()`` ignores the source; its kernels forward the
  reference's argument lists (``iterative_tracer.py:288-326, :515, :546``) to the
  CPU restatement of the kernels (``oracle/_build/liblpc_oracle.so``) with the
  launch's global size.  The device buffers are the numpy arrays the reference
  allocates, kept across iterations as the reference keeps them;
* the reference runs with the working directory at the reference directory (it
  opens its kernel file by a relative path, ``iterative_tracer.py:66``), with
  matplotlib's ``Agg`` backend, ``savefig`` / ``show`` as no-ops and its prints
  discarded.

Patches applied in the running process (never in the text):

* ``light_source`` sees numpy through :class:`_Numpy1` -- ``np.float`` (gone in
  numpy 1.24), and float counts given to ``np.linspace``, ``np.arange`` and
  ``np.zeros`` (``grid_rays``, ``light_source.py:68-91``: numpy 1 truncated them,
  numpy 2 raises).  Nothing else needed a patch for what is recorded here.
* ``plot_elevation_histogram``, ``get_beam_width_half_power`` and
  ``get_beam_HWHM`` return None and print their results; :func:`beam_values`
  reads the printed quantities from the function's frame as it returns
  (``sys.setprofile``).

What the reference cannot run here, and is therefore NOT pinned by this recipe:

* ``optical_elements.curve_to_mesh`` and ``extrude_by_vector(capped=True)``
  (need Shewchuk's ``triangle``);
* ``GeoObject.write_dxf``, ``light_source.save_dxf``,
  ``CL_Tracer.save_traced_scene`` (need ``dxfwrite``);
* ``CL_Tracer.replicate_lightsources_and_plot`` and ``plot_binned_data``
  (``gca(projection=)`` / ``normed=`` no longer exist in matplotlib / numpy),
  ``pickle_results`` / ``load_pickle_results`` (Python-2 pickles);
* ``setMaterial`` with an unknown type: the reference sets the fallback type and
  then raises NameError from its warning's ``print`` (``geo_optical_elements.py
  :52``); the state it leaves is recorded, the drop-in warns and goes on.

The catalogue of calls (:data:`RAY_CASES`, :data:`GEO_CASES`, :data:`CURVE_CASES`,
:func:`build_scene`, :data:`TRACE_CASES`) is plain data interpreted against a
module set ``M`` (``M.ls``, ``M.goe``): :func:`load` gives the reference's,
:func:`ours` the drop-in's.  ``python oracle/ref_host.py [--out DIR]``
regenerates the fixtures (byte-identical from run to run).
"""
from __future__ import annotations

import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import types
import warnings
import zipfile
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
PY_DIR = os.path.join(_HERE, "_ref", "py")
FIXTURE_DIR = os.path.join(ROOT, "tests", "golden", "ref_host")
MODULES = ("light_source", "geo_optical_elements", "iterative_tracer")
SOURCE = "reference python (lib2to3) + CPU oracle kernels"
FILE_LIMIT = 128 * 1024    # bytes per fixture file
FILE_BUDGET = FILE_LIMIT - 4096   # what the arrays of a file may take (the rest: args, source, zip trailer)
_reference_dir = None


def reference_dir():
    return _reference_dir or os.environ.get("LPC_REFERENCE_DIR", "/root/reference")


def set_reference_dir(path):
    global _reference_dir, _loaded
    _reference_dir, _loaded = path, None


def available():
    """Can the recipe run here?  -> (bool, reason)."""
    d = reference_dir()
    missing = [m for m in MODULES if not os.path.isfile(os.path.join(d, m + ".py"))]
    if missing:
        return False, "no reference sources under %s (%s)" % (d, ", ".join(missing))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            import lib2to3.refactor  # noqa: F401
    except ImportError:
        return False, "this Python has no lib2to3"
    return True, "reference at " + d


# -- stand-ins -------------------------------------------------------------------------------
class _Array:
    """pyopencl.array.Array: a host numpy array."""

    def __init__(self, a):
        self._a = a

    @property
    def data(self):
        return self._a

    @property
    def shape(self):
        return self._a.shape

    def __add__(self, scalar):
        return _Array(self._a + scalar)

    def get(self, queue=None):
        return self._a.copy()


class _Event:
    def wait(self):
        pass


def _f32(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous, (a.dtype, a.shape)
    return a


def _i32(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous, (a.dtype, a.shape)
    return a


class _Kernels:
    """Program(...).build(): the five kernels, argument lists as the reference passes them."""

    def __init__(self):
        import oracle
        self.L = oracle.lib()
        self.mesh_power = None      # float64[K]: measured power by hit mesh, as oracle.trace accumulates it

    def intersect(self, queue, gsize, lsize, o, d, dest, ent, imid, iidx, v0, v1, v2, mid, tmin, cnt, itmp,
                  mesh_count, tri_count, ray_count, max_ray_len):
        self.L.orc_intersect(int(gsize[0]), _f32(o), _f32(d), _f32(v0), _f32(v1), _f32(v2), _i32(mid),
                             int(mesh_count), int(tri_count), float(max_ray_len), _f32(tmin), _i32(cnt), _i32(itmp))
        return _Event()

    def intersect_postproc(self, queue, gsize, lsize, o, d, dest, prev, n1, n2, ent, imid, iidx, v0, v1, v2, mid,
                           mtyp, tmin, cnt, itmp, mesh_count, ray_count, max_ray_len):
        self.L.orc_intersect_postproc(int(gsize[0]), _f32(o), _f32(d), _f32(dest), _i32(prev), _i32(n1), _i32(n2),
                                      _i32(ent), _i32(imid), _i32(iidx), _i32(mtyp), _f32(tmin), _i32(cnt),
                                      _i32(itmp), int(mesh_count), float(max_ray_len))
        return _Event()

    def reflect_refract_rays(self, queue, gsize, lsize, o, dest, d, pw, ms, ent, n1, n2, ro, rd, rp, rm, to, td, tp,
                             tm, imid, iidx, v0, v1, v2, mid, mtyp, ior, refl, diss, ior_env, mesh_count, ray_count,
                             max_ray_len):
        self.L.orc_reflect_refract_rays(int(gsize[0]), _f32(o), _f32(dest), _f32(d), _f32(pw), _i32(ms), _i32(n1),
                                        _i32(n2), _f32(ro), _f32(rd), _f32(rp), _i32(rm), _f32(to), _f32(td),
                                        _f32(tp), _i32(tm), _i32(imid), _i32(iidx), _f32(v0), _f32(v1), _f32(v2),
                                        _i32(mtyp), _f32(ior), _f32(refl), _f32(diss), float(ior_env))
        n = int(gsize[0])
        if self.mesh_power is None:
            self.mesh_power = np.zeros(int(mesh_count), np.float64)
        m = ms.reshape(-1)[:n] >= 0.9
        np.add.at(self.mesh_power, imid.reshape(-1)[:n][m], pw.reshape(-1)[:n][m].astype(np.float64))
        return _Event()

    def angular_project(self, queue, gsize, lsize, pos, pwr, rot, pivot, x, y, pc):
        self.L.orc_angular_project(int(gsize[0]), _f32(pos), _f32(pwr), _f32(rot), _f32(pivot), _f32(x), _f32(y),
                                   _f32(pc))
        return _Event()

    def stereograph_project(self, queue, gsize, lsize, pos, pwr, rot, pivot, x, y, pc):
        self.L.orc_stereograph_project(int(gsize[0]), _f32(pos), _f32(pwr), _f32(rot), _f32(pivot), _f32(x),
                                       _f32(y), _f32(pc))
        return _Event()


def _fake_modules():
    """{name: module} of the stand-ins for pyopencl, pyopencl.array, dxfwrite, triangle."""
    cl = types.ModuleType("pyopencl")
    cla = types.ModuleType("pyopencl.array")

    class Device:
        name = "liblpc_oracle (CPU)"
        global_mem_size = 1 << 34

    class Platform:
        name = "CPU oracle"

        def get_devices(self):
            return [Device()]

    class Context:
        def __init__(self, devices=None):
            self.devices = devices

    class CommandQueue:
        def __init__(self, context=None):
            self.context = context

    class mem_flags:
        READ_ONLY, WRITE_ONLY, READ_WRITE, COPY_HOST_PTR = 1, 2, 4, 8

    class Program:
        def __init__(self, context, source):
            pass

        def build(self, options=None):
            return _Kernels()

    cl.get_platforms = lambda: [Platform()]
    cl.Context, cl.CommandQueue, cl.mem_flags, cl.Program = Context, CommandQueue, mem_flags, Program
    cla.Array = _Array
    cla.to_device = lambda queue, ary: _Array(np.array(ary, order="C"))
    cla.zeros = lambda queue, shape, dtype=np.float32: _Array(np.zeros(shape, dtype=dtype))
    cl.array = cla
    dxf = types.ModuleType("dxfwrite")
    dxf.DXFEngine = type("DXFEngine", (), {})
    return {"pyopencl": cl, "pyopencl.array": cla, "dxfwrite": dxf, "triangle": types.ModuleType("triangle")}


class _Numpy1:
    """numpy as ``grid_rays`` was written for (see the module docstring)."""
    float = float

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def _count(v):
        return int(v) if isinstance(v, (float, np.floating)) else v

    def linspace(self, start, stop, num=50, **kw):
        return np.linspace(start, stop, self._count(num), **kw)

    def arange(self, *a, **kw):
        if len(a) == 1 and isinstance(a[0], (float, np.floating)) and float(a[0]).is_integer():
            a = (int(a[0]),)
        return np.arange(*a, **kw)

    def zeros(self, shape, *a, **kw):
        shape = tuple(self._count(s) for s in shape) if isinstance(shape, tuple) else self._count(shape)
        return np.zeros(shape, *a, **kw)


# -- translation and loading -------------------------------------------------------------------
def translate():
    """reference *.py -> oracle/_ref/py/*.py (lib2to3, tabs expanded to 8)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3.refactor import RefactoringTool, get_fixers_from_package
        tool = RefactoringTool(get_fixers_from_package("lib2to3.fixes"))
    os.makedirs(PY_DIR, exist_ok=True)
    for m in MODULES:
        with open(os.path.join(reference_dir(), m + ".py"), encoding="latin-1") as f:
            text = f.read()
        if not text.endswith("\n"):
            text += "\n"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tree = tool.refactor_string(text, m + ".py")
        out = "\n".join(line.expandtabs(8) for line in str(tree).split("\n"))
        path = os.path.join(PY_DIR, m + ".py")
        if not os.path.exists(path) or open(path, encoding="latin-1").read() != out:
            with open(path, "w", encoding="latin-1") as f:
                f.write(out)


_loaded = None


def load():
    """The reference's three modules, translated and imported: a namespace with
    ``ls`` (light_source), ``goe`` (geo_optical_elements), ``it`` (iterative_tracer)."""
    global _loaded
    if _loaded is not None:
        return _loaded
    ok, why = available()
    if not ok:
        raise RuntimeError(why)
    import matplotlib
    matplotlib.use("Agg")
    translate()
    fakes = _fake_modules()
    saved = {k: sys.modules.get(k) for k in list(fakes) + list(MODULES)}
    sys.modules.update(fakes)
    mods = {}
    try:
        with quiet():
            for m in ("geo_optical_elements", "light_source", "iterative_tracer"):
                spec = importlib.util.spec_from_file_location(m, os.path.join(PY_DIR, m + ".py"))
                mod = importlib.util.module_from_spec(spec)
                sys.modules[m] = mod
                spec.loader.exec_module(mod)
                mods[m] = mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mods["light_source"].np = _Numpy1()
    _loaded = types.SimpleNamespace(ls=mods["light_source"], goe=mods["geo_optical_elements"],
                                    it=mods["iterative_tracer"], name="reference")
    return _loaded


def ours():
    """The drop-in's modules under the same names."""
    from lightpycl_amd import geo_optical_elements, light_source
    return types.SimpleNamespace(ls=light_source, goe=geo_optical_elements, it=None, name="lightpycl_amd")


@contextlib.contextmanager
def quiet():
    """Discard prints and warnings of the code inside."""
    with contextlib.redirect_stdout(io.StringIO()) as buf, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield buf


@contextlib.contextmanager
def reference_run():
    """Working directory at the reference, prints discarded, savefig / show no-ops."""
    import matplotlib.pyplot as plt
    import pylab
    cwd = os.getcwd()
    keep = (plt.savefig, plt.show, pylab.savefig, pylab.show)
    nop = lambda *a, **k: None  # noqa: E731
    plt.savefig = plt.show = pylab.savefig = pylab.show = nop
    os.chdir(reference_dir())
    try:
        with quiet() as buf:
            yield buf
    finally:
        os.chdir(cwd)
        plt.savefig, plt.show, pylab.savefig, pylab.show = keep
        plt.close("all")


# -- the catalogue: rays (section 2a) ------------------------------------------------------------
DIRECTIVITY = {"cos": lambda x, y: np.cos(y), "flat": lambda x, y: 1.0 + 0.0 * np.cos(y)}


def source_spec(ray_count, direction=(0, 0, 1), directivity="cos", power=1.0, center=(0, 0, 0, 0), then=()):
    return dict(ctor=dict(center=list(center), direction=list(direction), directivity=directivity, power=power,
                          ray_count=ray_count), then=[[m, kw] for m, kw in then])


def _ray_cases():
    cases = {}
    for seed in (1, 7, 21):
        for n in (1, 2, 500, 1500):
            for di, direction in enumerate(((0, 0, 1), (0, 0, -1), (0, 0.01, 1))):
                for dv in ("cos", "flat"):
                    cases["random_s%d_n%d_d%d_%s" % (seed, n, di, dv)] = dict(
                        seed=seed, sources=[source_spec(n, direction, dv, 1.0 if dv == "cos" else 1000.0)])
    for n in (1, 10, 500):                     # 10 -> 9 and 500 -> 484: the "next square" rule
        for di, direction in enumerate(((0, 0, 1), (0.3, -0.2, 1))):
            cases["grid_n%d_d%d" % (n, di)] = dict(seed=5, sources=[
                source_spec(n, direction, "cos", 2.0, (1, 2, 3, 0), then=[("grid_rays", {})])])
    for diameter in (1.0, 5.0):
        for di, direction in enumerate(((0, 0.01, 1), (1, 0, 0))):
            cases["collimated_%g_d%d" % (diameter, di)] = dict(seed=11, sources=[
                source_spec(300, direction, "flat", 1000.0, (0, 0, -10, 0),
                            then=[("random_collimated_rays", {"diameter": diameter})])])
    for axis in ("x", "y", "z", "q"):          # "q": the unknown-axis fallback
        cases["rotate_" + axis] = dict(seed=13, sources=[
            source_spec(200, (0, 0.01, 1), "cos", 10.0, (1, 0, 2, 0),
                        then=[("random_collimated_rays", {"diameter": 2.0}),
                              ("rotate_rays", {"axis": axis, "pivot": [0.5, -1.0, 2.0, 0], "ang": 0.7})])])
    cases["two_sources_one_seed"] = dict(seed=17, sources=[
        source_spec(120, (0, 0, 1), "cos", 1.0),
        source_spec(80, (0, 0.01, 1), "flat", 5.0, (0, 0, -10, 0), then=[("random_collimated_rays", {"diameter": 5.0})]),
        source_spec(50, (0, 0, -1), "cos", 2.0)])
    return cases


RAY_CASES = _ray_cases()


def make_source(M, spec):
    c = spec["ctor"]
    s = M.ls.light_source(center=np.array(c["center"], dtype=np.float32), direction=tuple(c["direction"]),
                          directivity=DIRECTIVITY[c["directivity"]], power=c["power"], ray_count=c["ray_count"])
    for meth, kw in spec.get("then", ()):
        getattr(s, meth)(**kw)
    return s


def run_ray_case(M, case):
    """-> {key: array}: every source's rays as the module leaves them."""
    out = {}
    with quiet():
        np.random.seed(case["seed"])
        for i, spec in enumerate(case["sources"]):
            s = make_source(M, spec)
            for k in ("rays_origin", "rays_dir", "rays_power"):
                out["s%d_%s" % (i, k)] = np.asarray(getattr(s, k))
            out["s%d_ray_count" % i] = np.asarray(s.ray_count)
    return out


# -- the catalogue: geometry (section 2b) ----------------------------------------------------------
_CURVE2 = [[1.0, 0.5], [2.0, 1.5]]
_CURVE5 = [[0.0, 0.0], [0.5, 1.0], [1.0, 1.25], [1.5, 1.0], [2.5, 0.25]]
_EYE = dict(r_cornea=5.0, r_lens=5.0, r_ac=7.8, d_ac=0.0, r_pc=6.5, d_pc=0.55, r_al=10.2, d_al=3.6, r_pl=-6.0,
            d_pl=7.6, r_r=-12.1, d_r=24.2)


def _eye_lens_args():
    e = _EYE
    return dict(
        cornea=dict(r1=e["r_ac"], r2=e["r_pc"], x1=e["d_ac"], x2=e["d_pc"], d=e["r_cornea"]),
        lens=dict(r1=e["r_al"], r2=e["r_pl"], x1=e["d_al"], x2=e["d_pl"], d=e["r_lens"]),
        aqueous=dict(r1=e["r_pc"], r2=e["r_al"], x1=e["d_pc"] * (1.0 + 1e-6), x2=e["d_al"] * (1.0 - 1e-6),
                     d=e["r_cornea"], d2=e["r_lens"]),
        vitreous=dict(r1=e["r_pl"], r2=e["r_r"] * (1.0 + 1e-6), x1=e["d_pl"] * (1.0 + 1e-6), x2=e["d_r"],
                      d=e["r_lens"], d2=e["r_lens"], sign2_arcsin=-1.0))


def _geo_cases():
    g = {}
    cube = dict(gen="cube", kwargs=dict(center=[0, 0, 20, 0], size=[10, 10, 10, 0]))
    g["cube"] = cube
    g["cube_offset"] = dict(gen="cube", kwargs=dict(center=[-20, 0, 22.5 * (1.0 - 1e-6), 0], size=[30, 30, 5, 0]))
    g["sphere"] = dict(gen="sphere", kwargs=dict(center=[30.0, -30.0, 100.0, 0], radius=10.0))
    g["hemisphere"] = dict(gen="hemisphere", kwargs=dict(center=[0, 0, 0, 0], radius=1000.0))
    g["hemisphere_retina"] = dict(gen="hemisphere", kwargs=dict(center=[0, 0, 12.1, 0], radius=12.1 * (1.0 - 1e-3)))
    g["parabolic_mirror"] = dict(gen="parabolic_mirror", kwargs=dict(focus=[0, 0, 0], focal_length=5.0, diameter=20.0,
                                                                     reflectivity=0.98))
    g["parabolic_mirror_offset"] = dict(gen="parabolic_mirror", kwargs=dict(focus=[1.0, 0.5, 0], focal_length=2.0,
                                                                            diameter=6.0, reflectivity=0.5))
    g["topless_cylinder"] = dict(gen="topless_cylinder", kwargs=dict(center=[0, 0, 0], diameter=20.0, height=10.0))
    g["topless_cylinder_offset"] = dict(gen="topless_cylinder", kwargs=dict(center=[1.0, 2.0, 0], diameter=3.0,
                                                                            height=4.0))
    for axis in ("x", "y", "z", "q"):
        for an, ang in (("2pi", 2 * np.pi), ("pi", np.pi), ("pi3", np.pi / 3)):
            for pts in (3, 36):
                for cn, curve in (("c2", _CURVE2), ("c5", _CURVE5)):
                    if pts == 36 and axis == "q":
                        continue               # the unknown-axis fallback: the 3-step sweeps only
                    g["revolve_%s_%s_%d_%s" % (axis, an, pts, cn)] = dict(
                        gen="revolve_curve", kwargs=dict(curve=curve, axis=axis, ang=ang, ang_pts=pts))
    g["extrude_open"] = dict(gen="extrude_by_vector", kwargs=dict(curve=_CURVE5, vector=[0.5, -0.25, 3.0],
                                                                 capped=False))
    g["lens_spherical_biconcave"] = dict(gen="lens_spherical_biconcave",
                                         kwargs=dict(focus=[0, 0, 0], r1=60., r2=6000., diameter=50.0, IOR=2.5))
    for name, kw in _eye_lens_args().items():
        g["spherical_lens_nofoc_" + name] = dict(gen="spherical_lens_nofoc", kwargs=kw)
    g["translate"] = dict(cube, then=[["translate", dict(vec=[1.5, -2.0, 0.25, 0])]])
    g["translate_revolve"] = dict(gen="revolve_curve", kwargs=dict(curve=_CURVE5, axis="x", ang=np.pi, ang_pts=4),
                                  then=[["translate", dict(vec=[1.5, -2.0, 0.25, 0])]])
    for axis in ("x", "y", "z", "q"):
        g["rotate_" + axis] = dict(cube, then=[["rotate", dict(axis=axis, angle=0.6, pivot=[1.0, -2.0, 3.0, 0])]])
        g["rotate_revolve_" + axis] = dict(gen="revolve_curve", kwargs=dict(curve=_CURVE5, axis="y", ang=np.pi / 3,
                                                                            ang_pts=3),
                                           then=[["rotate", dict(axis=axis, angle=-1.1, pivot=[0.5, 0.25, -1.0, 0])]])
    g["append"] = dict(cube, then=[["append_from", dict(gen="cube", kwargs=dict(center=[5, 5, 5, 0],
                                                                                size=[1, 2, 3, 0]))],
                                   ["append_from", dict(gen="revolve_curve", kwargs=dict(curve=_CURVE2, axis="z",
                                                                                         ang=np.pi, ang_pts=3))]])
    g["trimesh_roundtrip"] = dict(cube, then=[["trimesh_roundtrip", {}]])
    mats = dict(refractive=dict(mat_type="refractive", IOR=1.5, reflectivity=0.5, dissipation=0.1, AR_IOR=1.2,
                                AR_thickness=0.3),
                refractive_negative=dict(mat_type="refractive", IOR=-2.0),
                mirror=dict(mat_type="mirror", IOR=1.7, reflectivity=0.98, dissipation=0.2),
                terminator=dict(mat_type="terminator", IOR=1.7, reflectivity=0.3, dissipation=0.2),
                measure=dict(mat_type="measure", IOR=1.7, reflectivity=0.3, dissipation=0.2, AR_IOR=1.4),
                refractive_anisotropic=dict(mat_type="refractive_anisotropic", IOR=1.7, anisotropy=[1, 2, 3]),
                unknown=dict(mat_type="glass"),
                twice=dict(mat_type="mirror", reflectivity=0.9))
    for name, kw in mats.items():
        then = [["setMaterial", kw]]
        if name == "twice":                    # a refractive setting survives a later change of type
            then = [["setMaterial", mats["refractive"]], ["setMaterial", kw]]
        g["material_" + name] = dict(cube, then=then)
    return g


GEO_CASES = _geo_cases()
CURVE_CASES = {
    "lens_spherical_2r": dict(gen="lens_spherical_2r", kwargs=dict(focus=[0, 0, 0], r1=60., r2=6000., diameter=50.0,
                                                                   lens_sign=1, n=2.5)),
    "lens_spherical_2r_neg": dict(gen="lens_spherical_2r", kwargs=dict(focus=[1.0, -2.0], r1=40., r2=90.,
                                                                       diameter=15.0, lens_sign=-1, n=1.5)),
    "curve_lens_spherical_pp": dict(gen="curve_lens_spherical", kwargs=dict(focus=[0.0, 1.0], r1=30., diameter=20.,
                                                                            lens_direction=1, lens_sign=1, IOR=1.5)),
    "curve_lens_spherical_pn": dict(gen="curve_lens_spherical", kwargs=dict(focus=[0.0, 1.0], r1=30., diameter=20.,
                                                                            lens_direction=1, lens_sign=-1, IOR=1.5)),
    "curve_lens_spherical_np": dict(gen="curve_lens_spherical", kwargs=dict(focus=[2.0, 0.0], r1=30., diameter=20.,
                                                                            lens_direction=-1, lens_sign=1, IOR=1.7)),
    "curve_lens_spherical_nn": dict(gen="curve_lens_spherical", kwargs=dict(focus=[2.0, 0.0], r1=30., diameter=20.,
                                                                            lens_direction=-1, lens_sign=-1, IOR=1.7)),
    "curve_lens_spherical_biconcave": dict(gen="curve_lens_spherical_biconcave",
                                           kwargs=dict(focus=[0.0, 0.0], r1=30., r2=45., d=2.0, diameter=20.,
                                                       axis="x", IOR=1.5)),
}
#: generators and methods the reference cannot run here (no ``triangle``, no ``dxfwrite``, removed APIs)
CANNOT_RUN = ("optical_elements.curve_to_mesh", "optical_elements.extrude_by_vector(capped=True)",
              "GeoObject.write_dxf", "light_source.save_dxf", "CL_Tracer.save_traced_scene",
              "CL_Tracer.replicate_lightsources_and_plot", "CL_Tracer.plot_binned_data",
              "CL_Tracer.pickle_results", "CL_Tracer.load_pickle_results")


def make_geo(M, spec, raised=None):
    obj = getattr(M.goe.optical_elements(), spec["gen"])(**spec["kwargs"])
    for op, kw in spec.get("then", ()):
        try:
            if op == "append_from":
                other = make_geo(M, kw)
                obj.append(other.vertices, other.triangles)
            elif op == "trimesh_roundtrip":
                obj.trimesh_to_geoObject(obj.trimesh())
            else:
                getattr(obj, op)(**kw)
        except NameError as e:                 # the reference's unknown-material warning
            if raised is None:
                raise
            raised.append("%s: %s" % (op, type(e).__name__))
    return obj


def material_row(obj):
    b = obj.getMaterialBuf()
    return np.array([b["type"], b["IOR"], b["R"], b["dissipation"]], np.float64)


def geo_record(obj):
    tb = obj.tribuf()
    return dict(vertices=np.asarray(obj.vertices), triangles=np.asarray(obj.triangles), v0=np.asarray(tb[0]),
                v1=np.asarray(tb[1]), v2=np.asarray(tb[2]), material=material_row(obj),
                matType=np.array(str(obj.matType)), AR=np.array([obj.AR_IOR, obj.AR_thickness], np.float64))


def run_geo_case(M, spec):
    raised = []
    with quiet():
        out = geo_record(make_geo(M, spec, raised))
    out["raised"] = np.array(json.dumps(raised))
    return out


def run_curve_case(M, spec):
    with quiet():
        r = getattr(M.goe.optical_elements(), spec["gen"])(**spec["kwargs"])
    if isinstance(r, tuple):
        return dict(curve=np.asarray(r[0]), f=np.asarray(r[1]), d=np.asarray(r[2]))
    return dict(curve=np.asarray(r))


def random_cases(seed=2024, count=20):
    """Live mode's randomised argument sets: ``count`` per generator, from a seeded default_rng.
    -> (ray cases, geometry cases, curve cases)."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    ctr = lambda s=20.0: [u(-s, s), u(-s, s), u(-s, s), 0]  # noqa: E731
    rays, geo, curves = {}, {}, {}
    for i in range(count):
        direction = [u(-1, 1), u(-1, 1), u(-1, 1)] if i % 4 else [0, u(-1, 1), u(-1, 1)]
        dv = "cos" if i % 2 else "flat"
        n = int(rng.integers(1, 301))
        rays["random_%d" % i] = dict(seed=int(rng.integers(0, 2 ** 31)),
                                     sources=[source_spec(n, direction, dv, u(0.1, 1e3), ctr())])
        rays["grid_%d" % i] = dict(seed=0, sources=[source_spec(n, direction, dv, u(0.1, 1e3), ctr(),
                                                                then=[("grid_rays", {})])])
        rays["collimated_%d" % i] = dict(seed=int(rng.integers(0, 2 ** 31)), sources=[
            source_spec(n, direction, dv, u(0.1, 1e3), ctr(), then=[("random_collimated_rays",
                                                                     {"diameter": u(0.1, 10)})])])
        rays["rotate_%d" % i] = dict(seed=int(rng.integers(0, 2 ** 31)), sources=[
            source_spec(n, direction, dv, u(0.1, 1e3), ctr(),
                        then=[("rotate_rays", {"axis": "xyzXYZq"[i % 7], "pivot": ctr(), "ang": u(-7, 7)})])])
        geo["cube_%d" % i] = dict(gen="cube", kwargs=dict(center=ctr(), size=[u(.1, 50), u(.1, 50), u(.1, 50), 0]))
        curve = [[u(-5, 5), u(0, 5)] for _ in range(int(rng.integers(2, 7)))]
        geo["revolve_%d" % i] = dict(gen="revolve_curve", kwargs=dict(curve=curve, axis="xyzXYZq"[i % 7],
                                                                      ang=u(0.1, 2 * np.pi),
                                                                      ang_pts=int(rng.integers(3, 13))))
        geo["translate_rotate_%d" % i] = dict(geo["revolve_%d" % i], then=[
            ["translate", dict(vec=ctr())], ["rotate", dict(axis="xyzq"[i % 4], angle=u(-7, 7), pivot=ctr())],
            ["setMaterial", dict(mat_type=["refractive", "mirror", "measure", "terminator"][i % 4], IOR=u(-2, 3),
                                 reflectivity=u(0, 1), dissipation=u(0, 2))]])
        geo["extrude_%d" % i] = dict(gen="extrude_by_vector", kwargs=dict(curve=curve, vector=ctr()[:3],
                                                                         capped=False))
        geo["sphere_%d" % i] = dict(gen="sphere", kwargs=dict(center=ctr(), radius=u(0.5, 100)))
        geo["hemisphere_%d" % i] = dict(gen="hemisphere", kwargs=dict(center=ctr(), radius=u(0.5, 1000)))
        geo["parabolic_mirror_%d" % i] = dict(gen="parabolic_mirror", kwargs=dict(
            focus=ctr()[:3], focal_length=u(0.5, 10), diameter=u(1, 40), reflectivity=u(0, 1)))
        geo["topless_cylinder_%d" % i] = dict(gen="topless_cylinder", kwargs=dict(
            center=ctr()[:3], diameter=u(1, 40), height=u(1, 40)))
        r1, r2 = u(6, 20), u(6, 20)
        geo["spherical_lens_nofoc_%d" % i] = dict(gen="spherical_lens_nofoc", kwargs=dict(
            r1=r1, r2=-r2 if i % 2 else r2, x1=u(0, 3), x2=u(3, 6), d=u(1, 5), d2=u(1, 5),
            sign1_arcsin=1.0 if i % 3 else -1.0, sign2_arcsin=-1.0 if i % 2 else 1.0))
        geo["lens_spherical_biconcave_%d" % i] = dict(gen="lens_spherical_biconcave", kwargs=dict(
            focus=ctr()[:3], r1=u(60, 100), r2=u(100, 6000), diameter=u(5, 50), IOR=u(1.2, 2.5)))
        r1 = u(20, 60)
        curves["lens_spherical_2r_%d" % i] = dict(gen="lens_spherical_2r", kwargs=dict(
            focus=ctr()[:2], r1=r1, r2=u(20, 6000), diameter=u(1, 19), lens_sign=1 if i % 2 else -1, n=u(1.2, 2.5)))
        curves["curve_lens_spherical_%d" % i] = dict(gen="curve_lens_spherical", kwargs=dict(
            focus=ctr()[:2], r1=r1, diameter=u(1, 19), lens_direction=1 if i % 2 else -1,
            lens_sign=1 if i % 4 < 2 else -1, IOR=u(1.2, 2.5)))
        curves["curve_lens_spherical_biconcave_%d" % i] = dict(gen="curve_lens_spherical_biconcave", kwargs=dict(
            focus=ctr()[:2], r1=r1, r2=u(20, 60), d=u(0.5, 3), diameter=u(1, 19), axis="x", IOR=u(1.2, 2.5)))
    return rays, geo, curves


# -- the catalogue: scenes (section 2c), read off the reference's example scripts -----------------
_HALF = ((-np.pi / 2.0, np.pi / 2.0), (-np.pi / 2.0, np.pi / 2.0))
SCENE_CONSTANTS = {     # max_ray_len, ior_env, iterations, tau, histogram limits, histogram points
    "parabolic": dict(max_ray_len=1.0e3, ior_env=1.0, iterations=16, tau=0.99, hist_limits=_HALF, hist_points=100),
    "lens": dict(max_ray_len=2.0e3, ior_env=1.0, iterations=16, tau=0.99, hist_limits=_HALF, hist_points=30),
    "eye": dict(max_ray_len=4.0e1, ior_env=1.0, iterations=16, tau=0.99, hist_limits=_HALF, hist_points=90),
    "cube": dict(max_ray_len=2.0e3, ior_env=1.0, iterations=16, tau=0.99, hist_limits=_HALF, hist_points=30),
    "nested_cubes": dict(max_ray_len=2.0e2, ior_env=1.0, iterations=16, tau=0.99, hist_limits=_HALF,
                         hist_points=30),
}
SCENE_SIZES = dict(parabolic=(1500, 21), lens=(1500, 22), eye=(400, 23), cube=(1500, 24), nested_cubes=(10, 25))


def build_scene(M, name, n, seed, extra_sources=()):
    """(sources, meshes) of an example scene, call for call as the script makes them
    (example_directivity_parabolic_mirror.py:51-77, example_directivity_lens.py:48-68,
    example_human_eye.py:48-103, example_directivity_dissipative_cube.py:48-68,
    example_nested_cubes_refraction.py:52-85), np.random.seed(seed) first.
    ``extra_sources``: source specs constructed right after the script's own."""
    with quiet():
        np.random.seed(seed)
        zero = np.array([0, 0, 0, 0], dtype=np.float32)
        if name == "parabolic":
            ls0 = M.ls.light_source(center=zero, direction=(0, 0, -1), directivity=DIRECTIVITY["cos"], power=1.0,
                                    ray_count=n)
        elif name == "eye":
            ls0 = M.ls.light_source(center=np.array([0, 0, -10, 0], dtype=np.float32), direction=(0, 0.01, 1),
                                    directivity=DIRECTIVITY["flat"], power=1000., ray_count=n)
            ls0.random_collimated_rays(diameter=5.0)
        else:
            ls0 = M.ls.light_source(center=zero, direction=(0, 0, 1), directivity=DIRECTIVITY["cos"], power=1000.,
                                    ray_count=n)
        sources = [ls0] + [make_source(M, s) for s in extra_sources]
        oe = M.goe.optical_elements()
        if name == "parabolic":
            ms = oe.hemisphere(center=[0, 0, 0, 0], radius=500.0)
            ms.setMaterial(mat_type="measure")
            m2 = oe.parabolic_mirror(focus=(0, 0, 0), focal_length=5.0, diameter=20.0, reflectivity=0.98)
            m2.rotate(axis="y", angle=-np.pi / 2, pivot=(0, 0, 0, 0))
            meshes = [ms, m2]
        elif name == "lens":
            ms = oe.hemisphere(center=[0, 0, 0, 0], radius=1000.0)
            ms.setMaterial(mat_type="measure")
            m2 = oe.lens_spherical_biconcave(focus=(0, 0, 0), r1=60., r2=6000., diameter=50.0, IOR=2.5)
            m2.rotate(axis="y", angle=-np.pi / 2.0, pivot=(0, 0, 0, 0))
            meshes = [ms, m2]
        elif name == "cube":
            ms = oe.hemisphere(center=[0, 0, 0, 0], radius=1000.0)
            ms.setMaterial(mat_type="measure")
            m2 = oe.cube(center=(0, 0, 20, 0), size=[10, 10, 10, 0])
            m2.setMaterial(mat_type="refractive", IOR=1.0, dissipation=1.0)
            meshes = [ms, m2]
        elif name == "nested_cubes":
            meshes = []
            for ctr, size, ior in (((0, 0, 20, 0), [100, 100, 10, 0], 1.5),
                                   ((-20, 0, 22.5 * (1.0 - 1e-6), 0), [30, 30, 5, 0], -2.0),
                                   ((-20, 0, 27.5 * (1.0 + 1e-6), 0), [30, 30, 5, 0], -2.0),
                                   ((20, 0, 20, 0), [30, 30, 5, 0], -2.0)):
                m2 = oe.cube(center=ctr, size=size)
                m2.setMaterial(mat_type="refractive", IOR=ior)
                meshes.append(m2)
        elif name == "eye":
            e = _EYE
            retina = oe.hemisphere(center=[0, 0, e["d_r"] / 2.0, 0], radius=-e["r_r"] * (1.0 - 1e-3))
            retina.setMaterial(mat_type="measure")
            meshes = [retina]
            args = _eye_lens_args()
            for part, ior in (("cornea", 1.3771), ("lens", 1.4200), ("aqueous", 1.3374), ("vitreous", 1.336)):
                m = oe.spherical_lens_nofoc(**args[part])
                m.setMaterial(mat_type="refractive", IOR=ior)
                meshes.append(m)
        else:
            raise KeyError(name)
    return sources, meshes


def scene_record(sources, meshes):
    out = {}
    for i, s in enumerate(sources):
        for k in ("rays_origin", "rays_dir", "rays_power"):
            out["s%d_%s" % (i, k)] = np.asarray(getattr(s, k))
    for j, m in enumerate(meshes):
        tb = m.tribuf()
        for k in range(3):
            out["m%d_v%d" % (j, k)] = np.asarray(tb[k])
    out["materials"] = np.stack([material_row(m) for m in meshes])
    out["matTypes"] = np.array(json.dumps([str(m.matType) for m in meshes]))
    return out


def constants_record(c):
    return dict(max_ray_len=np.float32(c["max_ray_len"]), ior_env=np.float32(c["ior_env"]),
                iterations=np.int64(c["iterations"]), tau=np.float64(c["tau"]),
                hist_limits=np.array(c["hist_limits"], np.float64), hist_points=np.int64(c["hist_points"]))


# -- the catalogue: host loop and analyses (sections 2d, 2e) --------------------------------------
_SECOND = source_spec(200, (0, 0.01, 1), "flat", 500.0, (5.0, 0.0, 0.0, 0))
TRACE_CASES = {
    "parabolic": dict(scene="parabolic", n=1500, seed=21),
    "lens": dict(scene="lens", n=1500, seed=22),
    "eye": dict(scene="eye", n=400, seed=23),
    "cube": dict(scene="cube", n=1500, seed=24),
    "nested_cubes": dict(scene="nested_cubes", n=10, seed=25),
    "lens_two_sources": dict(scene="lens", n=300, seed=26, extra_sources=[_SECOND]),
    # trace_until_dissipated = 1: the threshold is 0, nothing is below it, the trace ends on the empty population
    "parabolic_until_empty": dict(scene="parabolic", n=500, seed=27, tau=1.0),
    "lens_four_iterations": dict(scene="lens", n=200, seed=28, iterations=4),
}
POLES = ([0, 0, 1, 0], [1, 0, 0, 0])
BEAM_POINTS = (90, 500)
STEREO_LIMITS = ((-1, 1), (-1, 1))


def trace_settings(case):
    c = dict(SCENE_CONSTANTS[case["scene"]])
    c["iterations"] = case.get("iterations", c["iterations"])
    c["tau"] = case.get("tau", c["tau"])
    return c


def beam_values(tracer, fn_name, **kw):
    """Call one of the reference's three beam functions (they return None) and read
    the quantities it prints from its frame as it returns."""
    names = dict(plot_elevation_histogram=("H", "x"),
                 get_beam_width_half_power=("pwr_cumsum", "elevation_hmax", "pwr_sum_hmax"),
                 get_beam_HWHM=("pwr0", "elevation_hmax", "pwr_sum_hmax"))[fn_name]
    got = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == fn_name and frame.f_locals.get("self") is tracer:
            got.update({k: frame.f_locals[k] for k in names})

    sys.setprofile(prof)
    try:
        ret = getattr(tracer, fn_name)(**kw)
    finally:
        sys.setprofile(None)
    assert ret is None and set(got) == set(names), (fn_name, ret, sorted(got))
    if fn_name == "plot_elevation_histogram":
        return dict(H=np.asarray(got["H"], np.float64), x=np.asarray(got["x"], np.float64))
    if fn_name == "get_beam_width_half_power":
        total = np.float64(got["pwr_cumsum"][-1])
    else:
        total = np.float64(np.asarray(sum(got["pwr0"])).reshape(-1)[0])       # the reference's sum(pwr0)
    return dict(total=total, elevation=np.asarray(got["elevation_hmax"], np.float64).reshape(-1),
                power=np.asarray(got["pwr_sum_hmax"], np.float64).reshape(-1))


def run_trace_case(M, case):
    """The reference's CL_Tracer on a trace case -> (record, stop reason, tracer)."""
    c = trace_settings(case)
    sources, meshes = build_scene(M, case["scene"], case["n"], case["seed"], case.get("extra_sources", ()))
    with reference_run() as buf:
        tr = M.it.CL_Tracer(platform_name="oracle", device_name="oracle")
        results = tr.iterative_tracer(light_source=sources, meshes=meshes, trace_iterations=c["iterations"],
                                      trace_until_dissipated=c["tau"], max_ray_len=np.float32(c["max_ray_len"]),
                                      ior_env=np.float32(c["ior_env"]))
        text = buf.getvalue()
        out = dict(iterations=np.int64(len(results)), counts=np.array([len(r[3]) for r in results], np.int64),
                   mesh_power=tr.prg.mesh_power.copy())
        for i, r in enumerate(results):
            for k, name in enumerate(("origin", "dest", "pow", "meas")):
                out["it%02d_%s" % (i, name)] = np.asarray(r[k])
        pos, pwr = tr.get_measured_rays()
        n_meas = 0 if pos is None else int(np.asarray(pos).shape[0])
        out["measured_count"] = np.int64(n_meas)
        if n_meas:
            out["measured_pos"], out["measured_pwr"] = np.asarray(pos), np.asarray(pwr)
            for mode, fn, lim in (("angular", tr.get_binned_data_angular, c["hist_limits"]),
                                  ("stereo", tr.get_binned_data_stereographic, STEREO_LIMITS)):
                H, xe, ye = fn(limits=lim, points=c["hist_points"])
                out[mode + "_H"], out[mode + "_xe"], out[mode + "_ye"] = H, xe, ye
            for p, pole in enumerate(POLES):
                for npts in BEAM_POINTS:
                    for short, fn in (("hist", "plot_elevation_histogram"), ("half", "get_beam_width_half_power"),
                                      ("hwhm", "get_beam_HWHM")):
                        # beam_values reads the function's frame through sys.setprofile: CPython only,
                        # and no other profiler (coverage, cProfile) may be active around this call
                        for k, v in beam_values(tr, fn, points=npts, pole=pole).items():
                            out["%s_p%d_n%d_%s" % (short, p, npts, k)] = v
    stop = ("threshold" if "Scene power is below" in text else "empty" if "No rays left" in text else "iterations")
    out["stop"] = np.array(stop)
    return out, stop, tr


#: keys of a trace record that are float64 analysis outputs: always stored in full (compared with a tolerance)
def is_analysis_key(k):
    return k.split("_")[0] in ("angular", "stereo", "hist", "half", "hwhm")


# -- fixtures -------------------------------------------------------------------------------------
def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digested(key, a):
    """The members that stand for an array too large for its file: shape, dtype, SHA-256, every 97th row."""
    return {key + "__shape": np.array(a.shape, np.int64), key + "__dtype": np.array(a.dtype.str),
            key + "__sha256": np.array(digest(a)), key + "__rows97": np.ascontiguousarray(a[::97])}


def _member(a):
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
    return buf.getvalue()


def _member_cost(name, a):
    """Bytes a member adds to the .npz: its deflated data, local header and central directory entry."""
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    return len(c.compress(_member(a))) + len(c.flush()) + 76 + 2 * len(name + ".npy")


def choose_members(arrays, always_full=(), budget=None):
    """{member: array} of a fixture file.  Everything is stored in full that fits the file: the arrays
    are taken whole in the order of what that costs over their digested form (cheapest first) for as
    long as the file stays within ``budget``; the rest are digested.  ``always_full``: keys stored whole
    whatever they cost (the float64 analysis outputs, which are compared with a tolerance)."""
    budget = FILE_BUDGET if budget is None else budget
    out, total, cand = {}, 0, []
    for k in sorted(arrays):
        a = np.asarray(arrays[k])
        full = _member_cost(k, a)
        if a.ndim == 0 or k in always_full:
            out[k] = a
            total += full
            continue
        dig = _digested(k, a)
        dcost = sum(_member_cost(n, v) for n, v in dig.items())
        cand.append((full - dcost, k, a, dig))
        total += dcost
    for extra, k, a, dig in sorted(cand, key=lambda c: (c[0], c[1])):
        if extra <= 0 or total + extra <= budget:
            out[k] = a
            total += extra
        else:
            out.update(dig)
    return out


def unpacked_keys(fix, prefix):
    """The keys stored under ``prefix/`` (full or digested), without the prefix."""
    keys = set()
    for k in fix:
        if k.startswith(prefix + "/"):
            keys.add(k[len(prefix) + 1:].split("__")[0])
    return sorted(keys)


def check(fix, key, got, what=""):
    """assert that ``got`` is the array recorded under ``key``: shape, dtype and every element (or,
    for a digested array, the sampled rows first and then the digest)."""
    got = np.asarray(got)
    if key in fix:
        want = fix[key]
        assert got.shape == want.shape and got.dtype == want.dtype, (what, key, got.shape, got.dtype, want.shape,
                                                                     want.dtype)
        np.testing.assert_array_equal(got, want, err_msg="%s %s" % (what, key))
        return
    assert key + "__sha256" in fix, "%s: fixture has no %s" % (what, key)
    assert got.shape == tuple(fix[key + "__shape"]) and got.dtype.str == str(fix[key + "__dtype"]), \
        (what, key, got.shape, got.dtype.str, tuple(fix[key + "__shape"]), str(fix[key + "__dtype"]))
    np.testing.assert_array_equal(got[::97], fix[key + "__rows97"], err_msg="%s %s, rows [::97]" % (what, key))
    assert digest(got) == str(fix[key + "__sha256"]), "%s %s: SHA-256 differs (sampled rows agree)" % (what, key)


def save_npz(path, arrays, args, always_full=()):
    """A deterministic .npz (fixed member order and time stamps) of ``arrays``, each in full if the
    file's 128 KB allow it (:func:`choose_members`)."""
    meta_cost = len(json.dumps(args, sort_keys=True)) // 2 + 1024
    arrays = choose_members(arrays, always_full, FILE_BUDGET - meta_cost)
    arrays["args"] = np.array(json.dumps(args, sort_keys=True))
    arrays["source"] = np.array(SOURCE)
    arrays["numpy"] = np.array(np.__version__)
    with zipfile.ZipFile(path, "w") as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, _member(arrays[k]), compresslevel=9)
    size = os.path.getsize(path)
    assert size <= FILE_LIMIT, "%s: %d bytes > %d" % (path, size, FILE_LIMIT)
    return size


def ray_groups():
    """Fixture file -> ray case names (a file per seed of the constructor cases)."""
    g = {}
    for name in RAY_CASES:
        f = "rays_seed%s" % name.split("_")[1][1:] if name.startswith("random_") else "rays_other"
        g.setdefault(f, []).append(name)
    return g


def geo_groups():
    g = {}
    big = ("sphere", "hemisphere", "parabolic_mirror", "topless_cylinder", "spherical_lens_nofoc",
           "lens_spherical_biconcave")
    for name, spec in GEO_CASES.items():
        f = ("revolve_" + spec["kwargs"]["axis"] if name.startswith("revolve_") else
             spec["gen"] if spec["gen"] in big else "small")
        g.setdefault("geometry_" + f, []).append(name)
    return g


FIXTURE_FILES = (sorted(ray_groups()) + sorted(geo_groups()) + ["curves"] + ["scene_" + n for n in SCENE_SIZES] +
                 ["trace_" + t for t in TRACE_CASES] + ["analyses_" + t for t in TRACE_CASES])


def generate(out_dir=FIXTURE_DIR, log=print):
    M = load()
    os.makedirs(out_dir, exist_ok=True)
    sizes = {}

    def grouped(groups, cases, run):
        for fname, names in groups.items():
            arrs = {}
            for name in names:
                for k, v in run(M, cases[name]).items():
                    arrs[name + "/" + k] = v
            sizes[fname] = save_npz(os.path.join(out_dir, fname + ".npz"), arrs, {n: cases[n] for n in names})

    grouped(ray_groups(), RAY_CASES, run_ray_case)
    grouped(geo_groups(), GEO_CASES, run_geo_case)
    grouped({"curves": list(CURVE_CASES)}, CURVE_CASES, run_curve_case)
    for name, (n, seed) in SCENE_SIZES.items():
        arrs = {}
        for k, v in scene_record(*build_scene(M, name, n, seed)).items():
            arrs[name + "/" + k] = v
        for k, v in constants_record(SCENE_CONSTANTS[name]).items():
            arrs[name + "/" + k] = v
        sizes["scene_" + name] = save_npz(os.path.join(out_dir, "scene_%s.npz" % name), arrs, dict(n=n, seed=seed))
    stops = {}
    for name, case in TRACE_CASES.items():
        rec, stops[name], _ = run_trace_case(M, case)
        arrs = {k: v for k, v in rec.items() if not is_analysis_key(k)}     # the loop's record and the
        ana = {k: v for k, v in rec.items() if is_analysis_key(k)}          # analyses: a file each
        ana["measured_count"] = rec["measured_count"]
        sizes["trace_" + name] = save_npz(os.path.join(out_dir, "trace_%s.npz" % name), arrs, case)
        sizes["analyses_" + name] = save_npz(os.path.join(out_dir, "analyses_%s.npz" % name), ana, case,
                                             always_full=set(ana))
    # both break conditions of the loop (iterative_tracer.py:383, :389) and the iteration cap are reached
    assert {"threshold", "empty", "iterations"} <= set(stops.values()), stops
    for k in sorted(sizes):
        log("%-28s %7d bytes" % (k + ".npz", sizes[k]))
    log("stop reasons: " + json.dumps(stops, sort_keys=True))
    return sizes


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE_DIR, help="directory of the fixtures (default: tests/golden/ref_host)")
    ap.add_argument("--reference", default=None, help="the reference's directory (default: $LPC_REFERENCE_DIR or "
                                                      "/root/reference)")
    a = ap.parse_args()
    if a.reference:
        set_reference_dir(a.reference)
    ok, why = available()
    if not ok:
        sys.exit("ref_host: " + why)
    generate(a.out)
