"""CPU tests of the surface map: the host reference helper (tests/surface_ref.py)
over the CPU oracle -- per mesh its deposited terms are the power budget's
absorbed + terminated + measured terms -- the premise of the constructed strip of
the GPU tests, and the library surface as far as it runs without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import budget_ref
import surface_ref
from test_budget_host import CASES, case_scene, rays_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REFS = {}


def cpu_reference(oracle_mod, name):
    if name not in _REFS:
        sc = case_scene(name)
        o, d, p = rays_of(sc)
        _REFS[name] = surface_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                        sc.ior_env, with_budget=True)
    return _REFS[name]


@pytest.mark.parametrize("name", CASES)
def test_deposited_is_the_budgets_mesh_term(oracle_mod, name):
    """Per mesh, the helper's deposited terms and budget_ref's absorbed +
    terminated + measured terms of the same bounces are one multiset; the
    incident terms are the hits' powers; every triangle belongs to its mesh."""
    ref = cpu_reference(oracle_mod, name)
    bud = ref["budget"]
    sc = case_scene(name)
    scene = oracle_mod.Scene(sc.meshes)
    assert ref["M"] == scene.tri_count and ref["K"] == len(sc.meshes)
    assert len(ref["tri"]) > 0
    assert ref["tri"].min() >= 0 and ref["tri"].max() < ref["M"]
    assert np.array_equal(scene.mesh_id[ref["tri"]], ref["mesh"])
    n_hits = 0
    for m in range(ref["K"]):
        want = np.concatenate([budget_ref.mesh_terms(bud, c, m) for c in ("absorbed", "terminated", "measured")])
        got = surface_ref.mesh_deposited(ref, m)
        assert len(got) == len(want), (name, m, len(got), len(want))
        assert np.array_equal(np.sort(got).view(np.int64), np.sort(want).view(np.int64)), (name, m)
        n_hits += len(got)
    t = budget_ref.totals(bud)
    assert n_hits == len(ref["tri"]) == t["absorbed"] + t["terminated"] + t["measured"]
    assert n_hits == t["power_in"] - t["escaped"]
    # incident differs from deposited exactly where a child was kept
    if name in ("eye", "mixed", "nested_cubes"):
        assert (ref["incident"] != ref["deposited"]).any()
    assert len(surface_ref.by_triangle(ref)) == len(np.unique(ref["tri"]))


STRIP_N = 6200      # more than 3 + 3 * 2 * table triangles: the conflict patterns fit


@pytest.mark.parametrize("kinds", [("terminator",), ("terminator", "measure", "mirror")])
def test_strip_premise(oracle_mod, kinds):
    """Under the CPU oracle every ray of the constructed strip hits its intended
    triangle, no ray excluded, and the helper's sums are the host's integer sums."""
    from lightpycl_amd import _lib
    meshes = surface_ref.strip_scene(STRIP_N, kinds)
    assert len(meshes) == -(-STRIP_N // surface_ref.STRIP_MESH)
    scale = 1.0 if kinds == ("terminator",) else 0.125
    pats = surface_ref.strip_patterns(4160, STRIP_N, _lib.SURFACE_LDS_ENTRIES)
    assert {"one", "own", "scatter7", "run3", "run64", "run65", "run100", "mod1024", "mod2048"} <= set(pats)
    for pname in ("scatter7", "mod2048", "run65"):
        t = pats[pname]
        o, d, p = surface_ref.strip_rays(t, scale)
        ref = surface_ref.trace(oracle_mod, meshes, o, d, p, 2, 1.0, np.float32(1e3), np.float32(1.0))
        first = ref["iters"][0]
        assert np.array_equal(first["tri"], t), (kinds, pname)
        assert np.array_equal(first["mesh"], t // surface_ref.STRIP_MESH)
        assert len(ref["tri"]) == len(t), "children of the mirrors hit nothing"
        want = surface_ref.strip_expected(STRIP_N, t, p, kinds)
        surface_ref.assert_surface(want, ref, f"{kinds} {pname}")
        if len(kinds) > 1 and pname != "run65":         # (run65's 64 targets are all of the first mesh)
            assert (want["incident"] != want["deposited"]).any()
        else:
            assert np.array_equal(want["incident"], want["deposited"])


def test_host_api():
    """The library exports the entry points, lpc.h declares them and the rule, the
    ABI version stays, _lib.py binds them and the Python layers take the keyword."""
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    L = _lib.load()
    assert L.lpc_abi_version() == 4
    for name in ("lpc_trace_set_surface", "lpc_trace_surface"):
        assert name in _lib.EXPORTED
        getattr(L, name)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib._PROTOS["lpc_trace_set_surface"] == [P, ctypes.c_int]
    assert _lib._PROTOS["lpc_trace_surface"] == [P, P, P, P, I64, P]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lpc.h")).read())
    assert "int lpc_trace_set_surface(lpc_handle *h, int on);" in hdr
    assert ("int lpc_trace_surface(lpc_handle *h, double *incident, double *deposited, int64_t *count, "
            "int64_t tri_cap, int64_t *tri_count);") in hdr
    assert "#define LPC_ABI_VERSION 4" in hdr
    assert f"#define LPC_SURFACE_LDS_ENTRIES {_lib.SURFACE_LDS_ENTRIES}" in hdr
    assert _lib.SURFACE_LDS_ENTRIES & (_lib.SURFACE_LDS_ENTRIES - 1) == 0
    assert _lib.SURFACE_COLUMNS == ("incident", "deposited", "count")
    # a null handle and a null count are refused
    m = ctypes.c_int64(7)
    assert L.lpc_trace_set_surface(None, 1) == -1
    assert L.lpc_trace_surface(None, None, None, None, 0, ctypes.byref(m)) == -1 and m.value == 7
    # the Python surface
    from lightpycl_amd.distributed import ShardedTrace  # noqa: F401
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import CL_Tracer
    from lightpycl_amd.pool import TracePool
    assert callable(Engine.set_surface) and callable(Engine.surface) and callable(CL_Tracer.surface_power)
    for fn in (CL_Tracer.iterative_tracer, TracePool.submit):
        assert inspect.signature(fn).parameters["surface_map"].default is False


def test_surface_dict_on_the_host():
    """surface_dict slices the flat arrays per mesh in the meshes' own triangle
    order and divides by float64 areas; a zero-area sliver is not hidden."""
    from lightpycl_amd.iterative_tracer import surface_dict, triangle_areas
    meshes = surface_ref.strip_scene(130)
    V = np.array(meshes[1].vertices, np.float64)
    V[3:6] = V[3]                               # triangle 1 of mesh 1: a point
    meshes[1].vertices = V
    area = triangle_areas(meshes[0])
    assert area.dtype == np.float64 and np.allclose(area, 0.375, rtol=0, atol=0)
    s = dict(incident=np.arange(130, dtype=np.float64), deposited=2.0 * np.arange(130), count=np.arange(130))
    d = surface_dict(s, meshes)
    assert d["offsets"] == [0, 64, 128] and [len(m["count"]) for m in d["meshes"]] == [64, 64, 2]
    assert d["incident"] is not None and len(d["deposited"]) == 130
    m1 = d["meshes"][1]
    assert m1["offset"] == 64 and m1["incident"][0] == 64.0 and m1["area"][1] == 0.0
    assert np.isinf(m1["irradiance"][1]) and np.isinf(m1["incident_irradiance"][1])
    assert m1["irradiance"][0] == 2.0 * 64 / 0.375 and m1["incident_irradiance"][2] == 66 / 0.375
    with pytest.raises(ValueError):
        surface_dict(dict(incident=np.zeros(3), deposited=np.zeros(3), count=np.zeros(3, np.int64)), meshes)


class _StubEngine:
    """An engine's ledger readers over fixed arrays (one rank of a sharded trace)."""

    def __init__(self, seed, iters=3, K=2, M=7, min_power=1e-6, budget_on=True, surface_on=True):
        from lightpycl_amd import _lib
        rng = np.random.default_rng(seed)
        self.min_power, self.budget_on, self.surface_on = min_power, budget_on, surface_on
        self.reads = []
        self._culled = (rng.integers(0, 50, iters), rng.random(iters))
        self._budget = {k: rng.random(iters) for k in _lib.BUDGET_SUMS}
        self._budget.update({k: rng.integers(0, 1000, iters) for k in _lib.BUDGET_COUNTS})
        self._budget.update(mesh_power=rng.random((K, 4)), mesh_count=rng.integers(0, 1000, (K, 4)))
        self._surface = dict(incident=rng.random(M), deposited=rng.random(M), count=rng.integers(0, 9, M))

    def culled(self):
        self.reads.append("culled")
        return self._culled

    def budget(self):
        self.reads.append("budget")
        return self._budget

    def surface(self):
        self.reads.append("surface")
        return self._surface


def _same(a, b, what=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            _same(a[k], b[k], f"{what}/{k}")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), what
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


def test_read_ledgers_on_the_host():
    """read_ledgers returns only what is on; with a summing ``reduce`` over two
    stub ranks it equals the dicts built from the element-wise sums (counts as
    int64), every rank exchanging vectors of the same sizes in the same order,
    the map's tables in pieces."""
    from lightpycl_amd import _lib
    from lightpycl_amd.ledgers import budget_dict, read_ledgers
    # one engine, no reduce: the readers' own values, and only those that are on
    e = _StubEngine(1)
    got = read_ledgers(e)
    assert list(got) == ["culled_counts", "culled_power", "power_budget", "surface"]
    assert e.reads == ["culled", "budget", "surface"]
    assert got["culled_counts"] == [int(v) for v in e._culled[0]] and all(type(v) is int for v in got["culled_counts"])
    assert got["culled_power"] == [float(v) for v in e._culled[1]]
    _same(got["power_budget"], budget_dict(e._budget, *e._culled), "budget")
    assert got["surface"] is e._surface
    off = _StubEngine(1, min_power=0.0, budget_on=False, surface_on=False)
    assert read_ledgers(off) == {} and off.reads == []
    only = _StubEngine(1, min_power=0.0, surface_on=False)
    got = read_ledgers(only)
    assert list(got) == ["power_budget"] and only.reads == ["budget"]
    assert not got["power_budget"]["n_culled"].any() and not got["power_budget"]["culled"].any()
    assert read_ledgers(object()) == {}             # an engine without the switches has no ledgers
    # two ranks: rank 1's vectors are recorded, rank 0's reduce adds them in order
    iters, piece = 3, 5
    r0, r1 = _StubEngine(2), _StubEngine(3)
    sent = []

    def record(v):
        assert v.dtype == np.float64 and v.ndim == 1
        sent.append(v.copy())
        return v

    read_ledgers(r1, reduce=record, iterations=iters, piece=piece)
    M, K = 7, 2
    assert [len(v) for v in sent] == [2 * iters, 13 * iters + 8 * K] + [5, 5, 5, 5, 1], [len(v) for v in sent]
    pending = list(sent)

    def add(v):
        w = pending.pop(0)
        assert v.dtype == np.float64 and v.shape == w.shape
        return v + w

    got = read_ledgers(r0, reduce=add, iterations=iters, piece=piece)
    assert not pending and 3 * M > piece
    cc = r0._culled[0] + r1._culled[0]
    cp = r0._culled[1] + r1._culled[1]
    b = {k: r0._budget[k] + r1._budget[k] for k in r0._budget}
    s = {k: r0._surface[k] + r1._surface[k] for k in _lib.SURFACE_COLUMNS}
    assert got["culled_counts"] == [int(v) for v in cc] and got["culled_power"] == [float(v) for v in cp]
    _same(got["power_budget"], budget_dict(b, cc, cp), "summed budget")
    for k in _lib.BUDGET_COUNTS + ("n_culled",):
        assert got["power_budget"][k].dtype == np.int64
    assert all(v.dtype == np.int64 for v in got["power_budget"]["mesh_count"].values())
    _same(got["surface"], s, "summed surface")
    assert got["surface"]["count"].dtype == np.int64 and got["surface"]["incident"].dtype == np.float64
