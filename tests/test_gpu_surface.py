"""GPU tests of the surface map (lpc_trace_set_surface / lpc_trace_surface).

1. A constructed strip of terminator triangles (tests/surface_ref.py): every
   ray's triangle and power are chosen, the powers are integers (or integers
   scaled by a power of two) and every sum is below 2^53 of its unit, so the three
   columns must equal the host's integer sums bit for bit in any atomic order.
2. Every trace path against the host helper over the reference's OWN kernels
   when they are built, else over the CPU oracle: counts exactly, every float64 sum
   within (n - 1) 2^-53 sum|terms| of the exactly rounded sum of the helper's terms.
3. Speculation and lifetime, 4. argument checks, 5. pool and two processes.

Each reference trace is computed once."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

import budget_ref
import cutoff_ref
import surface_ref
from test_budget_host import CASES, case_scene, rays_of
from test_gpu_budget import _engine_trace, _free_port, _live_bytes, _stats_bits, _thr, _trace_kw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SIZES = [1, 63, 64, 65, 255, 256, 257, 4160, 70001]
STRIP_N = 6200                  # the conflict patterns need 3 + 3 * 2 * table < N triangles
MRL, IOR = np.float32(1e3), np.float32(1.0)


def _table():
    from lightpycl_amd import _lib
    return _lib.SURFACE_LDS_ENTRIES


# -- 1. the constructed strip, exact --------------------------------------------------
_STRIPS = {}


@pytest.fixture(scope="module")
def strips():
    """Engines on strips, one per (triangle count, kinds), opened on first use."""
    from lightpycl_amd.engine import Engine

    def get(N, kinds=("terminator",)):
        key = (N, kinds)
        if key not in _STRIPS:
            e = Engine(0)
            e.upload_meshes(surface_ref.strip_scene(N, kinds))
            e.set_surface(True)
            _STRIPS[key] = e
        return _STRIPS[key]

    yield get
    for e in _STRIPS.values():
        e.close()
    _STRIPS.clear()


def _strip_trace(e, targets, scale=1.0):
    o, d, p = surface_ref.strip_rays(targets, scale)
    e.set_rays(o, d, p, MRL, IOR)
    stats, _ = e.run_local(2, 0.0)
    assert int(stats[0].n_in) == len(targets)
    return p, e.surface()


def _assert_exact(got, want, what):
    for k in ("count", "incident", "deposited"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])


@pytest.mark.parametrize("n", SIZES)
def test_strip_exact(strips, n):
    """All rays on one triangle, runs of equal targets, a scatter, and targets that
    share an entry of the kernel's LDS table: bit-equal to the host's sums."""
    e = strips(STRIP_N)
    pats = surface_ref.strip_patterns(n, STRIP_N, _table())
    want_names = {"one", "scatter7", "run3", "run64", "run65", "run100", f"mod{_table()}", f"mod{2 * _table()}"}
    if n <= STRIP_N:
        want_names.add("own")
    if n == 70001:
        want_names -= {"run3"}                  # 23 334 targets: the strip of test_strip_own_triangle_each has them
    assert set(pats) == want_names, sorted(pats)
    for name, t in pats.items():
        p, got = _strip_trace(e, t)
        assert float(p.astype(np.float64).sum()) < 2.0 ** 53
        _assert_exact(got, surface_ref.strip_expected(STRIP_N, t, p), f"{name} n={n}")


def test_strip_own_triangle_each(strips):
    """70 001 rays, each on a triangle of its own, and runs of 3 over 23 334
    triangles: the spread extreme (1 094 meshes)."""
    n = 70001
    e = strips(n)
    pats = surface_ref.strip_patterns(n, n, _table())
    for name in ("own", "run3"):
        p, got = _strip_trace(e, pats[name])
        _assert_exact(got, surface_ref.strip_expected(n, pats[name], p), f"{name} n={n}")
    assert int(got["count"].max()) == 3 and int(np.count_nonzero(got["count"])) == 23334


@pytest.mark.parametrize("n", SIZES)
def test_strip_measure_and_mirror(strips, n):
    """A measure mesh and a mirror with R = 0.5 between the terminators, powers
    (i + 1) / 8: deposited stays exact and is half the incident power on the mirror."""
    kinds = ("terminator", "measure", "mirror")
    e = strips(STRIP_N, kinds)
    pats = surface_ref.strip_patterns(n, STRIP_N, _table())
    mirror = np.array([(j // surface_ref.STRIP_MESH) % 3 == 2 for j in range(STRIP_N)])
    hit = np.zeros(STRIP_N, bool)
    names = [k for k in ("scatter7", "own", f"mod{_table()}", f"mod{2 * _table()}", "run3", "run65") if k in pats]
    assert len(names) >= 4
    for name in names:
        t = pats[name]
        p, got = _strip_trace(e, t, 0.125)
        want = surface_ref.strip_expected(STRIP_N, t, p, kinds)
        _assert_exact(got, want, f"mixed {name} n={n}")
        assert np.array_equal(got["deposited"][mirror], 0.5 * got["incident"][mirror])
        assert np.array_equal(got["deposited"][~mirror], got["incident"][~mirror])
        hit |= got["count"] > 0
    assert (hit & ~mirror).any() and (n < 65 or (hit & mirror).any())


@pytest.mark.parametrize("chunk", [256, 257, 1000])
def test_strip_chunks(chunk):
    """Several chunks per iteration add to one staging table."""
    from lightpycl_amd.engine import Engine
    n = 4160
    e = Engine(0)
    try:
        e.upload_meshes(surface_ref.strip_scene(STRIP_N))
        e.set_chunk(chunk)
        e.set_surface(True)
        pats = surface_ref.strip_patterns(n, STRIP_N, _table())
        for name in ("one", "scatter7", "run100", f"mod{2 * _table()}"):
            p, got = _strip_trace(e, pats[name])
            _assert_exact(got, surface_ref.strip_expected(STRIP_N, pats[name], p), f"{name} chunk {chunk}")
    finally:
        e.close()


# -- 2. against the reference ---------------------------------------------------------
_REFS = {}


def _case(oracle_mod, checker, name, f=0.0):
    """(scene, rays, cut, the helper's reference with the budget's of the same bounces)."""
    sc = case_scene(name)
    o, d, p = rays_of(sc)
    cut = cutoff_ref.cut_of(p, f) if f else np.float32(0.0)
    key = (name, f)
    if key not in _REFS:
        _REFS[key] = surface_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                       sc.ior_env, cut=cut, bounce_fn=checker[0], with_budget=True)
    ref = _REFS[key]
    assert len(ref["tri"]) > 0 and len(ref["iters"]) >= 1
    return sc, (o, d, p), cut, ref


def _assert_tracer_dict(s, sc, ref, what):
    """CL_Tracer.surface_power(): the flat arrays against the helper, the per-mesh
    slices against the flat arrays and the meshes' own triangles."""
    surface_ref.assert_surface(s, ref, what)
    assert len(s["meshes"]) == len(sc.meshes) == len(s["offsets"])
    lo = 0
    for m, g in zip(s["meshes"], sc.meshes):
        k = len(np.asarray(g.triangles))
        assert m["offset"] == lo and len(m["count"]) == k == len(m["area"])
        for col in ("incident", "deposited", "count"):
            assert np.array_equal(m[col], s[col][lo:lo + k], equal_nan=True)
        V, T = np.asarray(g.vertices, np.float64), np.asarray(g.triangles)
        a = 0.5 * np.linalg.norm(np.cross(V[T[:, 1], :3] - V[T[:, 0], :3], V[T[:, 2], :3] - V[T[:, 0], :3]), axis=1)
        assert np.array_equal(m["area"], a)
        ok = a > 0
        assert np.array_equal(m["irradiance"][ok], m["deposited"][ok] / a[ok])
        assert np.array_equal(m["incident_irradiance"][ok], m["incident"][ok] / a[ok])
        lo += k
    assert lo == ref["M"]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_modes(oracle_mod, checker, name, keep):
    """Aggregate mode (k_shade_stage's record) and results mode (k_shade_bud's)."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, _, ref = _case(oracle_mod, checker, name)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, surface_map=True))
        s = tr.surface_power()
        assert s is not None and tr.power_budget() is None
        assert list(tr.iteration_counts) == ref["counts"]
        _assert_tracer_dict(s, sc, ref, f"{name} keep={keep}")
        # a second trace on the same tracer: the map was cleared, not accumulated
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, surface_map=True))
        s2 = tr.surface_power()
        surface_ref.assert_surface(s2, ref, f"{name} keep={keep}, second trace")
        assert np.array_equal(s2["count"], s["count"])
        # and a trace without it reads None, the engine zeros
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep))
        assert tr.surface_power() is None
        z = tr.engine.surface()
        assert len(z["count"]) == ref["M"] and not z["count"].any() and not z["incident"].any()
    finally:
        tr.engine.close()


@pytest.mark.parametrize("path", ["chunks", "resort", "traced0", "staged", "rerun"])
@pytest.mark.parametrize("name", ["eye", "mixed"])
def test_paths(oracle_mod, checker, monkeypatch, name, path):
    """The trace paths of test_gpu_budget.py::test_paths, three traces each (the
    later ones on the first's speculation history)."""
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, name)
    if path == "resort":
        monkeypatch.setenv("LPC_RESORT_MIN", "1000")
    if path == "traced0":
        monkeypatch.setenv("LPC_TRACED", "0")
    thr = _thr(sc, p)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        if path == "chunks":
            e.set_chunk(1000)
            assert max(ref["counts"]) > 1000
        e.set_surface(True)
        first = None
        for rep in range(3):
            if path == "staged":
                e.stage_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _ = e.run_staged(sc.iterations, thr)
            elif path == "rerun":
                if rep == 0:
                    e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _ = e.run_local(sc.iterations, thr, reset=True)
            else:
                if rep == 0:
                    e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _, _ = _engine_trace(e, sc, thr)
            s = e.surface()
            assert [int(st.n_in) for st in stats] == ref["counts"]
            surface_ref.assert_surface(s, ref, f"{name} {path} trace {rep}")
            assert first is None or np.array_equal(s["count"], first)
            first = s["count"] if first is None else first
    finally:
        e.close()


def test_all_ledgers_chunked(oracle_mod, checker):
    """The cutoff, the budget and the map on one handle, several chunks per
    iteration, three traces (the later ones on the first's speculation history):
    the three ledgers share one slot per iteration, and each equals its helper's
    with equal exact parts in every trace."""
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import budget_dict
    sc, (o, d, p), cut, ref = _case(oracle_mod, checker, "eye", 1e-6)
    assert sum(len(c) for c in ref["budget"]["culled"]) > 0, "the case must cull"
    thr = _thr(sc, p)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_chunk(1000)
        assert max(ref["counts"]) > 1000
        e.set_min_power(cut)
        e.set_budget(True)
        e.set_surface(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        first = None
        for rep in range(3):
            stats, _, _ = _engine_trace(e, sc, thr)
            what = f"all ledgers, trace {rep}"
            assert [int(st.n_in) for st in stats] == ref["counts"]
            s, (cc, cp) = e.surface(), e.culled()
            b = budget_dict(e.budget(), cc, cp)
            surface_ref.assert_surface(s, ref, what)
            budget_ref.assert_budget(b, ref["budget"], what)
            cutoff_ref.assert_ledger(cc, cp, ref["budget"]["culled"], what)
            assert [int(c) for c in b["n_culled"]] == [int(c) for c in cc]
            exact = (s["count"].tolist(), {k: np.asarray(b[k]).tolist() for k in budget_ref.COUNTS},
                     {k: np.asarray(b["mesh_count"][k]).tolist() for k in budget_ref.MESH_CATS}, cc.tolist())
            assert first is None or exact == first, what
            first = exact if first is None else first
    finally:
        e.close()


def test_device_source(oracle_mod, checker):
    """An on_device=True source (lpc_trace_set_rays_dev)."""
    from lightpycl_amd import light_source as lsrc
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc = case_scene("mixed")
    np.random.seed(1)
    src = lsrc.light_source(center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1), power=1000.,
                            ray_count=2000, on_device=True)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer([src], sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                            max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False, surface_map=True)
        assert "sources" not in tr.phase_s and src.__dict__.get("_dev") is not None
        s = tr.surface_power()
        o, d, p = src.__dict__["_dev"].fetch()
    finally:
        tr.engine.close()
    ref = surface_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env,
                            bounce_fn=checker[0])
    assert len(ref["iters"]) >= 2 and (ref["incident"] != ref["deposited"]).any()
    _assert_tracer_dict(s, sc, ref, "device source")


@pytest.mark.parametrize("keep", [False, True])
def test_with_cutoff(oracle_mod, checker, keep):
    """With the cutoff (eye at 1e-6): the record is taken before the cutoff's
    decision, so a culled child still counts as kept in `deposited`."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, cut, ref = _case(oracle_mod, checker, "eye", 1e-6)
    assert sum(len(c) for c in ref["budget"]["culled"]) > 0 and len(ref["iters"]) >= 3, "the case must cull"
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, min_ray_power=cut, surface_map=True))
        s = tr.surface_power()
        assert list(tr.iteration_counts) == ref["counts"]
    finally:
        tr.engine.close()
    surface_ref.assert_surface(s, ref, f"eye cut keep={keep}")


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", ["eye", "mixed", "cube_field"])
def test_map_and_budget_together(oracle_mod, checker, name, keep):
    """One record feeds both kernels: each ledger equals its helper's, and per mesh
    the deposited sums over its triangles are the budget's absorbed + terminated +
    measured: counts exactly, sums within twice the helper's bound of the mesh's
    terms (the triangles' bounds add up to at most one, the three categories' to
    at most another)."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, _, ref = _case(oracle_mod, checker, name)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, power_budget=True, surface_map=True))
        s, b = tr.surface_power(), tr.power_budget()
    finally:
        tr.engine.close()
    surface_ref.assert_surface(s, ref, f"{name} both")
    budget_ref.assert_budget(b, ref["budget"], f"{name} both")
    for m, sm in enumerate(s["meshes"]):
        cats = ("absorbed", "terminated", "measured")
        assert int(sm["count"].sum()) == sum(int(b["mesh_count"][c][m]) for c in cats), (name, m)
        got = math.fsum(float(v) for v in sm["deposited"])
        want = math.fsum(float(b["mesh"][c][m]) for c in cats)
        tol = 2 * surface_ref.sum_tol(surface_ref.mesh_deposited(ref, m))
        print(name, "mesh", m, "deposited", got, "budget", want, "tol", tol)
        assert abs(got - want) <= tol, (name, m, got, want, tol)


def test_map_alone_leaves_the_budget_as_it_is(oracle_mod, checker):
    """Map on, budget off: k_budget_sum does not run -- lpc_trace_budget reports no
    rows and zero tables, as on a handle without the map."""
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "mixed")
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        e.set_surface(True)
        _engine_trace(e, sc, _thr(sc, p))
        surface_ref.assert_surface(e.surface(), ref, "map alone")
        b = e.budget()
        assert len(b["n_in"]) == 0 and len(b["power_in"]) == 0
        assert not b["mesh_power"].any() and not b["mesh_count"].any()
        # the budget alone afterwards: its ledger, and a map of zeros
        e.set_surface(False)
        e.set_budget(True)
        _engine_trace(e, sc, _thr(sc, p))
        budget_ref.assert_budget(e.budget(), ref["budget"], "budget after the map")
        assert not e.surface()["count"].any()
    finally:
        e.close()


# -- 3. speculation and lifetime ------------------------------------------------------
@pytest.mark.parametrize("name", ["eye", "mixed"])
def test_switch_changes_on_one_handle(oracle_mod, checker, name):
    """off, on, on, off on one handle: both "on" traces equal the helper's, with
    equal counts (every ray once: a dropped or re-run speculative iteration never
    reaches the table); the last reads zeros; each trace is bit-equal, in stats and
    measured record, to a handle that never had the map on."""
    from parity_util import measured_rows
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, name)
    thr = _thr(sc, p)

    def one(e):
        stats, cnt, mp = _engine_trace(e, sc, thr)
        return (_stats_bits(stats), int(cnt), np.asarray(mp).tolist(), measured_rows(*e.fetch_measured()))

    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        never = one(e)
    finally:
        e.close()
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        maps = []
        for k, on in enumerate((False, True, True, False)):
            e.set_surface(on)
            got = one(e)
            assert got[:3] == never[:3], (k, on)
            np.testing.assert_array_equal(got[3], never[3], err_msg=f"trace {k}")
            s = e.surface()
            if on:
                surface_ref.assert_surface(s, ref, f"{name} trace {k}")
            else:
                assert not s["count"].any() and not s["incident"].any() and not s["deposited"].any()
            maps.append(s)
        assert np.array_equal(maps[1]["count"], maps[2]["count"])
    finally:
        e.close()


def test_smaller_scene_after_larger_and_live_bytes(oracle_mod, checker):
    """The tables are re-made for another triangle count, and freed with the handle."""
    from lightpycl_amd.engine import Engine
    big, (ob, db, pb), _, ref_big = _case(oracle_mod, checker, "cube_field")
    small, (os_, ds, ps), _, ref_small = _case(oracle_mod, checker, "cube")
    assert ref_small["M"] < ref_big["M"]
    before = _live_bytes()
    e = Engine(0)
    try:
        e.set_surface(True)
        for sc, (o, d, p), ref in ((big, (ob, db, pb), ref_big), (small, (os_, ds, ps), ref_small),
                                   (big, (ob, db, pb), ref_big)):
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            _engine_trace(e, sc, _thr(sc, p))
            surface_ref.assert_surface(e.surface(), ref, f"{sc.name} after another scene")
        assert _live_bytes()[0] > before[0]
    finally:
        e.close()
    assert _live_bytes() == before


# -- 4. argument checks ---------------------------------------------------------------
def test_argument_checks(oracle_mod, checker):
    from lightpycl_amd import _lib
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "mixed")
    M = ref["M"]
    e = Engine(0)
    try:
        L, m = e.L, ctypes.c_int64(-1)
        # without a scene: LPC_E_STATE through the scene gate, nothing written
        assert L.lpc_trace_surface(e.h, None, None, None, 0, ctypes.byref(m)) == -3 and m.value == -1
        assert b"scene" in L.lpc_last_error(e.h)
        assert L.lpc_trace_surface(e.h, None, None, None, 0, None) == -1
        e.upload_meshes(sc.meshes)
        e.set_surface(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _engine_trace(e, sc, _thr(sc, p))
        # NULL arrays: only the triangle count
        assert L.lpc_trace_surface(e.h, None, None, None, 0, ctypes.byref(m)) == 0 and m.value == M
        # tri_cap < M with an array given: LPC_E_ARG, no array written
        inc, dep = np.full(M, 7.5, np.float64), np.full(M, 7.5, np.float64)
        cnt = np.full(M, 7, np.int64)
        m2 = ctypes.c_int64(-1)
        rc = L.lpc_trace_surface(e.h, _lib.ptr(inc), _lib.ptr(dep), _lib.ptr(cnt), M - 1, ctypes.byref(m2))
        assert rc == -1 and b"triangle" in L.lpc_last_error(e.h) and m2.value == M
        assert (inc == 7.5).all() and (dep == 7.5).all() and (cnt == 7).all()
        # any one array alone
        assert L.lpc_trace_surface(e.h, None, None, _lib.ptr(cnt), M, ctypes.byref(m2)) == 0
        assert L.lpc_trace_surface(e.h, None, _lib.ptr(dep), None, M, ctypes.byref(m2)) == 0
        assert (inc == 7.5).all()
        surface_ref.assert_surface(dict(incident=e.surface()["incident"], deposited=dep, count=cnt), ref, "one array")
        # cleared with the measured record
        e.reset()
        assert not e.surface()["count"].any()
    finally:
        e.close()


# -- 5. TracePool and two ranks -------------------------------------------------------
def test_pool_submit_with_surface(oracle_mod, checker):
    from lightpycl_amd.pool import TracePool
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "eye")
    with TracePool(sc.meshes, engines=2) as pool:
        # with, without, without, with: every batch sets its own switch (omitted = off)
        futs = [pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, surface_map=True),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, surface_map=True)]
        got = [f.result(timeout=120) for f in futs]
    for g, on in zip(got, (True, False, False, True)):
        assert g["counts"] == ref["counts"]
        if on:
            surface_ref.assert_surface(g["surface"], ref, "pool")
        else:
            assert "surface" not in g


def _child(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lightpycl_amd.distributed as lpd
    from lightpycl_amd.engine import Engine
    from test_budget_host import mixed_scene
    lpd.SURFACE_PIECE = 1000                        # the tables go in several pieces
    sc = mixed_scene()
    o, d, p = rays_of(sc)
    lo, hi = lpd.shard_bounds(len(p), rank, world)
    eng = Engine(0)
    eng.upload_meshes(sc.meshes)
    eng.set_surface(True)
    eng.set_rays(o[lo:hi], d[lo:hi], p[lo:hi], sc.max_ray_len, sc.ior_env)
    comm = lpd.TorchComm(dist)
    iter_comm = lpd.ShmComm.from_dist(dist)
    tr = lpd.ShardedTrace(eng, comm, iter_comm=iter_comm)
    in_pow = float(np.sum(p[lo:hi], dtype=np.float64))
    runs = []
    for rep in range(2):                            # the second on the first's speculation history
        eng.reset()
        r = tr.run(sc.iterations, sc.tau, in_pow)
        s = r["surface"]
        assert "power_budget" not in r
        runs.append(dict(counts=r["global_counts"], surface={k: np.asarray(s[k]).tolist() for k in s}))
    if rank == 0:
        with open(out_path, "w") as fh:
            json.dump(runs, fh)
    tr.close()
    iter_comm.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_two_processes(oracle_mod, checker, tmp_path):
    """Two processes, each tracing its shard of `mixed` with the map on: the
    rank-summed counts are exactly the single device's, the sums within the bound
    of the helper's."""
    import torch.multiprocessing as mp
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "mixed")
    assert 3 * ref["M"] > 1000, "several pieces"
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_surface(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _engine_trace(e, sc, _thr(sc, p))
        single = e.surface()
    finally:
        e.close()
    surface_ref.assert_surface(single, ref, "single device")
    out = str(tmp_path / "r.json")
    mp.spawn(_child, args=(2, _free_port(), out), nprocs=2, join=True)
    runs = json.load(open(out))
    assert len(runs) == 2
    for r in runs:
        assert r["counts"] == ref["counts"]
        s = dict(incident=np.asarray(r["surface"]["incident"], np.float64),
                 deposited=np.asarray(r["surface"]["deposited"], np.float64),
                 count=np.asarray(r["surface"]["count"], np.int64))
        assert np.array_equal(s["count"], single["count"])
        surface_ref.assert_surface(s, ref, "two ranks")
