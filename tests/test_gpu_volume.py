"""GPU tests of the volume map (lpc_trace_set_volume / lpc_trace_volume).

1. A constructed slab (tests/volume_ref.py): one dissipative cube whose IOR is
   the environment's, collimated +z rays through voxel centres, so every ray
   of the second iteration dissipates along its own column: every voxel against
   the helper within tol_v, and against the closed form D (W((k+1)/nz) - W(k/nz)).
2. The cases that dissipate, on every trace path, against the host helper over
   the reference's OWN kernels when they are built, else over the CPU oracle:
   segments exactly, every voxel within tol_v (derived in volume_ref), the
   identity against the power budget.
3. Switching and lifetime, 4. argument checks, 5. pool and two processes.

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
import volume_ref
from test_budget_host import case_scene, rays_of
from test_gpu_budget import _engine_trace, _free_port, _live_bytes, _stats_bits, _thr, _trace_kw
from test_volume_host import CASES, case_grids

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MRL, IOR = np.float32(1e3), np.float32(1.0)
SLAB_SIZES = [255, 256, 257, 4160]          # below, at and above one tile of the shading; many blocks


def _table():
    from lightpycl_amd import _lib
    return _lib.VOLUME_LDS_ENTRIES


def _kw(grid):
    return dict(lo=grid["lo"], hi=grid["hi"], shape=grid["shape"])


def _set(e, grid):
    e.set_volume(grid["lo"], grid["hi"], grid["shape"])


# -- 1. the constructed slab ----------------------------------------------------------
_SLABS = {}


@pytest.fixture(scope="module")
def slabs():
    """Engines on the slab, one per dissipation, opened on first use."""
    from lightpycl_amd.engine import Engine

    def get(diss):
        if diss not in _SLABS:
            e = Engine(0)
            e.upload_meshes(volume_ref.slab_scene(diss))
            _SLABS[diss] = e
        return _SLABS[diss]

    yield get
    for e in _SLABS.values():
        e.close()
    _SLABS.clear()


def _slab(slabs, oracle_mod, checker, n, shape, pname, diss=0.3, lo=volume_ref.SLAB_LO, hi=volume_ref.SLAB_HI):
    """One slab trace on the device and under the reference -> (map, Ref, columns)."""
    grid = volume_ref.grid_of(lo, hi, shape)
    # (the columns are those of the grid over the cube's own x, y: voxel centres of both)
    cols = volume_ref.slab_patterns(n, shape, _table())[pname]
    o, d, p = volume_ref.slab_rays(cols, shape)
    ref = volume_ref.trace(oracle_mod, volume_ref.slab_scene(diss), o, d, p, 2, 1.0, MRL, IOR, [grid],
                           bounce_fn=checker[0])["refs"][0]
    assert ref.per_iter == [0, n], (ref.per_iter, n)            # the premise: every ray, second iteration
    e = slabs(diss)
    _set(e, grid)
    e.set_rays(o, d, p, MRL, IOR)
    stats, _ = e.run_local(2, 0.0)
    assert int(stats[0].n_in) == n
    return e.volume(), ref, cols


def _assert_closed_form(v, ref, cols, what, zlo=volume_ref.SLAB_LO[2], zhi=volume_ref.SLAB_HI[2]):
    """Every column against D (W((k+1)/nz) - W(k/nz)) of its rays, within tol_v;
    what lies outside the z range against `outside`."""
    shape = ref.grid["shape"]
    terms, out_terms = {}, []
    for j, (O, E, a, D) in enumerate(ref.rays):
        sh, outside = volume_ref.slab_closed_form(D, a, shape[2], lo=zlo, hi=zhi)
        out_terms.append(float(outside))
        for k in range(shape[2]):
            terms.setdefault((int(cols[j][0]), int(cols[j][1]), k), []).append(float(sh[k]))
    want = np.zeros(shape, np.float64)
    for key, t in terms.items():
        want[key] = math.fsum(t)
    err = np.abs(np.asarray(v["deposited"]) - want)
    tol = ref.tol.reshape(shape)
    print(what, "closed form: max |err|", float(err.max()), "max tol", float(tol.max()))
    bad = np.argwhere(~(err <= tol))
    assert len(bad) == 0, (what, bad[:6], [(v["deposited"][tuple(b)], want[tuple(b)]) for b in bad[:6]])
    assert abs(v["outside"] - math.fsum(out_terms)) <= ref.tol_all(), (what, v["outside"], math.fsum(out_terms))


@pytest.mark.parametrize("pname", ["one", "each", "collide"])
@pytest.mark.parametrize("n", SLAB_SIZES)
def test_slab(slabs, oracle_mod, checker, n, pname):
    """16 x 16 x 8 = 2 048 voxels: twice the block table, so `collide` puts voxels
    of equal low bits into one block."""
    shape = (16, 16, 8)
    v, ref, cols = _slab(slabs, oracle_mod, checker, n, shape, pname)
    if pname == "collide":
        first = (cols[:, 0] * shape[1] + cols[:, 1]) * shape[2]
        assert len(np.unique(first)) > 1 and len(np.unique(first % _table())) == 1
    what = f"slab {pname} n={n}"
    volume_ref.assert_volume(v, ref, what)
    _assert_closed_form(v, ref, cols, what)
    assert v["outside"] == 0.0 and v["segments"] == n
    assert np.count_nonzero(v["deposited"]) == len(np.unique(cols, axis=0)) * shape[2]


@pytest.mark.parametrize("shape,n,pname", [((1, 1, 1), 257, "one"), ((33, 17, 5), 4160, "each"),
                                           ((33, 17, 5), 257, "one")])
def test_slab_grids(slabs, oracle_mod, checker, shape, n, pname):
    """A single voxel; an odd grid."""
    v, ref, cols = _slab(slabs, oracle_mod, checker, n, shape, pname)
    what = f"slab {shape} {pname} n={n}"
    volume_ref.assert_volume(v, ref, what)
    _assert_closed_form(v, ref, cols, what)
    assert v["outside"] == 0.0


def test_slab_half_box(slabs, oracle_mod, checker):
    """A box whose z range starts in the middle of the cube: the first half of
    every segment is `outside`."""
    lo, hi = (-5.0, -5.0, 20.0), (5.0, 5.0, 30.0)
    v, ref, cols = _slab(slabs, oracle_mod, checker, 4160, (16, 16, 8), "each", lo=lo, hi=hi)
    volume_ref.assert_volume(v, ref, "half box")
    _assert_closed_form(v, ref, cols, "half box", zlo=20.0, zhi=30.0)
    assert v["outside"] > 0.5 * math.fsum(ref.D) and not v["deposited"][:, :, 4:].any()


@pytest.mark.parametrize("n,pname", [(257, "each"), (4160, "one")])
def test_slab_small_a(slabs, oracle_mod, checker, n, pname):
    """A dissipation of 2e-6 (a = 2e-5): the expm1 branch near zero."""
    v, ref, cols = _slab(slabs, oracle_mod, checker, n, (16, 16, 8), pname, diss=2e-6)
    assert all(0.0 < a < 1e-4 for _, _, a, _ in ref.rays)
    what = f"small a {pname} n={n}"
    volume_ref.assert_volume(v, ref, what)
    _assert_closed_form(v, ref, cols, what)
    # an even spread: W(s) = s to 1e-5
    col = v["deposited"][tuple(cols[0])]
    assert np.all(np.abs(col / col.sum() - 1.0 / 8) < 1e-5)


# -- 2. against the reference ---------------------------------------------------------
_REFS = {}


def _case(oracle_mod, checker, name, f=0.0):
    """(scene, rays, cut, grids, the helper's reference per grid with the budget's)."""
    sc = case_scene(name)
    o, d, p = rays_of(sc)
    cut = cutoff_ref.cut_of(p, f) if f else np.float32(0.0)
    key = (name, f)
    if key not in _REFS:
        _REFS[key] = volume_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                      sc.ior_env, case_grids(name), cut=cut, bounce_fn=checker[0])
    ref = _REFS[key]
    assert all(r.segments > 0 for r in ref["refs"])
    return sc, (o, d, p), cut, case_grids(name), ref


def _assert_identity(v, b, ref, what):
    """sum(deposited) + outside against the library's own budget of the same
    trace: both lie within their bounds of the same exact sum."""
    dis = [float(t) for it in ref["budget"]["iters"] for t in it["dissipated"][0]]
    n_it = len(ref["budget"]["iters"])
    r = [x for x in ref["refs"] if tuple(x.grid["shape"]) == np.asarray(v["deposited"]).shape][0]
    # (the map within tol_all of the helper's total, that within tol_all of the exact sum of D)
    tol = 2 * r.tol_all() + sum(budget_ref.sum_tol(it["dissipated"][0]) for it in ref["budget"]["iters"]) + \
        n_it * 2.0 ** -53 * math.fsum(abs(t) for t in dis)
    total = math.fsum(np.asarray(v["deposited"]).ravel().tolist() + [float(v["outside"])])
    want = math.fsum(float(x) for x in b["dissipated"])
    print(what, "volume total", total, "budget dissipated", want, "tol", tol)
    assert abs(total - want) <= tol, (what, total, want, tol)
    assert int(v["segments"]) == int(np.sum(b["n_dissipated"])) == len(dis), what


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_modes(oracle_mod, checker, name, keep):
    """Aggregate mode (k_shade_stage's record) and results mode (k_shade_bud's),
    each grid of the case, the map with the budget on."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, _, grids, ref = _case(oracle_mod, checker, name)
    tr = CL_Tracer(device=0)
    try:
        for g, r in zip(grids, ref["refs"]):
            what = f"{name} keep={keep} grid {g['shape']}"
            tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, volume_map=_kw(g), power_budget=True))
            v, b = tr.volume_power(), tr.power_budget()
            assert v is not None and tr.surface_power() is None
            assert list(tr.iteration_counts) == ref["counts"]
            volume_ref.assert_volume(v, r, what)
            budget_ref.assert_budget(b, ref["budget"], what)
            _assert_identity(v, b, ref, what)
            assert v["total"] == math.fsum(v["deposited"].ravel().tolist() + [v["outside"]])
            assert [len(x) for x in v["edges"]] == [n + 1 for n in g["shape"]]
            assert all(np.array_equal(x, y) for x, y in zip(v["edges"], g["edges"]))
            cell = np.prod((g["hi"] - g["lo"]) / np.asarray(g["shape"], np.float64))
            assert np.array_equal(v["density"], v["deposited"] / cell)
        # a second trace on the last grid: the map was cleared, not accumulated
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, volume_map=_kw(grids[-1])))
        v2 = tr.volume_power()
        volume_ref.assert_volume(v2, ref["refs"][-1], f"{name} keep={keep}, second trace")
        assert tr.power_budget() is None
        # and a trace without it reads None, the engine zeros on the grid last set
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep))
        assert tr.volume_power() is None
        z = tr.engine.volume()
        assert z["deposited"].shape == grids[-1]["shape"] and not z["deposited"].any()
        assert z["outside"] == 0.0 and z["segments"] == 0
    finally:
        tr.engine.close()


@pytest.mark.parametrize("path", ["chunk256", "chunk257", "chunk1000", "resort", "traced0", "staged", "rerun"])
@pytest.mark.parametrize("name", ["mixed", "cube_field"])
def test_paths(oracle_mod, checker, monkeypatch, name, path):
    """The trace paths of test_gpu_surface.py::test_paths, three traces each (the
    later ones on the first's speculation history): the origins k_volume_sum
    reads from the chunk's rays are the ones the shading read on every path."""
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, name)
    if path == "resort":
        monkeypatch.setenv("LPC_RESORT_MIN", "1000")
    if path == "traced0":
        monkeypatch.setenv("LPC_TRACED", "0")
    thr = _thr(sc, p)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        if path.startswith("chunk"):
            e.set_chunk(int(path[5:]))
            assert max(ref["counts"]) > int(path[5:])
        g, r = grids[1], ref["refs"][1]
        _set(e, g)
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
            assert [int(st.n_in) for st in stats] == ref["counts"]
            volume_ref.assert_volume(e.volume(), r, f"{name} {path} trace {rep}")
    finally:
        e.close()


def test_all_four_ledgers_chunked(oracle_mod, checker):
    """The cutoff, the budget, the surface map and the volume map on one handle,
    several chunks per iteration, three traces: each ledger equals its helper's."""
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import budget_dict
    sc, (o, d, p), cut, grids, ref = _case(oracle_mod, checker, "mixed", 1e-3)
    assert sum(len(c) for c in ref["budget"]["culled"]) > 0, "the case must cull"
    sref = surface_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env,
                             cut=cut, bounce_fn=checker[0])
    thr = _thr(sc, p)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_chunk(1000)
        assert max(ref["counts"]) > 1000
        e.set_min_power(cut)
        e.set_budget(True)
        e.set_surface(True)
        _set(e, grids[0])
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        for rep in range(3):
            stats, _, _ = _engine_trace(e, sc, thr)
            what = f"all four ledgers, trace {rep}"
            assert [int(st.n_in) for st in stats] == ref["counts"]
            v, s, (cc, cp) = e.volume(), e.surface(), e.culled()
            b = budget_dict(e.budget(), cc, cp)
            volume_ref.assert_volume(v, ref["refs"][0], what)
            surface_ref.assert_surface(s, sref, what)
            budget_ref.assert_budget(b, ref["budget"], what)
            cutoff_ref.assert_ledger(cc, cp, ref["budget"]["culled"], what)
            _assert_identity(v, b, ref, what)
    finally:
        e.close()


def test_device_source(oracle_mod, checker):
    """An on_device=True source (lpc_trace_set_rays_dev)."""
    from lightpycl_amd import light_source as lsrc
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc = case_scene("mixed")
    g = case_grids("mixed")[1]
    np.random.seed(1)
    src = lsrc.light_source(center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1), power=1000.,
                            ray_count=2000, on_device=True)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer([src], sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                            max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False, volume_map=_kw(g))
        assert src.__dict__.get("_dev") is not None
        v = tr.volume_power()
        o, d, p = src.__dict__["_dev"].fetch()
    finally:
        tr.engine.close()
    ref = volume_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env, [g],
                           bounce_fn=checker[0])["refs"][0]
    assert ref.segments > 0 and ref.outside() > 0
    volume_ref.assert_volume(v, ref, "device source")


@pytest.mark.parametrize("keep", [False, True])
def test_with_cutoff(oracle_mod, checker, keep):
    """With the cutoff: the record is taken before the cutoff's decision, and the
    culled children are never traced, so never booked."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, cut, grids, ref = _case(oracle_mod, checker, "mixed", 1e-3)
    assert sum(len(c) for c in ref["budget"]["culled"]) > 0, "the case must cull"
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, min_ray_power=cut, volume_map=_kw(grids[0])))
        v = tr.volume_power()
        assert list(tr.iteration_counts) == ref["counts"]
    finally:
        tr.engine.close()
    volume_ref.assert_volume(v, ref["refs"][0], f"mixed cut keep={keep}")


# -- 3. switching and lifetime --------------------------------------------------------
def test_switching_on_one_handle(oracle_mod, checker):
    """On, off, another grid, the first again on one handle: every "on" trace equals
    the helper's on its grid, "off" reads zeros, and each trace is bit-equal, in
    stats and measured record, to a handle that never had the map on.  The map
    alone leaves the budget and the surface map as they are."""
    from parity_util import measured_rows
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, "mixed")
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
        z = e.volume()                                  # never set: an empty map
        assert z["shape"] == (0, 0, 0) and z["deposited"].size == 0 and z["segments"] == 0
        for k, gi in enumerate((None, 0, None, 1, 0)):
            if gi is None:
                e.set_volume(None)
            else:
                _set(e, grids[gi])
            got = one(e)
            assert got[:3] == never[:3], (k, gi)
            np.testing.assert_array_equal(got[3], never[3], err_msg=f"trace {k}")
            v = e.volume()
            if gi is None:
                assert not v["deposited"].any() and v["outside"] == 0.0 and v["segments"] == 0
            else:
                volume_ref.assert_volume(v, ref["refs"][gi], f"switching, trace {k}")
                b = e.budget()
                assert len(b["n_in"]) == 0 and not b["mesh_power"].any() and not b["mesh_count"].any()
                assert not e.surface()["count"].any()
        # another grid after a trace discards what was booked; the same grid keeps it
        _set(e, grids[0])
        assert e.volume()["segments"] == ref["refs"][0].segments
        _set(e, grids[1])
        v = e.volume()
        assert v["deposited"].shape == grids[1]["shape"] and not v["deposited"].any() and v["segments"] == 0
    finally:
        e.close()


def test_smaller_grid_after_larger_and_live_bytes(oracle_mod, checker):
    """The tables are re-made for another voxel count, and freed with the handle."""
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, "mixed")
    big = volume_ref.grid_of((-5.0, -5.0, 15.0), (5.0, 5.0, 25.0), (64, 64, 32))
    assert big["V"] > grids[0]["V"] > grids[1]["V"]
    before = _live_bytes()
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _set(e, big)
        _engine_trace(e, sc, _thr(sc, p))
        vb = e.volume()
        assert vb["segments"] == ref["refs"][0].segments
        # the large grid refines the case's first: its 8 x 8 x 4 blocks sum to it
        coarse = vb["deposited"].reshape(8, 8, 8, 8, 8, 4).sum(axis=(1, 3, 5))
        r0 = ref["refs"][0]
        assert np.all(np.abs(coarse - r0.deposited()) <= r0.tol.reshape(8, 8, 8) + 256 * 2.0 ** -53 * np.abs(coarse))
        for gi in (1, 0, 1):
            _set(e, grids[gi])
            _engine_trace(e, sc, _thr(sc, p))
            volume_ref.assert_volume(e.volume(), ref["refs"][gi], f"grid {gi} after a larger one")
        assert _live_bytes()[0] > before[0]
    finally:
        e.close()
    assert _live_bytes() == before


# -- 4. argument checks ---------------------------------------------------------------
def test_argument_checks(oracle_mod, checker):
    from lightpycl_amd import _lib
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, "mixed")
    g, r = grids[1], ref["refs"][1]
    V = g["V"]
    e = Engine(0)
    try:
        L = e.L
        dims = np.full(3, -1, np.int32)
        assert L.lpc_trace_volume(e.h, None, 0, _lib.ptr(dims), None, None) == 0 and dims.tolist() == [0, 0, 0]
        assert L.lpc_trace_volume(e.h, None, 0, None, None, None) == -1
        e.upload_meshes(sc.meshes)
        _set(e, g)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _engine_trace(e, sc, _thr(sc, p))

        def bad(lo, hi, shape):
            lo3, hi3 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            d3 = np.asarray(shape, np.int32)
            rc = L.lpc_trace_set_volume(e.h, _lib.ptr(lo3), _lib.ptr(hi3), _lib.ptr(d3))
            assert rc == -1 and b"grid" in L.lpc_last_error(e.h), (lo, hi, shape, rc)

        bad((0, 0, np.nan), (1, 1, 1), (2, 2, 2))
        bad((0, 0, 0), (1, np.inf, 1), (2, 2, 2))
        bad((0, 0, 0), (1, 0, 1), (2, 2, 2))
        bad((0, 2, 0), (1, 1, 1), (2, 2, 2))
        bad((0, 0, 0), (1, 1, 1), (0, 2, 2))
        bad((0, 0, 0), (1, 1, 1), (2, 1025, 2))
        bad((0, 0, 0), (1, 1, 1), (1024, 1024, 256))
        lo3 = np.zeros(3)
        assert L.lpc_trace_set_volume(e.h, _lib.ptr(lo3), None, None) == -1
        with pytest.raises(_lib.LpcError):
            e.set_volume((0, 0, 0), (1, 1, 1), (2, 2, 0))
        # a refused grid changes nothing: the map of the trace is still there
        volume_ref.assert_volume(e.volume(), r, "after refused grids")
        # cap < V with the array given: LPC_E_ARG, nothing written
        dep = np.full(V, 7.5, np.float64)
        out, seg = ctypes.c_double(-1.0), ctypes.c_int64(-1)
        rc = L.lpc_trace_volume(e.h, _lib.ptr(dep), V - 1, _lib.ptr(dims), ctypes.byref(out), ctypes.byref(seg))
        assert rc == -1 and (dep == 7.5).all() and out.value == -1.0 and seg.value == -1
        assert dims.tolist() == list(g["shape"])
        # the scalars alone
        assert L.lpc_trace_volume(e.h, None, 0, _lib.ptr(dims), ctypes.byref(out), ctypes.byref(seg)) == 0
        assert seg.value == r.segments and abs(out.value - r.outside()) <= r.tol_all()
        # cleared with the measured record
        e.reset()
        v = e.volume()
        assert not v["deposited"].any() and v["segments"] == 0 and v["outside"] == 0.0
    finally:
        e.close()


# -- 5. TracePool and two ranks -------------------------------------------------------
def test_pool_submit_with_volume(oracle_mod, checker):
    from lightpycl_amd.pool import TracePool
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, "mixed")
    args = (o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau)
    with TracePool(sc.meshes, engines=2) as pool:
        # with, without, without, with another grid: every batch sets its own switch (omitted = off)
        futs = [pool.submit(*args, volume_map=_kw(grids[0])), pool.submit(*args), pool.submit(*args),
                pool.submit(*args, volume_map=_kw(grids[1]))]
        got = [f.result(timeout=120) for f in futs]
    for g, gi in zip(got, (0, None, None, 1)):
        assert g["counts"] == ref["counts"]
        if gi is None:
            assert "volume" not in g
        else:
            volume_ref.assert_volume(g["volume"], ref["refs"][gi], "pool")


def _child(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lightpycl_amd.distributed as lpd
    from lightpycl_amd.engine import Engine
    from test_budget_host import mixed_scene
    lpd.SURFACE_PIECE = 100                         # the table goes in several pieces
    sc = mixed_scene()
    g = case_grids("mixed")[0]
    o, d, p = rays_of(sc)
    lo, hi = lpd.shard_bounds(len(p), rank, world)
    eng = Engine(0)
    eng.upload_meshes(sc.meshes)
    eng.set_volume(g["lo"], g["hi"], g["shape"])
    eng.set_rays(o[lo:hi], d[lo:hi], p[lo:hi], sc.max_ray_len, sc.ior_env)
    comm = lpd.TorchComm(dist)
    iter_comm = lpd.ShmComm.from_dist(dist)
    tr = lpd.ShardedTrace(eng, comm, iter_comm=iter_comm)
    in_pow = float(np.sum(p[lo:hi], dtype=np.float64))
    runs = []
    for rep in range(2):                            # the second on the first's speculation history
        eng.reset()
        r = tr.run(sc.iterations, sc.tau, in_pow)
        v = r["volume"]
        assert "power_budget" not in r and "surface" not in r and isinstance(v["segments"], int)
        runs.append(dict(counts=r["global_counts"], deposited=np.asarray(v["deposited"]).tolist(),
                         outside=v["outside"], segments=v["segments"]))
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
    rank-summed segments are exactly the single trace's, the voxels within the
    bound of the helper's."""
    import torch.multiprocessing as mp
    sc, (o, d, p), _, grids, ref = _case(oracle_mod, checker, "mixed")
    assert grids[0]["V"] + 2 > 100, "several pieces"
    out = str(tmp_path / "r.json")
    mp.spawn(_child, args=(2, _free_port(), out), nprocs=2, join=True)
    runs = json.load(open(out))
    assert len(runs) == 2
    for r in runs:
        assert r["counts"] == ref["counts"]
        v = dict(deposited=np.asarray(r["deposited"], np.float64), outside=r["outside"], segments=r["segments"])
        volume_ref.assert_volume(v, ref["refs"][0], "two ranks")
