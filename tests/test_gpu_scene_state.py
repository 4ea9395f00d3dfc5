"""The scene and the emitted rays are whole values of the handle (DESIGN.md
section 1): lpc_scene_upload validates its arguments before it touches the
handle, so a refused upload changes nothing; every compute entry point goes
through one gate and returns LPC_E_STATE without a scene; a smaller scene after
a larger one reuses the grow-only buffers.

Every case runs on an Engine of its own.  The refused uploads pass the rows and
counts of the scene in place, so no runtime, correct or not, is led past a
buffer by them."""
import ctypes

import numpy as np
import pytest

from lightpycl_amd import _lib, scenes
from lightpycl_amd._lib import ptr
from lightpycl_amd.engine import Engine, flatten_meshes

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3
N = 500
STAT_FIELDS = [f for f, _ in _lib.IterStats._fields_]


def _rays(sc):
    ls = sc.sources[0]
    p = np.asarray(ls.rays_power, np.float32).reshape(-1)
    thr = (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))
    return np.asarray(ls.rays_origin, np.float32), np.asarray(ls.rays_dir, np.float32), p, thr


def _trace(e, sc, thr):
    """One trace from the emitted rays: (stats rows, measured count, per-mesh power bytes, measured record bytes)."""
    st, (cnt, mp) = e.run_local(sc.iterations, thr, reset=True)
    rows = [tuple(getattr(s, f) for f in STAT_FIELDS) for s in st]
    return rows, cnt, mp.tobytes(), tuple(a.tobytes() for a in e.fetch_measured())


def _err(e):
    return (e.L.lpc_last_error(e.h) or b"").decode()


def _live_device_bytes():
    d, p = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.load().lpc_debug_live_bytes(ctypes.byref(d), ctypes.byref(p)))
    return d.value


def test_refused_upload_changes_nothing():
    sc = scenes.BUILDERS["nested_cubes"](n=N)
    v0, v1, v2, mesh_id, mat_type, ior, refl, diss = flatten_meshes(sc.meshes)
    M, K = len(mesh_id), len(mat_type)
    assert K >= 2 and np.all(np.diff(mesh_id) >= 0) and mesh_id[0] == 0
    o, d, p, thr = _rays(sc)
    e = Engine(0)
    try:
        e.upload_arrays(v0, v1, v2, mesh_id, mat_type, ior, refl, diss)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        first = _trace(e, sc, thr)
        assert len(first[0]) >= 2 and first[0][0][0] == N

        # the first two runs' mesh ids exchanged: run 0 would flush below slot 0
        swapped = mesh_id.copy()
        swapped[mesh_id == 0], swapped[mesh_id == 1] = 1, 0
        past = mesh_id.copy()
        past[M // 2] = K
        refusals = [
            ((M, swapped, K, ior), "writes below slot 0"),
            ((M, past, K, ior), f"mesh_id[{M // 2}] out of range"),
            ((0, mesh_id, K, ior), "scene needs >= 1 triangle"),
            ((M, mesh_id, K, None), "scene needs >= 1 triangle"),
        ]
        for (m, ids, k, ior_arg), text in refusals:
            rc = e.L.lpc_scene_upload(e.h, m, ptr(v0), ptr(v1), ptr(v2), ptr(ids), k, ptr(mat_type), ptr(ior_arg),
                                      ptr(refl), ptr(diss))
            assert rc == E_ARG, (text, rc)
            assert text in _err(e), (text, _err(e))
            # the old scene, its emitted rays and the trace state are as they were
            again = _trace(e, sc, thr)
            assert again[0] == first[0], text
            assert again[1:] == first[1:], text
    finally:
        e.close()


def test_every_compute_entry_point_needs_a_scene():
    sc = scenes.BUILDERS["nested_cubes"](n=N)
    o, d, p, thr = _rays(sc)
    e = Engine(0)
    try:
        L, h = e.L, e.h
        st = (_lib.IterStats * 4)()
        one = _lib.IterStats()
        k, c = ctypes.c_int32(0), ctypes.c_int64(0)
        mp = np.zeros(8, np.float64)
        trace_calls = {
            "lpc_trace_run": lambda: L.lpc_trace_run(h, 4, thr, st, ctypes.byref(k), ctypes.byref(c), ptr(mp), mp.size),
            "lpc_trace_reset": lambda: L.lpc_trace_reset(h),
            "lpc_trace_iterate": lambda: L.lpc_trace_iterate(h, None, None, None, None, None, ctypes.byref(one)),
        }
        calls = dict(trace_calls)
        calls.update({
            "lpc_trace_set_rays": lambda: L.lpc_trace_set_rays(h, N, ptr(o), ptr(d), ptr(p), np.float32(sc.max_ray_len),
                                                               np.float32(sc.ior_env)),
            # the gate comes before the buffers are looked at: none are passed
            "lpc_intersect": lambda: L.lpc_intersect(h, N, None, None, np.float32(sc.max_ray_len), None, None, None),
            "lpc_bounce_host": lambda: L.lpc_bounce_host(h, N, *([None] * 5), np.float32(sc.max_ray_len),
                                                         np.float32(sc.ior_env), *([None] * 12)),
            "lpc_trace_set_rays_dev": lambda: L.lpc_trace_set_rays_dev(h, None, 0, np.float32(sc.max_ray_len),
                                                                       np.float32(sc.ior_env)),
        })
        for name, call in calls.items():
            assert call() == E_STATE, name
            assert "no scene uploaded" in _err(e), (name, _err(e))
        # a scene, no emitted rays yet: the trace calls still refuse
        e.upload_meshes(sc.meshes)
        for name, call in trace_calls.items():
            assert call() == E_STATE, name
            assert "before trace_set_rays" in _err(e), (name, _err(e))
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        assert trace_calls["lpc_trace_reset"]() == 0
    finally:
        e.close()


def test_smaller_scene_after_a_larger_one_keeps_working():
    eye, cubes = scenes.BUILDERS["eye"](n=N), scenes.BUILDERS["nested_cubes"](n=N)
    assert len(eye.meshes) == 5 and len(eye.meshes) > len(cubes.meshes)
    e = Engine(0)
    try:
        first, grew = {}, []
        for sc in (eye, cubes, eye):
            o, d, p, thr = _rays(sc)
            before = _live_device_bytes()
            e.upload_meshes(sc.meshes)
            grew.append(_live_device_bytes() - before)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            got = _trace(e, sc, thr)
            assert got[0] and got[0][0][0] == N
            assert got == first.setdefault(sc.name, got), sc.name
            assert got == _trace(e, sc, thr), sc.name      # and again on the scene in place
        # the first eye upload allocated; its grow-only buffers serve the smaller
        # scene and the second eye upload (the piece tables of the scene before go)
        assert grew[0] > 0 and grew[1] <= 0 and grew[2] <= 0, grew
    finally:
        e.close()
