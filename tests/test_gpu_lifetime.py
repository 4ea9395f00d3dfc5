"""Nothing is left behind (lpc_debug_live_bytes): the library counts the device
and pinned bytes its owners hold, and after an engine, a staged batch that never
ran or a TracePool is closed both counters stand exactly where they stood before
it was opened -- whichever allocating paths the engine went through.

The counters are process-wide and the session's `engine` fixture stays open, so
every case reads them as a difference around engines of its own."""
import ctypes
import gc

import numpy as np
import pytest

from lightpycl_amd import _lib, scenes

pytestmark = pytest.mark.gpu


def _live():
    """(device bytes, pinned bytes) the library holds now."""
    d, p = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.load().lpc_debug_live_bytes(ctypes.byref(d), ctypes.byref(p)))
    return d.value, p.value


def _baseline():
    gc.collect()        # engines and device sources earlier tests dropped unclosed go now, not inside the case
    return _live()


def _rays(sc):
    ls = sc.sources[0]
    p = np.asarray(ls.rays_power, np.float32).reshape(-1)
    thr = (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))
    return np.asarray(ls.rays_origin, np.float32), np.asarray(ls.rays_dir, np.float32), p, thr


def test_counters_follow_an_allocation():
    from lightpycl_amd.engine import Engine
    base = _baseline()
    e = Engine(0)
    try:
        opened = _live()
        assert opened[0] > base[0] and opened[1] > base[1], (base, opened)   # the counters, the pinned copies
        sc = scenes.lens(n=1000, seed=1)
        e.upload_meshes(sc.meshes)
        assert _live()[0] > opened[0]
    finally:
        e.close()
    assert _live() == base


def test_engine_through_every_allocating_path_closes_clean():
    from lightpycl_amd.engine import Engine
    sc = scenes.eye(n=3000, seed=2)
    o, d, p, thr = _rays(sc)
    other = scenes.parabolic(n=1000)
    base = _baseline()
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        assert e.mesh_count == 5                            # the per-ray slot masks of the traced path are in use
        e.prof_enable(counters=True)                        # walk counters, fan-triangle flags
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        st, _ = e.run_local(sc.iterations, thr)             # traced path
        assert len(st) > 1
        e.set_chunk(1000)
        e.reset()
        e.run_local(sc.iterations, thr)                     # chunked traced: running row bases
        e.set_chunk(0)
        e.set_min_power(1e-9)
        e.reset()
        e.run_local(sc.iterations, thr)                     # the culled-power ledger
        e.reset()
        e.iterate(export=True)
        e.reset()
        e.iterate_export()                                  # export stream, its events and staging
        e.sync()
        e.stage_rays(o, d, p, sc.max_ray_len, sc.ior_env)   # copy stream, a slot's buffers, its helper
        e.run_staged(sc.iterations, thr)
        key, pos = np.random.RandomState(5).get_state()[1:3]
        src, _, _ = e.emit_hemisphere(key, pos, 2000, np.zeros(4, np.float32), np.eye(3), np.eye(3))
        assert src.n == 2000
        e.set_rays_dev([src], sc.max_ray_len, sc.ior_env)
        src.free()
        e.run_local(sc.iterations, 0.0)
        e.elev_scan([0.0, 0.0, 1.0, 0.0])                   # the resident measured record
        e.upload_meshes(other.meshes)                       # a second scene over the first
        assert _live()[0] > base[0]
    finally:
        e.close()
    assert _live() == base


def test_batch_staged_and_never_run_closes_clean():
    from lightpycl_amd.engine import Engine
    sc = scenes.lens(n=3000, seed=3)
    o, d, p, _ = _rays(sc)
    base = _baseline()
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.stage_rays(o, d, p, sc.max_ray_len, sc.ior_env)
    finally:
        e.close()                                           # joins the helper
    assert _live() == base


def test_trace_pool_rounds_close_clean():
    from lightpycl_amd.pool import TracePool
    sc = scenes.lens(n=3000, seed=4)
    o, d, p, _ = _rays(sc)
    base = _baseline()
    counts = []
    for _ in range(3):
        with TracePool(sc.meshes, engines=2) as pool:
            futs = [pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau) for _ in range(2)]
            counts.append([f.result(timeout=60)["counts"] for f in futs])
        assert _live() == base
    assert counts[1] == counts[0] and counts[2] == counts[0]
