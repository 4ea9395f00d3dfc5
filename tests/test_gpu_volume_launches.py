"""The kernels a trace launches with the volume map off, on, and off again,
listed by the HIP kernel records of torch.profiler (liblpc shares torch's HIP
runtime, lightpycl_amd/_lib.py): with the map off -- on a handle that had it on
before as well -- the kernel names are those of a handle that never had it;
with the map on and the other ledgers off, the fate-record instantiations and
k_volume_sum / k_volume_commit run and k_budget_sum and k_surface_sum do not."""
import collections

import numpy as np
import pytest

from test_budget_host import case_scene, rays_of

pytestmark = pytest.mark.gpu


def _kernels(fn):
    """Counter of the names of the lpck kernels launched by fn()."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = collections.Counter()
    for ev in prof.events():
        if "lpck::" in ev.name or ev.name.startswith("k_"):
            names[ev.name] += 1
    return names


def test_kernel_names_with_the_map_off_and_on():
    from lightpycl_amd.engine import Engine
    sc = case_scene("mixed")
    o, d, p = rays_of(sc)
    thr = (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))

    def trace(e):
        def run():
            e.reset()
            e.run_local(sc.iterations, thr)
            e.sync()
        return run

    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        # (the same history as the handle below: what a trace launches to restore
        # its buffers' clean state depends on the traces before it)
        trace(e)()
        never2 = _kernels(trace(e))
        trace(e)()
        never = _kernels(trace(e))
    finally:
        e.close()
    assert sum(never.values()) > 0, "the profiler lists no kernel of the library"
    assert any("k_shade_stage" in k for k in never) and any("k_stage_move" in k for k in never), sorted(never)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        e.set_volume((-5.0, -5.0, 15.0), (5.0, 5.0, 25.0), (8, 8, 8))
        trace(e)()
        on = _kernels(trace(e))
        e.set_volume(None)
        trace(e)()
        off = _kernels(trace(e))
    finally:
        e.close()
    print("never", dict(never))
    print("on", dict(on))
    assert not any("surface" in k or "budget" in k or "volume" in k for k in never), sorted(never)
    # (names, not counts: how many speculative iterations a trace enqueues depends on timing)
    assert set(off) == set(never), (sorted(off), sorted(never))
    assert any("k_volume_sum" in k for k in on) and any("k_volume_commit" in k for k in on), sorted(on)
    assert not any("k_budget" in k or "k_surface" in k for k in on), sorted(on)
    # the shading's names differ from the default's only in the record's template argument
    stage_on = sorted(k for k in on if "k_shade_stage" in k)
    stage_off = sorted(k for k in never2 if "k_shade_stage" in k)
    assert stage_on and stage_off
    if all("<" in k for k in stage_on + stage_off):     # (where the records carry the template arguments)
        assert not set(stage_on) & set(stage_off), (stage_on, stage_off)
    rest = lambda c: {k for k in c if "k_shade_stage" not in k and "k_volume" not in k}  # noqa: E731
    assert rest(on) == rest(never2), (sorted(rest(on)), sorted(rest(never2)))
