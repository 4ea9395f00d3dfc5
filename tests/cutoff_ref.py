"""The reference's host loop with the per-ray power cutoff -- TEST INFRASTRUCTURE.

``oracle.trace_rays`` (iterative_tracer.py:241-391) with one rule added to its
compaction (:366): a child the reference would keep (``meas == 0``) is culled
iff ``fabsf(child_pow) < cut``, compared in float32 on the power exactly as the
shading wrote it (no arithmetic: this loop and the device decide identically).
A NaN power is never culled; negative powers count by magnitude.  A culled child
is treated as terminated: it is not in the next population, so neither in its
count nor in the power left of the stop rule.  The current iteration's results
tuple (the parents) is unchanged, and emitted rays are never culled.

``bounce_fn`` is ``oracle.bounce`` (the CPU oracle) or the reference's own
kernels (``tests/ref_gpu.py``).  With ``cut = 0`` the loop is
``oracle.trace_rays`` operation for operation.
"""
from __future__ import annotations

import math

import numpy as np


def cut_of(power, f):
    """The cutoff ``f * p0`` as the float32 the library takes: p0 is the input
    power (float64 sum) divided by the ray count."""
    p = np.asarray(power, np.float32).reshape(-1)
    return np.float32(f * float(np.sum(p, dtype=np.float64)) / len(p))


def trace_rays(oracle_mod, origin, dirs, power, meshes, trace_iterations=100, trace_until_dissipated=0.99,
               max_ray_len=np.float32(1e3), ior_env=np.float32(1.0), cut=0.0, keep_results=True, bounce_fn=None,
               measured_out=None):
    """-> (results, info).  results: the per-iteration tuples (origin, dest, pow,
    meas) when ``keep_results``.  info: ``counts`` (population per iteration),
    ``mesh_power`` (float64 per mesh), ``input_power``, ``tri_count`` and
    ``culled``: per iteration the float32 powers of the culled children, in the
    reference's order ([reflected ; refracted], each in ray order).
    ``measured_out`` as in ``oracle.trace_rays``."""
    bounce_fn = oracle_mod.bounce if bounce_fn is None else bounce_fn
    cut = np.float32(cut)
    assert np.isfinite(cut) and cut >= 0
    max_ray_len = np.float32(max_ray_len)
    ior_env = np.float32(ior_env)
    origin = np.asarray(origin, np.float32)
    dirs = np.asarray(dirs, np.float32)
    power = np.asarray(power, np.float32)
    ray_count = origin.shape[0]
    input_power = oracle_mod.f32_sorted_sum(power)                 # :115
    rays_pow = np.array(power, dtype=np.float32)                   # :116
    rays_meas = np.zeros(ray_count, np.int32)                      # :117
    cur_mid = np.zeros(ray_count, np.int32) - 2                    # :118
    scene = oracle_mod.Scene(meshes)
    results, counts, culled = [], [], []
    mesh_power = np.zeros(scene.mesh_count, np.float64)
    for _ in range(int(trace_iterations)):                         # :241
        counts.append(ray_count)
        out = bounce_fn(scene, origin, dirs, rays_pow, rays_meas, cur_mid, max_ray_len, ior_env)
        rays_dest = out["dest"]
        rays_pow = out["pow"].reshape(np.shape(rays_pow))           # :347 keeps the input shape
        rays_meas = out["meas"]
        m = rays_meas >= 0.9
        np.add.at(mesh_power, out["isect_mid"][m], rays_pow.reshape(-1)[m].astype(np.float64))
        if measured_out is not None:
            measured_out.append((rays_dest[m], rays_pow.reshape(-1)[m], out["isect_mid"][m]))
        if keep_results:
            results.append((origin, rays_dest, rays_pow, rays_meas))   # :355
        keep = np.where(np.concatenate((out["r_meas"], out["t_meas"])) == 0)[0]   # :366
        child_pow = np.append(out["r_pow"], out["t_pow"], axis=0).astype(np.float32)
        # the cutoff: float32 |power| < float32 cut (False for NaN)
        with np.errstate(invalid="ignore"):
            drop = np.abs(child_pow[keep]) < cut
        culled.append(child_pow[keep][drop].copy())
        keep = keep[~drop]
        origin = np.append(out["r_origin"], out["t_origin"], axis=0).astype(np.float32)[keep]
        dirs = np.append(out["r_dir"], out["t_dir"], axis=0).astype(np.float32)[keep]
        rays_pow = child_pow[keep]
        rays_meas = np.append(out["r_meas"], out["t_meas"], axis=0).astype(np.int32)[keep]
        power_in_scene = oracle_mod.f32_sorted_sum(rays_pow)       # :372
        cur_mid = np.append(out["isect_mid"], out["isect_mid"], axis=0).astype(np.int32)[keep]
        ray_count = origin.shape[0]
        if power_in_scene < (1.0 - trace_until_dissipated) * input_power:   # :383
            break
        if ray_count == 0:                                         # :389
            break
    info = dict(counts=counts, mesh_power=mesh_power, input_power=input_power, tri_count=scene.tri_count,
                culled=culled)
    return results, info


def aggregate(oracle_mod, bounce_fn, meshes, o4, d4, pw, iterations, tau, max_ray_len, ior_env, cut):
    """parity_util.ref_aggregate with the cutoff: (counts, per-mesh power, sorted
    measured rows) and the culled powers per iteration."""
    from parity_util import measured_rows
    meas = []
    _, info = trace_rays(oracle_mod, o4, d4, pw, meshes, iterations, tau, max_ray_len, ior_env, cut=cut,
                         keep_results=False, bounce_fn=bounce_fn, measured_out=meas)
    if meas:
        pos = np.concatenate([m[0] for m in meas])
        p = np.concatenate([m[1] for m in meas])
        mm = np.concatenate([m[2] for m in meas])
    else:
        pos, p, mm = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)
    return (list(info["counts"]), np.asarray(info["mesh_power"]), measured_rows(pos, p, mm)), info["culled"]


def assert_ledger(counts, powers, culled, what=""):
    """The library's ledger against the helper's culled powers: counts equal,
    each iteration's float64 power within (n - 1) 2^-53 sum|p| (a float64 sum of
    n float32 terms in another order) of the exactly rounded sum."""
    assert len(counts) == len(culled) and len(powers) == len(culled), (what, len(counts), len(culled))
    assert [int(c) for c in counts] == [len(c) for c in culled], (what, list(counts), [len(c) for c in culled])
    for it, (got, c) in enumerate(zip(powers, culled)):
        terms = [float(v) for v in c]
        want = math.fsum(terms)
        tol = max(len(terms) - 1, 0) * 2.0 ** -53 * math.fsum(abs(v) for v in terms)
        assert abs(float(got) - want) <= tol, (what, it, float(got), want, tol)
