"""The surface map formed on the host -- TEST INFRASTRUCTURE.

``cutoff_ref.trace_rays`` run with a ``bounce_fn`` wrapper, as
``budget_ref.trace`` runs it, around ``oracle.bounce`` (the CPU oracle) or the
reference's own kernels (``tests/ref_gpu.py``).  From each bounce's per-ray
outputs -- ``isect_idx``, ``isect_mid``, ``pow``, ``r_pow`` / ``r_meas``,
``t_pow`` / ``t_meas`` -- the wrapper forms, for every ray whose nearest hit
exists (``isect_mid >= 0``), the float64 terms include/lpc.h fixes, booked to the
triangle ``isect_idx``:

    incident   float64(p)                                  every hit
    deposited  float64(p)                                  hit mesh of type 2 or 3
               (float64(p) - float64(kr)) - float64(kt)    every other hit mesh

with kr = r_pow where r_meas == 0 else 0, kt likewise, before any cutoff.  The
terms are kept as flat lists with their triangle and mesh, so a map summed in any
order can be compared by the budget's rule: counts equal, each float64 sum within
(n - 1) 2^-53 sum|terms| of ``math.fsum(terms)``.
"""
from __future__ import annotations

import math

import numpy as np

import budget_ref
import cutoff_ref

U = budget_ref.U


def bounce_terms(scene, out):
    """One iteration's terms -> dict(tri, mesh (int32), incident, deposited (float64))
    over the rays that hit."""
    f64 = np.float64
    p = np.asarray(out["pow"], np.float32).reshape(-1)
    hit = np.asarray(out["isect_mid"], np.int32).reshape(-1)
    tri = np.asarray(out["isect_idx"], np.int32).reshape(-1)
    kr = np.where(np.asarray(out["r_meas"]).reshape(-1) == 0, np.asarray(out["r_pow"], np.float32).reshape(-1),
                  np.float32(0.0)).astype(np.float32)
    kt = np.where(np.asarray(out["t_meas"]).reshape(-1) == 0, np.asarray(out["t_pow"], np.float32).reshape(-1),
                  np.float32(0.0)).astype(np.float32)
    K = scene.mesh_count
    h = hit >= 0
    mt = np.where(h, scene.mat_type[np.clip(hit, 0, K - 1)], -1)
    whole = (mt == 2) | (mt == 3)
    with np.errstate(invalid="ignore"):
        dep = np.where(whole, p.astype(f64), (p.astype(f64) - kr.astype(f64)) - kt.astype(f64))
    return dict(tri=tri[h], mesh=hit[h], incident=p.astype(f64)[h], deposited=dep[h])


def trace(oracle_mod, meshes, origin, dirs, power, iterations, tau, max_ray_len, ior_env, cut=0.0, bounce_fn=None,
          keep_results=False, with_budget=False):
    """-> dict(tri, mesh, incident, deposited: the trace's terms in bounce order,
    iters: the per-iteration dicts, counts, M: the scene's triangle count, K;
    budget: budget_ref's reference of the same bounces when with_budget)."""
    inner = oracle_mod.bounce if bounce_fn is None else bounce_fn
    iters, bud = [], []
    box = {}

    def wrapped(scene, o, d, pw, ms, mid, mrl, ior):
        p_in = np.array(pw, dtype=np.float32).reshape(-1)
        out = inner(scene, o, d, pw, ms, mid, mrl, ior)
        iters.append(bounce_terms(scene, out))
        if with_budget:
            bud.append(budget_ref.bounce_terms(scene, p_in, out))
        box["M"] = int(scene.tri_count)
        return out

    res, info = cutoff_ref.trace_rays(oracle_mod, origin, dirs, power, meshes, iterations, tau, max_ray_len, ior_env,
                                      cut=cut, keep_results=keep_results, bounce_fn=wrapped)
    ref = dict(iters=iters, counts=list(info["counts"]), K=len(meshes), M=box.get("M", 0), results=res)
    for k in ("tri", "mesh", "incident", "deposited"):
        ref[k] = (np.concatenate([it[k] for it in iters]) if iters else np.zeros(0))
    if with_budget:
        ref["budget"] = dict(iters=bud, culled=info["culled"], counts=list(info["counts"]),
                             mesh_power=np.asarray(info["mesh_power"]), K=len(meshes), results=res)
    return ref


def by_triangle(ref):
    """-> {triangle: (incident terms, deposited terms)} of the triangles that were hit."""
    order = np.argsort(ref["tri"], kind="stable")
    tri = ref["tri"][order]
    inc, dep = ref["incident"][order], ref["deposited"][order]
    cuts = np.flatnonzero(np.diff(tri)) + 1
    lo = np.concatenate(([0], cuts))
    hi = np.concatenate((cuts, [len(tri)]))
    return {int(tri[a]): (inc[a:b], dep[a:b]) for a, b in zip(lo, hi) if b > a}


def mesh_deposited(ref, mesh):
    """Every deposited term booked to a triangle of `mesh`."""
    return ref["deposited"][ref["mesh"] == mesh]


def sum_tol(terms):
    return max(len(terms) - 1, 0) * U * math.fsum(abs(float(v)) for v in terms)


def assert_surface(s, ref, what="", factor=1.0):
    """A library map (``Engine.surface()``'s dict: flat ``incident``, ``deposited``,
    ``count``) against the helper's terms: every triangle's count equal, every sum
    within `factor` times the bound (NaN sums where the terms hold a NaN)."""
    M = ref["M"]
    inc, dep, cnt = (np.asarray(s[k]) for k in ("incident", "deposited", "count"))
    assert len(inc) == len(dep) == len(cnt) == M, (what, len(inc), len(dep), len(cnt), M)
    want_cnt = np.bincount(ref["tri"], minlength=M) if len(ref["tri"]) else np.zeros(M, np.int64)
    assert len(want_cnt) == M, (what, "a triangle index outside the scene")
    bad = np.flatnonzero(cnt != want_cnt)
    assert len(bad) == 0, (what, "counts", bad[:8], cnt[bad[:8]], want_cnt[bad[:8]])
    groups = by_triangle(ref)
    untouched = np.ones(M, bool)
    for t, (ti, td) in groups.items():
        untouched[t] = False
        for got, terms, col in ((inc[t], ti, "incident"), (dep[t], td, "deposited")):
            want = math.fsum(float(v) for v in terms)
            if math.isnan(want):
                assert math.isnan(float(got)), (what, col, t)
                continue
            tol = factor * sum_tol(terms)
            assert abs(float(got) - want) <= tol, (what, col, t, float(got), want, tol)
    assert not inc[untouched].any() and not dep[untouched].any(), (what, "power on a triangle that was never hit")


# -- the constructed strip ---------------------------------------------------------
# N triangles in the plane z = 0, triangle j around (2 j, 0) (its centroid, exact
# in float32), one mesh per STRIP_MESH triangles; ray i falls from z = 1 straight
# down onto the centroid of triangle target(i).  Every ray's fate is known without
# a trace, so the expected map is a host sum.
STRIP_MESH = 64


def strip_scene(N, kinds=("terminator",)):
    """-> the strip's meshes; mesh m is of kind kinds[m % len(kinds)] ("terminator",
    "measure", or "mirror" with R = 0.5)."""
    from lightpycl_amd import geo_optical_elements as goe
    meshes = []
    for m, lo in enumerate(range(0, N, STRIP_MESH)):
        j = np.arange(lo, min(lo + STRIP_MESH, N), dtype=np.float64)
        V = np.zeros((3 * len(j), 4), np.float64)
        V[0::3, 0], V[0::3, 1] = 2 * j - 0.5, -0.25
        V[1::3, 0], V[1::3, 1] = 2 * j + 0.5, -0.25
        V[2::3, 0], V[2::3, 1] = 2 * j, 0.5
        T = np.arange(3 * len(j), dtype=np.int32).reshape(-1, 3)
        kind = kinds[m % len(kinds)]
        g = goe.GeoObject(V, T, mat_type=kind)
        if kind == "mirror":
            g.reflectivity = 0.5                # setMaterial does not store a mirror's reflectivity
        meshes.append(g)
    return meshes


def strip_rays(targets, scale=1.0):
    """-> origin (n,4), direction (n,4), power (n,) float32: ray i onto triangle
    targets[i] with power (i + 1) * scale (scale a power of two)."""
    t = np.asarray(targets, np.int64)
    n = len(t)
    o = np.zeros((n, 4), np.float32)
    o[:, 0], o[:, 2] = 2.0 * t, 1.0
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = -1.0
    p = ((np.arange(n, dtype=np.float64) + 1.0) * scale).astype(np.float32)
    assert np.array_equal(o[:, 0].astype(np.int64), 2 * t) and np.array_equal(p.astype(np.float64) / scale,
                                                                              np.arange(n) + 1.0)
    return o, d, p


def strip_expected(N, targets, power, kinds=("terminator",)):
    """The strip's map as integer sums on the host (exact: every sum is an integer
    multiple of a power of two below 2^53 of it) -> dict of Engine.surface()'s shape."""
    t = np.asarray(targets, np.int64)
    p = np.asarray(power, np.float32)
    kind = np.array([kinds[(j // STRIP_MESH) % len(kinds)] for j in range(N)])[t] if len(t) else np.zeros(0, str)
    kr = np.where(kind == "mirror", p * np.float32(0.5), np.float32(0.0)).astype(np.float32)
    dep = np.where(kind == "mirror", p.astype(np.float64) - kr.astype(np.float64), p.astype(np.float64))
    return dict(incident=np.bincount(t, weights=p.astype(np.float64), minlength=N),
                deposited=np.bincount(t, weights=dep, minlength=N),
                count=np.bincount(t, minlength=N).astype(np.int64))


def strip_patterns(n, N, table):
    """The target patterns of n rays on N triangles (`table`: the entries of the
    kernel's LDS table) -> {name: targets}; a pattern that needs more triangles
    than N is left out."""
    i = np.arange(n, dtype=np.int64)
    pat = {"one": np.full(n, min(5, N - 1), np.int64), "scatter7": (7 * i) % N}
    if n <= N:
        pat["own"] = i.copy()
    for run in (3, 64, 65, 100):
        if (n - 1) // run < N:
            pat[f"run{run}"] = i // run
    for mod in (table, 2 * table):              # the same table entry, other triangles: the conflict path
        if 3 * mod + 3 < N:
            pat[f"mod{mod}"] = 3 + mod * (i % 4)
    return pat
