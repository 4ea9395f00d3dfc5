"""Seeded triangle soups and aimed rays for the tests of the hierarchy build
(tests/test_build_host.py) and of the walk (tests/test_gpu_soup.py).

A soup is a flat scene as ``lpc_scene_upload`` takes it: ``v0, v1, v2`` as (M, 4)
float32 rows, a sorted ``mesh_id`` and per-mesh material tables.  Nothing here is
shaped like a real optical element: triangle counts, tree shapes, sliver
populations and hit multiplicities are chosen to reach the edges of the build
and the walk, not to look like a lens.

Kinds:
  uniform    centres in a 20-box, edge scales 0.05 / 0.5 / 3
  clustered  three tight clusters of 0.02-size triangles, 8 apart on each axis
  coplanar   axis-aligned right triangles of leg 2 in the plane z = 5, drawn from
             M/4 distinct positions: each position holds about 4 coincident
             duplicates, so the lowest-index-on-equal-t rule decides the result
  mixed      edge scale 10^U(-4, 1.5); 30 % needles (second edge nearly parallel
             to the first, 1e-5 off); 5 % with a zero edge: slivers, thin
             triangles, "never" triangles, runs without a hierarchy triangle
"""
from __future__ import annotations

import types

import numpy as np

KINDS = ("uniform", "clustered", "coplanar", "mixed")
SIZES = (1, 7, 8, 9, 63, 64, 65, 511, 513, 4097)
# material per mesh, cycled: refractive, mirror, measure, terminator (kept children
# exist from the first two, so a second level of rays starts on surfaces)
_MATS = ((0, 1.5, 0.0, 0.02), (1, 1.0, 0.9, 0.0), (3, 1.0, 0.0, 0.0), (2, 1.0, 0.0, 0.0))


def _seed(kind, M, K, seed):
    return [KINDS.index(kind), int(M), int(K), int(seed)]


def _rows(x):
    out = np.zeros((x.shape[0], 4), np.float32)
    out[:, :3] = x
    return out


def materials(K, mats=_MATS):
    mat_type = np.array([mats[j % len(mats)][0] for j in range(K)], np.int32)
    ior = np.array([mats[j % len(mats)][1] for j in range(K)], np.float32)
    refl = np.array([mats[j % len(mats)][2] for j in range(K)], np.float32)
    diss = np.array([mats[j % len(mats)][3] for j in range(K)], np.float32)
    return mat_type, ior, refl, diss


def triangles(kind, M, rng):
    """(v0, v1, v2) as float64 (M, 3) of one soup kind."""
    if kind == "uniform":
        c = rng.uniform(-10.0, 10.0, (M, 3))
        s = rng.choice([0.05, 0.5, 3.0], (M, 1))
        return c, c + s * rng.normal(size=(M, 3)), c + s * rng.normal(size=(M, 3))
    if kind == "clustered":
        c = 8.0 * rng.integers(0, 3, (M, 1)) + 0.1 * rng.normal(size=(M, 3))
        return c, c + 0.02 * rng.normal(size=(M, 3)), c + 0.02 * rng.normal(size=(M, 3))
    if kind == "coplanar":
        npos = max(1, M // 4)
        # positions on a 1/4 grid of the 20-box: exact in float32, so duplicates coincide bit for bit
        pos = np.concatenate([rng.integers(-40, 33, (npos, 2)) / 4.0, np.full((npos, 1), 5.0)], axis=1)
        p = pos[rng.integers(0, npos, M)]
        return p, p + np.array([2.0, 0.0, 0.0]), p + np.array([0.0, 2.0, 0.0])
    if kind == "mixed":
        c = rng.uniform(-10.0, 10.0, (M, 3))
        s = 10.0 ** rng.uniform(-4.0, 1.5, (M, 1))
        e1 = s * rng.normal(size=(M, 3))
        e2 = s * rng.normal(size=(M, 3))
        u = rng.random(M)
        needle = u < 0.30
        off = rng.normal(size=(M, 3))
        e2n = e1 * rng.uniform(0.3, 1.5, (M, 1)) + 1e-5 * np.linalg.norm(e1, axis=1, keepdims=True) * off
        e2 = np.where(needle[:, None], e2n, e2)
        e1 = np.where(((u >= 0.30) & (u < 0.325))[:, None], 0.0, e1)
        e2 = np.where(((u >= 0.325) & (u < 0.35))[:, None], 0.0, e2)
        return c, c + e1, c + e2
    raise ValueError(kind)


def soup(kind, M, K=1, seed=0):
    """-> (v0, v1, v2, mesh_id, mat_type, ior, refl, diss), the arguments of
    ``Engine.upload_arrays``.  mesh_id: M sorted random ids below K (an id may be
    absent: its slot then stays empty, or takes the run before it, as the
    reference's slot arithmetic has it)."""
    rng = np.random.default_rng(_seed(kind, M, K, seed))
    a, b, c = triangles(kind, M, rng)
    mesh_id = np.sort(rng.integers(0, K, M)).astype(np.int32)
    return (_rows(a), _rows(b), _rows(c), mesh_id) + materials(K)


def aimed_rays(arrs, n, seed=0, sigmas=(0.1, 5.0, 100.0), lengths=(0.05, 1.0, 12.0)):
    """n rays aimed at random barycentric points of random triangles of the soup
    (30 % on an edge, 10 % on a vertex), origins offset from the target by
    N(0, sigma) with sigma drawn per ray, direction length drawn per ray.
    -> (origin (n,4), dir (n,4), power (n,)) float32."""
    v0, v1, v2 = (np.float64(a[:, :3]) for a in arrs[:3])
    M = v0.shape[0]
    rng = np.random.default_rng([77, M, int(n), int(seed)])
    t = rng.integers(0, M, n)
    bu, bv = rng.random(n), rng.random(n)
    fold = bu + bv > 1.0
    bu, bv = np.where(fold, 1.0 - bu, bu), np.where(fold, 1.0 - bv, bv)
    u = rng.random(n)
    edge = rng.integers(0, 3, n)
    on_edge = u < 0.30
    s = rng.random(n)
    bu = np.where(on_edge, np.where(edge == 0, s, np.where(edge == 1, 0.0, s)), bu)
    bv = np.where(on_edge, np.where(edge == 0, 0.0, np.where(edge == 1, s, 1.0 - s)), bv)
    on_vertex = (u >= 0.30) & (u < 0.40)
    bu = np.where(on_vertex, np.where(edge == 1, 1.0, 0.0), bu)
    bv = np.where(on_vertex, np.where(edge == 2, 1.0, 0.0), bv)
    tgt = v0[t] + bu[:, None] * (v1[t] - v0[t]) + bv[:, None] * (v2[t] - v0[t])
    sig = rng.choice(list(sigmas), (n, 1))
    org = tgt + sig * rng.normal(size=(n, 3))
    d = tgt - org
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    d *= rng.choice(list(lengths), (n, 1))
    return _rows(org), _rows(d), np.ones(n, np.float32)


def scene_scale(arrs):
    """Half the diagonal of the finite vertex box, as lpc_scene_upload computes
    it (float32 extents, summed in float64; 1 for an empty or point box)."""
    v = np.concatenate([a[:, :3] for a in arrs[:3]]).astype(np.float32)
    diag2 = 0.0
    for k in range(3):
        c = v[:, k][np.isfinite(v[:, k])]
        if c.size == 0:
            continue
        ext = np.float32(c.max()) - np.float32(c.min())
        if np.isfinite(ext):
            diag2 += float(ext) * float(ext)
    return 0.5 * np.sqrt(diag2) if diag2 > 0.0 else 1.0


def runs_of(mesh_id):
    """(run_lo, run_hi, slot) of the runs of equal mesh id, as lpc_scene_upload
    forms them: a run flushes into the slot of the next run's id - 1, the last
    one into its own id (the reference's sequential loop)."""
    mesh_id = np.asarray(mesh_id, np.int32)
    lo = np.flatnonzero(np.concatenate(([True], mesh_id[1:] != mesh_id[:-1]))).astype(np.int32)
    hi = np.concatenate((lo[1:], [mesh_id.size])).astype(np.int32)
    slot = np.concatenate((mesh_id[lo[1:]] - 1, mesh_id[lo[-1:]])).astype(np.int32)
    return lo, hi, slot


def oracle_scene(arrs):
    """The flat arrays as the object ``oracle.bounce`` and the reference-kernel
    runner read (the attributes of ``oracle.Scene``)."""
    v0, v1, v2, mesh_id, mat_type, ior, refl, diss = arrs
    C = np.ascontiguousarray
    return types.SimpleNamespace(mesh_count=int(len(mat_type)), tri_count=int(v0.shape[0]), v0=C(v0, np.float32),
                                 v1=C(v1, np.float32), v2=C(v2, np.float32), mesh_id=C(mesh_id, np.int32),
                                 mat_type=C(mat_type, np.int32), ior=C(ior, np.float32), refl=C(refl, np.float32),
                                 diss=C(diss, np.float32))


class SoupMesh:
    """One mesh of a soup with the two methods a whole trace reads."""

    def __init__(self, v0, v1, v2, mat):
        self._v = [np.asarray(a, np.float32) for a in (v0, v1, v2)]
        self._mat = {"type": int(mat[0]), "IOR": float(mat[1]), "R": float(mat[2]), "dissipation": float(mat[3])}

    def tribuf(self):
        return [a.tolist() for a in self._v]

    def getMaterialBuf(self):
        return dict(self._mat)


def meshes_of(arrs):
    """The soup as a list of mesh objects (every id below K present)."""
    v0, v1, v2, mesh_id, mat_type, ior, refl, diss = arrs
    out = []
    for j in range(len(mat_type)):
        m = mesh_id == j
        assert m.any(), "meshes_of: a mesh without triangles"
        out.append(SoupMesh(v0[m], v1[m], v2[m], (mat_type[j], ior[j], refl[j], diss[j])))
    return out


def kept_children(out, cap=None):
    """The second level of rays: the reference's kept children of a bounce
    (origin, dir, power, previous mesh), the first `cap` of them."""
    keep = np.where(np.concatenate((out["r_meas"], out["t_meas"])) == 0)[0][:cap]
    o2 = np.concatenate((out["r_origin"], out["t_origin"]))[keep]
    d2 = np.concatenate((out["r_dir"], out["t_dir"]))[keep]
    p2 = np.concatenate((out["r_pow"], out["t_pow"]))[keep]
    m2 = np.concatenate((out["isect_mid"], out["isect_mid"]))[keep]
    return o2, d2, p2, m2
