"""Inputs of tests/test_gpu_iter_launches.py that a host test pins as well
(tests/test_iter_launches_host.py) -- TEST INFRASTRUCTURE.

The measure hemisphere of ``scenes.synthetic`` is a half circle revolved about
the x axis.  At its pole on the negative x axis the curve's last point lies
1.2e-13 off the axis, so the first triangle of every angle step there has two
vertices that differ by less than the float32 spacing of the third: its edges
E1 and E2 are the same float32 vectors, E1 x E2 = 0, and no hierarchy record
can hold it -- it is a sliver record, decided by the sliver units alone.  The
exact test's determinant is then rounding noise, and a ray that passes close
to such a triangle's edge can get its nearest hit there.
"""
from __future__ import annotations

import numpy as np

POLE_SIZES = (513, 4159)            # an unsorted and a sorted population


def zero_cross(v0, v1, v2):
    """Which triangles have E1 x E2 = 0 in float32, every component."""
    e1 = (np.asarray(v1, np.float32)[:, :3] - np.asarray(v0, np.float32)[:, :3]).astype(np.float32)
    e2 = (np.asarray(v2, np.float32)[:, :3] - np.asarray(v0, np.float32)[:, :3]).astype(np.float32)
    return np.all(np.cross(e1, e2).astype(np.float32) == 0, axis=1)


def pole_rays(S, n):
    """n rays from the source's centre aimed along the long edge of the
    hemisphere's zero-cross triangles at the negative x pole; ray i carries the
    power i + 1.  S: the scene as ``oracle.Scene`` holds it (mesh 0 the
    hemisphere).  -> (origin (n,4), dir (n,4), power (n,)) float32."""
    v0, v1 = np.float64(S.v0[:, :3]), np.float64(S.v1[:, :3])
    z = zero_cross(S.v0, S.v1, S.v2) & (np.asarray(S.mesh_id) == 0) & (S.v1[:, 0] < 0)
    tri = np.flatnonzero(z)
    assert tri.size >= 64, tri.size
    rng = np.random.default_rng([31, int(n)])
    t = tri[rng.integers(0, tri.size, n)]
    s = rng.uniform(0.05, 0.95, n)[:, None]
    tgt = v1[t] + s * (v0[t] - v1[t])
    o4 = np.zeros((n, 4), np.float32)
    d4 = np.zeros((n, 4), np.float32)
    d4[:, :3] = tgt / np.linalg.norm(tgt, axis=1, keepdims=True)
    return o4, d4, np.arange(1, n + 1, dtype=np.float32)


def nearest_on_zero_cross(S, out):
    """How many rays of a bounce ``out`` have their nearest hit on a triangle
    with E1 x E2 = 0."""
    z = zero_cross(S.v0, S.v1, S.v2)
    hit = np.asarray(out["isect_mid"]) >= 0
    idx = np.asarray(out["isect_idx"])
    assert np.all((idx[hit] >= 0) & (idx[hit] < z.size))
    return int(np.sum(z[idx[hit]]))
