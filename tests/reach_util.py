"""Scenes whose hits depend on the length of a ray's direction, for the tests of
the direction-length bounds (tests/test_reach_host.py, tests/test_gpu_reach.py)
-- TEST INFRASTRUCTURE, in the style of soup_util, fate_util and stack_util.

Moller-Trumbore rejects a triangle when |DEN| <= 1e-6 with DEN = E1 . (D x E2),
and the reference never normalises D: a triangle of cross product c = |E1 x E2|
met head-on is hit only by directions longer than L = 1e-6 / c.  Two clusters of
64 such triangles in the plane z = 5, every triangle with its own interior:

  tiny     right triangles with legs 2e-4 on a 1e-3 grid, L_tiny = 25: "never a
           candidate" for filter_record while Dcap is 16 (4e-8 * 16 < 1e-6)
  needle   legs 0.03, the second 5e-7 off the first, L_needle = 66.7: kappa = 0.9,
           a sliver for filter_record, with sliver_dmin = 65.4 just below L

The scene around a cluster (a mesh each; rays travel along +z from z = 2):

  plate    optional, type 0, IOR 1.0 in an environment of IOR 3.0: a sheet at z = 4
           over the cluster and its far side at z = 9 behind everything, so a ray
           counts two crossings, enters it (n1 = 3, n2 = 1) and its transmitted
           child is sqrt(9 |D|^2 - 8) long at normal incidence, about 3 |D|
  mirror   optional, beside the plate at z = 4: a reflected child keeps |D|, the
           short control of the second population
  cluster  type 3 (measure)
  back     measure, z = 7, x in [-6, 3]     term   terminator, z = 7, x in [3, 6]
  front    measure, z = -1: catches what comes back

Rays: `special` (aimed at cluster interiors, longer than L), `control` (the same
aim, shorter than L), `bulk` (short, aimed at the large surfaces or travelling
in the plane z = 2, which holds no surface).
"""
from __future__ import annotations

import types

import numpy as np

from soup_util import _rows, meshes_of, oracle_scene  # noqa: F401  (re-exported)

MAX_RAY_LEN = np.float32(100.0)
IOR_ENV_PLATE = np.float32(3.0)
Z_FRONT, Z_EMIT, Z_PLATE, Z_CLUSTER, Z_BACK, Z_REAR = -1.0, 2.0, 4.0, 5.0, 7.0, 9.0
SIDE = 8                                # a cluster is SIDE x SIDE triangles
AIM = (0.3, 0.3)                        # barycentric aim point inside a triangle
DEN_MIN = 1e-6                          # Moller-Trumbore's EPSILON_NUM
# (type, IOR, R, dissipation)
_MAT = dict(plate=(0, 1.0, 0.0, 0.0), mirror=(1, 1.0, 0.9, 0.0), cluster=(3, 1.0, 0.0, 0.0),
            back=(3, 1.0, 0.0, 0.0), term=(2, 1.0, 0.0, 0.0), front=(3, 1.0, 0.0, 0.0))
PLATE_BOX = (-1.0, 1.0, -1.0, 1.0)      # x0, x1, y0, y1
MIRROR_BOX = (2.0, 4.0, -1.0, 1.0)


def _quad(x0, x1, y0, y1, z):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x0, y1, z), (x1, y1, z)
    return [(a, b, c), (d, c, b)]


def tiny_cluster(leg=2e-4, z=Z_CLUSTER):
    """SIDE^2 right triangles with legs `leg` at the points of a 1e-3 grid."""
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    v0 = np.stack([1e-3 * i.ravel(), 1e-3 * j.ravel(), np.full(SIDE * SIDE, z)], axis=1)
    return v0, v0 + np.array([leg, 0.0, 0.0]), v0 + np.array([0.0, leg, 0.0])


def needle_cluster(leg=0.03, off=5e-7, z=Z_CLUSTER):
    """SIDE^2 needles along x: E1 = (leg, 0, 0), E2 = (0.8 leg, off, 0); columns 0.04
    apart in x, rows 1e-3 apart in y (small y keeps `off` well resolved in float32)."""
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    v0 = np.stack([0.04 * i.ravel(), 1e-3 * j.ravel(), np.full(SIDE * SIDE, z)], axis=1)
    return v0, v0 + np.array([leg, 0.0, 0.0]), v0 + np.array([0.8 * leg, off, 0.0])


def threshold_lengths(v0, v1, v2):
    """1e-6 / |E1 x E2| per triangle, from the float32 vertices and float32 edges as
    the kernels form them."""
    a, b, c = (np.asarray(x, np.float32)[:, :3] for x in (v0, v1, v2))
    e1, e2 = np.float64(b - a), np.float64(c - a)
    return DEN_MIN / np.linalg.norm(np.cross(e1, e2), axis=1)


def scene(cluster="tiny", plate=False, leg=None):
    """-> a namespace: ``arrs`` (the arguments of Engine.upload_arrays), ``mesh``
    (name -> mesh id), ``tris`` (the cluster's triangle indices), ``L`` (the
    cluster's threshold lengths, min and max), ``ior_env``, ``cluster``."""
    if cluster == "tiny":
        cl = tiny_cluster(**({} if leg is None else dict(leg=leg)))
    else:
        cl = needle_cluster(**({} if leg is None else dict(leg=leg)))
    parts = []
    if plate:
        parts.append(("plate", _quad(*PLATE_BOX, Z_PLATE) + _quad(-6.0, 6.0, -6.0, 6.0, Z_REAR)))
        parts.append(("mirror", _quad(*MIRROR_BOX, Z_PLATE)))
    parts.append(("cluster", list(zip(*cl))))
    parts += [("back", _quad(-6.0, 3.0, -6.0, 6.0, Z_BACK)), ("term", _quad(3.0, 6.0, -6.0, 6.0, Z_BACK)),
              ("front", _quad(-6.0, 6.0, -6.0, 6.0, Z_FRONT))]
    t = np.asarray([tri for _, tris in parts for tri in tris], np.float64)
    ids = np.repeat(np.arange(len(parts)), [len(tris) for _, tris in parts]).astype(np.int32)
    m = np.asarray([_MAT[name] for name, _ in parts], np.float64)
    arrs = (_rows(t[:, 0]), _rows(t[:, 1]), _rows(t[:, 2]), ids, m[:, 0].astype(np.int32), m[:, 1].astype(np.float32),
            m[:, 2].astype(np.float32), m[:, 3].astype(np.float32))
    mesh = {name: j for j, (name, _) in enumerate(parts)}
    tris = np.flatnonzero(ids == mesh["cluster"])
    L = threshold_lengths(*(a[tris] for a in arrs[:3]))
    return types.SimpleNamespace(arrs=arrs, mesh=mesh, tris=tris, L=(float(L.min()), float(L.max())), cluster=cluster,
                                 plate=bool(plate), ior_env=IOR_ENV_PLATE if plate else np.float32(1.0))


def child_length(length, r=3.0):
    """|D| of the transmitted child of a ray of |D| = length at normal incidence,
    n1 / n2 = r (reflect_refract with an unnormalised direction: cosT1 = |D|)."""
    return float(np.sqrt(1.0 - r * r * (1.0 - length * length)))


def aim_points(sc, which):
    """The aim point (x, y) inside cluster triangle which[k] (cycled), float64 from
    the float32 vertices."""
    t = sc.tris[np.asarray(which) % len(sc.tris)]
    a, b, c = (np.float64(x[t, :3]) for x in sc.arrs[:3])
    p = a + AIM[0] * (b - a) + AIM[1] * (c - a)
    return p[:, :2]


def _along_z(xy, length):
    n = len(xy)
    o = np.concatenate([xy, np.full((n, 1), Z_EMIT)], axis=1)
    d = np.zeros((n, 3))
    d[:, 2] = length
    return o, d


def population(sc, n, special_at=(), special_len=0.0, control_len=1.0, n_control=32, bulk_len=1.0, seed=0):
    """n rays of a scene without a plate: `special` rays (|D| = special_len, aimed
    at cluster interiors) at the indices special_at, n_control `control` rays
    (the same aims, |D| = control_len) spread over the rest, and `bulk` rays of
    |D| = bulk_len: 3 in 4 from near the emitter plane towards a random point of the
    surfaces at z = 7, 1 in 4 travelling inside the plane z = 2 (they hit nothing).
    -> (origin (n,4), dir (n,4), power (n,)) float32 and a namespace of index
    arrays: special, control, away."""
    rng = np.random.default_rng([401, int(n), int(seed), len(special_at)])
    special = np.asarray(sorted(int(i) % n for i in special_at), np.int64)
    rest = np.setdiff1d(np.arange(n), special)
    control = rest[np.linspace(0, len(rest) - 1, min(n_control, len(rest))).astype(np.int64)] if n_control else rest[:0]
    control = np.unique(control)
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    # bulk
    src = np.stack([rng.uniform(-5.0, 5.0, n), rng.uniform(-5.0, 5.0, n), np.full(n, Z_EMIT)], axis=1)
    tgt = np.stack([rng.uniform(-5.5, 5.5, n), rng.uniform(-5.5, 5.5, n), np.full(n, Z_BACK)], axis=1)
    away = rng.random(n) < 0.25
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    dd = np.where(away[:, None], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1), tgt - src)
    dd *= bulk_len / np.linalg.norm(dd, axis=1, keepdims=True)
    o[:], d[:] = src, dd
    for idx, length in ((special, special_len), (control, control_len)):
        if len(idx):
            o[idx], d[idx] = _along_z(aim_points(sc, np.arange(len(idx))), length)
    away[special] = False
    away[control] = False
    pw = (1.0 + 0.125 * (np.arange(n) % 7)).astype(np.float32)
    return _rows(o), _rows(d), pw, types.SimpleNamespace(special=special, control=control, away=np.flatnonzero(away))


def away_population(n, length=1.0, seed=0):
    """n rays travelling inside the plane z = 2: they hit nothing."""
    rng = np.random.default_rng([402, int(n), int(seed)])
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    o = np.stack([rng.uniform(-5.0, 5.0, n), rng.uniform(-5.0, 5.0, n), np.full(n, Z_EMIT)], axis=1)
    d = length * np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1)
    return _rows(o), _rows(d), np.ones(n, np.float32)


def plate_population(sc, n, plate_at, length, seed=0):
    """n rays of one length along +z in a scene with a plate: the rays at the
    indices plate_at go through the plate at the cluster's aim points (their
    transmitted children are about three times as long), the others alternate
    between the mirror (children of the same length) and the back surface.
    -> (origin, dir, power) and a namespace: plate, mirror, back (index arrays)."""
    assert sc.plate
    rng = np.random.default_rng([403, int(n), int(seed)])
    plate = np.asarray(sorted(int(i) % n for i in plate_at), np.int64)
    rest = np.setdiff1d(np.arange(n), plate)
    mirror, back = rest[0::2], rest[1::2]
    xy = np.zeros((n, 2))
    x0, x1, y0, y1 = MIRROR_BOX
    xy[mirror] = np.stack([rng.uniform(x0 + 0.1, x1 - 0.1, len(mirror)), rng.uniform(y0 + 0.1, y1 - 0.1, len(mirror))], axis=1)
    xy[back] = np.stack([rng.uniform(-5.5, -1.5, len(back)), rng.uniform(-5.5, 5.5, len(back))], axis=1)
    xy[plate] = aim_points(sc, np.arange(len(plate)))
    o, d = _along_z(xy, length)
    pw = (1.0 + 0.125 * (np.arange(n) % 7)).astype(np.float32)
    return _rows(o), _rows(d), pw, types.SimpleNamespace(plate=plate, mirror=mirror, back=back)


def cluster_hits(sc, out, idx=None):
    """How many of the rays idx (all) of a bounce end on the cluster."""
    mid = np.asarray(out["isect_mid"]).reshape(-1)
    return int(np.sum((mid if idx is None else mid[idx]) == sc.mesh["cluster"]))
