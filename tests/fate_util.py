"""A scene whose ray fates are constructed, for the tests of the traced
compaction (tests/test_fate_host.py, tests/test_gpu_compaction.py) -- TEST
INFRASTRUCTURE.

Scene: unit-square patches, two triangles each, in the plane z = 0, side by
side along x (patch j covers x in [j, j + 1], y in [0, 1]); each patch is its
own mesh and every vertex coordinate is an integer.  A collimated beam from
z = 1 straight down gives every ray the fate of the patch it is aimed at:

  mirror      type 1, reflectivity 1.0    reflected child only, power = parent's
  matched     type 0, IOR = ior_env       both children; reflected power exactly 0,
                                          refracted power = parent's
  glass       type 0, IOR 1.5, diss 0.02  both children, non-trivial powers
  measure     type 3                      measured, no child
  terminator  type 2                      nothing
  vanish      type 4                      meas 0, no child
  gap         no patch (and no floor)     no hit

A ceiling at z = 2 and a floor at z = -1 (two triangles each, over the patches
but not under the gap) catch the second iteration: reflected children end on
the ceiling, refracted ones on the floor.  Far-away one-triangle filler meshes
raise the mesh count K without ever being hit.

Rays: origin (x, y, 1), direction (0, 0, -1), (x, y) unique per ray on a 2^-10
grid strictly inside one triangle of the target patch, clear of its borders, of
its diagonal and of the diagonal of the ceiling and the floor.  A child's origin is
(ox + 0 t, oy + 0 t, .) = the parent's x and y bit for bit, so (x, y) names the
parent in every block of the next population and in the measured record.  Power
is float32(i + 1).
"""
from __future__ import annotations

import types

import numpy as np

from soup_util import _rows

FATES = ("mirror", "matched", "glass", "measure", "terminator", "vanish", "gap")
# (type, IOR, R, dissipation)
_MAT = dict(mirror=(1, 1.0, 1.0, 0.0), matched=(0, 1.0, 0.0, 0.0), glass=(0, 1.5, 0.0, 0.02),
            measure=(3, 1.0, 0.0, 0.0), terminator=(2, 1.0, 0.0, 0.0), vanish=(4, 1.0, 0.0, 0.0))
MAX_RAY_LEN = np.float32(10.0)
IOR_ENV = np.float32(1.0)
GRID = 1024                         # (x, y) on a 2^-10 grid
_EDGE, _DIAG = 16, 32               # grid steps kept clear of the borders / of the diagonal

# measure meshes in all -> (measure patches, ceiling, floor)
MEASURE_LAYOUTS = {0: (0, "terminator", "terminator"), 1: (1, "terminator", "terminator"),
                   2: (1, "measure", "terminator"), 4: (2, "measure", "measure"), 5: (3, "measure", "measure")}


def _quad(x0, x1, z):
    """Two triangles over x in [x0, x1], y in [0, 1] at height z; the diagonal runs
    from (x1, 0) to (x0, 1)."""
    a, b, c, d = (x0, 0, z), (x1, 0, z), (x0, 1, z), (x1, 1, z)
    return [(a, b, c), (d, c, b)]


def scene(measure_patches=1, ceiling="measure", floor="terminator", K=None, all_matched=False):
    """-> a namespace: ``arrs`` (the arguments of Engine.upload_arrays), ``patch``
    (fate -> list of mesh ids; the mesh id is the patch's x), ``kinds`` (the
    fates this scene can give), ``gap_x``, ``ceiling`` / ``floor`` (mesh ids),
    ``n_measure_meshes``, ``K``.  ``K``: filler meshes up to that mesh count.
    ``all_matched``: the same geometry with every patch of the matched material
    (every ray aimed at a patch then keeps both children)."""
    order = ["mirror", "matched", "glass"] + ["measure"] * measure_patches + ["terminator", "vanish"]
    tris, ids, mats, patch = [], [], [], {}
    for j, kind in enumerate(order):
        tris += _quad(j, j + 1, 0)
        ids += [j, j]
        mats.append(_MAT["matched" if all_matched else kind])
        patch.setdefault(kind, []).append(j)
    P = len(order)
    for j, (kind, z) in enumerate(((ceiling, 2), (floor, -1))):
        assert kind in ("measure", "terminator")
        tris += _quad(0, P, z)
        ids += [P + j, P + j]
        mats.append(_MAT[kind])
    base = P + 2
    K = base if K is None else int(K)
    assert K >= base
    for j in range(base, K):            # never hit: the beam stays below x = P + 2, z <= 1
        x = 64 + 2 * j
        tris.append(((x, 64, 32), (x + 1, 64, 32), (x, 65, 32)))
        ids.append(j)
        mats.append(_MAT["terminator"])
    t = np.asarray(tris, np.float64)
    m = np.asarray(mats, np.float64)
    arrs = (_rows(t[:, 0]), _rows(t[:, 1]), _rows(t[:, 2]), np.asarray(ids, np.int32), m[:, 0].astype(np.int32),
            m[:, 1].astype(np.float32), m[:, 2].astype(np.float32), m[:, 3].astype(np.float32))
    kinds = tuple(k for k in FATES if k == "gap" or k in patch)
    n_meas = int(np.sum(arrs[4] == 3))
    return types.SimpleNamespace(arrs=arrs, patch=patch, kinds=kinds, gap_x=P + 1, ceiling=P, floor=P + 1,
                                 n_measure_meshes=n_meas, K=K, tri_count=len(tris))


def layout(n_measure, K=None, all_matched=False):
    """The scene with ``n_measure`` measure meshes in all (0, 1, 2, 4 or 5)."""
    p, c, f = MEASURE_LAYOUTS[n_measure]
    sc = scene(p, c, f, K, all_matched)
    assert all_matched or sc.n_measure_meshes == n_measure
    return sc


# -- fate patterns: kind index (into FATES) per ray ----------------------------------
def uniform(kind):
    def f(n, kinds):
        return np.full(n, FATES.index(kind), np.int32)
    f.label = f"uniform-{kind}"
    f.needs = (kind,)
    return f


def halves(a, b):
    def f(n, kinds):
        out = np.full(n, FATES.index(b), np.int32)
        out[: (n + 1) // 2] = FATES.index(a)
        return out
    f.label = f"halves-{a}-{b}"
    f.needs = (a, b)
    return f


def cycle():
    def f(n, kinds):
        k = np.array([FATES.index(x) for x in kinds], np.int32)
        return k[np.arange(n) % len(k)]
    f.label = "cycle"
    f.needs = ()
    return f


def random(seed):
    def f(n, kinds):
        k = np.array([FATES.index(x) for x in kinds], np.int32)
        return k[np.random.default_rng([911, int(seed), int(n)]).integers(0, len(k), n)]
    f.label = f"random{seed}"
    f.needs = ()
    return f


def all_patterns():
    return [uniform(k) for k in FATES] + [halves("matched", "terminator"), halves("terminator", "matched"),
                                          cycle(), random(1)]


_PTS = None


def _points():
    """The grid points strictly inside the lower-left triangle of the unit
    square, clear of its borders and of the diagonal, in a fixed shuffled order."""
    global _PTS
    if _PTS is None:
        a, b = np.meshgrid(np.arange(_EDGE, GRID), np.arange(_EDGE, GRID), indexing="ij")
        ok = a + b <= GRID - _DIAG
        pts = np.stack([a[ok], b[ok]], axis=1).astype(np.int64)
        _PTS = pts[np.random.default_rng(4242).permutation(len(pts))]
    return _PTS


def rays(sc, fates):
    """The beam for the fate of every ray -> (origin (n,4), dir (n,4), power (n,))
    float32.  A patch's rays take its points in turn, in the lower triangle and
    mirrored into the upper one alternately."""
    fates = np.asarray(fates, np.int32)
    n = len(fates)
    pts = _points()
    gx = np.zeros(n, np.int64)          # (x, y) in grid steps
    gy = np.zeros(n, np.int64)
    k = np.arange(2 * len(pts))
    up = (k & 1) == 1
    ca, cb = np.where(up, GRID - pts[k >> 1, 0], pts[k >> 1, 0]), np.where(up, GRID - pts[k >> 1, 1], pts[k >> 1, 1])
    for ki, kind in enumerate(FATES):
        sel = np.flatnonzero(fates == ki)
        if sel.size == 0:
            continue
        xs = [sc.gap_x] if kind == "gap" else sc.patch[kind]
        for q, x0 in enumerate(xs):     # several patches of a kind: the kind's rays in turn
            s = sel[q::len(xs)]
            if s.size == 0:
                continue
            # clear of the ceiling's and the floor's diagonal too, from (P, 0) to (0, 1):
            # a child crossing both of their triangles would count two hits, be taken as
            # entering from its parent's patch, and a glass child would dissipate on the way
            far = np.abs(x0 * GRID + ca + sc.ceiling * cb - sc.ceiling * GRID) >= _DIAG
            assert int(far.sum()) >= s.size, "more rays than grid points in a patch"
            gx[s] = x0 * GRID + ca[far][: s.size]
            gy[s] = cb[far][: s.size]
    o = np.zeros((n, 4), np.float32)
    o[:, 0] = gx / GRID                 # exact: at most 4 + 10 significant bits
    o[:, 1] = gy / GRID
    o[:, 2] = 1.0
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = -1.0
    p = (np.arange(n) + 1).astype(np.float32)
    assert len(np.unique(gx * (2 * GRID) + gy)) == n
    return o, d, p


def target_mesh(sc, fates):
    """The mesh every ray is aimed at (-1: the gap), as ``rays`` assigns them."""
    fates = np.asarray(fates, np.int32)
    out = np.full(len(fates), -1, np.int32)
    for ki, kind in enumerate(FATES):
        if kind == "gap":
            continue
        sel = np.flatnonzero(fates == ki)
        xs = sc.patch.get(kind, [])
        for q, x0 in enumerate(xs):
            out[sel[q::len(xs)]] = x0
    return out


# (meas, r_meas, t_meas) of each fate
_FATE_OUT = dict(mirror=(0, 0, -1), matched=(0, 0, 0), glass=(0, 0, 0), measure=(1, -1, -1),
                 terminator=(-1, -1, -1), vanish=(0, -1, -1), gap=(-1, -1, -1))


def intended(sc, fates):
    """-> dict(meas, r_meas, t_meas, isect_mid): what a bounce of ``rays(sc, fates)``
    must give."""
    fates = np.asarray(fates, np.int32)
    tab = np.array([_FATE_OUT[k] for k in FATES], np.int32)
    return dict(meas=tab[fates, 0], r_meas=tab[fates, 1], t_meas=tab[fates, 2], isect_mid=target_mesh(sc, fates))


def ray_key(xy):
    """(x, y) rows -> one integer per row, exact for grid points: the name of the
    parent ray."""
    xy = np.asarray(xy, np.float64)
    k = xy[:, 0] * GRID * (2 * GRID) + xy[:, 1] * GRID
    assert np.all(k == np.round(k)), "an origin off the grid"
    return k.astype(np.int64)


def parents_of(keys, emitted_keys):
    """Index of the emitted ray with each key (every key must name one)."""
    order = np.argsort(emitted_keys)
    pos = np.searchsorted(emitted_keys[order], keys)
    assert np.all(pos < len(order)) and np.array_equal(emitted_keys[order][pos], keys), "a row that names no emitted ray"
    return order[pos]


def check_fates(sc, fates, o, p, out):
    """The host-only condition: a bounce ``out`` (oracle.bounce layout) of the
    emitted rays gives every ray its intended fate, and the identity relations
    hold: child origin x, y = the parent's; mirror r_pow == pow; matched r_pow == 0
    and t_pow == pow.  No ray is excluded."""
    fates = np.asarray(fates, np.int32)
    want = intended(sc, fates)
    for k in ("meas", "r_meas", "t_meas", "isect_mid"):
        np.testing.assert_array_equal(np.asarray(out[k]).reshape(-1), want[k], err_msg=k)
    for c in ("r_origin", "t_origin"):
        np.testing.assert_array_equal(out[c][:, :2], o[:, :2], err_msg=c)
    pw = np.asarray(out["pow"], np.float32).reshape(-1)
    mir, mat, gla = (fates == FATES.index(k) for k in ("mirror", "matched", "glass"))
    np.testing.assert_array_equal(out["r_pow"][mir], pw[mir])
    np.testing.assert_array_equal(pw[mir | mat], p[mir | mat])
    np.testing.assert_array_equal(out["r_pow"][mat], np.zeros(int(mat.sum()), np.float32))
    np.testing.assert_array_equal(out["t_pow"][mat], pw[mat])
    if gla.any():                       # non-trivial shares, the smallest reflection above 0.039
        assert np.all(out["r_pow"][gla] > 0.039) and np.all(out["t_pow"][gla] > out["r_pow"][gla])
