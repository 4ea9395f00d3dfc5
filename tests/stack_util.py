"""A scene of layer stacks: what intersect_postproc resolves for nested, adjacent
and coincident media, one column per situation -- TEST INFRASTRUCTURE for
tests/test_stack_host.py and tests/test_gpu_stack.py, in the style of fate_util.

Column c is the unit square x in [c, c + 1], y in [0, 1]; a column is a list of
(z, mesh) layers, each a quad (fate_util._quad) of that mesh at height z.  A beam
from z = 1 straight down meets every layer of its column at t = 1 - z; how many
layers of a mesh lie under the ray is that mesh's hit count, so an odd number of
layers says the ray starts inside the mesh.  max_ray_len = 10, so EPSILON is
1e-5: NEAR (4e-6) is a gap inside EPSILON, layers further apart are at least
3e-5 apart.  A measuring ceiling at z = 2 catches the reflected children, a
measuring floor at z = -6 lies under every column.

Every column declares what the reference must resolve for its emitted rays:
(hit mesh, n1, n2, the layer whose t the destination takes).  Meshes are named;
FULL has eight (A, B, C glass; a mirror, a measure surface, a type-4 mesh, the
ceiling, the floor), REDUCED four (A, B, C and one measure mesh holding ceiling
and floor) with the columns that need no other mesh.
"""
from __future__ import annotations

import types

import numpy as np

import fate_util as fu
from soup_util import _rows

MAX_RAY_LEN = np.float32(10.0)
IOR_ENV = np.float32(1.0)
NEAR = 4e-6
# (type, IOR, R, dissipation)
MATERIALS = dict(A=(0, 1.5, 0.0, 0.0), B=(0, 1.3, 0.0, 0.05), C=(0, 1.7, 0.0, 0.0), MIR=(1, 1.0, 0.9, 0.0),
                 MEAS=(3, 1.0, 0.0, 0.0), T4=(4, 1.2, 0.0, 0.0), CEIL=(3, 1.0, 0.0, 0.0), FLOOR=(3, 1.0, 0.0, 0.0),
                 M=(3, 1.0, 0.0, 0.0))
FULL = ("A", "B", "C", "MIR", "MEAS", "T4", "CEIL", "FLOOR")
REDUCED = ("A", "B", "C", "M")
TERMINATOR = (2, 1.0, 0.0, 0.0)


def _col(name, layers, hit, n1, n2, t_layer):
    return types.SimpleNamespace(name=name, layers=layers, hit=hit, n1=n1, n2=n2, t_layer=t_layer)


# name, layers, then the declared (hit mesh, n1, n2, layer of t) of a ray emitted from outside (prev -2)
COLUMNS = (
    _col("slab alone", [(0, "A"), (-0.5, "A")], "A", None, "A", 0),
    _col("inside a slab", [(0, "A")], "A", "A", None, 0),
    _col("inside A inside B", [(0, "A"), (-0.5, "B")], "A", "A", "B", 0),
    _col("inside A, C then B still to exit", [(0, "A"), (-0.5, "C"), (-1, "B")], "A", "A", "C", 0),
    _col("inside A, B then C still to exit", [(0, "A"), (-0.5, "B"), (-1, "C")], "A", "A", "B", 0),
    _col("inside A, B and C exit at equal t", [(0, "A"), (-0.5, "B"), (-0.5, "C")], "A", "A", "C", 0),
    _col("exit A, enter B near", [(0, "A"), (-NEAR, "B"), (-0.5, "B")], "A", "A", "B", 1),
    _col("exit B, enter A near", [(0, "B"), (-NEAR, "A"), (-0.5, "A")], "B", "B", "A", 1),
    _col("exit A and B near, inside C", [(0, "A"), (-NEAR, "B"), (-0.5, "C")], "A", "A", "C", 1),
    _col("enter A and B near", [(0, "A"), (-NEAR, "B"), (-0.5, "B"), (-1, "A")], "A", None, "B", 1),
    _col("coplanar: A exits, B enters", [(0, "A"), (0, "B"), (-0.5, "B")], "A", "A", "B", 0),
    _col("coplanar: A enters, B exits", [(0, "A"), (0, "B"), (-0.5, "A")], "A", None, "A", 0),
    _col("coplanar: B exits, C enters, inside A", [(0, "B"), (0, "C"), (-0.5, "C"), (-1, "A")], "B", "B", "C", 0),
    _col("mirror, glass near behind", [(0, "MIR"), (-NEAR, "A"), (-0.5, "A")], "MIR", "MIR", "A", 1),
    _col("measure, glass near behind", [(0, "MEAS"), (-NEAR, "A"), (-0.5, "A")], "MEAS", "MEAS", "A", 1),
    _col("mirror inside dissipative glass", [(0, "B"), (-0.3, "MIR"), (-0.6, "MIR"), (-1, "B")], "B", None, "B", 0),
    _col("type-4 slab around glass", [(0, "T4"), (-0.3, "A"), (-0.6, "A"), (-1, "T4")], "T4", None, "T4", 0),
    _col("inside glass inside a type-4 slab", [(0, "A"), (-1, "T4")], "A", "A", "T4", 0),
    _col("type 4 near in front of glass", [(0, "T4"), (-NEAR, "A"), (-0.5, "A"), (-1, "T4")], "T4", None, "A", 1),
    _col("glass, type 4 near behind", [(0, "A"), (-NEAR, "T4"), (-0.5, "A"), (-1, "T4")], "A", None, "T4", 1),
)


def columns(meshes):
    """The columns whose layers name only `meshes`."""
    return tuple(c for c in COLUMNS if all(m in meshes for _, m in c.layers))


def scene(meshes=FULL, K=None):
    """-> a namespace: ``arrs`` (the arguments of Engine.upload_arrays), ``cols``
    (the columns, in x order), ``id`` (mesh name -> mesh id), ``K``.  ``K``: never-hit
    filler meshes (fate_util's) up to that mesh count."""
    cols = columns(meshes)
    ident = {m: j for j, m in enumerate(meshes)}
    per_mesh = {m: [] for m in meshes}
    for c, col in enumerate(cols):
        for z, m in col.layers:
            per_mesh[m] += fu._quad(c, c + 1, z)
        if "M" in ident:                # one measure mesh: ceiling and floor
            per_mesh["M"] += fu._quad(c, c + 1, 2) + fu._quad(c, c + 1, -6)
        else:
            per_mesh["CEIL"] += fu._quad(c, c + 1, 2)
            per_mesh["FLOOR"] += fu._quad(c, c + 1, -6)
    tris, ids, mats = [], [], []
    for m in meshes:                    # triangles sorted by mesh
        assert per_mesh[m], f"mesh {m} has no layer"
        tris += per_mesh[m]
        ids += [ident[m]] * len(per_mesh[m])
        mats.append(MATERIALS[m])
    base = len(meshes)
    K = base if K is None else int(K)
    assert K >= base
    for j in range(base, K):            # never hit: the beam and its children stay in x < len(cols), |z| <= 6
        x = 64 + 2 * j
        tris.append(((x, 64, 32), (x + 1, 64, 32), (x, 65, 32)))
        ids.append(j)
        mats.append(TERMINATOR)
    t = np.asarray(tris, np.float64)
    mt = np.asarray(mats, np.float64)
    arrs = (_rows(t[:, 0]), _rows(t[:, 1]), _rows(t[:, 2]), np.asarray(ids, np.int32), mt[:, 0].astype(np.int32),
            mt[:, 1].astype(np.float32), mt[:, 2].astype(np.float32), mt[:, 3].astype(np.float32))
    return types.SimpleNamespace(arrs=arrs, cols=cols, id=ident, K=K)


def rays(cols):
    """One ray per entry of `cols` (column numbers), from z = 1 straight down, each
    at its own grid point strictly inside the lower triangle of its column's quads;
    power i + 1."""
    cols = np.asarray(cols, np.int64)
    n = len(cols)
    pts = fu._points()[:n]
    o = np.zeros((n, 4), np.float32)
    o[:, 0] = cols + pts[:, 0] / fu.GRID
    o[:, 1] = pts[:, 1] / fu.GRID
    o[:, 2] = 1.0
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = -1.0
    return o, d, np.arange(1, n + 1, dtype=np.float32)


def cycle(sc, n):
    """n rays cycling through the scene's columns."""
    return np.arange(n) % len(sc.cols)


def declared(sc, cols):
    """-> dict(isect_mid, n1, n2, t): what every ray of rays(cols) must resolve to.
    t is the float32 parameter of the declared layer as Moller-Trumbore returns it
    for these quads and rays: o.z - z in float32 arithmetic, 1 - z."""
    cols = np.asarray(cols, np.int64)
    name = lambda m: -1 if m is None else sc.id[m]
    tab = np.array([[name(c.hit), name(c.n1), name(c.n2)] for c in sc.cols], np.int32)
    z = np.array([c.layers[c.t_layer][0] for c in sc.cols], np.float64)
    return dict(isect_mid=tab[cols, 0], n1=tab[cols, 1], n2=tab[cols, 2], z=z[cols])


def check_declared(sc, cols, out):
    """A bounce `out` (oracle.bounce layout) of rays(cols), emitted with prev -2,
    shows every column's declared situation; and each mesh's hit count under the
    ray is its number of layers in the column."""
    cols = np.asarray(cols, np.int64)
    want = declared(sc, cols)
    for k in ("isect_mid", "n1", "n2"):
        got = np.asarray(out[k]).reshape(-1)
        bad = np.flatnonzero(got != want[k])
        assert bad.size == 0, (f"{k}: column '{sc.cols[cols[bad[0]]].name}' gives {got[bad[0]]}, declared "
                               f"{want[k][bad[0]]}")
    # the destination lies on the declared layer: z of dest against the layer's z, to
    # within the rounding of 1 + |z| (2 ulp of 1), far below the 4e-6 between NEAR layers
    dz = np.asarray(out["dest"], np.float64)[:, 2]
    bad = np.flatnonzero(np.abs(dz - want["z"]) > 2.4e-7)
    assert bad.size == 0, (f"dest: column '{sc.cols[cols[bad[0]]].name}' ends at z = {dz[bad[0]]!r}, declared "
                           f"{want['z'][bad[0]]!r}")
    if "isects_count" in out:
        cnt = np.asarray(out["isects_count"])
        for c, col in enumerate(sc.cols):
            rows = cnt[cols == c]
            for m, j in sc.id.items():
                layers = sum(1 for _, mm in col.layers if mm == m)
                if m == "FLOOR" or m == "M":
                    layers += 1
                assert np.all(rows[:, j] == layers), (col.name, m, rows[:, j], layers)
