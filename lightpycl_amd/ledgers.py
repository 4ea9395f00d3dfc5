"""The ledgers a trace keeps on the device (``Engine.set_min_power``,
``set_budget``, ``set_surface``, ``set_volume``) as the Python layers return
them: :func:`read_ledgers` at a trace's end, :func:`budget_dict`,
:func:`surface_dict`, :func:`volume_dict`."""
from __future__ import annotations

import math

import numpy as np

from . import _lib


def triangle_areas(mesh):
    """Areas of a mesh's triangles in its own triangle order, ``0.5 |E1 x E2|``
    in float64 from the mesh's vertices as they are held on the host (not the
    float32 rows of the upload)."""
    V, T = getattr(mesh, "vertices", None), getattr(mesh, "triangles", None)
    try:
        V = np.asarray(V, np.float64)
        T = np.asarray(T)
        ok = V.ndim == 2 and V.shape[1] >= 3 and T.ndim == 2 and T.shape[1] == 3 and T.dtype.kind in "iu"
    except Exception:
        ok = False
    if ok:
        a, b, c = (V[T[:, k], :3] for k in range(3))
    else:                                       # general vertex containers: the reference's tribuf() lists
        tb = mesh.tribuf()
        a, b, c = (np.asarray(tb[k], np.float64).reshape(-1, 4)[:, :3] for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def surface_dict(s, meshes):
    """The surface map as the tracer returns it, from ``Engine.surface()`` (or
    the ranks' sum of it) and the traced meshes.

    ``meshes``: per mesh, in the order of the trace's ``meshes``, a dict of
    arrays in that mesh's own triangle order: ``incident`` (float64: the power of
    every ray whose nearest hit is the triangle), ``deposited`` (float64: what
    stayed there -- the whole ray on a terminator or measure mesh, else the ray
    less its kept children: ``(1 - R) p`` on a mirror, the Fresnel split's
    float32 residue on a refractive surface), ``count`` (int64 hits), ``area``
    (:func:`triangle_areas`), ``irradiance`` = deposited / area and
    ``incident_irradiance`` = incident / area (a zero-area sliver gives inf or
    nan: it is not hidden), and ``offset``, the mesh's first triangle in the flat
    arrays.  ``incident``, ``deposited``, ``count``: the flat arrays over all
    triangles, the order of the scene upload (the reference's ``isect_idx``).
    Per mesh, ``deposited`` sums to the power budget's absorbed + terminated +
    measured of that mesh."""
    inc, dep = np.asarray(s["incident"], np.float64), np.asarray(s["deposited"], np.float64)
    cnt = np.asarray(s["count"], np.int64)
    out = {"incident": inc, "deposited": dep, "count": cnt, "meshes": [], "offsets": []}
    lo = 0
    for m in meshes:
        area = triangle_areas(m)
        hi = lo + len(area)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["meshes"].append({"offset": lo, "incident": inc[lo:hi], "deposited": dep[lo:hi], "count": cnt[lo:hi],
                                  "area": area, "irradiance": dep[lo:hi] / area,
                                  "incident_irradiance": inc[lo:hi] / area})
        out["offsets"].append(lo)
        lo = hi
    if lo != len(cnt):
        raise ValueError(f"surface map: the meshes hold {lo} triangles, the scene {len(cnt)}")
    return out


def volume_dict(v):
    """The volume map as the tracer returns it, from ``Engine.volume()`` (or the
    ranks' sum of it): where the power budget's ``dissipated`` landed.

    ``deposited``: float64 (nx, ny, nz), the power dissipated in every voxel;
    ``density`` = deposited / voxel volume; ``edges``: three float64 arrays of nx
    + 1, ny + 1, nz + 1 voxel edges, ``lo + k (hi - lo) / n``; ``outside``: the
    dissipated power that fell outside the grid's box; ``segments``: the rays
    booked (int, the budget's summed ``n_dissipated``); ``total`` = sum(deposited)
    + outside, the budget's ``dissipated`` summed over meshes and iterations."""
    dep = np.asarray(v["deposited"], np.float64)
    lo, hi = np.asarray(v["lo"], np.float64), np.asarray(v["hi"], np.float64)
    edges = [lo[k] + np.arange(n + 1, dtype=np.float64) * (hi[k] - lo[k]) / n for k, n in enumerate(dep.shape)]
    cell = float(np.prod((hi - lo) / np.asarray(dep.shape, np.float64))) if dep.size else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        density = dep / cell
    outside = float(v["outside"])
    return {"deposited": dep, "density": density, "edges": edges, "outside": outside,
            "segments": int(v["segments"]), "total": math.fsum(dep.ravel().tolist() + [outside])}


def budget_dict(b, culled_counts=(), culled_power=()):
    """The power budget as the tracer returns it, from ``Engine.budget()`` and the
    culled-power ledger of the same trace (empty: no cutoff).

    Per iteration (arrays over the trace's iterations): ``power_in`` and the six
    float64 sums ``dissipated`` (Beer-Lambert loss inside a medium), ``escaped``
    (no hit within max_ray_len), ``terminated`` (terminator surfaces),
    ``measured`` (measure surfaces), ``absorbed`` (what every other hit did not
    hand to its children: (1 - R) p on a mirror, the whole ray on a type-4 or
    unknown surface and on the NaN-TIR path, the float32 residue of the Fresnel
    split on a refractive surface) and ``kept`` (the children's power before
    any cutoff), with the exact counts ``n_in``, ``n_dissipated``, ``n_escaped``,
    ``n_terminated``, ``n_measured``, ``n_absorbed``; ``culled`` and ``n_culled``
    from the cutoff's ledger (zeros without one).

    ``mesh``: ``{category: float64[K]}`` and ``mesh_count``: ``{category:
    int64[K]}`` for dissipated (the medium's mesh), absorbed, terminated and
    measured (the hit mesh), summed over the trace.

    ``left``: the last iteration's kept power minus its culled power, the power
    of the population the stop rule left untraced.  ``closure``: the residue of
    the whole-trace identity, ``power_in[0]`` minus every iteration's
    dissipated, escaped, terminated, measured, absorbed and culled power minus
    ``left``: float64 rounding of the sums when the ledger is whole."""
    n = len(b["n_in"])
    out = {k: np.asarray(b[k]) for k in _lib.BUDGET_SUMS + _lib.BUDGET_COUNTS}
    cp = np.zeros(n, np.float64)
    cc = np.zeros(n, np.int64)
    m = min(n, len(culled_power))
    cp[:m] = np.asarray(culled_power, np.float64)[:m]
    cc[:m] = np.asarray(culled_counts, np.int64)[:m]
    out["culled"], out["n_culled"] = cp, cc
    out["mesh"] = {k: np.asarray(b["mesh_power"])[:, j].copy() for j, k in enumerate(_lib.BUDGET_MESH)}
    out["mesh_count"] = {k: np.asarray(b["mesh_count"])[:, j].copy() for j, k in enumerate(_lib.BUDGET_MESH)}
    left = float(out["kept"][-1] - cp[-1]) if n else 0.0
    spent = [float(v) for k in ("dissipated", "escaped", "terminated", "measured", "absorbed", "culled")
             for v in out[k]]
    out["left"] = left
    out["closure"] = math.fsum([float(out["power_in"][0])] + [-v for v in spent] + [-left]) if n else 0.0
    return out


def read_ledgers(engine, reduce=None, iterations=None, piece=1 << 20):
    """The ledgers of the trace ``engine`` has just run -> a dict of those that
    are on (a reader waits for the stream): ``culled_counts`` / ``culled_power``
    per iteration with a cutoff set, ``power_budget`` (:func:`budget_dict`,
    joined with the culled ledger), ``surface`` (the dict of ``Engine.surface()``),
    ``volume`` (the dict of ``Engine.volume()``).

    ``reduce``: a callable that sums a float64 vector over the ranks of a sharded
    trace, every rank calling alike: one exchange for the culled ledger; one for
    the budget, ``iterations`` rows of 13 and the (K, 4) tables; the map's three
    tables, and the volume map's voxels with ``outside`` and ``segments`` behind
    them, in pieces of at most ``piece`` values (a comm's payload is an int32
    count of float64) -- sizes that no rank's data changes.  Counts are exact in
    float64 and come back as int64."""
    out = {}
    if getattr(engine, "min_power", 0.0) > 0.0:
        cc, cp = engine.culled()
        if reduce is not None:
            k = len(cc)
            tot = reduce(np.concatenate((np.asarray(cc, np.float64), np.asarray(cp, np.float64))))
            cc, cp = tot[:k], tot[k:2 * k]
        out["culled_counts"] = [int(v) for v in cc]
        out["culled_power"] = [float(v) for v in cp]
    if getattr(engine, "budget_on", False):
        b = engine.budget()
        if reduce is not None:
            names = _lib.BUDGET_SUMS + _lib.BUDGET_COUNTS
            rows = np.zeros((len(names), int(iterations)), np.float64)
            for j, name in enumerate(names):
                v = np.asarray(b[name], np.float64)[:rows.shape[1]]
                rows[j, :len(v)] = v
            kk = b["mesh_power"].size
            tot = reduce(np.concatenate((rows.ravel(), b["mesh_power"].ravel(),
                                         b["mesh_count"].astype(np.float64).ravel())))
            rows = tot[:rows.size].reshape(rows.shape)
            b = {name: (rows[j] if name in _lib.BUDGET_SUMS else np.rint(rows[j]).astype(np.int64))
                 for j, name in enumerate(names)}
            b["mesh_power"] = tot[rows.size:rows.size + kk].reshape(-1, 4)
            b["mesh_count"] = np.rint(tot[rows.size + kk:]).astype(np.int64).reshape(-1, 4)
        out["power_budget"] = budget_dict(b, out.get("culled_counts", ()), out.get("culled_power", ()))
    if getattr(engine, "surface_on", False):
        s = engine.surface()
        if reduce is not None:
            m = len(s["count"])
            flat = np.concatenate([np.asarray(s[k], np.float64) for k in _lib.SURFACE_COLUMNS])
            tot = np.empty_like(flat)
            for lo in range(0, len(flat), piece):
                tot[lo:lo + piece] = reduce(flat[lo:lo + piece])
            s = {"incident": tot[:m].copy(), "deposited": tot[m:2 * m].copy(),
                 "count": np.rint(tot[2 * m:]).astype(np.int64)}
        out["surface"] = s
    if getattr(engine, "volume_on", False):
        v = engine.volume()
        if reduce is not None:
            flat = np.concatenate((v["deposited"].ravel(), [v["outside"], float(v["segments"])]))
            tot = np.empty_like(flat)
            for lo in range(0, len(flat), piece):
                tot[lo:lo + piece] = reduce(flat[lo:lo + piece])
            v = dict(v, deposited=tot[:-2].reshape(v["shape"]).copy(), outside=float(tot[-2]),
                     segments=int(np.rint(tot[-1])))
        out["volume"] = v
    return out
