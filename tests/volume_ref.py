"""The volume map formed on the host -- TEST INFRASTRUCTURE.

``cutoff_ref.trace_rays`` run with a ``bounce_fn`` wrapper, as
``budget_ref.trace`` runs it, around ``oracle.bounce`` (the CPU oracle) or the
reference's own kernels (``tests/ref_gpu.py``).  From
each bounce the wrapper collects, per ray, the origin ``O``, ``dest``, ``n1``,
the power before (``p_in``) and after (``pow``), and forms for every ray that
took the dissipation branch the terms include/lpc.h fixes, in numpy float64:

    D = float64(p_in) - float64(p)         a = float64(diss[n1]) |E - O|
    W(s) = expm1(-a s) / expm1(-a)  (a > 0),   s  (a == 0)
    voxel v receives D (W(s_out) - W(s_in)) per interval of s inside v

by a method that shares nothing with the library's stepping: per ray every
plane-crossing parameter in (0,1) over the three axes is gathered with the clip
to the box, the parameters are sorted, and each interval's voxel is that of its
midpoint, looked up among the edges ``lo + k (hi - lo) / n``.

The terms are kept per voxel, so sums in any order compare against
``math.fsum``.  Tolerance (derived, not measured): a ray carries

    c_r = 2^-46 |D_r| max(1, a_r) kappa_r

with kappa_r the largest, over the axes on which the segment has a non-zero
extent, of (largest coordinate magnitude among lo, hi, O, E on that axis) /
|extent on that axis| (1 for a point).  A crossing parameter carries a few units
of 2^-53 kappa_r, dW/ds <= 1.6 max(1, a), and 2^-46 leaves a factor 64 for the
handful of operations on each side and the difference between expm1
implementations.  ``deposited[v]`` must lie within tol_v = sum of c_r over the
rays whose reference path touches v or one of its 26 neighbours; ``outside`` and
the total within the sum of c_r over all rays.  :func:`assert_condition` checks
that the summed tolerance is at most 2^-20 sum|D_r|: a misplaced or missed
segment moves its whole share, so the tolerance cannot hide one.
"""
from __future__ import annotations

import math

import numpy as np

import budget_ref
import cutoff_ref

EPS_TOL = 2.0 ** -46
CONDITION = 2.0 ** -20


def grid_of(lo, hi, shape):
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    shape = tuple(int(v) for v in shape)
    edges = [lo[k] + np.arange(n + 1, dtype=np.float64) * (hi[k] - lo[k]) / n for k, n in enumerate(shape)]
    return dict(lo=lo, hi=hi, shape=shape, edges=edges, V=int(np.prod(shape)))


def W_of(a, s):
    s = np.asarray(s, np.float64)
    if a > 0.0:
        w = np.expm1(-a * s) / np.expm1(-a)
        return np.where(s <= 0.0, 0.0, np.where(s >= 1.0, 1.0, w))
    return s.copy()


def kappa_of(grid, O, E):
    d = E - O
    k = [max(abs(grid["lo"][j]), abs(grid["hi"][j]), abs(O[j]), abs(E[j])) / abs(d[j]) for j in range(3) if d[j] != 0.0]
    return max(k) if k else 1.0


def segment(grid, O, E, a, D):
    """One ray's terms -> (voxels int64, -1: outside; shares float64), intervals
    in the order of s, none of zero length."""
    O, E = np.asarray(O, np.float64), np.asarray(E, np.float64)
    lo, hi, shape = grid["lo"], grid["hi"], grid["shape"]
    if not (np.all(np.isfinite(O)) and np.all(np.isfinite(E)) and np.isfinite(a)):
        return np.array([-1], np.int64), np.array([D], np.float64)
    d = E - O

    def voxel(X):
        X = np.atleast_2d(X)
        inside = np.all((X >= lo) & (X <= hi), axis=1)
        ijk = [np.clip(np.searchsorted(grid["edges"][k], X[:, k], "right") - 1, 0, shape[k] - 1) for k in range(3)]
        v = (ijk[0] * shape[1] + ijk[1]) * shape[2] + ijk[2]
        return np.where(inside, v, -1).astype(np.int64)

    if not d.any():
        return voxel(O), np.array([D], np.float64)
    ts = [np.array([0.0, 1.0])]
    for k in range(3):
        if d[k] != 0.0:
            t = (np.concatenate((grid["edges"][k], [lo[k], hi[k]])) - O[k]) / d[k]
            ts.append(t[(t > 0.0) & (t < 1.0)])
    ts = np.unique(np.concatenate(ts))
    mid = 0.5 * (ts[:-1] + ts[1:])
    v = voxel(O[None, :] + mid[:, None] * d[None, :])
    w = W_of(a, ts)
    return v, D * np.diff(w)


def neighbourhood(shape, vox):
    """The voxels of `vox` (linear, >= 0) with their 26 neighbours, unique."""
    vox = np.unique(vox[vox >= 0])
    if not len(vox):
        return vox
    iz = vox % shape[2]
    iy = (vox // shape[2]) % shape[1]
    ix = vox // (shape[1] * shape[2])
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                x, y, z = ix + dx, iy + dy, iz + dz
                ok = (x >= 0) & (x < shape[0]) & (y >= 0) & (y < shape[1]) & (z >= 0) & (z < shape[2])
                out.append(((x * shape[1] + y) * shape[2] + z)[ok])
    return np.unique(np.concatenate(out))


class Ref:
    """The reference of one trace on one grid: per-voxel term lists, the
    tolerances, the counts."""

    def __init__(self, grid):
        self.grid = grid
        self.terms = {}                 # voxel (-1: outside) -> [shares]
        self.tol = np.zeros(grid["V"], np.float64)
        self.c = []                     # c_r per booked ray
        self.D = []                     # D_r per booked ray
        self.segments = 0
        self.per_iter = []              # booked rays per iteration
        self.rays = []                  # (O, E, a, D) per booked ray

    def book(self, O, E, a, D):
        g = self.grid
        v, sh = segment(g, O, E, a, D)
        for vi, s in zip(v.tolist(), sh.tolist()):
            self.terms.setdefault(vi, []).append(s)
        fin = np.all(np.isfinite(O)) and np.all(np.isfinite(E)) and np.isfinite(a)
        c = EPS_TOL * abs(D) * max(1.0, a if fin else 1.0) * (kappa_of(g, O, E) if fin else 1.0)
        self.tol[neighbourhood(g["shape"], v)] += c
        self.c.append(c)
        self.D.append(D)
        self.rays.append((np.array(O, np.float64), np.array(E, np.float64), float(a), float(D)))
        self.segments += 1

    def deposited(self):
        out = np.zeros(self.grid["V"], np.float64)
        for v, t in self.terms.items():
            if v >= 0:
                out[v] = math.fsum(t)
        return out.reshape(self.grid["shape"])

    def outside(self):
        return math.fsum(self.terms.get(-1, []))

    def total(self):
        return math.fsum(s for t in self.terms.values() for s in t)

    def tol_all(self):
        return math.fsum(self.c)


def bounce_rays(scene, o, p_in, out):
    """One iteration's booked rays -> (O (m,3), E (m,3), a (m,), D (m,)) float64."""
    f64 = np.float64
    p_in = np.asarray(p_in, np.float32).reshape(-1)
    p = np.asarray(out["pow"], np.float32).reshape(-1)
    n1 = np.asarray(out["n1"], np.int32).reshape(-1)
    O = np.asarray(o, np.float32).reshape(len(p), -1)[:, :3].astype(f64)
    E = np.asarray(out["dest"], np.float32).reshape(len(p), -1)[:, :3].astype(f64)
    K = scene.mesh_count
    n1c = np.clip(n1, 0, K - 1)
    dis = (n1 >= 0) & (scene.mat_type[n1c] == 0) & (scene.diss[n1c] > np.float32(0.000001))
    with np.errstate(invalid="ignore", over="ignore"):
        D = (p_in.astype(f64) - p.astype(f64))[dis]
        length = np.sqrt(np.sum((E[dis] - O[dis]) ** 2, axis=1))
        a = scene.diss[n1c].astype(f64)[dis] * length
    return O[dis], E[dis], a, D


def trace(oracle_mod, meshes, origin, dirs, power, iterations, tau, max_ray_len, ior_env, grids, cut=0.0,
          keep_results=False, bounce_fn=None):
    """-> dict(refs: one Ref per grid of `grids` (dicts of grid_of), budget:
    budget_ref's reference of the same bounces, counts).  bounce_fn: the
    reference's own kernels (tests/ref_gpu.py) in place of ``oracle.bounce``."""
    inner = oracle_mod.bounce if bounce_fn is None else bounce_fn
    refs = [Ref(g) for g in grids]
    bud = []

    def wrapped(scene, o, d, pw, ms, mid, mrl, ior):
        p_in = np.array(pw, dtype=np.float32).reshape(-1)
        o_in = np.array(o, dtype=np.float32)
        out = inner(scene, o, d, pw, ms, mid, mrl, ior)
        O, E, a, D = bounce_rays(scene, o_in, p_in, out)
        for r in refs:
            for j in range(len(D)):
                r.book(O[j], E[j], float(a[j]), float(D[j]))
            r.per_iter.append(len(D))
        bud.append(budget_ref.bounce_terms(scene, p_in, out))
        return out

    res, info = cutoff_ref.trace_rays(oracle_mod, origin, dirs, power, meshes, iterations, tau, max_ray_len, ior_env,
                                      cut=cut, keep_results=keep_results, bounce_fn=wrapped)
    budget = dict(iters=bud, culled=info["culled"], counts=list(info["counts"]),
                  mesh_power=np.asarray(info["mesh_power"]), K=len(meshes), results=res)
    return dict(refs=refs, budget=budget, counts=list(info["counts"]))


def assert_condition(ref, what=""):
    """The summed tolerance cannot hide a segment (asserted on the reference side
    of every case)."""
    mag = math.fsum(abs(d) for d in ref.D)
    assert ref.tol_all() <= CONDITION * mag, (what, ref.tol_all(), CONDITION * mag)


def assert_volume(got, ref, what=""):
    """A library map (``Engine.volume()``'s dict or ``volume_dict``'s) against the
    reference: segments exact, every voxel within tol_v, outside and the total
    within the sum of c_r."""
    assert_condition(ref, what)
    dep = np.asarray(got["deposited"], np.float64)
    assert dep.shape == tuple(ref.grid["shape"]), (what, dep.shape, ref.grid["shape"])
    assert int(got["segments"]) == ref.segments, (what, "segments", int(got["segments"]), ref.segments)
    want = ref.deposited()
    err = np.abs(dep - want).ravel()
    print(what, "voxels", dep.size, "segments", ref.segments, "max |err|", float(err.max(initial=0.0)),
          "max err/tol", float(np.max(err[ref.tol > 0] / ref.tol[ref.tol > 0], initial=0.0)),
          "outside err", abs(float(got["outside"]) - ref.outside()), "tol", ref.tol_all())
    bad = np.flatnonzero(~(err <= ref.tol))
    assert len(bad) == 0, (what, bad[:8], dep.ravel()[bad[:8]], want.ravel()[bad[:8]], ref.tol[bad[:8]])
    tol = ref.tol_all()
    assert abs(float(got["outside"]) - ref.outside()) <= tol, (what, "outside", got["outside"], ref.outside(), tol)
    total = math.fsum(dep.ravel().tolist() + [float(got["outside"])])
    assert abs(total - ref.total()) <= tol, (what, "total", total, ref.total(), tol)


# -- the constructed slab ------------------------------------------------------------
SLAB_LO, SLAB_HI = (-5.0, -5.0, 15.0), (5.0, 5.0, 25.0)


def slab_scene(dissipation=0.3):
    """One dissipative cube [-5,5]^2 x [15,25] whose IOR is the environment's:
    a +z ray enters undeviated at z = 15 with its whole power (first iteration)
    and dissipates along its own column to z = 25 (second iteration)."""
    from lightpycl_amd import geo_optical_elements as goe
    m = goe.optical_elements().cube(center=(0, 0, 20, 0), size=[10, 10, 10, 0])
    m.setMaterial(mat_type="refractive", IOR=1.0, dissipation=dissipation)
    return [m]


def slab_rays(columns, shape, lo=SLAB_LO, hi=SLAB_HI, power=None):
    """Collimated +z rays from z = 0, ray j through the centre of column
    columns[j] = (ix, iy) of the grid `shape` over lo .. hi (x, y)."""
    columns = np.asarray(columns, np.int64).reshape(-1, 2)
    n = len(columns)
    o = np.zeros((n, 4), np.float32)
    for k in range(2):
        o[:, k] = lo[k] + (columns[:, k] + 0.5) * (hi[k] - lo[k]) / shape[k]
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = 1.0
    p = (1.0 + (np.arange(n) % 7) / 8.0).astype(np.float32) if power is None else np.asarray(power, np.float32)
    return o, d, p


def slab_patterns(n, shape, table):
    """Column choices of n rays on the grid `shape` -> {name: (n, 2) columns}.
    ``one``: every ray in one column; ``each``: one ray per column, round
    robin; ``collide``: columns whose voxels collide modulo `table` (the
    k_volume_sum block table), when the grid has such columns."""
    nx, ny, nz = shape
    cols = np.array([(i, j) for i in range(nx) for j in range(ny)], np.int64)
    out = {"one": np.tile(cols[len(cols) // 2], (n, 1)), "each": cols[np.arange(n) % len(cols)]}
    first = (cols[:, 0] * ny + cols[:, 1]) * nz            # a column's first voxel
    same = cols[first % table == first[len(cols) // 3] % table]
    if len(same) > 1:
        out["collide"] = same[np.arange(n) % len(same)]
    return out


def slab_closed_form(D, a, nz, z0=15.0, z1=25.0, lo=SLAB_LO[2], hi=SLAB_HI[2]):
    """A column's shares D (W((k+1)/nz) - W(k/nz)) for a segment z0 .. z1 on a
    grid whose z range lo .. hi contains it or cuts it: -> (nz shares, outside)."""
    edges = lo + np.arange(nz + 1, dtype=np.float64) * (hi - lo) / nz
    s = np.clip((edges - z0) / (z1 - z0), 0.0, 1.0)
    w = W_of(a, s)
    shares = D * np.diff(w)
    return shares, D * (w[0] + (1.0 - w[-1]))
