"""Constructed rows for reflect_refract_rays -- TEST INFRASTRUCTURE, shared by
tests/test_shade_rows_host.py (shade() of lpc_math.hpp on the host) and
tests/test_gpu_shade_tables.py (the drop-in kernel on the device).

One scene carries every material the shading tells apart:

  0  glass IOR 1.5            4  mirror R 0.9        8   type 4
  1  glass IOR 1.3, diss .05  5  mirror R 1.0        9   glass IOR 1.4, dissipation 1e-6 exactly
  2  glass IOR -2.0           6  terminator          10  glass IOR 1.6, dissipation the float after 1e-6
  3  glass IOR 1.0            7  measure

(the kernel dissipates when `diss > 1e-6f`: mesh 9 does not, mesh 10 does).  Every
mesh has four triangles: a unit right triangle in the plane z = 0 (its normal is
exactly (0, 0, 1): cross = (0, 0, 1), rsqrt(1) = 1) and a tilted one, each in both
windings.  Meshes 0 and 4 also have a triangle with edges of 1e-13 (the squared
normal underflows: normalize rescales up) and, unless left out, one with edges
of 5e9 (it overflows: normalize rescales down).

A row is the input of one ray: the triangle it is said to have hit, n1, n2,
meas_in, direction, power, origin and destination -- postproc's outputs, set
freely here, geometry or not.  Groups:

  sweep     every (triangle, n1, n2), n1 and n2 in {-1, each glass}, meas_in 0, in
            64 directions from normal to grazing.  The steps are uniform in the
            cosine of incidence, 1 - k/63: none of them falls within rounding of a
            critical angle of the table's index pairs (uniform steps in the angle
            would put 30 degrees exactly on |n2/n1| = 1/2, uniform steps in the sine
            2/3 on 1/1.5), so the sweep's decisions do not hang on the last bit of a
            normal; the critical group does that on purpose, on the exact normal.
  meas      the same with meas_in -1 and 1, four directions.
  nohit     isect_mid = -1 with every meas_in.
  critical  on the z = 0 triangle of mesh 0, for each (n1, n2) with |n1| > |n2|: the
            33 directions (s, 0, -sqrt(1 - s^2)) whose sine s steps ulp by ulp
            through |n2 / n1|.
  length    a dissipative n1 (meshes 1 and 10, and 9 which must not dissipate) with
            dest - origin of length 1e-25, 1 and 1e25 along an axis and a diagonal.
  odd       directions with an infinite or NaN component, and the zero direction:
            the NaN-TIR path (neither comparison true).

Powers cycle through 1, 0, -8, 1e-38 and inf by row.
"""
from __future__ import annotations

import types

import numpy as np

IOR_ENV = np.float32(1.0)
MAX_RAY_LEN = np.float32(1000.0)
_D6 = np.float32(0.000001)
# (type, IOR, R, dissipation)
MATERIALS = ((0, 1.5, 0.0, 0.0), (0, 1.3, 0.0, 0.05), (0, -2.0, 0.0, 0.0), (0, 1.0, 0.0, 0.0), (1, 1.0, 0.9, 0.0),
             (1, 1.0, 1.0, 0.0), (2, 1.0, 0.0, 0.0), (3, 1.0, 0.0, 0.0), (4, 1.0, 0.0, 0.0),
             (0, 1.4, 0.0, float(_D6)), (0, 1.6, 0.0, float(np.nextafter(_D6, np.float32(1.0)))))
GLASS = (0, 1, 2, 3, 9, 10)
MEDIA = (-1,) + GLASS
POWERS = np.array([1.0, 0.0, -8.0, 1e-38, np.inf], np.float32)
NDIR = 64
NCRIT = 33

_FLAT = ((0, 0, 0), (1, 0, 0), (0, 1, 0))
_TILT = ((0.3, -0.2, 0.1), (1.1, 0.4, 0.7), (-0.2, 0.9, 0.5))
_TINY = ((0, 0, 0), (1e-13, 0, 0), (0, 1e-13, 1e-13))
_HUGE = ((0, 0, 0), (5e9, 0, 0), (0, 5e9, 5e9))


def _flip(t):
    return (t[0], t[2], t[1])


def scene(with_huge=True):
    """-> namespace: arrs (Engine.upload_arrays' arguments), and per triangle its
    mesh, its kind (flat+, flat-, tilt+, tilt-, tiny, huge) and its float64 unit
    normal by winding."""
    tris, ids, kinds = [], [], []
    for m in range(len(MATERIALS)):
        mine = [("flat+", _FLAT), ("flat-", _flip(_FLAT)), ("tilt+", _TILT), ("tilt-", _flip(_TILT))]
        if m in (0, 4):
            mine.append(("tiny", _TINY))
        if m == 0 and with_huge:
            mine.append(("huge", _HUGE))
        for kind, t in mine:
            tris.append(t)
            ids.append(m)
            kinds.append(kind)
    t = np.asarray(tris, np.float64)
    mt = np.asarray(MATERIALS, np.float64)
    rows4 = lambda x: np.concatenate([x.astype(np.float32), np.zeros((len(x), 1), np.float32)], axis=1)
    diss = np.array([m[3] for m in MATERIALS], np.float32)
    assert diss[9] == _D6 and diss[10] > _D6 and diss[10] == np.nextafter(_D6, np.float32(1.0))
    arrs = (rows4(t[:, 0]), rows4(t[:, 1]), rows4(t[:, 2]), np.asarray(ids, np.int32), mt[:, 0].astype(np.int32),
            mt[:, 1].astype(np.float32), mt[:, 2].astype(np.float32), diss)
    f = np.float64(np.float32(t))                    # the normal of the float32 vertices, as the kernel forms it
    nrm = np.cross(f[:, 1] - f[:, 0], f[:, 2] - f[:, 1])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return types.SimpleNamespace(arrs=arrs, mesh=np.asarray(ids, np.int32), kind=kinds, normal=nrm, with_huge=with_huge)


def _tangent(n):
    a = np.where(np.abs(n[:, [0]]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    u = np.cross(n, a)
    return u / np.linalg.norm(u, axis=1)[:, None]


def _ior(sc, m):
    return np.where(np.asarray(m) < 0, IOR_ENV, sc.arrs[5][np.maximum(m, 0)])


def rows(sc):
    """-> namespace of per-row arrays: origin, dest, dir (n, 4), pow, meas, n1, n2,
    imid, iidx, and `group` (name per row), `pair` (critical group: index of its
    (n1, n2) pair, else -1)."""
    T = len(sc.mesh)
    tri, n1, n2, dirs, meas, group, pair, org, dst = [], [], [], [], [], [], [], [], []
    dest0 = np.array([0.25, 0.25, 0.0])

    def add(name, ti, a, b, d, ms, o=None, e=None, pr=-1):
        k = len(ti)
        tri.append(np.asarray(ti, np.int64)); n1.append(np.broadcast_to(a, k)); n2.append(np.broadcast_to(b, k))
        dirs.append(np.asarray(d, np.float64).reshape(k, 3)); meas.append(np.broadcast_to(ms, k))
        group.extend([name] * k)
        pair.append(np.broadcast_to(pr, k))
        dst.append(np.broadcast_to(dest0 if e is None else e, (k, 3)))
        org.append(np.broadcast_to(dest0 + np.array([0.0, 0.0, 1.0]) if o is None else o, (k, 3)))

    nrm, tan = sc.normal, _tangent(sc.normal)
    cos = 1.0 - np.arange(NDIR) / (NDIR - 1.0)
    sin = np.sqrt(1.0 - cos * cos)
    # (triangle, direction): incidence against the winding normal of the "+" triangles;
    # the other winding of the same triangle meets the same directions from behind (the
    # back-face flip), the tiny and the huge triangle every second direction
    sgn = np.ones((T, NDIR))
    for i, k in enumerate(sc.kind):
        if k.endswith("-"):
            sgn[i] = -1.0
        elif k in ("tiny", "huge"):
            sgn[i, 1::2] = -1.0
    d_all = -(sgn * cos[None, :])[:, :, None] * nrm[:, None, :] + sin[None, :, None] * tan[:, None, :]
    ti_all = np.repeat(np.arange(T), NDIR)
    for a in MEDIA:
        for b in MEDIA:
            add("sweep", ti_all, a, b, d_all.reshape(-1, 3), 0)
            sub = [0, 21, 42, 63]
            for ms in (-1, 1):
                add("meas", np.repeat(np.arange(T), len(sub)), a, b, d_all[:, sub].reshape(-1, 3), ms)
    for ms in (-1, 0, 1):               # no hit: isect_mid -1 (tri -1)
        add("nohit", np.full(4, -1), -1, 0, d_all[0, [0, 21, 42, 63]], ms)
        add("nohit", np.full(4, -1), 1, -1, d_all[0, [0, 21, 42, 63]], ms)
    flat = next(i for i in range(T) if sc.mesh[i] == 0 and sc.kind[i] == "flat+")
    npair = 0
    for a in MEDIA:
        for b in MEDIA:
            ia, ib = abs(float(_ior(sc, a))), abs(float(_ior(sc, b)))
            if not ia > ib:
                continue
            s = np.float32(ib / ia)
            for _ in range(NCRIT // 2):
                s = np.nextafter(s, np.float32(0.0))
            ss = []
            for _ in range(NCRIT):
                ss.append(s)
                s = np.nextafter(s, np.float32(2.0))
            ss = np.asarray(ss, np.float64)
            d = np.stack([ss, np.zeros(NCRIT), -np.sqrt(1.0 - ss * ss)], axis=1)
            add("critical", np.full(NCRIT, flat), a, b, d, 0, pr=npair)
            npair += 1
    for a in (1, 9, 10):
        for L in (1e-25, 1.0, 1e25):
            for u in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8), (1 / 3 ** 0.5,) * 3):
                e = dest0 if L == 1.0 else np.zeros(3)
                o = e - L * np.asarray(u)
                for tix in (flat, flat + 2):
                    add("length", [tix, tix], a, 0, d_all[tix, [5, 40]], 0, o=o, e=e)
    odd = [(np.inf, 0, -1), (np.nan, 0, -1), (0, 0, 0), (0, 0, -np.inf), (1e30, 0, -1e30)]
    mirror = next(i for i in range(T) if sc.mesh[i] == 4 and sc.kind[i] == "tilt+")
    for tix in (flat, flat + 2, mirror):
        for a, b in ((-1, 0), (0, -1), (2, 1)):
            add("odd", np.full(len(odd), tix), a, b, np.asarray(odd, np.float64), 0)

    tri = np.concatenate(tri)
    n = len(tri)
    C = np.ascontiguousarray

    def v4(x):
        out = np.zeros((n, 4), np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            out[:, :3] = np.concatenate(x).astype(np.float32)
        return out
    imid = np.where(tri >= 0, sc.mesh[np.maximum(tri, 0)], -1).astype(np.int32)
    grp = np.asarray(group)
    pw = POWERS[np.arange(n) % len(POWERS)].copy()
    pw[grp == "critical"] = np.float32(1.0)
    return types.SimpleNamespace(n=n, origin=v4(org), dest=v4(dst), dir=v4(dirs), pow=pw,
                                 meas=C(np.concatenate(meas), np.int32), n1=C(np.concatenate(n1), np.int32),
                                 n2=C(np.concatenate(n2), np.int32), imid=C(imid), iidx=C(np.where(tri >= 0, tri, 0), np.int32),
                                 tri=tri, group=grp, pair=np.concatenate(pair), npair=npair)


OUT = ("pow", "meas", "r_dir", "r_pow", "r_meas", "t_dir", "t_pow", "t_meas")


def oracle_shade(oracle_mod, sc, R):
    """orc_reflect_refract_rays on the rows -> dict of OUT."""
    L = oracle_mod.lib()
    n = R.n
    v0, v1, v2, _, mat, ior, refl, diss = sc.arrs
    pw, ms = R.pow.copy(), R.meas.copy()
    F4 = lambda: np.zeros((n, 4), np.float32)
    ro, rd, to, td = F4(), F4(), F4(), F4()
    rp, tp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rm, tm = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.orc_reflect_refract_rays(n, R.origin, R.dest, R.dir, pw, ms, R.n1, R.n2, ro, rd, rp, rm, to, td, tp, tm, R.imid,
                               R.iidx, v0, v1, v2, mat, ior, refl, diss, IOR_ENV)
    return dict(pow=pw, meas=ms, r_dir=rd, r_pow=rp, r_meas=rm, t_dir=td, t_pow=tp, t_meas=tm)


def host_shade(lib, sc, R):
    """shade() of lpc_math.hpp, host build (postproc_tables.harness().lib) -> dict of OUT."""
    n = R.n
    v0, v1, v2, _, mat, ior, refl, diss = sc.arrs
    pw, ms = R.pow.copy(), R.meas.copy()
    rd, td = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    rp, tp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rm, tm = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.shade_rows(n, R.origin, R.dest, R.dir, pw, ms, R.n1, R.n2, R.imid, R.iidx, v0, v1, v2, mat, ior, refl, diss,
                   IOR_ENV, rd, rp, rm, td, tp, tm)
    return dict(pow=pw, meas=ms, r_dir=rd, r_pow=rp, r_meas=rm, t_dir=td, t_pow=tp, t_meas=tm)


def fresnel_rows(sc, R):
    """The rows that reach reflect_refract: meas_in 0 on a glass or mirror triangle."""
    mat = sc.arrs[4]
    return (R.meas == 0) & (R.imid >= 0) & np.isin(mat[np.maximum(R.imid, 0)], (0, 1))


def nan_rows(sc, R, judge):
    """The NaN-TIR rows as a judge's output shows them: reflect_refract was reached
    and neither branch marked the reflected child as kept."""
    return fresnel_rows(sc, R) & (judge["r_meas"] == -1)


def check_coverage(sc, R, judge):
    """From a judge's output alone: the rows reach every special case."""
    mat = sc.arrs[4]
    fr = fresnel_rows(sc, R)
    nan = nan_rows(sc, R, judge)
    hitmat = np.where(R.imid >= 0, mat[np.maximum(R.imid, 0)], -1)
    glass = fr & (hitmat == 0) & ~nan
    refracted = glass & (judge["t_meas"] == 0)
    tir = glass & (judge["t_meas"] == -1) & (judge["r_meas"] == 0)
    # the critical group: both sides of total reflection for every pair
    for p in range(R.npair):
        g = (R.group == "critical") & (R.pair == p)
        assert g.sum() == NCRIT
        assert (g & refracted).any() and (g & tir).any(), (p, int((g & refracted).sum()), int((g & tir).sum()))
    assert R.npair >= 15
    # the back-face flip: the reflected direction leaves on the side the ray came from,
    # r_dir - dir = 2 cosT1 * (the normal used); against the winding normal it is negative
    # exactly when the normal was flipped
    ok = fr & ~nan & np.all(np.isfinite(R.dir), axis=1) & (R.group == "sweep")
    side = np.einsum("ij,ij->i", np.float64(judge["r_dir"][:, :3]) - np.float64(R.dir[:, :3]), sc.normal[np.maximum(R.tri, 0)])
    assert (ok & (side < -1e-3)).any() and (ok & (side > 1e-3)).any()
    for k in ("tiny", "huge") if sc.with_huge else ("tiny",):
        on = ok & np.isin(R.tri, [i for i, kk in enumerate(sc.kind) if kk == k])
        assert (on & (np.abs(side) > 1e-3)).any(), f"no reflected ray off the {k} triangle"
    # dissipation applied / not applied
    changed = judge["pow"].view(np.int32) != R.pow.view(np.int32)
    assert not changed[R.n1 < 0].any() and not changed[R.n1 == 9].any() and not changed[R.n1 == 0].any()
    live = np.isfinite(R.pow) & (R.pow != 0)
    for m in (1, 10):
        assert (changed & (R.n1 == m) & live).any(), m
    assert (live & (R.n1 == 9) & (R.group == "length")).any()
    ln = np.linalg.norm(np.float64(R.dest[:, :3]) - np.float64(R.origin[:, :3]), axis=1)
    for lo, hi in ((1e-26, 1e-24), (0.5, 2.0), (1e24, 1e26)):
        on = (ln > lo) & (ln < hi) & (R.group == "length") & live & np.isin(R.n1, (1, 10))
        # (over 1e-25 the factor exp(-diss * length) rounds to 1: the row is there for length's rescaling)
        assert on.any() and (changed[on].all() if lo > 1e-20 else not changed[on].any()), (lo, hi)
    # each material branch
    assert refracted.any() and tir.any()
    mirror = fr & (hitmat == 1) & ~nan
    assert (mirror & (judge["r_meas"] == 0) & (judge["t_meas"] == -1)).any()
    dead = (judge["r_meas"] == -1) & (judge["t_meas"] == -1)
    assert (dead & (hitmat == 2) & (judge["meas"] == -1) & (R.meas == 0)).any()          # terminator
    assert (dead & (hitmat == 3) & (judge["meas"] == 1) & (R.meas == 0)).any()           # measure
    assert (dead & (hitmat == 4) & (judge["meas"] == 0) & (R.meas == 0)).any()           # type 4
    assert (dead & (R.imid < 0) & (judge["meas"] == -1) & (R.meas == 1)).any()           # no hit ends a measured ray too
    for ms in (-1, 1):                  # a ray that is not live on glass: no children, its state kept
        assert (dead & (hitmat == 0) & (R.meas == ms) & (judge["meas"] == ms)).any()
    assert nan.any() and (nan & (hitmat == 0)).any() and (nan & (hitmat == 1)).any()
    return dict(nan=int(nan.sum()), fresnel=int(fr.sum()), refracted=int(refracted.sum()), tir=int(tir.sum()))
