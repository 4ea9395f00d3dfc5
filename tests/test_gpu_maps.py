"""One-pass maps on the GPU (lpc_map_hist) against the
reference's own projection kernels for the points and np.histogram2d for the bins.

The counts are exact (they pin the bin of every point whatever the order of
summation).  The float64 sums are the reference's addends in another order, so a
bin of m addends w differs from numpy's sequential sum by at most
    2 * m * 2^-53 * sum |w|
(two recursive summations of the same m numbers, each within (m - 1) u sum |w| of
the exact sum, u = 2^-53).  No tolerance here is measured."""
import ctypes
import gc

import numpy as np
import pytest

from lightpycl_amd import _lib, scenes
from lightpycl_amd.iterative_tracer import CL_Tracer

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
HALF_PI = ((-np.pi / 2, np.pi / 2), (-np.pi / 2, np.pi / 2))
LIMITS = {0: HALF_PI, 1: ((-1.0, 1.0), (-1.0, 1.0)), 2: ((-1000.0, 1000.0), (-900.0, 900.0))}


@pytest.fixture(scope="module")
def ref(exact_ref):
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    return exact_ref


def _hemisphere(n, seed=5):
    """n points on the upper hemisphere of radius 1000, powers in (0, 1]."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v[:, 2] = np.abs(v[:, 2])
    v /= np.maximum(np.linalg.norm(v, axis=1), 1e-30)[:, None]
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = 1000.0 * v
    return pos, (1.0 - rng.random(n)).astype(np.float32)


def _quarter_turns(axis, k):
    """k rotations by multiples of a quarter turn, entries exactly 0 or +-1: the
    rotated float32 coordinates are exact whatever the order of the arithmetic."""
    c, s = [1, 0, -1, 0], [0, 1, 0, -1]
    out = np.zeros((k, 4, 4), np.float32)
    for j in range(k):
        cj, sj = c[j % 4], s[j % 4]
        out[j, :3, :3] = ([[cj, -sj, 0], [sj, cj, 0], [0, 0, 1]] if axis == "z" else
                          [[1, 0, 0], [0, cj, -sj], [0, sj, cj]])
    return out


def _ref_points(ref, pos, pw, mode, rots, pivot=None):
    """x, y, weight of every (rotation, point): the reference's kernels for the two
    projections; for the planar view the positions themselves, rotated exactly."""
    xs, ys, ps = [], [], []
    if mode == 2:
        if rots is None:
            return pos[:, 0].copy(), pos[:, 1].copy(), pw.copy()
        assert pivot is None and np.all(np.isin(rots, (-1.0, 0.0, 1.0)))
        for R in rots:
            uv = pos[:, :3].astype(np.float64) @ R[:2, :3].astype(np.float64).T
            assert np.array_equal(uv.astype(np.float32), uv)
            xs.append(uv[:, 0].astype(np.float32))
            ys.append(uv[:, 1].astype(np.float32))
            ps.append(pw)
    else:
        for R in ([None] if rots is None else rots):
            x, y, pc = ref.project(pos, pw, "angular" if mode == 0 else "stereo", rot=R, pivot=pivot)
            xs.append(x)
            ys.append(y)
            ps.append(pc)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ps)


def _div(mode, limits, points):
    if mode == 2:
        return np.float64(1.0)
    px, py = (points, points) if np.ndim(points) == 0 else points
    return (np.float64(limits[0][1] - limits[0][0]) / np.float64(px)) * (np.float64(limits[1][1] - limits[1][0]) / np.float64(py))


def _reference_maps(x, y, pc, limits, points, div):
    """count, H, sum |w|, H2 of numpy over the reference's points; edges."""
    ok = ~(np.isnan(x) | np.isnan(y))                   # a NaN coordinate lies in no bin
    x, y = x[ok].astype(np.float64), y[ok].astype(np.float64)
    w = pc[ok].astype(np.float64) / div
    kw = dict(bins=points, range=limits)
    cnt, xe, ye = np.histogram2d(x, y, **kw)
    Hr = np.histogram2d(x, y, weights=w, **kw)[0]
    Ha = np.histogram2d(x, y, weights=np.abs(w), **kw)[0]
    H2r = np.histogram2d(x, y, weights=w * w, **kw)[0]
    return cnt, Hr, Ha, H2r, xe, ye


def _check(out, x, y, pc, limits, points, div):
    cnt, Hr, Ha, H2r, xe, ye = _reference_maps(x, y, pc, limits, points, div)
    H = out[0]
    np.testing.assert_array_equal(out[1], xe)
    np.testing.assert_array_equal(out[2], ye)
    assert H.shape == Hr.shape and H.dtype == np.float64
    nan = np.isnan(Hr)
    np.testing.assert_array_equal(np.isnan(H), nan)
    err = np.abs(np.where(nan, 0.0, H) - np.where(nan, 0.0, Hr))
    bound = 2.0 * cnt * U * np.where(nan, 0.0, Ha)
    print("max |H - Href| %.3e, max bound %.3e, points in bins %d" % (err.max(), bound.max(), cnt.sum()))
    assert np.all(err <= bound)
    if len(out) == 5:
        np.testing.assert_array_equal(out[3], cnt)      # exact
        assert out[3].dtype == np.int64
        H2 = out[4]
        np.testing.assert_array_equal(np.isnan(H2), nan)
        err2 = np.abs(np.where(nan, 0.0, H2) - np.where(nan, 0.0, H2r))
        assert np.all(err2 <= 2.0 * cnt * U * np.where(nan, 0.0, H2r))
    return cnt, Hr


# n, rotations, axis, bins, mode, statistics, pivot.  A block keeps 143 360 B of the map
# in LDS, 8 B per bin and 20 B with the statistics, and a larger map goes in up to 6
# slices of that size: 30x30 is one slice both ways, 128x128 one slice without the
# statistics and three with them; 300x300 with the statistics (13 slices) and 500x500
# without (14) are on the global-atomic path.  (2100, 2) has more edges than a block
# keeps in LDS; 70 rotations take two sweeps of 64.
CASES = [
    (0, 1, "z", (3, 5), 0, True, None),
    (1, 1, "z", 1, 0, True, None),
    (63, 2, "x", (3, 5), 1, False, None),
    (64, 7, "z", 30, 0, True, None),
    (65, 1, "z", 30, 2, True, None),
    (255, 2, "x", 128, 0, False, None),
    (257, 7, "x", 128, 1, True, None),
    (257, 36, "z", 300, 1, True, None),
    (257, 7, "z", 500, 1, False, None),
    (257, 2, "z", (2100, 2), 0, True, None),
    (1000, 36, "z", 30, 0, True, None),
    (1000, 70, "x", 30, 0, True, None),
    (1000, 2, "z", 300, 2, True, None),
    (1000, 7, "x", (3, 5), 2, False, None),
    (1000, 7, "z", 30, 0, True, (1.5, -2.0, 3.0, 0.0)),
    (70001, 7, "z", 300, 0, True, None),
    (70001, 2, "x", 500, 0, False, None),
    (70001, 36, "x", 30, 0, False, None),
    (70001, 1, "z", 128, 1, False, None),
    (70001, 2, "x", 128, 2, True, None),
]


@pytest.mark.parametrize("n,n_rot,axis,points,mode,stats,pivot", CASES)
def test_map_against_reference(engine, ref, n, n_rot, axis, points, mode, stats, pivot):
    pos, pw = _hemisphere(n)
    if mode == 2:
        rots = None if n_rot == 1 else _quarter_turns(axis, n_rot)
    else:
        rots = CL_Tracer._source_rots(axis, n_rot)
    lim = LIMITS[mode]
    out = engine.map_hist(pos, pw, lim, points, mode=mode, rots=rots, pivot=pivot, stats=stats)
    assert len(out) == (5 if stats else 3)
    x, y, pc = _ref_points(ref, pos, pw, mode, rots, pivot)
    cnt, Hr = _check(out, x, y, pc, lim, points, _div(mode, lim, points))
    if n > 1 and pivot is None:
        assert cnt.sum() > 0 and Hr.sum() > 0                 # the comparison is not empty


def test_one_hot_bin(engine, ref):
    """Whole waves in one bin: identical points turned about their own axis."""
    n = 70001
    pos = np.zeros((n, 4), np.float32)
    pos[:, 2] = 1000.0
    pw = (1.0 - np.random.default_rng(3).random(n)).astype(np.float32)
    rots = CL_Tracer._source_rots("z", 7)
    for points in (30, 300):                                  # LDS and (13 slices) global atomics
        out = engine.map_hist(pos, pw, HALF_PI, points, rots=rots, stats=True)
        x, y, pc = _ref_points(ref, pos, pw, 0, rots)
        cnt, _ = _check(out, x, y, pc, HALF_PI, points, _div(0, HALF_PI, points))
        assert cnt.max() == 7 * n and np.count_nonzero(cnt) == 1


def test_edges_and_invalid_points(engine, ref):
    lim, points = ((-8.0, 8.0), (-8.0, 8.0)), 16
    g = np.arange(-8, 9, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    out_hi, out_lo = np.nextafter(np.float32(8), np.float32(np.inf)), np.nextafter(np.float32(-8), np.float32(-np.inf))
    extra = np.array([[out_hi, 0], [0, out_hi], [out_lo, 0], [0, out_lo], [out_hi, out_lo], [np.inf, 1], [1, -np.inf],
                      [np.nan, 2], [0.5, 0.5], [0.5, 0.5]], np.float32)
    xy = np.concatenate([np.stack([X.ravel(), Y.ravel()], axis=1), extra])
    pos = np.zeros((len(xy), 4), np.float32)
    pos[:, :2] = xy
    pos[:, 2] = 7.0
    pw = (1.0 + np.arange(len(xy)) % 5).astype(np.float32)
    pw[-1] = np.nan                                           # poisons the bin of (0.5, 0.5) alone
    out = engine.map_hist(pos, pw, lim, points, mode=2, stats=True)
    cnt, Hr = _check(out, pos[:, 0], pos[:, 1], pw, lim, points, 1.0)
    H, _, _, C, H2 = out
    assert np.isnan(H).sum() == 1 and np.isnan(H[8, 8]) and np.isnan(H2[8, 8]) and C[8, 8] == 3
    assert C.sum() == 17 * 17 + 2                             # every grid point, none of the outside ones
    assert C[15, 15] == 4 and C[0, 0] == 1 and C[15, 0] == 2  # the last edge belongs to the last bin
    # a zero position has no direction: NaN projection, dropped
    pos, pw = _hemisphere(300)
    pos[::7, :3] = 0.0
    rots = CL_Tracer._source_rots("x", 2)
    out = engine.map_hist(pos, pw, HALF_PI, 30, mode=0, rots=rots, stats=True)
    x, y, pc = _ref_points(ref, pos, pw, 0, rots)
    assert np.isnan(x).sum() == 2 * len(pos[::7])
    cnt, _ = _check(out, x, y, pc, HALF_PI, 30, _div(0, HALF_PI, 30))
    assert 0 < cnt.sum() <= 2 * (300 - len(pos[::7]))


# -- traced: the tracer's entry points in both modes -----------------------------------
@pytest.fixture(scope="module")
def traced(ref):
    sc = scenes.lens(n=4000, seed=9)
    out = {}
    for keep in (True, False):
        tr = CL_Tracer(device=0)
        tr.iterative_tracer(sc.sources, sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                            max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=keep)
        pos, pwr = tr.get_measured_rays()
        out[keep] = (tr, np.asarray(pos, np.float32), np.asarray(pwr, np.float32).reshape(-1))
    return out


@pytest.mark.parametrize("axis,sources", [("z", 36), ("z", 12), ("x", 7)])
def test_replicated_sources_on_device(traced, ref, axis, sources):
    lim, pts = HALF_PI, 30
    div = _div(0, lim, pts)
    rots = CL_Tracer._source_rots(axis, sources)
    counts = {}
    for keep in (True, False):
        tr, pos, pw = traced[keep]
        x, y, pc = _ref_points(ref, pos, pw, 0, rots)
        assert x.size == sources * len(pw)
        if axis == "z":
            inside = (np.abs(x.astype(np.float64)) <= np.pi / 2) & (np.abs(y.astype(np.float64)) <= np.pi / 2)
            assert inside.mean() >= 0.99
        out = tr.replicate_lightsources_and_plot(limits=lim, points=pts, axis=axis, sources=sources, plot=False,
                                                 on_device=True)
        assert len(out) == 3 and tr.hist_data is out
        cnt, Hr = _check(out, x, y, pc, lim, pts, div)
        assert Hr.sum() > 0
        H, xe, ye, count, rel = tr.binned_stats("angular", lim, pts, axis=axis, sources=sources)
        _check((H, xe, ye), x, y, pc, lim, pts, div)
        np.testing.assert_array_equal(count, cnt)
        H2r = _reference_maps(x, y, pc, lim, pts, div)[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel_ref = np.sqrt(H2r) / np.abs(Hr)
        # NaN for an empty bin, and 0 / 0 for one whose rays carry no power
        np.testing.assert_array_equal(np.isnan(rel), (cnt == 0) | (Hr == 0.0))
        assert np.isnan(rel[cnt == 0]).all()
        full = ~np.isnan(rel_ref)
        # sqrt halves H2's relative error (2 m u, positive addends), the division adds H's (2 m u)
        # and a few roundings of its own and of the reference's
        assert np.all(np.abs(rel[full] - rel_ref[full]) <= (4.0 * cnt[full] + 8.0) * U * rel_ref[full])
        counts[keep] = count
    np.testing.assert_array_equal(counts[True], counts[False])   # the same set of rays


def test_planar_map_on_device(traced):
    lim, pts = ((-1000.0, 1000.0), (-1000.0, 1000.0)), 40
    counts = {}
    for keep in (True, False):
        tr, pos, pw = traced[keep]
        host = tr.get_binned_data(limits=lim, points=pts)
        out = tr.get_binned_data(limits=lim, points=pts, on_device=True)
        assert len(out) == 3 and tr.hist_data is out
        cnt, Hr = _check(out, pos[:, 0], pos[:, 1], pw, lim, pts, 1.0)
        assert Hr.sum() > 0
        np.testing.assert_array_equal(host[0], Hr)
        H, xe, ye, count, rel = tr.binned_stats("planar", lim, pts)
        _check((H, xe, ye), pos[:, 0], pos[:, 1], pw, lim, pts, 1.0)
        np.testing.assert_array_equal(count, cnt)
        np.testing.assert_array_equal(np.isnan(rel), (cnt == 0) | (Hr == 0.0))
        one = (cnt == 1) & (Hr != 0.0)
        assert np.all(rel[one] == 1.0)                           # one ray in a bin: sqrt(w^2) / |w|
        counts[keep] = count
    np.testing.assert_array_equal(counts[True], counts[False])


def test_defaults_untouched(traced, engine):
    lim, pts = HALF_PI, 30
    for keep in (True, False):
        tr = traced[keep][0]
        before = tr.replicate_lightsources_and_plot(limits=lim, points=pts, sources=12, plot=False)
        planar = tr.get_binned_data(points=50, limits=((-1000, 1000), (-1000, 1000)))
        tr.replicate_lightsources_and_plot(limits=lim, points=pts, sources=12, plot=False, on_device=True)
        tr.get_binned_data(points=50, limits=((-1000, 1000), (-1000, 1000)), on_device=True)
        after = tr.replicate_lightsources_and_plot(limits=lim, points=pts, sources=12, plot=False)
        planar2 = tr.get_binned_data(points=50, limits=((-1000, 1000), (-1000, 1000)))
        for a, b in zip(before + planar, after + planar2):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # lpc_project_hist around lpc_map_hist: 40 points on a spiral, at most two to a bin, so
    # its atomic sums do not depend on their order
    k = np.arange(40)
    el, az = (k + 1) * (np.pi / 2) / 41.0, k * 2.399963229728653
    pos = np.zeros((40, 4), np.float32)
    pos[:, 0], pos[:, 1], pos[:, 2] = 500 * np.sin(el) * np.cos(az), 500 * np.sin(el) * np.sin(az), 500 * np.cos(el)
    pw = (1.0 + k % 3).astype(np.float32)
    H0, xe, ye, x, y, _ = engine.project_hist(pos, pw, lim, 64, want_xy=True)
    assert np.histogram2d(x, y, bins=64, range=lim)[0].max() <= 2 and H0.sum() > 0
    engine.map_hist(pos, pw, lim, 64, rots=CL_Tracer._source_rots("z", 7), stats=True)
    H1 = engine.project_hist(pos, pw, lim, 64)[0]
    assert np.array_equal(H0.view(np.uint64), H1.view(np.uint64))


# -- refusals, lifetime, a trace in flight --------------------------------------------
def _raw_call(eng, mode=0, n=4, pos=True, pwr=True, n_rot=1, nx=4, ny=4, xe=True, ye=True, H=True):
    P = _lib.ptr
    pos4, pw = np.ones((4, 4), np.float32), np.ones(4, np.float32)
    ex = np.linspace(-2.0, 2.0, max(nx, 1) + 1)
    ey = np.linspace(-2.0, 2.0, max(ny, 1) + 1)
    Hbuf = np.full((max(nx, 1), max(ny, 1)) if nx * ny <= 1 << 20 else (1, 1), -3.0)
    rc = eng.L.lpc_map_hist(eng.h, mode, n, P(pos4) if pos else None, P(pw) if pwr else None, None, n_rot, None,
                            P(ex) if xe else None, nx, P(ey) if ye else None, ny, 1.0, P(Hbuf) if H else None, None, None)
    return rc, Hbuf


def test_refusals(engine):
    rc, H = _raw_call(engine)
    assert rc == 0 and np.all(H >= 0.0)                       # the call the refusals below vary is a good one
    bad = [dict(mode=-1), dict(mode=3), dict(n_rot=0), dict(n_rot=-2), dict(nx=0), dict(ny=0), dict(ny=-5),
           dict(xe=False), dict(ye=False), dict(H=False), dict(pwr=False), dict(n=-1), dict(nx=65536, ny=65536)]
    for kw in bad:
        rc, H = _raw_call(engine, **kw)
        assert rc == -1, kw                                    # LPC_E_ARG
        assert b"map_hist" in engine.L.lpc_last_error(engine.h), kw
        assert np.all(H == -3.0), kw                           # nothing ran, nothing was copied back
    assert engine.L.lpc_map_hist(None, 0, 0, None, None, None, 1, None, None, 1, None, 1, 1.0, None, None, None) == -1
    # an empty input gives zeros
    H, _, _, C, H2 = engine.map_hist(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), HALF_PI, 5, stats=True)
    assert not H.any() and not C.any() and not H2.any()


def _live():
    d, p = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.load().lpc_debug_live_bytes(ctypes.byref(d), ctypes.byref(p)))
    return d.value, p.value


def test_every_map_path_closes_clean_and_waits_for_a_trace():
    from lightpycl_amd.engine import Engine
    sc = scenes.lens(n=3000, seed=4)
    ls = sc.sources[0]
    o, d = np.asarray(ls.rays_origin, np.float32), np.asarray(ls.rays_dir, np.float32)
    p = np.asarray(ls.rays_power, np.float32).reshape(-1)
    thr = (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))
    pos, pw = _hemisphere(2000)
    gc.collect()
    base = _live()
    e = Engine(0)
    try:
        H, _, _, C, _ = e.map_hist(None, None, HALF_PI, 30, stats=True)     # no trace yet: an empty record
        assert not H.any() and not C.any()
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        e.run_local(sc.iterations, thr, wait=False)                          # lpc_trace_run_async
        lim = ((-1000.0, 1000.0), (-1000.0, 1000.0))
        H, xe, ye, C, _ = e.map_hist(None, None, lim, 40, mode=2, stats=True)   # waits for the trace
        rpos, rpw, _ = e.fetch_measured()
        assert len(rpw) > 0
        np.testing.assert_array_equal(C, np.histogram2d(rpos[:, 0], rpos[:, 1], bins=40, range=lim)[0])
        assert C.sum() > 0
        for mode, points, stats, rots in [(0, 30, True, CL_Tracer._source_rots("z", 7)), (1, 128, False, None),
                                          (0, 300, True, CL_Tracer._source_rots("x", 70)), (2, (2100, 2), True, None)]:
            e.map_hist(pos, pw, LIMITS[mode], points, mode=mode, rots=rots, stats=stats)
            e.map_hist(None, None, LIMITS[mode], points, mode=mode, rots=rots, stats=stats)
        assert _live()[0] > base[0]
    finally:
        e.close()
    assert _live() == base
