"""Beam analysis on the device (lpc_elev_scan / _hist / _digit_pass / _power_below,
Engine.elev_*, CL_Tracer's on_device=True) against numpy and against the host
path of the same tracer, which restates the reference (iterative_tracer.py:420-501).

Elevation tolerance.  The cosine is bit-equal to numpy's for the axis-aligned
poles used here (tests/test_beam_host.py); the elevation is acos of it, ocml's on
the device and numpy's on the host.  The largest |device - host| elevation
measured over the traced cases below was 4.44e-16 (one ulp(pi)); the bound is
8 times that (the margin allows for another CPU's vectorised arccos), far below
the margins the tests assert on their inputs (>= 1e6 ulp(pi))."""
import beam_ref
import numpy as np
import pytest

from lightpycl_amd import beam, scenes

pytestmark = pytest.mark.gpu

ULP_PI = float(np.spacing(np.pi))
ELEV_MEASURED = 4.44e-16                       # max |elev_out - host elevation|, traced cases
ELEV_TOL = max(8 * ELEV_MEASURED, 4 * ULP_PI)
SUM_RTOL = 1e-12                               # float64 sums in atomic order (as test_gpu_postproc.py)

POLE_Z, POLE_X, POLE_NY = [0, 0, 1, 0], [1, 0, 0, 0], [0, -1, 0, 0]


def host_elevation(pos, pole):
    """The reference's expression (iterative_tracer.py:425-428)."""
    with np.errstate(all="ignore"):
        pos0 = np.array(np.divide(pos, np.matrix(np.linalg.norm(pos, axis=1)).T))
        return np.arccos(np.dot(pos0, pole)).reshape(-1)


def points(n, seed=0):
    rng = np.random.default_rng(100 + seed + n)
    pos = (rng.normal(size=(n, 4)) * rng.choice([1e-2, 1.0, 50.0], (n, 1))).astype(np.float32)
    pos[::2, 3] = 0.0                                               # rows as the device record's, and with w
    pw = rng.uniform(0.0, 2.0, n).astype(np.float32)
    return pos, pw


# -- host points through the C ABI -----------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("pole", [POLE_Z, POLE_NY])
def test_scan_and_first_digit_pass_vs_numpy(engine, n, pole):
    pos, pw = points(n)
    e = host_elevation(pos, pole) if n else np.zeros(0)
    s = engine.elev_scan(pole, pos4=pos, pwr=pw)                   # the new symbol: fails without the feature
    assert (s.n_valid, s.n_invalid, s.n_negative) == (n, 0, 0)
    if n == 0:
        assert np.isnan(s.e_min) and np.isnan(s.e_max) and s.total_power == 0.0
    else:
        print("e_min/e_max error", abs(s.e_min - e.min()), abs(s.e_max - e.max()))
        assert abs(s.e_min - e.min()) <= ELEV_TOL and abs(s.e_max - e.max()) <= ELEV_TOL
        np.testing.assert_allclose(s.total_power, pw.astype(np.float64).sum(), rtol=SUM_RTOL)
    bp, bc, bk = engine.elev_digit_pass(pole, 0, 52, 12, pos4=pos, pwr=pw)
    assert bp.shape == bc.shape == bk.shape == (4096,)
    d = (beam.key_of(e) >> np.uint64(52)).astype(np.int64)
    np.testing.assert_array_equal(bc, np.bincount(d, minlength=4096))
    np.testing.assert_allclose(bp, np.bincount(d, weights=pw.astype(np.float64), minlength=4096), rtol=SUM_RTOL)
    for b in np.flatnonzero(bc):
        assert abs(beam.elev_of(bk[b]) - e[d == b].max()) <= ELEV_TOL
    assert not bk[bc == 0].any()


@pytest.mark.parametrize("n,bins", [(257, 90), (4097, 4096), (4097, 5000)])
def test_hist_power_below_and_descent_on_the_devices_own_elevations(engine, n, bins):
    """With the elevations the device reports (elev_out) every bin membership,
    every comparison and the selected ray are exact: only the sums' order is free.
    bins: the LDS kernel (<= 4096 bins) and the global-atomics one."""
    pos, pw = points(n, seed=1)
    pos[5::7] = pos[3]                                              # repeated elevations
    pw[::11] = 0.0
    H, edges, e = engine.elev_hist(bins, POLE_Z, want_elev=True, pos4=pos, pwr=pw)
    assert e.shape == (n,) and np.abs(e - host_elevation(pos, POLE_Z)).max() <= ELEV_TOL
    assert edges[0] == e.min() and edges[-1] == e.max()
    Hn, en = np.histogram(e, bins=bins, weights=pw.astype(np.float64))
    np.testing.assert_array_equal(edges, en)
    np.testing.assert_allclose(H, Hn, rtol=SUM_RTOL, atol=SUM_RTOL * Hn.max())
    H2, _ = engine.elev_hist(bins, POLE_Z, range=(0.5, 2.0), pos4=pos, pwr=pw)    # values outside are dropped
    Hn2, _ = np.histogram(e, bins=bins, range=(0.5, 2.0), weights=pw.astype(np.float64))
    np.testing.assert_allclose(H2, Hn2, rtol=SUM_RTOL, atol=SUM_RTOL * Hn2.max())
    thr = float(e[3])                                               # a repeated elevation
    for incl in (False, True):
        sel = (e <= thr) if incl else (e < thr)
        p, c, em = engine.elev_power_below(POLE_Z, thr, incl, pos4=pos, pwr=pw)
        assert c == sel.sum() and em == e[sel].max()
        np.testing.assert_allclose(p, pw[sel].astype(np.float64).sum(), rtol=SUM_RTOL)
    p, c, em = engine.elev_power_below(POLE_Z, 0.0, False, pos4=pos, pwr=pw)
    assert (p, c) == (0.0, 0) and np.isnan(em)
    want = beam_ref.half_power_sorted(e, pw)
    for bits in (11, 12, 7):
        got = beam.half_power(lambda: engine.elev_scan(POLE_Z, pos4=pos, pwr=pw),
                              lambda pf, sh, b: engine.elev_digit_pass(POLE_Z, pf, sh, b, pos4=pos, pwr=pw),
                              lambda t, i: engine.elev_power_below(POLE_Z, t, i, pos4=pos, pwr=pw), bits=bits)
        assert got.key == want.key and got.elevation == want.elevation
        np.testing.assert_allclose([got.total, got.cum_power], [want.total, want.cum_power], rtol=SUM_RTOL)


def test_invalid_points_are_counted_and_left_out(engine):
    pos, pw = points(300, seed=2)
    pos[[0, 77, 299]] = 0.0                                         # zero rows: 0/0
    pw[[0, 77]] = 1e6
    pw[5] = -1.0                                                    # a negative and a NaN power among the valid
    pw[6] = np.nan
    s = engine.elev_scan(POLE_Z, pos4=pos, pwr=pw)
    assert (s.n_valid, s.n_invalid, s.n_negative) == (297, 3, 2) and np.isnan(s.total_power)
    pw[[5, 6]] = 0.5
    for pole in (POLE_Z, [0, 0, 2, 0]):                            # a non-unit pole: |cos| > 1 has no elevation
        e = host_elevation(pos, pole)
        ok = np.isfinite(e)
        assert (~ok).sum() > (3 if pole[2] == 2 else 2)
        s = engine.elev_scan(pole, pos4=pos, pwr=pw)
        assert (s.n_valid, s.n_invalid, s.n_negative) == (ok.sum(), (~ok).sum(), 0)
        np.testing.assert_allclose(s.total_power, pw[ok].astype(np.float64).sum(), rtol=SUM_RTOL)
        assert abs(s.e_min - e[ok].min()) <= ELEV_TOL and abs(s.e_max - e[ok].max()) <= ELEV_TOL
        with pytest.raises(ValueError):
            engine.elev_hist(90, pole, pos4=pos, pwr=pw)            # np.histogram: non-finite range
        H, edges, ed = engine.elev_hist(90, pole, range=(0.0, np.pi), want_elev=True, pos4=pos, pwr=pw)
        assert np.array_equal(np.isnan(ed), ~ok)
        np.testing.assert_allclose(H.sum(), pw[ok].astype(np.float64).sum(), rtol=SUM_RTOL)
        bp, bc, _ = engine.elev_digit_pass(pole, 0, 53, 11, pos4=pos, pwr=pw)
        assert bc.sum() == ok.sum()
        p, c, _ = engine.elev_power_below(pole, 4.0, True, pos4=pos, pwr=pw)
        assert c == ok.sum()


def test_equal_elevations_widen_the_range_as_numpy(engine):
    pos = np.tile(np.float32([[0.3, -1.2, 0.7, 0.0]]), (130, 1))
    pw = np.linspace(0.5, 1.5, 130).astype(np.float32)
    e = host_elevation(pos, POLE_Z)
    assert e.min() == e.max()
    Hn, en = np.histogram(e, bins=90, weights=pw.astype(np.float64))
    H, edges = engine.elev_hist(90, POLE_Z, pos4=pos, pwr=pw)
    s = engine.elev_scan(POLE_Z, pos4=pos, pwr=pw)
    assert s.e_min == s.e_max and abs(s.e_min - e[0]) <= ELEV_TOL
    assert edges[0] == s.e_min - 0.5 and edges[-1] == s.e_max + 0.5
    np.testing.assert_allclose(edges, en, rtol=0, atol=ELEV_TOL)
    np.testing.assert_allclose(H, Hn, rtol=SUM_RTOL, atol=SUM_RTOL * Hn.max())
    assert np.count_nonzero(H) == 1


def test_bad_arguments_are_errors(engine):
    from lightpycl_amd._lib import LpcError
    pos, pw = points(10)
    with pytest.raises(ValueError):
        engine.elev_scan([0, 0, 1], pos4=pos, pwr=pw)
    for shift, bits in ((60, 12), (0, 0), (-1, 4), (0, 13)):
        with pytest.raises((ValueError, LpcError)):
            engine.elev_digit_pass(POLE_Z, 0, shift, bits, pos4=pos, pwr=pw)


# -- traced records ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced():
    from lightpycl_amd.iterative_tracer import CL_Tracer
    out = {}
    for name, sc in (("lens", scenes.lens(n=3000, seed=9)), ("parabolic", scenes.parabolic(n=3000, seed=3))):
        for keep in (True, False):
            tr = CL_Tracer(device=0)
            tr.iterative_tracer(sc.sources, sc.meshes, trace_iterations=sc.iterations,
                                trace_until_dissipated=sc.tau, max_ray_len=sc.max_ray_len, ior_env=sc.ior_env,
                                keep_results=keep)
            out[name, keep] = tr
    return out


@pytest.fixture()
def no_pdf(monkeypatch, tmp_path):
    """plot_elevation_histogram draws and saves a PDF: keep the drawing, skip the file."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(plt, "savefig", lambda *a, **k: None)
    yield
    plt.close("all")


@pytest.mark.parametrize("npts", [90, 500])
@pytest.mark.parametrize("pole", [POLE_Z, POLE_X])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", ["lens", "parabolic"])
def test_on_device_analyses_vs_host_path(traced, no_pdf, name, keep, pole, npts):
    tr = traced[name, keep]
    pos, pwr = tr.get_measured_rays()
    pw = np.float64(pwr).reshape(-1)
    if name == "lens":
        assert pos.shape[0] == 5764
    assert not np.isnan(pos).any() and (pw >= 0).all()
    e = host_elevation(pos, pole)
    # -- the conditions under which host and device must agree, on the host values
    Hn, edges = np.histogram(e, bins=npts, weights=pw)
    gap = np.abs(e[:, None] - edges[None, 1:-1]).min()
    order = np.argsort(e, kind="stable")
    cums = np.cumsum(pw[order])
    dh = np.sort(np.abs(cums - cums[-1] / 2.0))
    # rays sharing the elevation of the ray the host path reports: only for such a tied group may the
    # reference's cumulative value come from inside the group (parabolic against pole z, nowhere else)
    crossing = e[order][np.argmin(np.abs(cums - cums[-1] / 2.0))]
    tied = int((e == crossing).sum()) > 1
    assert tied == (name == "parabolic" and pole == POLE_Z)
    xc = (edges[0:-1] + edges[1:]) / 2.0
    Hs = Hn / np.sin(xc)
    dm = np.sort(np.abs(Hs - Hs.max() / 2.0))
    print("edge gap [ulp(pi)] %.3g, half-power margin %.3g, HWHM margin %.3g, distinct %d of %d, "
          "rays at the crossing elevation %d"
          % (gap / ULP_PI, (dh[1] - dh[0]) / cums[-1], (dm[1] - dm[0]) / Hs.max(), np.unique(e).size, e.size,
             int((e == crossing).sum())))
    assert gap > 1e6 * ULP_PI
    assert dh[1] - dh[0] > 1e-6 * cums[-1]
    assert dm[1] - dm[0] > 1e-4 * Hs.max()
    # -- the device's elevations (the figure behind ELEV_TOL)
    src = {} if keep is False else dict(pos4=pos, pwr=pw)
    _, _, ed = tr.engine.elev_hist(npts, pole, want_elev=True, **src)
    err = np.abs(ed - e).max()
    print("max |device - host| elevation %.3g (%.2f ulp(pi))" % (err, err / ULP_PI))
    assert err <= ELEV_TOL
    # -- histogram
    H0, x0 = tr.plot_elevation_histogram(points=npts, pole=pole)
    H1, x1 = tr.plot_elevation_histogram(points=npts, pole=pole, on_device=True)
    np.testing.assert_allclose(x1, x0, rtol=0, atol=ELEV_TOL)
    np.testing.assert_allclose(H1, H0, rtol=SUM_RTOL, atol=SUM_RTOL * np.abs(H0).max())
    # -- half power
    t0, a0, c0 = tr.get_beam_width_half_power(points=npts, pole=pole)
    t1, a1, c1 = tr.get_beam_width_half_power(points=npts, pole=pole, on_device=True)
    assert np.shape(a0) == np.shape(a1) == (1,) and np.shape(c0) == np.shape(c1) == (1,)
    np.testing.assert_allclose(t1, t0, rtol=SUM_RTOL)
    np.testing.assert_allclose(a1, a0, rtol=0, atol=ELEV_TOL * 180.0 / np.pi)
    if not tied:                     # a tied group: the reference may report a value from inside it
        np.testing.assert_allclose(c1, c0, rtol=SUM_RTOL)
    # -- HWHM
    t0, a0, w0 = tr.get_beam_HWHM(points=npts, pole=pole)
    t1, a1, w1 = tr.get_beam_HWHM(points=npts, pole=pole, on_device=True)
    assert np.shape(a0) == np.shape(a1) == (1,)
    np.testing.assert_allclose(t1, t0, rtol=SUM_RTOL)
    np.testing.assert_allclose(a1, a0, rtol=0, atol=ELEV_TOL * 180.0 / np.pi)
    np.testing.assert_allclose(w1, w0, rtol=SUM_RTOL)


def test_default_keyword_is_the_host_path(traced, monkeypatch):
    """on_device=False (the default) takes no device pass."""
    tr = traced["lens", False]
    for name in ("elev_scan", "elev_hist", "elev_digit_pass", "elev_power_below"):
        monkeypatch.setattr(type(tr.engine), name, lambda *a, **k: pytest.fail("device pass on the host path"))
    tr.get_beam_width_half_power()
    tr.get_beam_HWHM(points=90)
    tr.get_beam_HWHM(points=90, on_device=False)
