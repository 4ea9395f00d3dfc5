"""Beam analysis on the device (lpc_elev_scan / _hist / _digit_pass / _power_below,
Engine.elev_*, CL_Tracer's on_device=True) against numpy and against the host
path of the same tracer, which restates the reference (iterative_tracer.py:420-501).

Elevation tolerance.  The cosine is bit-equal to numpy's for the axis-aligned
poles used here (tests/test_beam_host.py); the elevation is acos of it, ocml's on
the device and numpy's on the host.  The largest |device - host| elevation
measured over the traced cases below was 4.44e-16 (one ulp(pi)); the bound is
8 times that (the margin allows for another CPU's vectorised arccos), far below
the margins the tests assert on their inputs (>= 1e6 ulp(pi)).  ELEV_TOL and
SUM_RTOL live in tests/beam_ref.py, which tests/test_ref_host.py shares."""
import beam_ref
import numpy as np
import pytest
from beam_ref import ELEV_TOL, SUM_RTOL, ULP_PI, no_pdf  # noqa: F401  (no_pdf: a fixture)

from lightpycl_amd import beam, scenes

pytestmark = pytest.mark.gpu

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


# -- past one grid of rows: the grid-stride step of the four elevation kernels ------------
def _cus(engine):
    """The CU count that caps the kernels' grids (elev_grid: h->cus, read from
    hipDeviceProp_t::multiProcessorCount, the property torch reports)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert engine.info()[1] == cus
    return cus


@pytest.fixture(scope="module")
def big(engine):
    """n = 8 cus 256 + 64 cus + 257 points: the scan, histogram and below kernels
    (8 blocks per CU) take 2 trips, the 11-bit digit kernel (4) 3, the 12-bit one
    (2) 5; the last trip is partly filled (n is odd: the last block is ragged) and
    most blocks have none.  Repeated elevations, zero powers, three zero rows
    (no elevation) beyond the first trip.  -> points, the host elevations and the
    device's own (elev_out)."""
    cus = _cus(engine)
    first = 8 * cus * 256
    n = first + 64 * cus + 257
    pos, pw = points(n, seed=5)
    pos[5::7] = pos[3]
    pw[::11] = 0.0
    zero = np.array([first + 1, first + 32 * cus + 5, n - 2])
    pos[zero] = 0.0
    e = host_elevation(pos, POLE_Z)
    ok = np.isfinite(e)
    assert (~ok).sum() == 3 and not ok[zero].any()
    _, _, ed = engine.elev_hist(90, POLE_Z, range=(0.0, np.pi), want_elev=True, pos4=pos, pwr=pw)
    return dict(cus=cus, first=first, n=n, pos=pos, pw=pw, e=e, ok=ok, ed=ed, src=dict(pos4=pos, pwr=pw))


def test_big_scan_and_elev_out(engine, big):
    e, ok, ed, pw = big["e"], big["ok"], big["ed"], big["pw"]
    assert ed.shape == (big["n"],)
    assert np.array_equal(np.isnan(ed), ~ok)                       # every row written, the last trip's too
    err = np.abs(ed[ok] - e[ok])
    print("max |elev_out - host| %.3g, beyond the first trip %.3g" % (err.max(), err[big["first"] - 3:].max()))
    assert err.max() <= ELEV_TOL
    s = engine.elev_scan(POLE_Z, **big["src"])
    assert (s.n_valid, s.n_invalid, s.n_negative) == (big["n"] - 3, 3, 0)
    assert abs(s.e_min - e[ok].min()) <= ELEV_TOL and abs(s.e_max - e[ok].max()) <= ELEV_TOL
    assert s.e_min == ed[ok].min() and s.e_max == ed[ok].max()
    np.testing.assert_allclose(s.total_power, pw[ok].astype(np.float64).sum(), rtol=SUM_RTOL)


def _check_digit_pass(engine, big, P, prefix, shift, bits):
    bp, bc, bk = engine.elev_digit_pass(POLE_Z, prefix, shift, bits, **big["src"])
    wp, wc, wk = P.digit_pass(prefix, shift, bits)
    assert bc.shape == (1 << bits,) and wc.sum() > 0
    np.testing.assert_array_equal(bc, wc)
    np.testing.assert_array_equal(bk, wk)                           # each bin's largest key, of elev_out
    np.testing.assert_allclose(bp, wp, rtol=SUM_RTOL)
    return bc


def test_big_digit_passes(engine, big):
    P = beam_ref.NumpyPasses(big["ed"], big["pw"])
    bc = _check_digit_pass(engine, big, P, 0, 52, 12)
    assert bc.sum() == big["n"] - 3
    top = int(np.argmax(bc))                                        # a populated prefix, one level down
    assert bc[top] > 4096
    c12 = _check_digit_pass(engine, big, P, top, 40, 12)
    c11 = _check_digit_pass(engine, big, P, top, 41, 11)
    assert c12.sum() == c11.sum() == bc[top]
    _check_digit_pass(engine, big, P, 0, 53, 11)                    # the 11-bit kernel over every row


@pytest.mark.parametrize("bins", [90, 5000])
def test_big_hist(engine, big, bins):
    """The LDS kernel (90 bins) and the global-atomics one (5000) against
    np.histogram of the device's own elevations."""
    ok, ed = big["ok"], big["ed"]
    w = big["pw"].astype(np.float64)
    lo, hi = float(ed[ok].min()), float(ed[ok].max())
    H, edges, ed2 = engine.elev_hist(bins, POLE_Z, range=(lo, hi), want_elev=True, **big["src"])
    np.testing.assert_array_equal(ed2, ed)                          # NaN rows equal as NaN
    Hn, en = np.histogram(ed[ok], bins=bins, range=(lo, hi), weights=w[ok])
    np.testing.assert_array_equal(edges, en)
    np.testing.assert_allclose(H, Hn, rtol=SUM_RTOL, atol=SUM_RTOL * Hn.max())
    H2, _ = engine.elev_hist(bins, POLE_Z, range=(0.5, 2.0), **big["src"])
    Hn2, _ = np.histogram(ed[ok], bins=bins, range=(0.5, 2.0), weights=w[ok])
    np.testing.assert_allclose(H2, Hn2, rtol=SUM_RTOL, atol=SUM_RTOL * Hn2.max())


def test_big_power_below_and_half_power(engine, big):
    ok, ed, pw, src = big["ok"], big["ed"], big["pw"], big["src"]
    thr = float(ed[3])                                              # a repeated elevation
    assert (ed == thr).sum() > big["n"] // 8
    for incl in (False, True):
        sel = ok & ((ed <= thr) if incl else (ed < thr))
        p, c, em = engine.elev_power_below(POLE_Z, thr, incl, **src)
        assert c == sel.sum() and em == ed[sel].max()
        np.testing.assert_allclose(p, pw[sel].astype(np.float64).sum(), rtol=SUM_RTOL)
    want = beam_ref.half_power_sorted(ed, pw)
    for bits in (11, 12):
        got = beam.half_power(lambda: engine.elev_scan(POLE_Z, **src),
                              lambda pf, sh, b: engine.elev_digit_pass(POLE_Z, pf, sh, b, **src),
                              lambda t, i: engine.elev_power_below(POLE_Z, t, i, **src), bits=bits)
        assert got.key == want.key and got.elevation == want.elevation
        np.testing.assert_allclose([got.total, got.cum_power], [want.total, want.cum_power], rtol=SUM_RTOL)


def test_big_device_record_vs_the_same_points_from_the_host(engine, no_pdf):
    """The device-resident record (px / py / pz planes, aggregate mode only) past
    one grid of rows: every pass and the three on_device analyses over it against
    the same engine's passes over fetch_measured() handed back as host points.
    Same elevations on both sides, so counts, ranges and selected keys are exact
    and only the sums' order is free."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    first = 8 * _cus(engine) * 256
    sc = scenes.lens(n=int(first / 1.75) + 1000, seed=9)            # ~1.92 measured rays per emitted ray
    tr = CL_Tracer(device=0)
    tr.iterative_tracer(sc.sources, sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                        max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False)
    eng = tr.engine
    pos, pw, _ = eng.fetch_measured()
    print("measured rays", pos.shape[0], "first trip", first)
    assert pos.shape[0] > first + 256
    src = dict(pos4=pos, pwr=pw)
    dev = {}
    for pole in (POLE_Z, POLE_X):
        s0, s1 = eng.elev_scan(pole), eng.elev_scan(pole, **src)
        assert s0[:5] == s1[:5] and s0.n_valid == pos.shape[0]
        np.testing.assert_allclose(s0.total_power, s1.total_power, rtol=SUM_RTOL)
        for prefix, shift, bits in ((0, 52, 12), (0, 53, 11)):
            a, b = eng.elev_digit_pass(pole, prefix, shift, bits), eng.elev_digit_pass(pole, prefix, shift, bits, **src)
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2], b[2])
            np.testing.assert_allclose(a[0], b[0], rtol=SUM_RTOL)
        thr = (s0.e_min + s0.e_max) / 2.0
        a, b = eng.elev_power_below(pole, thr, True), eng.elev_power_below(pole, thr, True, **src)
        assert a[1:] == b[1:] and 0 < a[1] < pos.shape[0]
        np.testing.assert_allclose(a[0], b[0], rtol=SUM_RTOL)
        _, _, e0 = eng.elev_hist(90, pole, want_elev=True)
        _, _, e1 = eng.elev_hist(90, pole, want_elev=True, **src)
        np.testing.assert_array_equal(e0, e1)
        for npts in (90, 5000):
            dev[tuple(pole), npts] = (tr.plot_elevation_histogram(points=npts, pole=pole, on_device=True),
                                      tr.get_beam_width_half_power(points=npts, pole=pole, on_device=True),
                                      tr.get_beam_HWHM(points=npts, pole=pole, on_device=True))
    assert tr._elev_device(POLE_Z)[1] == {}                         # so far: the device-resident record
    # the same tracer over the fetched rays as host points (results mode's source of _elev_device)
    tr._aggregate = False
    tr.results = [(pos, pos, pw, np.ones(pos.shape[0], np.int32))]
    src2 = tr._elev_device(POLE_Z)[1]                               # from here on: these host points
    assert set(src2) == {"pos4", "pwr"} and src2["pos4"].shape == pos.shape
    np.testing.assert_array_equal(src2["pos4"], pos)
    np.testing.assert_array_equal(src2["pwr"], pw)
    for (pole, npts), ((H0, x0), (t0, a0, c0), (u0, b0, w0)) in dev.items():
        pole = list(pole)
        H1, x1 = tr.plot_elevation_histogram(points=npts, pole=pole, on_device=True)
        np.testing.assert_array_equal(x0, x1)
        np.testing.assert_allclose(H0, H1, rtol=SUM_RTOL, atol=SUM_RTOL * np.abs(H1).max())
        t1, a1, c1 = tr.get_beam_width_half_power(points=npts, pole=pole, on_device=True)
        np.testing.assert_array_equal(a0, a1)
        assert np.shape(a0) == np.shape(c0) == (1,)
        np.testing.assert_allclose([t0, c0[0]], [t1, c1[0]], rtol=SUM_RTOL)
        u1, b1, w1 = tr.get_beam_HWHM(points=npts, pole=pole, on_device=True)
        np.testing.assert_array_equal(b0, b1)
        np.testing.assert_allclose([u0, float(w0)], [u1, float(w1)], rtol=SUM_RTOL)
