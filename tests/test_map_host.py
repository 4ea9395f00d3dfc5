"""CPU tests of the device maps: the bin rule shared with the HIP kernels
(lpc_math.hpp bin_index, compiled for the host) against numpy's, and the argument
conversion of Engine.map_hist over a stand-in for the library."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "csrc", "_build", "libbin_harness.so")


@pytest.fixture(scope="module")
def bin_eval():
    src = os.path.join(ROOT, "tests", "csrc", "bin_harness.cpp")
    hdr = os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_math.hpp")
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "lightpycl_amd", "csrc"), src, "-o", SO], check=True)
    L = ctypes.CDLL(SO)
    D = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.bin_eval.argtypes = [D, ctypes.c_longlong, D, ctypes.c_int, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    L.bin_eval.restype = None

    def run(v, e):
        v = np.ascontiguousarray(v, np.float64)
        e = np.ascontiguousarray(e, np.float64)
        out = np.full(v.size, -7, np.int32)
        L.bin_eval(v, v.size, e, e.size - 1, out)
        return out
    return run


def numpy_bin(v, e):
    """np.histogramdd's bin of v (numpy/lib/histograms.py): searchsorted(e, v, 'right')
    - 1, a value equal to the last edge moved into the last bin, -1 for what numpy
    counts as an outlier (outside the edges, NaN)."""
    nb = e.size - 1
    b = np.searchsorted(e, v, side="right") - 1
    b[v == e[-1]] = nb - 1
    b[(b < 0) | (b >= nb)] = -1
    return b.astype(np.int32)


def _hist_edges(lo, hi, points):
    return np.histogram2d(np.zeros(0), np.zeros(0), bins=points, range=((lo, hi), (lo, hi)))[1]


EDGES = {
    "half_pi_30": _hist_edges(-np.pi / 2, np.pi / 2, 30),
    "unit_500": _hist_edges(-1.0, 1.0, 500),
    "ten_500": _hist_edges(-10.0, 10.0, 500),
    "one_bin": _hist_edges(0.0, 1.0, 1),
    "geometric_40": 1e-3 * 1.5 ** np.arange(40),           # non-uniform: the uniform guess is far off
    "steps_33": np.cumsum(np.r_[-5.0, np.tile([1e-9, 3.0, 0.25, 40.0], 8)]),   # widths over ten decades
}


def _values(e):
    rng = np.random.default_rng(11)
    f32 = e.astype(np.float32)
    near = [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
            f32.astype(np.float64), np.nextafter(f32, np.float32(-np.inf)).astype(np.float64),
            np.nextafter(f32, np.float32(np.inf)).astype(np.float64)]
    span = e[-1] - e[0]
    inside = rng.uniform(e[0], e[-1], 10_000)
    outside = np.r_[e[0] - rng.uniform(0, 3 * span, 500) - 1e-12, e[-1] + rng.uniform(0, 3 * span, 500) + 1e-12]
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e308, -1e308])
    return np.concatenate(near + [inside, outside, special])


@pytest.mark.parametrize("name", sorted(EDGES))
def test_bin_rule_is_numpys(bin_eval, name):
    e = np.ascontiguousarray(EDGES[name], np.float64)
    assert np.all(np.diff(e) > 0)
    v = _values(e)
    got = bin_eval(v, e)
    ref = numpy_bin(v, e)
    np.testing.assert_array_equal(got, ref)
    assert (ref >= 0).sum() >= 10_000 and (ref < 0).sum() >= 1_000
    # the rule the 2-D histogram itself applies (one row of bins along y)
    ok = ~np.isnan(v)
    H = np.histogram2d(v[ok], np.zeros(ok.sum()), bins=(e, np.array([-1.0, 1.0])))[0][:, 0]
    np.testing.assert_array_equal(np.bincount(got[got >= 0], minlength=e.size - 1), H)


def test_bin_rule_on_huge_and_repeated_edges(bin_eval):
    """The guess overflows (an infinite span) or is useless (equal edges): the
    answer still comes from the edges."""
    e = np.array([-1e308, -1.0, 0.0, 2.0, 1e308])
    v = np.array([-1e308, -2.0, -1.0, -0.5, 0.0, 1.0, 2.0, 1e300, 1e308, np.inf, np.nan])
    np.testing.assert_array_equal(bin_eval(v, e), numpy_bin(v, e))
    e = np.array([0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0])       # monotone, not strictly
    v = np.array([-0.1, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.1])
    np.testing.assert_array_equal(bin_eval(v, e), numpy_bin(v, e))


# -- Engine.map_hist's argument conversion ----------------------------------------------
def _fake_engine(calls):
    from lightpycl_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.h = None
    eng.L = types.SimpleNamespace(lpc_map_hist=lambda *a: calls.append(a) or 0)
    return eng


def test_map_hist_points_int_and_pair():
    calls = []
    eng = _fake_engine(calls)
    lim = ((-1.0, 1.0), (-2.0, 2.0))
    pos = np.arange(12, dtype=np.float64).reshape(3, 4)
    H, xe, ye = eng.map_hist(pos, [1, 2, 3], lim, 4)
    _, xr, yr = np.histogram2d(np.zeros(0), np.zeros(0), bins=4, range=lim)
    np.testing.assert_array_equal(xe, xr)
    np.testing.assert_array_equal(ye, yr)
    assert H.shape == (4, 4) and H.dtype == np.float64
    a = calls[-1]
    assert a[1] == 0 and a[2] == 3 and a[6] == 1 and a[9] == 4 and a[11] == 4
    assert a[5] is None and a[7] is None                              # rots=None, pivot=None -> NULL
    assert a[12] == float(np.float64(2.0 / 4) * np.float64(4.0 / 4))  # dx*dy
    assert a[14] is None and a[15] is None                            # no statistics asked for
    out = eng.map_hist(pos, [1, 2, 3], lim, (3, 5), mode=1, stats=True)
    assert len(out) == 5
    H, xe, ye, cnt, H2 = out
    _, xr, yr = np.histogram2d(np.zeros(0), np.zeros(0), bins=(3, 5), range=lim)
    np.testing.assert_array_equal(xe, xr)
    np.testing.assert_array_equal(ye, yr)
    assert H.shape == cnt.shape == H2.shape == (3, 5) and cnt.dtype == np.int64
    a = calls[-1]
    assert a[1] == 1 and a[9] == 3 and a[11] == 5
    assert a[12] == float(np.float64(2.0 / 3) * np.float64(4.0 / 5))
    assert a[14] is not None and a[15] is not None
    # the planar view weighs by the power itself
    eng.map_hist(pos, [1, 2, 3], lim, (3, 5), mode=2)
    assert calls[-1][1] == 2 and calls[-1][12] == 1.0
    # the device-resident record: no points, n = 0
    eng.map_hist(None, None, lim, 4)
    assert calls[-1][2] == 0 and calls[-1][3] is None and calls[-1][4] is None


def test_map_hist_rotation_stack_and_refusals():
    from lightpycl_amd.engine import Engine
    calls = []
    eng = _fake_engine(calls)
    lim = ((-1.0, 1.0), (-1.0, 1.0))
    pos, pw = np.zeros((2, 4), np.float32), np.ones(2, np.float32)
    eng.map_hist(pos, pw, lim, 4, rots=np.eye(4))                     # one matrix: a stack of one
    assert calls[-1][6] == 1 and calls[-1][5] is not None
    eng.map_hist(pos, pw, lim, 4, rots=np.stack([np.eye(4)] * 7), pivot=[1, 2, 3, 0])
    assert calls[-1][6] == 7 and calls[-1][7] is not None
    args = Engine._map_args(pos, pw, lim, 4, 0, np.stack([np.eye(4, dtype=np.float64)] * 3), [1, 2, 3, 0])
    assert args[3].dtype == np.float32 and args[3].shape == (3, 4, 4) and args[3].flags["C_CONTIGUOUS"]
    assert args[4].dtype == np.float32 and args[4].shape == (4,)
    n = len(calls)
    for bad in (np.zeros((3, 3)), np.zeros((2, 3, 4)), np.zeros((0, 4, 4)), np.zeros(16)):
        with pytest.raises(ValueError):
            eng.map_hist(pos, pw, lim, 4, rots=bad)
    with pytest.raises(ValueError):
        eng.map_hist(pos, pw, lim, 4, mode=3)
    with pytest.raises(ValueError):
        eng.map_hist(pos, np.ones(3), lim, 4)                         # one power per point
    assert len(calls) == n                                            # a refused call reaches no library call
