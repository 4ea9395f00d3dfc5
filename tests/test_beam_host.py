"""CPU tests of the beam analysis: the elevation arithmetic shared with the HIP
kernels (lpc_math.hpp elev_cos, compiled for the host) against numpy's, and the
selection driver lightpycl_amd.beam.half_power over a numpy stand-in for the
device passes."""
import ctypes
import os
import subprocess

import beam_ref
import numpy as np
import pytest

from lightpycl_amd import beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "csrc", "_build", "libelev_harness.so")


@pytest.fixture(scope="module")
def elev_eval():
    src = os.path.join(ROOT, "tests", "csrc", "elev_harness.cpp")
    hdr = os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_math.hpp")
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "lightpycl_amd", "csrc"), src, "-o", SO], check=True)
    L = ctypes.CDLL(SO)
    F = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    D = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.elev_eval.argtypes = [F, ctypes.c_longlong, D, D, D]
    L.elev_eval.restype = None

    def run(pos4, pole):
        pos4 = np.ascontiguousarray(pos4, np.float32)
        n = pos4.shape[0]
        c, e = np.zeros(n), np.zeros(n)
        L.elev_eval(pos4, n, np.ascontiguousarray(pole, np.float64), c, e)
        return c, e
    return run


def _cosine_inputs():
    rng = np.random.default_rng(7)
    rnd = (rng.normal(size=(10_000, 4)) * rng.choice([1e-3, 1.0, 30.0, 1e4], (10_000, 1))).astype(np.float32)
    rnd[:5000, 3] = 0.0                                           # the device record's rows: w = 0
    axes = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 2, 0, 0], [0, -3, 0, 0], [0, 0, 0.5, 0], [0, 0, -7, 0],
                     [0, 0, 0, 1], [-0.0, 0, 5, 0]], np.float32)
    tiny = (rng.normal(size=(64, 4)) * 1e-40).astype(np.float32)  # denormals: squares underflow to 0
    small = (rng.normal(size=(64, 4)) * 1e-20).astype(np.float32)  # squares are denormal
    huge = (rng.normal(size=(64, 4)) * 1e30).astype(np.float32)   # squares overflow to inf
    zero = np.zeros((1, 4), np.float32)
    return np.concatenate([rnd, axes, tiny, small, huge, zero])


@pytest.mark.parametrize("pole", [[0, 0, 1, 0], [1, 0, 0, 0], [0, -1, 0, 0]])
def test_cosine_is_numpys_bit_for_bit(elev_eval, pole):
    """For an axis-aligned pole the cosine is exact, so lpc_math.hpp's must equal
    numpy's dot(pos / norm(pos, axis=1), pole) bit for bit: same float32 norm (the
    sum order of add.reduce over a row), same float32 division."""
    pos = _cosine_inputs()
    with np.errstate(all="ignore"):
        ref = np.dot(pos / np.linalg.norm(pos, axis=1)[:, None], pole)
        ref_e = np.arccos(ref)
    assert ref.dtype == np.float64
    c, e = elev_eval(pos, pole)
    nan = np.isnan(ref)
    assert nan[-1] and np.isnan(c[-1]) and np.isnan(e[-1])        # the zero row
    assert np.array_equal(np.isnan(c), nan)
    assert np.array_equal(c[~nan].view(np.uint64), ref[~nan].view(np.uint64))
    assert (~nan).sum() > 10_000
    # the elevation: two acos implementations, a few ulp(pi) at the most; never -0, never negative
    ok = np.isfinite(ref_e)
    assert np.array_equal(np.isfinite(e), ok)
    assert np.max(np.abs(e[ok] - ref_e[ok])) <= 4 * np.spacing(np.pi)
    assert not np.signbit(e[ok]).any()
    k = beam.key_of(e[ok])
    order = np.argsort(e[ok], kind="stable")
    assert np.all(k[order][1:] >= k[order][:-1])                  # the key is monotone in e


# -- beam.half_power over the numpy stand-in -----------------------------------------
def _descent(e, p, **kw):
    P = beam_ref.NumpyPasses(e, p, **kw)
    return beam.half_power(P.scan, P.digit_pass, P.power_below)


def _direct(e, p):
    """Sort and cumsum over the groups of equal elevation, written out plainly."""
    e = np.asarray(e, np.float64)
    p = np.asarray(np.asarray(p, np.float32), np.float64)
    groups = sorted(set(e.tolist()))
    cum, acc = [], 0.0
    for g in groups:
        acc += float(p[e == g].sum())
        cum.append(acc)
    half = sum(p.tolist()) / 2.0
    j = next((i for i, c in enumerate(cum) if c >= half), len(groups) - 1)
    if j > 0 and abs(cum[j - 1] - half) <= abs(cum[j] - half):
        j -= 1
    return groups[j], cum[j]


def _check(e, p):
    r = _descent(e, p)
    ge, gc = _direct(e, p)
    total = float(np.asarray(p, np.float32).astype(np.float64).sum())
    assert r.elevation == ge
    assert r.cum_power == pytest.approx(gc, rel=1e-12, abs=0.0)
    assert r.total == pytest.approx(total, rel=1e-12)
    s = beam_ref.half_power_sorted(e, p)
    assert s.elevation == ge and s.cum_power == pytest.approx(gc, rel=1e-12, abs=0.0)
    return r


@pytest.mark.parametrize("n", [1, 2, 3])
def test_half_power_tiny(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        _check(rng.uniform(0, np.pi, n), rng.uniform(0.1, 1.0, n).astype(np.float32))
    r = _check(np.arange(1, n + 1) * 0.25, np.ones(n, np.float32))
    assert r.passes == 6                                         # ceil(64 / 11)


def test_half_power_all_elevations_equal():
    r = _check(np.full(100, 0.75), np.linspace(1, 2, 100).astype(np.float32))
    assert r.elevation == 0.75 and r.cum_power == pytest.approx(r.total, rel=1e-12)
    r = _check(np.zeros(5), np.ones(5, np.float32))               # on the pole: key 0
    assert r.elevation == 0.0 and r.key == 0


def test_half_power_tie_at_half_takes_the_lower():
    e = np.array([0.1, 0.2, 0.3, 0.4])
    r = _check(e, np.array([1, 1, 1, 1], np.float32))             # C = 1 2 3 4, half = 2: exact hit
    assert r.elevation == 0.2 and r.cum_power == 2.0
    r = _check(e, np.array([1, 2, 1, 0], np.float32))             # C = 1 3 4 4, half = 2: 1 and 3 tie
    assert r.elevation == 0.1 and r.cum_power == 1.0
    r = _check(np.array([0.5, 0.5, 0.9, 0.9]), np.array([1, 1, 3, 1], np.float32))   # groups C = 2 6, half 3
    assert r.elevation == 0.5 and r.cum_power == 2.0


def test_half_power_random_and_zero_powers():
    rng = np.random.default_rng(11)
    e = np.arccos(rng.uniform(-1, 1, 5000))
    p = rng.uniform(0, 1, 5000).astype(np.float32)
    _check(e, p)
    e[rng.integers(0, 5000, 700)] = e[rng.integers(0, 5000, 700)]  # repeated elevations
    _check(e, p)
    p[rng.random(5000) < 0.4] = 0.0                                # powers with zeros
    _check(e, p)
    p[:] = 0.0
    p[[17, 4000]] = 1.0                                           # only two rays carry power: a tie
    r = _check(e, p)
    assert r.elevation == min(e[17], e[4000])
    # other pass widths reach the same ray
    P = beam_ref.NumpyPasses(e, p)
    for bits in (1, 5, 8, 12):
        assert beam.half_power(P.scan, P.digit_pass, P.power_below, bits=bits).key == r.key
    with pytest.raises(ValueError):
        beam.half_power(P.scan, P.digit_pass, P.power_below, bits=13)


def test_half_power_ends_on_an_existing_key_when_pass_sums_disagree():
    """Atomic order is not fixed: the sums of two passes over the same rays may
    differ in their last bits.  The descent must still end on a ray that exists,
    next to the exact answer."""
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        e = np.arccos(rng.uniform(-1, 1, n))
        if trial % 3 == 0:
            e = np.round(e, 1)                                     # many ties
        p = rng.uniform(0, 1, n).astype(np.float32)
        if trial % 4 == 0:                                        # half falls exactly on a cumulative value
            p = np.ones(n, np.float32)
        r = _descent(e, p, perturb=np.random.default_rng(trial))
        ue = np.unique(e)
        assert r.elevation in ue
        exact = beam_ref.half_power_sorted(e, p)
        i, j = np.searchsorted(ue, r.elevation), np.searchsorted(ue, exact.elevation)
        assert abs(int(i) - int(j)) <= 1
        assert r.cum_power == pytest.approx(
            float(np.asarray(p, np.float64)[e <= r.elevation].sum()), rel=1e-12)


def test_half_power_negative_power_asks_for_the_host_path():
    e = np.array([0.1, 0.2, 0.3])
    with pytest.raises(beam.NonMonotonePower):
        _descent(e, np.array([1.0, -0.5, 1.0], np.float32))
    with pytest.raises(beam.NonMonotonePower):
        _descent(e, np.array([1.0, np.nan, 1.0], np.float32))
    assert issubclass(beam.NonMonotonePower, ValueError)
    with pytest.raises(ValueError):
        _descent(np.array([np.nan]), np.array([1.0], np.float32))  # no valid ray
    # invalid rays are left out and counted
    P = beam_ref.NumpyPasses(np.array([0.1, np.nan, 0.3]), np.array([1, 100, 1], np.float32))
    s = P.scan()
    assert (s.n_valid, s.n_invalid, s.total_power) == (2, 1, 2.0)
    assert beam.half_power(P.scan, P.digit_pass, P.power_below).elevation == 0.1
