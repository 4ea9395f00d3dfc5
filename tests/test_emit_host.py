"""CPU tests of the device-born light sources: the arithmetic the HIP kernels share
with the host (lightpycl_amd/csrc/lpc_emit.hpp, compiled here with g++) against
numpy's generator, bit for bit, and against lightpycl_amd.light_source's host
path at the same seed, to within the final float32 rounding."""
import ctypes
import os
import subprocess

import emit_util as eu
import numpy as np
import pytest

from lightpycl_amd import light_source as lsrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "csrc", "_build", "libemit_harness.so")


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(ROOT, "tests", "csrc", "emit_harness.cpp")
    hdrs = [os.path.join(ROOT, "lightpycl_amd", "csrc", f) for f in ("lpc_emit.hpp", "lpc_math.hpp")]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "lightpycl_amd", "csrc"), src, "-o", SO], check=True)
    L = ctypes.CDLL(SO)
    F = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    D = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    U = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    LL, DBL = ctypes.c_longlong, ctypes.c_double
    L.mt_fill.argtypes = [U, ctypes.POINTER(ctypes.c_int), LL, ctypes.c_void_p]
    L.emit_hemisphere.argtypes = [D, LL, LL, LL, F, D, D, DBL, DBL, F, F, F]
    L.emit_collimated.argtypes = [D, LL, LL, LL, DBL, F, D, D, F, DBL, F, F, F]
    L.rays_rotate.argtypes = [F, F, LL, D, D]
    for f in (L.mt_fill, L.emit_hemisphere, L.emit_collimated, L.rays_rotate):
        f.restype = None
    return L


def _fill(L, key, pos, n, skip=False):
    key = np.array(key, dtype=np.uint32)
    p = ctypes.c_int(int(pos))
    out = None if skip else np.empty(n, np.float64)
    L.mt_fill(key, ctypes.byref(p), n, None if skip else out.ctypes.data_as(ctypes.c_void_p))
    return out, key, p.value


def _mat9(M):
    return np.ascontiguousarray(np.asarray(M, np.float64)[:3, :3]).reshape(9)


@pytest.mark.parametrize("n", eu.GEN_COUNTS)
def test_generator_is_numpys_bit_for_bit(harness, n):
    for name, key, pos in eu.generator_states():
        ref, rkey, rpos = eu.numpy_stream(key, pos, n)
        got, gkey, gpos = _fill(harness, key, pos, n)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (name, n)
        assert gpos == rpos and np.array_equal(gkey, rkey), (name, n, gpos, rpos)
        # a skip leaves the same state, and a fill after it is the tail of one fill
        _, skey, spos = _fill(harness, key, pos, n, skip=True)
        assert spos == rpos and np.array_equal(skey, rkey), (name, n)
        tail, _, _ = _fill(harness, skey, spos, 700)
        whole, _, _ = eu.numpy_stream(key, pos, n + 700)
        assert np.array_equal(tail.view(np.uint64), whole[n:].view(np.uint64)), (name, n)


def _draws(L, n, calls):
    """The draws of the calls-th pair of rand(n, 1) calls after np.random.seed(SEED),
    made by the shared generator."""
    key, pos = np.random.RandomState(eu.SEED).get_state()[1:3]
    d = None
    for _ in range(calls):
        d, key, pos = _fill(L, key, pos, 2 * n)
    return d


def _emit(L, n, direction, power, collimated, first=0, count=None):
    count = n - first if count is None else count
    c4 = eu.center()
    o, d, p = np.empty((count, 4), np.float32), np.empty((count, 4), np.float32), np.empty(count, np.float32)
    if not collimated:
        elev0, az0 = lsrc._pointing(direction, use_arctan2_always=False)
        L.emit_hemisphere(_draws(L, n, 1), n, first, count, c4, _mat9(lsrc._Rx(elev0)), _mat9(lsrc._Rz(az0)),
                          float(power), 1.0, o, d, p)
        return o, d, p.reshape(-1, 1)
    elev0, az0 = lsrc._pointing(direction, use_arctan2_always=True)
    row = np.zeros((1, 4)).astype(np.float32)
    row[:, 2] = 1.0
    row = np.array(np.dot(np.dot(row, lsrc._Rx(elev0)), lsrc._Rz(az0))).astype(np.float32)
    L.emit_collimated(_draws(L, n, 2), n, first, count, float(eu.DIAMETER), c4, _mat9(lsrc._Rx(elev0)),
                      _mat9(lsrc._Rz(az0)), np.ascontiguousarray(row.reshape(-1)[:3]), float(power), o, d, p)
    return o, d, p


@pytest.mark.parametrize("power", eu.POWERS)
@pytest.mark.parametrize("direction", eu.DIRECTIONS)
@pytest.mark.parametrize("n", eu.SIZES)
def test_hemisphere_matches_the_host_source(harness, n, direction, power):
    ref = eu.host_source(n, direction, power)
    o, d, p = _emit(harness, n, direction, power, collimated=False)
    what = f"hemisphere n={n} dir={direction} power={power}"
    assert np.array_equal(o, np.asarray(ref.rays_origin)), what
    eu.check_rows(d, np.asarray(ref.rays_dir), 1.0, what + " dir")
    eu.check_power(p, ref.rays_power, n, power, what)


@pytest.mark.parametrize("power", eu.POWERS)
@pytest.mark.parametrize("direction", eu.DIRECTIONS)
@pytest.mark.parametrize("n", eu.SIZES)
def test_collimated_matches_the_host_source(harness, n, direction, power):
    ref = eu.host_source(n, direction, power, collimated=True)
    o, d, p = _emit(harness, n, direction, power, collimated=True)
    what = f"collimated n={n} dir={direction} power={power}"
    eu.check_rows(o, np.asarray(ref.rays_origin), eu.origin_scale(False), what + " origin")
    eu.check_rows(d, np.asarray(ref.rays_dir), 1.0, what + " dir")
    eu.check_power(p, ref.rays_power, n, power, what)
    assert np.array_equal(p, ref.rays_power), what                   # equal powers: bit-equal for n <= 2^24


@pytest.mark.parametrize("collimated", [False, True])
@pytest.mark.parametrize("axis", ["x", "y", "z"])
@pytest.mark.parametrize("direction", eu.DIRECTIONS)
@pytest.mark.parametrize("n", eu.SIZES)
def test_rotate_matches_the_host_source(harness, n, direction, axis, collimated):
    before = eu.host_source(n, direction, 1, collimated=collimated)
    o = np.ascontiguousarray(before.rays_origin, np.float32).copy()
    d = np.ascontiguousarray(before.rays_dir, np.float32).copy()
    before.rotate_rays(axis=axis, pivot=list(eu.PIVOT), ang=eu.ROT_ANGLE)
    piv = np.array(eu.PIVOT, np.float64)
    harness.rays_rotate(o, d, n, _mat9(lsrc._rot(axis)(eu.ROT_ANGLE)), piv)
    what = f"rotate {axis} n={n} dir={direction} collimated={collimated}"
    eu.check_rows(o, before.rays_origin, eu.origin_scale(True), what + " origin")
    eu.check_rows(d, before.rays_dir, 1.0, what + " dir")


def test_shards_concatenate_to_the_whole(harness):
    n = 4099
    for collimated in (False, True):
        whole = _emit(harness, n, (1, 2, 3), 1000, collimated)
        parts = [_emit(harness, n, (1, 2, 3), 1000, collimated, first=a, count=b - a)
                 for a, b in ((0, 1000), (1000, 1063), (1063, n))]
        for k in range(3):
            assert np.array_equal(np.concatenate([q[k] for q in parts]), whole[k]), (collimated, k)


def test_cos_power_is_a_host_directivity():
    np.random.seed(3)
    a = lsrc.light_source(ray_count=257)
    np.random.seed(3)
    b = lsrc.light_source(ray_count=257, directivity=lsrc.cos_power(1))
    assert np.array_equal(a.rays_power, b.rays_power) and np.array_equal(a.rays_dir, b.rays_dir)
    np.random.seed(3)
    c = lsrc.light_source(ray_count=257, directivity=lsrc.cos_power(0))
    assert np.array_equal(c.rays_power, np.full((257, 1), np.float32(1) / np.float32(257)))
    with pytest.raises(ValueError):
        lsrc.cos_power(-1)


def test_on_device_without_a_gpu_raises_and_draws_nothing():
    from lightpycl_amd import _lib
    np.random.seed(5)
    before = np.random.get_state()
    try:
        s = lsrc.light_source(ray_count=10, on_device=True)
    except _lib.LpcError:
        after = np.random.get_state()
        assert after[2] == before[2] and np.array_equal(after[1], before[1])
        return
    assert s.__dict__.get("_dev") is not None                       # a GPU is present: a device source
    assert np.random.get_state()[2] == 20


def test_on_device_refuses_what_it_cannot_emit():
    """Raised before any draw: np.random's state stays where it was."""
    np.random.seed(5)
    before = np.random.get_state()
    with pytest.raises(TypeError, match="cos_power"):
        lsrc.light_source(ray_count=10, directivity=lambda az, el: np.cos(el) ** 2, on_device=True)
    with pytest.raises(ValueError):
        lsrc.light_source(ray_count=10, on_device=True, shard=(5, 6))
    with pytest.raises(ValueError):
        lsrc.light_source(ray_count=10, on_device=True, shard=(-1, 3))
    after = np.random.get_state()
    assert after[2] == before[2] and np.array_equal(after[1], before[1])
