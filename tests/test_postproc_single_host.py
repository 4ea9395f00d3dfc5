"""postproc_single (lpc_math.hpp) against postproc, on the host: the shading's
single-slot path rests on the two being equal wherever postproc_single's
`generic` flag stays clear, and on the flag being set nowhere else.

For every K in 1..16 the harness (tests/csrc/postproc_harness.cpp) runs every
written slot j0, every prev in {-2, -1, 0..K-1}, every count 0..3 and every t0
of the list below over a set of material tables, all other slots clean
(max_ray_len, -1, 0), and compares the six fields of PostOut (t_min by its bits).

Material tables: all 5^K of them up to K = 5.  From K = 6 on the full product
is out of reach (5^16 = 1.5e11), and postproc reads a table only through "is
slot j refractive (0 or 4)" at j0 and at the other slots; so the tables are a
background type in every slot (each of the five) with one slot of each other
type (each slot in turn), j0 running over every slot of each table, plus 40
tables from a fixed pseudo-random stream.  That holds every combination of: j0
of each type, no other refractive slot, exactly one (before or after j0, at
every distance), several, all.  test_every_refractive_pattern closes the gap:
all 2^K refractive / non-refractive tables for every K up to 16 -- everything
postproc can tell apart in a table -- over every j0 and t0, with prev in
{-2, 0} and counts 0 and 1 (the full prev and count ranges run over the tables
above).

t0: small, mid, the three floats on each side of max_ray_len (1 - 1e-6), that
value itself, the three floats below max_ray_len (inside EPSILON) and
max_ray_len (a count with a clean key: no hit)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "csrc", "_build", "libpostproc_harness.so")

MAX_RAY_LENS = (1000.0, 1.0, 37.5)


@pytest.fixture(scope="module")
def sweep():
    src = os.path.join(ROOT, "tests", "csrc", "postproc_harness.cpp")
    hdr = os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_math.hpp")
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "lightpycl_amd", "csrc"), src, "-o", SO], check=True)
    L = ctypes.CDLL(SO)
    F = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    I64 = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    I32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    L.postproc_single_sweep.argtypes = [ctypes.c_int32, ctypes.c_float, F, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        I64, I32]
    L.postproc_single_sweep.restype = None

    L.postproc_single_sweep_patterns.argtypes = [ctypes.c_int32, ctypes.c_float, F, ctypes.c_int, I64, I32]
    L.postproc_single_sweep_patterns.restype = None

    def run(K, max_ray_len, t0s, exhaustive, nrand=0, patterns=False):
        out = np.zeros(3, np.int64)
        bad = np.zeros(8, np.int32)
        t0s = np.ascontiguousarray(t0s, np.float32)
        if patterns:
            L.postproc_single_sweep_patterns(K, max_ray_len, t0s, len(t0s), out, bad)
        else:
            L.postproc_single_sweep(K, max_ray_len, t0s, len(t0s), int(exhaustive), nrand, out, bad)
        return int(out[0]), int(out[1]), int(out[2]), bad.tolist()
    return run


def t0_list(max_ray_len):
    m = np.float32(max_ray_len)
    edge = np.float32(m * (np.float32(1.0) - np.float32(1e-6)))
    below, above = [], []
    lo = hi = edge
    for _ in range(3):
        lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        below.append(lo)
        above.append(hi)
    near = []
    v = m
    for _ in range(3):
        v = np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
        near.append(v)
    ts = [np.float32(1e-4) * m, np.float32(0.37) * m, *below, edge, *above, *near, m]
    ts = np.unique(np.asarray(ts, np.float32))
    assert ts[-1] == m and np.all(ts[:-1] < m)
    return ts


@pytest.mark.parametrize("K", list(range(1, 17)))
def test_postproc_single_equals_postproc(sweep, K):
    for mrl in MAX_RAY_LENS:
        ts = t0_list(mrl)
        cases, fired, bad, first = sweep(K, mrl, ts, exhaustive=K <= 5, nrand=40)
        assert cases > 0
        assert bad == 0, (f"K={K} max_ray_len={mrl}: {bad} of {cases} cases; first: j0={first[1]} prev={first[2]} "
                          f"count={first[3]} t0={ts[first[4]]!r} materials(base 5)={first[5]} "
                          f"{'fields differ, flag clear' if first[6] == 1 else 'flag set, fields equal'}")
        # the flag is set somewhere exactly when a second slot can be refractive, and
        # never for the two t0 well inside max_ray_len or the slot without a hit
        assert (fired > 0) == (K > 1)
        assert fired <= cases * (len(ts) - 3) // len(ts)


@pytest.mark.parametrize("K", list(range(1, 17)))
def test_every_refractive_pattern(sweep, K):
    mrl = MAX_RAY_LENS[0]
    ts = t0_list(mrl)
    cases, fired, bad, first = sweep(K, mrl, ts, exhaustive=False, patterns=True)
    assert cases == (1 << K) * K * 2 * 2 * len(ts)
    assert bad == 0, (f"K={K}: {bad} of {cases} cases; first: j0={first[1]} prev={first[2]} count={first[3]} "
                      f"t0={ts[first[4]]!r} materials(base 5)={first[5]} "
                      f"{'fields differ, flag clear' if first[6] == 1 else 'flag set, fields equal'}")
    assert (fired > 0) == (K > 1)


def test_flag_clear_without_other_refractive_slot(sweep):
    """One mesh: no clean refractive slot exists, so the flag is never set, even
    for a hit inside EPSILON of max_ray_len."""
    for mrl in MAX_RAY_LENS:
        cases, fired, bad, _ = sweep(1, mrl, t0_list(mrl), exhaustive=True)
        assert cases > 0 and fired == 0 and bad == 0
