"""CPU tests of the per-ray power cutoff: the reference-side helper
(tests/cutoff_ref.py, the reference's host loop with the rule) over the CPU
oracle, the bound it documents, and the library surface
as far as it runs without a device."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import cutoff_ref
from lightpycl_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


_CACHE = {}


def _trace(oracle_mod, name, n, f):
    """(counts, per-mesh power, measured rows), culled powers per iteration, cut:
    the helper over the CPU oracle, computed once per case."""
    key = (name, n, f)
    if key not in _CACHE:
        sc = scenes.BUILDERS[name](n=n)
        o, d, p = rays_of(sc)
        cut = cutoff_ref.cut_of(p, f) if f else np.float32(0.0)
        agg, culled = cutoff_ref.aggregate(oracle_mod, None, sc.meshes, o, d, p, sc.iterations, sc.tau,
                                           sc.max_ray_len, sc.ior_env, cut)
        _CACHE[key] = (agg, culled, cut)
    return _CACHE[key]


@pytest.mark.parametrize("name,n", [("eye", 400), ("cube", 2000), ("nested_cubes", 2000), ("lens", 1000)])
def test_cut_zero_is_the_reference_loop(oracle_mod, name, n):
    """cut = 0: the helper is oracle.trace_rays, results tuples and all."""
    sc = scenes.BUILDERS[name](n=n)
    o, d, p = rays_of(sc)
    ref, rinfo = oracle_mod.trace_rays(o, d, p, sc.meshes, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env)
    got, ginfo = cutoff_ref.trace_rays(oracle_mod, o, d, p, sc.meshes, sc.iterations, sc.tau, sc.max_ray_len,
                                       sc.ior_env, cut=0.0)
    assert ginfo["counts"] == rinfo["counts"] and len(got) == len(ref)
    np.testing.assert_array_equal(ginfo["mesh_power"], rinfo["mesh_power"])
    assert ginfo["input_power"] == rinfo["input_power"]
    for a, b in zip(got, ref):
        for x, y in zip(a, b):
            assert np.asarray(x).shape == np.asarray(y).shape
            np.testing.assert_array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32))
    assert all(len(c) == 0 for c in ginfo["culled"])


@pytest.mark.parametrize("name,n,f", [("eye", 400, 1e-6), ("synthetic_dense", 2000, 1e-6), ("cube", 2000, 1e-4)])
def test_measured_power_bound(oracle_mod, name, n, f):
    """Non-negative powers, passive materials, equal iteration counts: for each
    measure mesh 0 <= M_uncut - M_cut <= total culled power (the cut trace's rays
    are a subset of the uncut trace's; the missing measured rays descend from
    culled ones).  Slack (n_measured - 1) 2^-53 M for each of the two float64 sums."""
    (cu, mu, ru), culled_u, _ = _trace(oracle_mod, name, n, 0.0)
    (cc, mc, rc), culled_c, cut = _trace(oracle_mod, name, n, f)
    assert cut > 0 and all(len(c) == 0 for c in culled_u)
    assert len(cu) == len(cc), (cu, cc)                        # the bound's precondition
    assert np.all(ru[:, 3] >= 0) and np.all(rc[:, 3] >= 0)
    allc = np.concatenate(culled_c)
    assert len(allc) > 0 and np.all(allc >= 0) and np.all(allc < cut)
    total = math.fsum(float(v) for v in allc)
    # populations: the cut trace's are a subset
    assert all(a <= b for a, b in zip(cc, cu)) and sum(cc) < sum(cu)
    u = 2.0 ** -53
    seen = 0
    for j in range(len(mu)):
        su, sc_ = ru[ru[:, 4] == j, 3], rc[rc[:, 4] == j, 3]
        if len(su) == 0 and len(sc_) == 0:
            continue
        seen += 1
        slack = (max(len(su), 1) - 1) * u * abs(mu[j]) + (max(len(sc_), 1) - 1) * u * abs(mc[j])
        print(name, "mesh", j, "M_uncut", mu[j], "M_cut", mc[j], "diff", mu[j] - mc[j], "culled", total,
              "slack", slack)
        # the float64 sums of the two traces, and their exactly rounded sums
        assert mc[j] <= mu[j] + slack
        assert mu[j] - mc[j] <= total + slack
        eu, ec = math.fsum(su.tolist()), math.fsum(sc_.tolist())
        assert ec <= eu                                          # M_cut <= M_uncut
        assert eu - ec <= total + slack
    assert seen >= 1


def test_cut_measured_rays_are_a_subset(oracle_mod):
    """The cut trace's measured rays are among the uncut trace's, bit for bit."""
    (_, _, ru), _, _ = _trace(oracle_mod, "cube", 2000, 0.0)
    (_, _, rc), _, _ = _trace(oracle_mod, "cube", 2000, 1e-4)
    have = {}
    for r in map(tuple, ru.tolist()):
        have[r] = have.get(r, 0) + 1
    for r in map(tuple, rc.tolist()):
        assert have.get(r, 0) > 0, r
        have[r] -= 1
    assert len(rc) < len(ru)


def test_negative_powers_are_judged_by_magnitude(oracle_mod):
    """nested_cubes (a negative-index material): some culled children carry
    negative power, and every culled child has |p| < cut.  The counts are the
    helper's own over the CPU oracle."""
    (counts, _, rows), culled, cut = _trace(oracle_mod, "nested_cubes", 2000, 1e-3)
    allc = np.concatenate(culled)
    assert np.any(allc < 0) and np.any(allc > 0)
    assert np.all(np.abs(allc) < cut)
    assert counts == [2000, 2978, 2905, 3901]
    assert [len(c) for c in culled] == [0, 0, 297, 495]
    assert int((allc < 0).sum()) == 1


def test_nan_is_never_culled(oracle_mod):
    """The predicate on its own: NaN is kept, -0.0 / denormals below a positive
    cut are culled, cut 0 culls nothing."""
    p = np.array([np.nan, -np.nan, 0.0, -0.0, 1e-40, -1e-40, 1e-3, -1e-3, np.inf, -np.inf], np.float32)
    with np.errstate(invalid="ignore"):
        drop = np.abs(p) < np.float32(1e-3)
        none = np.abs(p) < np.float32(0.0)
    assert drop.tolist() == [False, False, True, True, True, True, False, False, False, False]
    assert not none.any()


# -- the library surface, without a device ---------------------------------------
def test_symbols_and_signatures():
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    L = _lib.load()
    assert L.lpc_abi_version() == 4                               # appended entry points: the ABI version stays
    for name in ("lpc_trace_set_min_power", "lpc_trace_culled"):
        assert name in _lib.EXPORTED
        getattr(L, name)
    assert _lib._PROTOS["lpc_trace_set_min_power"] == [ctypes.c_void_p, ctypes.c_float]
    assert _lib._PROTOS["lpc_trace_culled"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.c_void_p]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lpc.h")).read())
    assert "int lpc_trace_set_min_power(lpc_handle *h, float min_power);" in hdr
    assert ("int lpc_trace_culled(lpc_handle *h, int64_t *count, double *power, int32_t cap, int32_t *n_iter);"
            in hdr)
    assert "#define LPC_ABI_VERSION 4" in hdr
    # the predicate lives in one place
    math_h = open(os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_math.hpp")).read()
    assert "power_culled(float child_pow, float cut)" in math_h


def test_python_surface():
    from lightpycl_amd.distributed import ShardedTrace  # noqa: F401
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import CL_Tracer
    from lightpycl_amd.pool import TracePool
    assert callable(Engine.set_min_power) and callable(Engine.culled) and callable(CL_Tracer.power_culled)
    for fn in (CL_Tracer.iterative_tracer, TracePool.submit):
        par = inspect.signature(fn).parameters["min_ray_power"]
        assert par.default == 0.0
    assert "power / ray_count" in CL_Tracer.iterative_tracer.__doc__


@pytest.mark.parametrize("bad", [-1.0, -1e-30, float("nan"), float("inf"), float("-inf")])
def test_set_min_power_rejects_bad_values(bad):
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    L = _lib.load()
    assert L.lpc_trace_set_min_power(None, ctypes.c_float(bad)) == -1      # LPC_E_ARG
    assert b"finite" in L.lpc_last_error(None)


def test_entry_points_refuse_a_null_handle():
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    L = _lib.load()
    assert L.lpc_trace_set_min_power(None, ctypes.c_float(0.0)) == -1
    assert L.lpc_trace_set_min_power(None, ctypes.c_float(1e-6)) == -1
    n = ctypes.c_int32(7)
    assert L.lpc_trace_culled(None, None, None, 0, ctypes.byref(n)) == -1
