"""CPU tests of the volume map: the host reference helper (tests/volume_ref.py)
over the CPU oracle -- its identity against the power budget's dissipated terms
on the cases that dissipate --, the library's own walk routine
(lpc_volume_segment_host, the code the device runs) against the helper, the
premise of the constructed slab of the GPU tests, and the library surface as
far as it runs without a device."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import budget_ref
import volume_ref
from test_budget_host import case_scene, rays_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["cube", "cube_field", "mixed"]
A_VALUES = [0.0, 1e-12, 1.0, 40.0, 5000.0]


def case_grids(name):
    """Per case: a grid over the dissipating bodies and an odd one that cuts
    them (so `outside` > 0)."""
    if name == "cube_field":
        return [volume_ref.grid_of((-25.0, -25.0, 39.0), (25.0, 25.0, 42.5), (20, 20, 4)),
                volume_ref.grid_of((-3.1, -7.3, 39.6), (9.7, 4.9, 41.1), (7, 5, 3))]
    return [volume_ref.grid_of((-5.0, -5.0, 15.0), (5.0, 5.0, 25.0), (8, 8, 8)),
            volume_ref.grid_of((-1.3, -6.1, 17.2), (6.4, 2.2, 22.9), (7, 5, 3))]


_REFS = {}


def cpu_reference(oracle_mod, name):
    if name not in _REFS:
        sc = case_scene(name)
        o, d, p = rays_of(sc)
        _REFS[name] = volume_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                       sc.ior_env, case_grids(name))
    return _REFS[name]


@pytest.mark.parametrize("name", CASES)
def test_identity(oracle_mod, name):
    """sum(voxels) + outside is the budget's dissipated, segments its n_dissipated;
    the tolerance cannot hide a segment."""
    ref = cpu_reference(oracle_mod, name)
    dis = [float(v) for it in ref["budget"]["iters"] for v in it["dissipated"][0]]
    assert len(dis) > 0
    for r in ref["refs"]:
        volume_ref.assert_condition(r, name)
        assert r.segments == len(dis) == budget_ref.totals(ref["budget"])["dissipated"]
        assert r.per_iter == [len(it["dissipated"][0]) for it in ref["budget"]["iters"]]
        want = math.fsum(dis)
        print(name, r.grid["shape"], "total", r.total(), "budget", want, "outside", r.outside(), "tol", r.tol_all())
        assert abs(r.total() - want) <= r.tol_all(), (name, r.total(), want, r.tol_all())
        assert np.array_equal(np.asarray(r.D), np.asarray(dis))
    assert abs(ref["refs"][1].outside()) > 0.0


# -- the library's routine against the helper ----------------------------------------
def host_segment(L, grid, O, E, a, D, cap=4096):
    from lightpycl_amd import _lib
    lo, hi = np.ascontiguousarray(grid["lo"]), np.ascontiguousarray(grid["hi"])
    dims = np.asarray(grid["shape"], np.int32)
    O, E = np.ascontiguousarray(O, np.float64), np.ascontiguousarray(E, np.float64)
    idx, share = np.zeros(cap, np.int64), np.zeros(cap, np.float64)
    n = ctypes.c_int64(0)
    _lib.check(L.lpc_volume_segment_host(_lib.ptr(lo), _lib.ptr(hi), _lib.ptr(dims), _lib.ptr(O), _lib.ptr(E),
                                         float(a), float(D), _lib.ptr(idx), _lib.ptr(share), cap, ctypes.byref(n)))
    assert 0 < n.value <= cap
    return idx[:n.value], share[:n.value]


def check_segment(L, grid, O, E, a, D, what):
    """Per voxel and for `outside`, the routine's shares against the helper's
    within c_r; no zero-length interval booked twice to hide one."""
    gi, gs = host_segment(L, grid, O, E, a, D)
    wi, ws = volume_ref.segment(grid, np.asarray(O, np.float64), np.asarray(E, np.float64), a, D)
    fin = np.all(np.isfinite(O)) and np.all(np.isfinite(E))
    c = volume_ref.EPS_TOL * abs(D) * max(1.0, a) * (volume_ref.kappa_of(grid, np.asarray(O, np.float64),
                                                                       np.asarray(E, np.float64)) if fin else 1.0)
    got, want = {}, {}
    for v, s in zip(gi.tolist(), gs.tolist()):
        got.setdefault(v, []).append(s)
    for v, s in zip(wi.tolist(), ws.tolist()):
        want.setdefault(v, []).append(s)
    worst = 0.0
    for v in set(got) | set(want):
        e = abs(math.fsum(got.get(v, [])) - math.fsum(want.get(v, [])))
        worst = max(worst, e)
        assert e <= c, (what, v, got.get(v), want.get(v), c)
    assert abs(math.fsum(gs.tolist()) - D) <= c, (what, "sum", math.fsum(gs.tolist()), D)
    return worst, c


@pytest.fixture(scope="module")
def lib():
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    return _lib.load()


GRID = volume_ref.grid_of((-1.5, 2.0, 10.0), (5.5, 7.0, 13.0), (7, 5, 3))


@pytest.mark.parametrize("a", A_VALUES)
def test_routine_random(lib, a):
    """2 000 random segments through a 7x5x3 grid: through it, starting or ending
    inside, wholly outside."""
    rng = np.random.default_rng(11)
    lo, hi = GRID["lo"], GRID["hi"]
    ext = hi - lo
    O = lo - 0.6 * ext + rng.random((2000, 3)) * 2.2 * ext
    E = lo - 0.6 * ext + rng.random((2000, 3)) * 2.2 * ext
    D = rng.random(2000) * 3.0 + 0.1
    kinds = {"through": 0, "inside": 0, "outside": 0}
    ratio = 0.0
    for j in range(2000):
        gi, _ = host_segment(lib, GRID, O[j], E[j], a, D[j])
        ins = [bool(np.all((X >= lo) & (X <= hi))) for X in (O[j], E[j])]
        kinds["outside" if np.all(gi < 0) else ("inside" if any(ins) else "through")] += 1
        w, c = check_segment(lib, GRID, O[j], E[j], a, D[j], ("random", a, j))
        ratio = max(ratio, w / c)
    print("a", a, kinds, "max err / c_r", ratio)
    assert min(kinds.values()) > 50, kinds


@pytest.mark.parametrize("a", A_VALUES)
def test_routine_axis_parallel(lib, a):
    """Axis-parallel segments through voxel centres, both directions, from
    outside to outside, and starting or ending inside a voxel."""
    lo, hi, shape = GRID["lo"], GRID["hi"], GRID["shape"]
    w = (hi - lo) / np.asarray(shape)
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        for i in range(shape[o1]):
            for j in range(shape[o2]):
                for s0, s1 in ((-0.7, shape[ax] + 0.6), (shape[ax] + 0.3, -0.4), (1.5, shape[ax] + 2.0),
                               (-1.0, shape[ax] - 0.5), (0.25, shape[ax] - 0.25)):
                    O, E = np.zeros(3), np.zeros(3)
                    O[o1] = E[o1] = lo[o1] + (i + 0.5) * w[o1]
                    O[o2] = E[o2] = lo[o2] + (j + 0.5) * w[o2]
                    O[ax], E[ax] = lo[ax] + s0 * w[ax], lo[ax] + s1 * w[ax]
                    gi, gs = host_segment(lib, GRID, O, E, a, 2.0)
                    inside = gi[gi >= 0]
                    assert len(np.unique(inside)) == len(inside) >= shape[ax] - 1, (ax, i, j, gi)
                    check_segment(lib, GRID, O, E, a, 2.0, ("axis", ax, i, j, s0, s1, a))


def test_routine_degenerate(lib):
    """E == O inside and outside, a NaN endpoint, a non-finite a, a NaN D."""
    ctr = np.array([2.2, 4.4, 11.1])
    v = int(volume_ref.segment(GRID, ctr, ctr, 1.0, 3.0)[0][0])
    assert v >= 0
    gi, gs = host_segment(lib, GRID, ctr, ctr, 1.0, 3.0)
    assert gi.tolist() == [v] and gs.tolist() == [3.0]
    out = np.array([9.0, 4.4, 11.1])
    gi, gs = host_segment(lib, GRID, out, out, 1.0, 3.0)
    assert gi.tolist() == [-1] and gs.tolist() == [3.0]
    for k in range(3):
        for bad in (np.nan, np.inf):
            E = ctr.copy()
            E[k] = bad
            for O_, E_ in ((ctr, E), (E, ctr)):
                gi, gs = host_segment(lib, GRID, O_, E_, 1.0, 3.0)
                assert gi.tolist() == [-1] and gs.tolist() == [3.0], (k, bad, gi, gs)
    for bad in (np.nan, np.inf):
        gi, gs = host_segment(lib, GRID, ctr, ctr + 1.0, bad, 3.0)
        assert gi.tolist() == [-1] and gs.tolist() == [3.0]
    gi, gs = host_segment(lib, GRID, ctr - 4.0, ctr + 4.0, 1.0, np.nan)
    assert len(gi) >= 3 and np.all(np.isnan(gs))
    # a far smaller than the spacing of float64 near 1: 1 - exp(-a s) would be 0 / 0
    gi, gs = host_segment(lib, GRID, ctr - 4.0, ctr + 4.0, 1e-300, 3.0)
    assert np.all(np.isfinite(gs)) and abs(math.fsum(gs.tolist()) - 3.0) <= 3.0 * 2.0 ** -50


# -- the constructed slab's premise ---------------------------------------------------
SLAB_SHAPES = [(16, 16, 8), (1, 1, 1), (33, 17, 5)]


@pytest.mark.parametrize("shape", SLAB_SHAPES)
def test_slab_premise(oracle_mod, shape):
    """Under the oracle every second-iteration ray that carries power dissipates
    in the cube along its own column, none is excluded, and the helper's shares
    are the closed form's."""
    from lightpycl_amd import _lib
    diss = 0.3
    grid = volume_ref.grid_of(volume_ref.SLAB_LO, volume_ref.SLAB_HI, shape)
    for pname, cols in volume_ref.slab_patterns(300, shape, _lib.VOLUME_LDS_ENTRIES).items():
        o, d, p = volume_ref.slab_rays(cols, shape)
        ref = volume_ref.trace(oracle_mod, volume_ref.slab_scene(diss), o, d, p, 2, 1.0, np.float32(1e3),
                               np.float32(1.0), [grid])
        r = ref["refs"][0]
        volume_ref.assert_condition(r, (shape, pname))
        assert r.per_iter == [0, len(p)], (shape, pname, r.per_iter)
        assert r.outside() == 0.0
        want = np.zeros(shape, np.float64)
        terms = {}
        for j, (O, E, a, D) in enumerate(r.rays):
            assert O[2] == 15.0 and E[2] == 25.0 and O[0] == E[0] == np.float64(o[j, 0]) and O[1] == E[1]
            assert D > 0.0
            assert a == float(np.float64(np.float32(diss)) * 10.0)
            sh, outside = volume_ref.slab_closed_form(D, a, shape[2])
            assert outside == 0.0
            for k in range(shape[2]):
                terms.setdefault((int(cols[j][0]), int(cols[j][1]), k), []).append(float(sh[k]))
        for key, t in terms.items():
            want[key] = math.fsum(t)
        assert np.all(np.abs(want - r.deposited()) <= r.tol.reshape(shape)), (shape, pname)
        assert np.count_nonzero(r.deposited()) == len(np.unique(cols, axis=0)) * shape[2]
    if shape == (16, 16, 8):
        assert "collide" in volume_ref.slab_patterns(300, shape, _lib.VOLUME_LDS_ENTRIES)


# -- the library surface, without a device -------------------------------------------
def test_host_api(lib):
    """The library exports the entry points, lpc.h declares them and states the
    rule, the ABI version stays, _lib.py binds them, the Python layers take the
    keyword, and the host entry checks its arguments."""
    from lightpycl_amd import _lib
    L = lib
    assert L.lpc_abi_version() == 4
    for name in ("lpc_trace_set_volume", "lpc_trace_volume", "lpc_volume_segment_host"):
        assert name in _lib.EXPORTED
        getattr(L, name)
    P, I64, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert _lib._PROTOS["lpc_trace_set_volume"] == [P, P, P, P]
    assert _lib._PROTOS["lpc_trace_volume"] == [P, P, I64, P, P, P]
    assert _lib._PROTOS["lpc_volume_segment_host"] == [P, P, P, P, P, F64, F64, P, P, I64, P]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lpc.h")).read())
    assert ("int lpc_trace_set_volume(lpc_handle *h, const double *lo3, const double *hi3, "
            "const int32_t *dims3);") in hdr
    assert ("int lpc_trace_volume(lpc_handle *h, double *deposited, int64_t cap, int32_t *dims3, "
            "double *outside, int64_t *segments);") in hdr
    assert "#define LPC_VOLUME_LDS_ENTRIES 1024" in hdr and _lib.VOLUME_LDS_ENTRIES == 1024
    assert "expm1(-a s) / expm1(-a)" in hdr
    assert "#define LPC_ABI_VERSION 4" in hdr
    # null handles and arguments are refused
    d3 = np.zeros(3, np.int32)
    lo, hi = np.zeros(3), np.ones(3)
    dims = np.array([2, 2, 2], np.int32)
    assert L.lpc_trace_set_volume(None, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(dims)) == -1
    assert L.lpc_trace_volume(None, None, 0, _lib.ptr(d3), None, None) == -1
    O, E = np.full(3, 0.25), np.full(3, 0.75)
    idx, share = np.zeros(8, np.int64), np.zeros(8, np.float64)
    n = ctypes.c_int64(-1)

    def seg(lo_, hi_, dims_, cap=8, np_=n):
        return L.lpc_volume_segment_host(_lib.ptr(lo_), _lib.ptr(hi_), _lib.ptr(dims_), _lib.ptr(O), _lib.ptr(E), 1.0,
                                         1.0, _lib.ptr(idx), _lib.ptr(share), cap, ctypes.byref(np_))

    assert seg(lo, hi, dims) == 0 and n.value == 2 and idx[:2].tolist() == [0, 7]
    assert seg(hi, lo, dims) == -1                                              # lo >= hi
    assert seg(lo, lo, dims) == -1
    assert seg(np.array([0.0, np.nan, 0.0]), hi, dims) == -1
    assert seg(lo, np.array([1.0, np.inf, 1.0]), dims) == -1
    for bad in ([0, 2, 2], [2, 1025, 2], [2, 2, -1]):
        assert seg(lo, hi, np.array(bad, np.int32)) == -1, bad
    assert seg(lo, hi, np.array([1024, 1024, 256], np.int32)) == -1             # 2^28 voxels
    assert seg(lo, hi, np.array([1024, 1024, 128], np.int32)) == 0              # 2^27
    assert seg(lo, hi, dims, cap=1) == 0 and n.value == 2                        # the count needed
    assert L.lpc_volume_segment_host(_lib.ptr(lo), _lib.ptr(hi), _lib.ptr(dims), _lib.ptr(O), _lib.ptr(E), 1.0, 1.0,
                                     None, None, 8, ctypes.byref(n)) == -1
    # the Python surface
    from lightpycl_amd import ledgers
    from lightpycl_amd.distributed import ShardedTrace  # noqa: F401
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import CL_Tracer
    from lightpycl_amd.pool import TracePool
    assert callable(Engine.set_volume) and callable(Engine.volume) and callable(CL_Tracer.volume_power)
    for fn in (CL_Tracer.iterative_tracer, TracePool.submit):
        assert inspect.signature(fn).parameters["volume_map"].default is None
    v = ledgers.volume_dict(dict(deposited=np.arange(24, dtype=np.float64).reshape(2, 3, 4), outside=1.5, segments=7,
                                 lo=np.zeros(3), hi=np.array([2.0, 3.0, 8.0]), shape=(2, 3, 4)))
    assert v["deposited"].shape == (2, 3, 4) and v["total"] == 276.0 + 1.5 and v["segments"] == 7
    assert [len(e) for e in v["edges"]] == [3, 4, 5] and np.array_equal(v["edges"][2], [0.0, 2.0, 4.0, 6.0, 8.0])
    assert np.array_equal(v["density"], v["deposited"] / 2.0)


class _FakeEngine:
    min_power, budget_on, surface_on, volume_on = 0.0, False, False, True

    def __init__(self, dep, outside, segments):
        self.v = dict(deposited=dep, outside=outside, segments=segments, lo=np.zeros(3), hi=np.ones(3), shape=dep.shape)

    def volume(self):
        return dict(self.v)


def test_read_ledgers_volume():
    """read_ledgers' volume key: alone as the engine gives it; with reduce= summed
    in pieces, segments rounded back to int."""
    from lightpycl_amd import ledgers
    dep = np.arange(30, dtype=np.float64).reshape(2, 3, 5)
    e = _FakeEngine(dep, 0.5, 9)
    out = ledgers.read_ledgers(e)
    assert set(out) == {"volume"} and out["volume"]["segments"] == 9
    sizes = []

    def reduce(v):
        sizes.append(len(v))
        return 2.0 * v

    out = ledgers.read_ledgers(e, reduce=reduce, iterations=3, piece=7)
    v = out["volume"]
    assert sizes == [7, 7, 7, 7, 4]
    assert np.array_equal(v["deposited"], 2.0 * dep) and v["outside"] == 1.0
    assert v["segments"] == 18 and isinstance(v["segments"], int)
