"""The emitted rays' counting sort (k_bkey / k_bprefix / k_bscatter / k_bsort2)
and the fused gather (k_gather_roots) at the smallest shapes at which their
blocks can go wrong, against rocPRIM's radix sort of the same key window
(LPC_BSORT=0).

A stable sort by one key has one result, so the two paths must agree on the
whole permutation.  Every ray carries a distinct power (index + 1, exact in
float32 below 2^24) and the measured rows are compared element for element, in
order: the order of each iteration's measured rows is the order of its
population, which is the emitted rays' permutation carried through the trace.
"""
import os
import re

import numpy as np
import pytest

from lightpycl_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERATIONS = 6


def _define(name):
    """The source's default of a compile-time constant: the edge sizes below fit
    the library as the tree builds it, not one built with -DLPC_BS_RPB=..."""
    src =open(os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_kernels.hip")).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, src, re.M).group(1))


B = _define("LPC_BS_RPB")           # rays per k_bkey / k_bscatter block, entries per k_bsort2 chunk
MAXB = _define("LPC_BS_MAXB")       # largest hi bucket the counting sort admits
SORT_MIN = 4096                     # kSortMin: smaller populations are traced unsorted

# partial last blocks, partial last waves, a last k_gather_roots block with fewer
# than its four packets.  A population below SORT_MIN is traced unsorted and
# reaches none of these kernels, so the "two blocks and a 63-lane last wave" and
# "three blocks and one ray" shapes are taken at the smallest whole number of
# blocks that is sorted: K blocks + 63 rays and K + 1 blocks + 1 ray, K from B
# (2 B + 63 and 3 B + 1 themselves where B >= 2048).
K = max(2, -(-SORT_MIN // B))
POINT_N = sorted({n for n in (SORT_MIN, SORT_MIN + 1, B - 1, B, B + 1) if n >= SORT_MIN}
                 | {K * B + 63, (K + 1) * B + 1})
CASES = [("point", n) for n in POINT_N] + [("cone", 20000), ("same", 5000), ("beam", 12000)]


@pytest.fixture(scope="module")
def scene():
    return scenes.synthetic(n=16, seed=7, iterations=ITERATIONS)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _hi_buckets(d4):
    """Counts of the direction key's hi digit (k_raykey: octahedral map, 8 bits
    per axis, Morton-interleaved; the hi digit is the upper four bits of both)."""
    d = d4[:, :3].astype(np.float32)
    assert np.all(d[:, 2] > 0)
    l1 = np.abs(d).sum(axis=1, dtype=np.float32)
    u = np.clip((d[:, 0] / l1 * np.float32(0.5) + np.float32(0.5)) * np.float32(256), 0, 255).astype(np.int64)
    v = np.clip((d[:, 1] / l1 * np.float32(0.5) + np.float32(0.5)) * np.float32(256), 0, 255).astype(np.int64)
    return np.bincount((u >> 4) * 16 + (v >> 4), minlength=256)


def _rays(kind, n, meshes):
    rng = np.random.default_rng(1000 + n)
    o4 = np.zeros((n, 4), np.float32)
    d4 = np.zeros((n, 4), np.float32)
    if kind == "point":             # point source, cosine-weighted hemisphere: 16 direction bits, two levels
        r, phi = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        d4[:, :3] = _unit(np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - r * r) + 1e-3], axis=1))
    elif kind == "cone":            # a narrow cone astride one hi-bucket border: buckets of several chunks
        d4[:, :3] = _unit(np.stack([rng.uniform(0.0125, 0.1125, n), rng.uniform(-0.05, 0.05, n), np.ones(n)], axis=1))
        h = _hi_buckets(d4)
        assert 2 <= np.count_nonzero(h) <= 3 and h.max() > B and h.max() <= MAXB, h[h > 0]
    elif kind == "same":            # every ray identical: one 8-bit level (lb == 0), one bucket
        d4[:, :3] = _unit([0.03, 0.02, 1.0])
    elif kind == "beam":            # one direction, origins across the scene box: 15 bits, a 7-bit lo digit
        v = np.concatenate([np.asarray(m.vertices, np.float32).reshape(-1, 4)[:, :3] for m in meshes])
        o4[:, :3] = rng.uniform(v.min(0), v.max(0), (n, 3)).astype(np.float32)
        d4[:, :3] = np.array([0.0, 0.0, 1.0], np.float32)
    pw = np.arange(1, n + 1, dtype=np.float32)
    return o4, d4, pw


def _trace(sc, o4, d4, pw, reps):
    """`reps` back-to-back traces on one fresh engine: each one's per-iteration
    stats, per-mesh power and measured record."""
    from lightpycl_amd.engine import Engine
    thr = (1.0 - sc.tau) * float(np.sum(pw, dtype=np.float64))
    out = []
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o4, d4, pw, sc.max_ray_len, sc.ior_env)
        for _ in range(reps):
            e.reset()
            stats, (cnt, mp) = e.run_local(sc.iterations, thr)
            st = [(int(s.n_in), int(s.n_reflect), int(s.n_refract), int(s.n_measured), float(s.power_next))
                  for s in stats]
            pos, p, mm = e.fetch_measured()
            assert cnt == len(p)
            out.append((st, mp.copy(), pos.copy(), p.copy(), mm.copy()))
    finally:
        e.close()
    return out


def _assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: per-mesh power")
    for x, y, k in zip(a[2:], b[2:], ("position", "power", "mesh")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: measured {k}, in order")


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_counting_sort_orders_as_radix_sort(scene, monkeypatch, kind, n):
    """Default path (counting sort where it fits) twice back to back on one
    engine, then the same rays with LPC_BSORT=0 (rocPRIM) on another: stats,
    per-mesh power and the measured rows in order are equal.  The second trace
    of the first engine shows that neither the digit counts nor any counter
    word of the first leaks into it."""
    o4, d4, pw = _rays(kind, n, scene.meshes)
    monkeypatch.delenv("LPC_BSORT", raising=False)
    first, second = _trace(scene, o4, d4, pw, reps=2)
    monkeypatch.setenv("LPC_BSORT", "0")
    radix, = _trace(scene, o4, d4, pw, reps=1)
    assert len(first[0]) >= 1 and len(first[3]) > 0, "the case measures nothing"
    _assert_same(second, first, f"{kind} {n}: second trace against the first")
    _assert_same(first, radix, f"{kind} {n}: counting sort against rocPRIM")
