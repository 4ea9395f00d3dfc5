"""Enumerated slot tables for intersect_postproc -- TEST INFRASTRUCTURE, shared by
tests/test_postproc_tables_host.py (postproc<KU> of lpc_math.hpp on the host) and
tests/test_gpu_shade_tables.py (the drop-in kernel on the device).

A row is what one ray's intersect left behind: K slots of (t, count, idx), the
ray's previous mesh and the scene's material types.  Origin 0 and direction
(1, 0, 0) make dest.x the t_min postproc settled on.

Per-slot alphabet, a = 0.37 max_ray_len, EPSILON = 1e-6 max_ray_len, in float32:

  0  a                         a tie with the nearest hit
  1  fl(a + EPSILON / 2)       inside EPSILON
  2  fl(a + EPSILON)           the boundary itself (the kernel compares with this sum)
  3  the float after it        just outside EPSILON
  4  0.8 max_ray_len           a far hit
  5  the float below max_ray_len
  6  max_ray_len               the clean key

crossed with the count's parity (1: exiting, 2: entering) and refractive (types
0, 4) or not (types 1, 2, 3): 28 symbols per slot.  On top of the symbol a hash
of (row, slot) turns some counts 1 into 3 and 2 into 0 and picks idx; a clean key
keeps its non-zero count in half the cases (a count without a key: hits beyond
max_ray_len).  The concrete type of slot j is the (v + j)-th of its class, cycled,
with a variant v in 0..5 per row (exhaustive rows) or per block of 1000 rows
(sampled rows, which also share the block's refractive pattern): the oracle takes
one material table per call, so rows come in groups of one table (`table`).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "csrc", "_build", "libpostproc_tables_harness.so")

MAX_RAY_LENS = (1000.0, 1.0, 37.5)
NT, NSYM = 7, 28
EXHAUSTIVE_K = (1, 2, 3, 4)
SAMPLED_K = (5, 8, 9, 12, 13, 16, 17, 33, 65)
SAMPLED_ROWS = 200_000
BLOCK_ROWS = 1000
REFRACTIVE, OTHER = np.array([0, 4], np.int32), np.array([1, 2, 3], np.int32)


def alphabet(mrl):
    m = np.float32(mrl)
    eps = np.float32(0.000001) * m
    a = np.float32(0.37) * m
    edge = np.float32(a + eps)
    ts = np.array([a, np.float32(a + eps / np.float32(2)), edge, np.nextafter(edge, np.float32(np.inf)),
                   np.float32(0.8) * m, np.nextafter(m, np.float32(-np.inf)), m], np.float32)
    assert np.all(np.diff(ts) > 0), "the alphabet's values are distinct and ascending"
    return ts


def _hash(r, j, salt):
    """A fixed integer mix of (row, slot): which concrete value a symbol takes."""
    x = (np.asarray(r, np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15)
         + np.asarray(j, np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(salt) * np.uint64(0x165667B19E3779F9))
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return (x >> np.uint64(8)).astype(np.int64)


def _rows(K, mrl, prev, ti, parity, refr, row0, variant):
    """Symbols (ti, parity, refr: (n, K) arrays) -> a row set.  row0: the number of
    the first row in its stream (the hash's row).  variant (n,): see above."""
    n = ti.shape[0]
    r, j = np.arange(row0, row0 + n), np.arange(K)
    ts = alphabet(mrl)
    t = ts[ti]
    h = _hash(r, j, 1)
    cnt = np.where(parity == 1, np.where(h % 4 == 0, 3, 1), np.where(h % 4 == 0, 0, 2)).astype(np.int32)
    clean = ti == NT - 1
    cnt = np.where(clean & ((h >> 2) % 2 == 0), 0, cnt).astype(np.int32)
    idx = (_hash(r, j, 2) % 100_000).astype(np.int32)
    idx = np.where(clean & (cnt == 0), -1, idx).astype(np.int32)
    vj = np.asarray(variant, np.int64)[:, None] + j[None, :]
    mat = np.where(refr, REFRACTIVE[vj % 2], OTHER[vj % 3]).astype(np.int32)
    C = np.ascontiguousarray
    # rows of one material table share a key (5 types: base 5, folded)
    table = np.zeros(n, np.int64)
    for c in range(K):
        table = (table * 5 + mat[:, c]) % 2305843009213693951
    return types.SimpleNamespace(K=K, mrl=np.float32(mrl), n=n, prev=C(prev, np.int32), mat=C(mat), t=C(t, np.float32),
                                 cnt=C(cnt), idx=C(idx), table=table)


def exhaustive_rows(K, mrl, prev):
    """Every one of the 28^K symbol tables, for one prev."""
    n = NSYM ** K
    code = np.arange(n, dtype=np.int64)
    sym = np.stack([(code // NSYM ** j) % NSYM for j in range(K)], axis=1)
    row0 = (prev + 2) * n
    return _rows(K, mrl, np.full(n, prev, np.int32), sym % NT, 1 + (sym // NT) % 2, (sym // (2 * NT)) == 1,
                 row0, _hash(np.arange(row0, row0 + n), [0], 3)[:, 0] % 6)


def exhaustive_count(K):
    return NSYM ** K * (K + 2)


def sampled_rows(K, mrl, n=SAMPLED_ROWS):
    """n rows from a fixed stream: one slot at `a`, the others active with a
    per-row probability (a few slots, a quarter, all) and then biased to the values
    near `a`; inactive slots clean.  prev: -2, -1 or a mesh."""
    rng = np.random.default_rng([20240611, K])
    q = np.array([min(1.0, 3.0 / K), 0.25, 1.0])[rng.integers(0, 3, n)][:, None]
    active = rng.random((n, K)) < q
    ti = rng.choice(NT, size=(n, K), p=[0.22, 0.18, 0.15, 0.15, 0.17, 0.06, 0.07])
    ti = np.where(active, ti, NT - 1)
    ti[np.arange(n), rng.integers(0, K, n)] = 0
    parity = rng.integers(1, 3, (n, K))
    block = np.arange(n) // BLOCK_ROWS
    nb = int(block[-1]) + 1
    pr = np.array([0.2, 0.5, 0.9])[rng.integers(0, 3, nb)][:, None]
    refr = (rng.random((nb, K)) < pr)[block]
    u = rng.random(n)
    prev = np.where(u < 0.25, -2, np.where(u < 0.375, -1, rng.integers(0, K, n))).astype(np.int32)
    return _rows(K, mrl, prev, ti, parity, refr, 0, block % 6)


def take(rows, sel):
    C = np.ascontiguousarray
    return types.SimpleNamespace(K=rows.K, mrl=rows.mrl, n=len(rows.prev[sel]), prev=C(rows.prev[sel]), mat=C(rows.mat[sel]),
                                 t=C(rows.t[sel]), cnt=C(rows.cnt[sel]), idx=C(rows.idx[sel]), table=rows.table[sel])


def with_materials(rows, mat_type):
    """The rows under one scene's material table (the device kernels read the
    uploaded scene's)."""
    out = take(rows, slice(None))
    out.mat = np.ascontiguousarray(np.broadcast_to(np.asarray(mat_type, np.int32), (rows.n, rows.K)))
    out.table = np.zeros(rows.n, np.int64)
    return out


def ray_buffers(n):
    """origin 0, direction +x as (n, 4) rows."""
    o = np.zeros((n, 4), np.float32)
    d = np.zeros((n, 4), np.float32)
    d[:, 0] = 1.0
    return o, d


FIELDS = ("isect_mid", "isect_idx", "n1", "n2", "entering", "t_min")


def oracle_postproc(oracle_mod, rows):
    """orc_intersect_postproc per row -> (n, 6) int32: hit_mesh, hit_idx, n1, n2,
    entering (-1 where the oracle leaves it unwritten: no hit), the bits of dest.x."""
    L = oracle_mod.lib()
    n, K = rows.n, rows.K
    o, d = ray_buffers(n)
    out = np.zeros((n, 6), np.int32)
    # the oracle reads one material table per call: rows grouped by theirs
    order = np.argsort(rows.table, kind="stable")
    ks = rows.table[order]
    starts = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    ends = np.concatenate((starts[1:], [n]))
    assert len(starts) <= 1024, "more material tables than the row sets are built with"
    C = np.ascontiguousarray
    for a, b in zip(starts, ends):
        s = order[a:b]
        m = len(s)
        dst = np.zeros((m, 4), np.float32)
        a1, a2, am, ai = (np.zeros(m, np.int32) for _ in range(4))
        ae = np.full(m, -1, np.int32)
        assert np.all(rows.mat[s] == rows.mat[s[0]]), "rows of one group share a material table"
        L.orc_intersect_postproc(m, C(o[s]), C(d[s]), dst, C(rows.prev[s]), a1, a2, ae, am, ai, C(rows.mat[s[0]]),
                                 C(rows.t[s]).reshape(-1), C(rows.cnt[s]).reshape(-1), C(rows.idx[s]).reshape(-1), K, rows.mrl)
        out[s] = np.stack([am, ai, a1, a2, ae, dst[:, 0].view(np.int32)], axis=1)
    return out


def harness():
    """The host build of postproc<KU> (tests/csrc/postproc_tables_harness.cpp),
    with the flags tests/test_postproc_single_host.py uses -> run(rows) ->
    (postproc<0>, postproc<KU>) as (n, 6) int32 arrays, and the library (shade_rows)."""
    src = os.path.join(ROOT, "tests", "csrc", "postproc_tables_harness.cpp")
    hdr = os.path.join(ROOT, "lightpycl_amd", "csrc", "lpc_math.hpp")
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "lightpycl_amd", "csrc"), src, "-o", SO], check=True)
    L = ctypes.CDLL(SO)
    F = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    I = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    L.postproc_tables.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_float, I, I, F, I, I, I, I]
    L.postproc_tables.restype = None
    L.postproc_tables_ku.argtypes = [ctypes.c_int32]
    L.postproc_tables_ku.restype = ctypes.c_int32
    L.shade_rows.argtypes = [ctypes.c_int64, F, F, F, F, I, I, I, I, I, F, F, F, I, F, F, F, ctypes.c_float,
                             F, F, I, F, F, I]
    L.shade_rows.restype = None

    def run(rows):
        out0 = np.zeros((rows.n, 6), np.int32)
        outku = np.zeros((rows.n, 6), np.int32)
        L.postproc_tables(rows.n, rows.K, rows.mrl, rows.prev, rows.mat.reshape(-1), rows.t.reshape(-1),
                          rows.cnt.reshape(-1), rows.idx.reshape(-1), out0.reshape(-1), outku.reshape(-1))
        return out0, outku
    run.lib = L
    return run


def outcomes(rows, out):
    """What the oracle's output `out` (oracle_postproc) shows on the rows, as boolean
    arrays.  With h the hit mesh and T = dest.x:

      entering_takeover   n2 is a mesh other than h whose count is even and whose t is
                          T: the max-min rule took an entering slot
      exiting_minmax      T is not t[h] (the max-min rule moved the hit to another
                          slot) and n2's count is odd and its t beyond fl(t[h] +
                          EPSILON): the slot taken was exiting and min-max gave n2
      exiting_alone       T is not t[h], and n2 is what the first part left (h when
                          h's count is even, else -1): an exiting slot taken, no
                          min-max slot
      n2_other            hit_mesh != n2 != -1
      tie_first           another slot holds t[h] exactly (and h is the lowest such)
      tie_second          entering_takeover, and another refractive slot holds T
                          exactly with n2 the highest such
    """
    n, K = rows.n, rows.K
    h, n2 = out[:, 0].astype(np.int64), out[:, 3].astype(np.int64)
    T = out[:, 5].view(np.float32)
    hit = h >= 0
    ar = np.arange(n)
    hs, n2s = np.where(hit, h, 0), np.where(n2 >= 0, n2, 0)
    th, tn = rows.t[ar, hs], rows.t[ar, n2s]
    cn, ch = rows.cnt[ar, n2s], rows.cnt[ar, hs]
    eps = np.float32(0.000001) * rows.mrl
    lim = (th + eps).astype(np.float32)
    moved = hit & (T != th)
    ent_take = hit & (n2 >= 0) & (n2 != h) & (cn % 2 == 0) & (tn == T)
    ex_mm = moved & (n2 >= 0) & (cn % 2 == 1) & (tn > lim)
    first_n2 = np.where(ch % 2 == 0, h, -1)
    ex_alone = moved & (n2 == first_n2)
    n2_other = hit & (n2 >= 0) & (n2 != h)
    same_h = (rows.t == th[:, None]) & hit[:, None]
    tie_first = same_h.sum(axis=1) > 1
    first_of = np.argmax(same_h, axis=1)
    refr = (rows.mat == 0) | (rows.mat == 4)
    same_T = (rows.t == T[:, None]) & refr & ent_take[:, None]
    tie_second = same_T.sum(axis=1) > 1
    last_of = K - 1 - np.argmax(same_T[:, ::-1], axis=1)
    return dict(entering_takeover=ent_take, exiting_minmax=ex_mm, exiting_alone=ex_alone, n2_other=n2_other,
                tie_first=tie_first, tie_first_lowest=~tie_first | (first_of == h),
                tie_second=tie_second, tie_second_highest=~tie_second | (last_of == n2))
