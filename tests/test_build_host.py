"""The host build of the scene records (lpc_build.hpp, build_scene_records) and a
CPU model of the walk over the records it returns, on the triangle soups of
soup_util.py: no GPU.

Structure of the records (partition into hierarchy / slivers / never, leaf refs
through xorder, one parent per node, contiguous levels of ceil(count / 8) nodes,
padded children that pass for no ray, slivers ascending in dmin), byte equality
for any thread count, the too-deep refusal, and the model walk of
tests/csrc/build_model.hpp: per (ray, run) the walk from every possible piece cut,
with filter_test plain and FMA-contracted (and, for rays that start on a
surface, the half-line form at the cut), gives brute force's (tmin, idx, count)
bit for bit -- and brute force is the CPU oracle's own slot arrays.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import soup_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
LIBSRC = os.path.join(ROOT, "lightpycl_amd", "csrc")
BUILD = os.path.join(CSRC, "_build")
DEPS = [os.path.join(CSRC, "build_model.hpp"), os.path.join(LIBSRC, "lpc_build.hpp"),
        os.path.join(LIBSRC, "lpc_math.hpp")]

DCAP, THIN_K, STACK = 16.0, 1.0, 64         # lpc_runtime.hip: dcap_init, kThin, LPC_STACK
MAX_RAY_LEN = np.float32(1e3)
N_RAYS = 4000
# the soups' seed: chosen so that the reference alone meets the conditions on the inputs
# asserted below (every case hits with >= 25 % of its rays, the small mixed ones included)
SEED = 3
CASES = [(kind, M, K) for kind in su.KINDS for M in su.SIZES for K in (1, 3)]

NODE = np.dtype([("cx", "f4", 8), ("cy", "f4", 8), ("cz", "f4", 8), ("negB", "f4", 8), ("negA", "f4", 8),
                 ("ref", "i4", 8), ("pad", "i4", 16)])
FILT = np.dtype([("cx", "f4"), ("cy", "f4"), ("cz", "f4"), ("negB", "f4"), ("negA", "f4"), ("idx", "i4"),
                 ("pad0", "i4"), ("pad1", "i4")])
SLIVER = np.dtype([(k, "f4") for k in ("v0x", "v0y", "v0z", "e2x", "e2y", "e2z", "a", "b")] + [("idx", "i4")] +
                  [(k, "f4") for k in ("e1x", "e1y", "e1z", "dmin")] + [("ax1", "i4")])


def _stale(out, srcs):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs)


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(CSRC, "build_harness.cpp")
    so = os.path.join(BUILD, "libbuild_harness.so")
    os.makedirs(BUILD, exist_ok=True)
    if _stale(so, [src] + DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + LIBSRC,
                        src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.bh_build.restype = ctypes.c_void_p
    L.bh_build.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_double] * 3 + [ctypes.c_int] * 2
    L.bh_free.argtypes = [ctypes.c_void_p]
    L.bh_error.restype = ctypes.c_char_p
    L.bh_error.argtypes = [ctypes.c_void_p]
    L.bh_sizes.argtypes = [ctypes.c_void_p] * 2
    L.bh_records.argtypes = [ctypes.c_void_p] * 11
    L.bh_classify.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_double] * 3 + [ctypes.c_void_p]
    L.bh_sphere_eval.argtypes = [ctypes.c_int] + [ctypes.c_float] * 5 + [ctypes.c_longlong] + [ctypes.c_void_p] * 3
    L.bh_model_walk.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong] + [ctypes.c_void_p] * 2 + [
        ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 4
    for fn in (L.bh_free, L.bh_sizes, L.bh_records, L.bh_classify, L.bh_sphere_eval, L.bh_model_walk):
        fn.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Records:
    """build_scene_records of a soup, its records as arrays."""

    def __init__(self, L, arrs, threads=1, stack_max=STACK, dcap=DCAP):
        self.L, self.arrs = L, arrs
        v0, v1, v2, mesh_id = arrs[:4]
        self.M = v0.shape[0]
        self.scale = su.scene_scale(arrs)
        self.h = L.bh_build(self.M, _p(v0), _p(v1), _p(v2), _p(mesh_id), dcap, self.scale, THIN_K, stack_max, threads)
        self.err = L.bh_error(self.h).decode()
        sz = np.zeros(10, np.int64)
        L.bh_sizes(self.h, _p(sz))
        assert (sz[7], sz[8], sz[9]) == (NODE.itemsize, SLIVER.itemsize, FILT.itemsize)
        nr = int(sz[3])
        self.n_slivers, self.n_thin = int(sz[5]), int(sz[6])
        self.nodes = np.zeros(sz[0], NODE)
        self.node_self = np.zeros(sz[0] if not self.err else 0, FILT)
        self.slivers = np.zeros(sz[1], SLIVER)
        self.xorder = np.zeros(sz[2], np.int32)
        self.run_lo, self.run_hi, self.run_slo, self.run_shi = (np.zeros(nr, np.int32) for _ in range(4))
        self.levels = np.zeros(sz[4], np.int32)
        self.level_off = np.zeros(nr + 1, np.int32)
        if not self.err:
            L.bh_records(self.h, _p(self.nodes), _p(self.node_self), _p(self.slivers), _p(self.xorder), _p(self.run_lo),
                         _p(self.run_hi), _p(self.run_slo), _p(self.run_shi), _p(self.levels), _p(self.level_off))

    def run_levels(self, r):
        """[(first node, count)] of run r, top down."""
        w = self.levels[self.level_off[r]:self.level_off[r + 1]]
        return [(int(w[2 * i]), int(w[2 * i + 1])) for i in range(len(w) // 2)]

    def arrays(self):
        return (self.nodes, self.node_self, self.slivers, self.xorder, self.run_lo, self.run_hi, self.run_slo,
                self.run_shi, self.levels, self.level_off)

    def classify(self):
        cls = np.zeros(self.M, np.int32)
        v0, v1, v2 = self.arrs[:3]
        self.L.bh_classify(self.M, _p(v0), _p(v1), _p(v2), DCAP, self.scale, THIN_K, _p(cls))
        return cls

    def model_walk(self, o4, d4, half):
        n, nr = o4.shape[0], self.run_lo.size
        stats = np.zeros(6, np.int64)
        bt, bi, bc = np.zeros((n, nr), np.float32), np.zeros((n, nr), np.int32), np.zeros((n, nr), np.int32)
        v0, v1, v2 = self.arrs[:3]
        o4, d4 = np.ascontiguousarray(o4, np.float32), np.ascontiguousarray(d4, np.float32)
        self.L.bh_model_walk(self.h, _p(v0), _p(v1), _p(v2), n, _p(o4), _p(d4), MAX_RAY_LEN, int(half), _p(stats),
                             _p(bt), _p(bi), _p(bc))
        return stats, bt, bi, bc

    def close(self):
        if self.h:
            self.L.bh_free(self.h)
            self.h = None


_cache = {}


def case(L, kind, M, K):
    """The soup, its records and its first-level rays, built once per module run."""
    key = (kind, M, K)
    if key not in _cache:
        arrs = su.soup(kind, M, K, seed=SEED)
        _cache[key] = (arrs, Records(L, arrs), su.aimed_rays(arrs, N_RAYS, seed=2))
    return _cache[key]


def _ids(c):
    return f"{c[0]}-M{c[1]}-K{c[2]}"


# ---------------------------------------------------------------------------
# structure
@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_records_structure(lib, c):
    arrs, R, _ = case(lib, *c)
    assert R.err == ""
    cls = R.classify()
    nr = R.run_lo.size
    lo, hi, _ = su.runs_of(arrs[3])
    np.testing.assert_array_equal(R.run_lo, lo)
    np.testing.assert_array_equal(R.run_hi, hi)
    # the lists agree with the per-triangle rules and with the counters
    assert R.n_slivers == R.slivers.size == int(np.sum(cls >= 2))
    assert R.n_thin == int(np.sum(cls == 3))
    assert R.xorder.size == int(np.sum(cls == 0))
    assert R.run_shi[-1] == R.slivers.size and R.run_slo[0] == 0
    np.testing.assert_array_equal(R.run_slo[1:], R.run_shi[:-1])
    xpos = 0                                         # the runs' positions in xorder follow each other
    parents = np.zeros(R.nodes.size, np.int32)
    roots = []
    node_at = 0
    for r in range(nr):
        tri = np.arange(R.run_lo[r], R.run_hi[r])
        sl = R.slivers[R.run_slo[r]:R.run_shi[r]]
        # slivers: of this run, each once, ascending in dmin
        np.testing.assert_array_equal(np.sort(sl["idx"]), tri[cls[tri] >= 2])
        assert np.all(np.diff(sl["dmin"]) >= 0)
        levels = R.run_levels(r)
        n_hier = int(np.sum(cls[tri] == 0))
        if n_hier == 0:
            assert levels == []
            continue
        # levels: top down, each ceil(count below / 8) nodes, contiguous, the run's
        # nodes bottom level first
        want = [-(-n_hier // 8)]
        while want[-1] > 1:
            want.append(-(-want[-1] // 8))
        assert [cnt for _, cnt in levels] == want[::-1]
        first = node_at
        for f, cnt in levels[::-1]:
            assert f == first
            first += cnt
        node_at = first
        roots.append(levels[0][0])
        for lv, (f, cnt) in enumerate(levels):
            N = R.nodes[f:f + cnt]
            used = N["negA"] != np.inf               # a padded child is a "never" record
            # children fill a node from the left; only the level's last node is padded
            assert np.all(used[:, 0]) and np.all(used[:-1])
            assert np.all(np.diff(used.astype(np.int8), axis=1) <= 0)
            assert np.all(N["ref"][~used] == ~0) and np.all(N["negB"][~used] == 0)
            ref = N["ref"][used]                     # row-major: the children in order
            if lv + 1 < len(levels):                 # the nodes of the level below, in order
                nf, ncnt = levels[lv + 1]
                np.testing.assert_array_equal(ref, np.arange(nf, nf + ncnt))
                np.add.at(parents, ref, 1)
            else:                                    # leaf refs: ~position, positions in order
                np.testing.assert_array_equal(~ref, np.arange(xpos, xpos + n_hier))
        xs = R.xorder[xpos:xpos + n_hier]
        np.testing.assert_array_equal(np.sort(xs), tri[cls[tri] == 0])   # each hierarchy triangle once, own run
        xpos += n_hier
    assert node_at == R.nodes.size and xpos == R.xorder.size
    # one parent per node, none for the run roots
    want_par = np.ones(R.nodes.size, np.int32)
    want_par[roots] = 0
    np.testing.assert_array_equal(parents, want_par)
    # "never": what is in neither list can never be hit (zero edge, or |E1||E2| Dcap < 1e-6)
    never = np.flatnonzero(cls == 1)
    e1 = np.float64(arrs[1][never, :3] - arrs[0][never, :3])
    e2 = np.float64(arrs[2][never, :3] - arrs[0][never, :3])
    prod = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    assert np.all(prod * DCAP * (1 + 1e-4) < 1e-6)


def test_padded_children_pass_for_no_ray(lib):
    """A padded child (negA = +inf) fails every evaluation of the test, for
    ordinary rays and for NaN, infinite and zero rays."""
    arrs, R, (o4, d4, _) = case(lib, "uniform", 9, 1)
    pad = R.nodes["negA"] == np.inf
    assert pad.any()
    o4, d4 = o4[:64].copy(), d4[:64].copy()
    o4[0, 0] = np.nan
    d4[1, :3] = 0
    d4[2, 1] = np.inf
    d4[3, 2] = np.nan
    out = np.zeros(64, np.float32)
    i, k = np.argwhere(pad)[0]
    N = R.nodes[i]
    for kind in (0, 1, 2):
        lib.bh_sphere_eval(kind, N["cx"][k], N["cy"][k], N["cz"][k], N["negB"][k], N["negA"][k], 64, _p(o4), _p(d4),
                           _p(out))
        assert not np.any(out <= 0), kind


def test_soups_reach_the_edges(lib):
    """The generator produces what the build's side paths need: a run with
    slivers and no hierarchy triangle, a case with >= 100 slivers and a thin
    triangle, never triangles."""
    bare = big = never = 0
    for c in CASES:
        if c[0] != "mixed":
            continue
        arrs, R, _ = case(lib, *c)
        cls = R.classify()
        never += int(np.sum(cls == 1))
        for r in range(R.run_lo.size):
            bare += R.run_levels(r) == [] and R.run_shi[r] > R.run_slo[r]
        big += R.n_slivers >= 100 and R.n_thin >= 1
    assert bare >= 1 and big >= 1 and never >= 1


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_records_independent_of_thread_count(lib, c):
    arrs, R, _ = case(lib, *c)
    for threads in (2, 5, 16):
        Q = Records(lib, arrs, threads=threads)
        try:
            assert Q.err == ""
            assert (Q.n_slivers, Q.n_thin) == (R.n_slivers, R.n_thin)
            for a, b in zip(R.arrays(), Q.arrays()):
                assert a.tobytes() == b.tobytes()
        finally:
            Q.close()


def test_too_deep_is_refused(lib):
    """7 * levels + 1 stack entries are needed (7 siblings wait per level): one
    fewer is refused with the error string, exactly that many is accepted."""
    for c in (("uniform", 4097, 1), ("clustered", 513, 3), ("coplanar", 9, 1)):
        arrs, R, _ = case(lib, *c)
        levels = max(len(R.run_levels(r)) for r in range(R.run_lo.size))
        assert levels >= {4097: 4, 513: 3, 9: 1}[c[1]]          # deep, middling and flat hierarchies
        Q = Records(lib, arrs, threads=2, stack_max=7 * levels)
        assert Q.err == "mesh hierarchy too deep"
        Q.close()
        Q = Records(lib, arrs, threads=2, stack_max=7 * levels + 1)
        assert Q.err == ""
        assert Q.nodes.tobytes() == R.nodes.tobytes()
        Q.close()


# ---------------------------------------------------------------------------
# the model walk
def _check_walk(R, o4, d4, half, what):
    stats, bt, bi, bc = R.model_walk(o4, d4, half)
    assert stats[1] >= o4.shape[0] * R.run_lo.size * (4 if half else 2)
    assert stats[0] == 0, (f"{what}: {stats[0]} of {stats[1]} model results differ from brute force; first at ray "
                           f"{stats[2]} run {stats[3]} cut level {stats[4]} variant {stats[5]}")
    return bt, bi, bc


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_model_walk_equals_brute_force(lib, oracle_mod, c):
    kind, M, K = c
    arrs, R, (o4, d4, pw) = case(lib, *c)
    n = o4.shape[0]
    bt, bi, bc = _check_walk(R, o4, d4, False, "first level")
    # brute force is the reference: the oracle's slot arrays, run r in its slot
    S = su.oracle_scene(arrs)
    z = np.zeros(n, np.int32)
    ref = oracle_mod.bounce(S, o4, d4, pw, z, np.full(n, -2, np.int32), MAX_RAY_LEN, 1.0)
    _, _, slot = su.runs_of(arrs[3])
    assert len(set(slot.tolist())) == slot.size
    np.testing.assert_array_equal(ref["isect_min_ray_len"][:, slot], bt)
    np.testing.assert_array_equal(ref["isects_count"][:, slot], bc)
    near = bt < MAX_RAY_LEN
    np.testing.assert_array_equal(ref["isect_idx_tmp"][:, slot][near], bi[near])
    empty = np.setdiff1d(np.arange(K), slot)
    assert np.all(ref["isects_count"][:, empty] == 0)
    # the case is not vacuous
    hit = ref["isects_count"].max(axis=1) > 0
    assert hit.sum() >= 0.25 * n, (int(hit.sum()), n)
    if kind == "coplanar" and M >= 7 and K == 1:
        multi = ref["isects_count"].max(axis=1) > 1
        assert multi.sum() >= 0.80 * hit.sum(), (int(multi.sum()), int(hit.sum()))
    # second level: the reference's kept children, which start on a surface
    o2, d2, _, _ = su.kept_children(ref, cap=N_RAYS)
    if K == 1:                                       # one refractive mesh: every nearest hit leaves children
        assert o2.shape[0] > 0
    if o2.shape[0]:
        _check_walk(R, o2, d2, True, "second level")


# ---------------------------------------------------------------------------
def test_build_and_walk_under_sanitizers(lib, oracle_mod, tmp_path):
    """tests/csrc/build_san_main.cpp (a stand-alone program: the build with 1 and 5
    threads, the too-deep refusal, the model walk) compiled with AddressSanitizer
    and UBSan and run as a child process: exit status 0, no report."""
    exe = os.path.join(BUILD, "build_san_main")
    src = os.path.join(CSRC, "build_san_main.cpp")
    if _stale(exe, [src] + DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + LIBSRC, src, "-o", exe], check=True)
    cases = [("mixed", 1, 3), ("mixed", 9, 3), ("mixed", 513, 3), ("coplanar", 65, 1), ("clustered", 64, 3),
             ("uniform", 4097, 1)]
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        arrs, R, (o4, d4, _) = case(lib, *c)
        o4, d4 = o4[:400], d4[:400]
        blob.append(struct.pack("<iiifdd", arrs[0].shape[0], o4.shape[0], 1, float(MAX_RAY_LEN), DCAP, R.scale))
        blob += [np.ascontiguousarray(a).tobytes() for a in (arrs[0], arrs[1], arrs[2], arrs[3], o4, d4)]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("mismatches 0") == len(cases), p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
