"""The launches of every iteration at the shapes at which they can go wrong:

  (a) the merged sliver units' packet bounds as extra blocks of the k_roots_s
      launch (LPC_PACKET_FOLD, the default) against k_packet as a launch of its
      own (LPC_PACKET_FOLD=0): whole traces, twice per engine so that the second
      trace's chained populations are device-sized, and one bounce per size
      against the reference;
  (b) k_roots_s with its records in dynamic LDS at the piece counts where the
      tasks per packet S and the batch count change;
  (c) a device-sized iteration whose population exceeds its prediction, so that
      one block of k_roots_s, k_shade_stage and k_stage_move takes several tiles.

Expected values come from the `checker` fixture (the reference's own kernels,
bit for bit, or the CPU oracle under test_gpu_parity._cmp_bounce's bars).  Every
ray carries a distinct power (index + 1, exact in float32), and measured rows
are compared in order.  tests/test_iter_launches_host.py shows on the CPU that
the pole cases end on triangles only the sliver units hold.
"""
import os
import re

import numpy as np
import pytest

import fate_util as fu
import iter_launch_util as ilu
import soup_util as su
from lightpycl_amd import scenes
from test_gpu_compaction import _assert_agg, _read_layout, _ref_trace, _run, _setup
from test_gpu_parity import _cmp_bounce
from test_gpu_soup import MRL

pytestmark = pytest.mark.gpu

ITERATIONS = 6
# edges of a 128-ray packet and of a four-packet block of the added range (1 .. 513),
# the 16-packet k_roots_s block (1 023 .. 1 025), the smallest sorted shapes, whose
# emitted rays go through k_gather_roots and keep k_packet (4 096 .. 4 159)
SIZES = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4096, 4097, 4159)
FOLD_ON, FOLD_OFF = {}, {"LPC_PACKET_FOLD": "0"}
_KNOBS = ("LPC_PACKET_FOLD", "LPC_ROOTS_LDS", "LPC_SLIVER_MERGE", "LPC_SPEC", "LPC_HOSTPROF")


def _open(cfg):
    """A fresh engine under the policy `cfg` (the knobs are read when it opens)."""
    from lightpycl_amd.engine import Engine
    old = {k: os.environ.pop(k, None) for k in _KNOBS}
    try:
        os.environ.update(cfg)
        return Engine(0)
    finally:
        for k in _KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def scene():
    return scenes.synthetic(n=16, seed=7, iterations=ITERATIONS)


@pytest.fixture(scope="module")
def ref_scene(oracle_mod, scene):
    return oracle_mod.Scene(scene.meshes)


@pytest.fixture(scope="module")
def engines(scene):
    """One engine per policy for the whole module: fold on, fold off."""
    es = [_open(FOLD_ON), _open(FOLD_OFF)]
    try:
        for e in es:
            e.upload_meshes(scene.meshes)
        yield es
    finally:
        for e in es:
            e.close()


def _sphere_rays(n):
    """n rays from the source's centre into the nine refractive spheres (ray i at
    sphere i mod 9, inside 0.8 of its radius): nearly every ray keeps children for
    several iterations.  Power i + 1."""
    rng = np.random.default_rng([52, n])
    i = np.arange(n) % 9
    c = np.stack([(i % 3 - 1) * 30.0, (i // 3 - 1) * 30.0, np.full(n, 100.0)], axis=1)
    v = rng.normal(size=(n, 3))
    v *= (8.0 * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    if n == 1:
        v[:] = 0.0
    t = c + v
    o4 = np.zeros((n, 4), np.float32)
    d4 = np.zeros((n, 4), np.float32)
    d4[:, :3] = t / np.linalg.norm(t, axis=1, keepdims=True)
    return o4, d4, np.arange(1, n + 1, dtype=np.float32)


def _trace2(e, sc, o4, d4, pw):
    """Two back-to-back traces of the rays on `e`: each one's per-iteration stats,
    per-mesh power and measured record."""
    thr = (1.0 - sc.tau) * float(np.sum(pw, dtype=np.float64))
    e.set_rays(o4, d4, pw, sc.max_ray_len, sc.ior_env)
    out = []
    for _ in range(2):
        e.reset()
        stats, (cnt, mp) = e.run_local(sc.iterations, thr)
        st = [(int(s.n_in), int(s.n_reflect), int(s.n_refract), int(s.n_measured), float(s.power_next)) for s in stats]
        pos, p, mm = e.fetch_measured()
        assert cnt == len(p)
        out.append((st, np.array(mp), pos.copy(), p.copy(), mm.copy()))
    return out


def _assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes(), f"{what}: per-mesh power bits"
    for x, y, k in zip(a[2:], b[2:], ("position", "power", "mesh")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: measured {k}, in order")


def _fold_case(engines, checker, scene, ref_scene, rays, what, bounce_on):
    o4, d4, pw = rays
    n = len(pw)
    on = _trace2(engines[0], scene, o4, d4, pw)
    off = _trace2(engines[1], scene, o4, d4, pw)
    _assert_same(on[0], off[0], f"{what}: fold on against fold off, first trace")
    _assert_same(on[1], off[1], f"{what}: fold on against fold off, second trace")
    _assert_same(on[1], on[0], f"{what}: second trace against the first")
    # one of the two policies against the reference
    z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
    g = engines[bounce_on].bounce(o4, d4, pw, z, pm, scene.max_ray_len, scene.ior_env)
    o = checker[0](ref_scene, o4, d4, pw, z, pm, scene.max_ray_len, scene.ior_env)
    _cmp_bounce(g, o, checker[1])
    return on[0], o


@pytest.mark.parametrize("n", SIZES)
def test_fold_on_equals_fold_off(engines, checker, scene, ref_scene, n):
    """Rays into the refractive spheres: the emitted population is n rays (below
    4 096 it takes k_roots_s host-sized, from there k_gather_roots), its children
    chain through k_roots_s, device-sized in the second trace."""
    first, _ = _fold_case(engines, checker, scene, ref_scene, _sphere_rays(n), f"spheres {n}", SIZES.index(n) % 2)
    st = first[0]
    assert len(st) >= 3 and st[1][0] > 0 and st[2][0] > 0, st      # chained populations exist
    assert len(first[3]) > 0, "the case measures nothing"


@pytest.mark.parametrize("n", ilu.POLE_SIZES)
def test_fold_at_the_pole(engines, checker, scene, ref_scene, n):
    """Rays at the hemisphere's pole: some end on triangles with E1 x E2 = 0, which
    only the sliver units test, from the packet bounds the folded range wrote."""
    first, o = _fold_case(engines, checker, scene, ref_scene, ilu.pole_rays(ref_scene, n), f"pole {n}",
                          ilu.POLE_SIZES.index(n) % 2)
    assert ilu.nearest_on_zero_cross(ref_scene, o) > 0
    assert first[0][0][3] == n                                      # every ray measured on the hemisphere


@pytest.mark.parametrize("cfg", [{"LPC_SLIVER_MERGE": "-1"}, {"LPC_SLIVER_MERGE": "4000000"}, {"LPC_ROOTS_LDS": "0"}],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_other_policies_keep_their_results(engines, checker, scene, ref_scene, cfg):
    """The side-stream policies keep k_packet and k_slivers; LPC_ROOTS_LDS=0 asks
    for a full batch's LDS.  Traces equal the default policy's, a bounce the
    reference's."""
    e = _open(cfg)
    try:
        e.upload_meshes(scene.meshes)
        for rays, what in ((_sphere_rays(129), "spheres 129"), (ilu.pole_rays(ref_scene, 513), "pole 513"),
                           (_sphere_rays(4159), "spheres 4159")):
            o4, d4, pw = rays
            n = len(pw)
            got = _trace2(e, scene, o4, d4, pw)
            want = _trace2(engines[0], scene, o4, d4, pw)
            _assert_same(got[0], want[0], f"{cfg} {what}: first trace")
            _assert_same(got[1], want[1], f"{cfg} {what}: second trace")
            z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
            g = e.bounce(o4, d4, pw, z, pm, scene.max_ray_len, scene.ior_env)
            _cmp_bounce(g, checker[0](ref_scene, o4, d4, pw, z, pm, scene.max_ray_len, scene.ior_env), checker[1])
    finally:
        e.close()


# ---------------------------------------------------------------------------
# (b) piece tables.  One-triangle meshes: a run of one hierarchy triangle is one
# piece at every cut, so F such meshes are F pieces, no gate.  A gated table: one
# mesh of T coplanar right triangles, cut at its leaf level (ceil(T / 8) pieces,
# one group).  Mesh 0 also holds needles, so the launch has sliver units and the
# packet bounds are folded in.
N_PIECE_RAYS = 1237                 # 20 packets: two 16-packet blocks at S = 1, three packet-bound blocks
PIECES = [("fillers", 64), ("fillers", 65), ("fillers", 128), ("fillers", 129), ("fillers", 1024), ("fillers", 1025),
          ("gated", 65), ("gated", 129)]


def _right_triangles(M, rng):
    """M axis-aligned right triangles of leg 2 at distinct 1/4-grid positions of a
    20-box, in planes z = 0, 1, .. (hierarchy triangles, as the coplanar soup's)."""
    cells = rng.permutation(72 * 72 * 8)[:M]
    p = np.stack([(cells % 72 - 40) / 4.0, (cells // 72 % 72 - 40) / 4.0, (cells // (72 * 72)).astype(np.float64)],
                 axis=1)
    return p, p + np.array([2.0, 0.0, 0.0]), p + np.array([0.0, 2.0, 0.0])


def _needles(M, rng):
    c = rng.uniform(-8.0, 8.0, (M, 3))
    e1 = rng.normal(size=(M, 3))
    e2 = e1 * rng.uniform(0.3, 1.5, (M, 1)) + 1e-5 * np.linalg.norm(e1, axis=1, keepdims=True) * rng.normal(size=(M, 3))
    return c, c + e1, c + e2


def _piece_scene(kind, pieces):
    rng = np.random.default_rng([63, pieces, kind == "gated"])
    nn = 24
    if kind == "fillers":
        a, b, c = _right_triangles(pieces, rng)
        ids = np.arange(pieces)
        K = pieces
    else:
        a, b, c = _right_triangles(8 * pieces - 3, rng)     # ceil(T / 8) leaves
        ids = np.zeros(8 * pieces - 3, np.int64)
        K = 1
    na, nb, nc = _needles(nn, rng)
    v = [np.concatenate((x, y)) for x, y in ((na, a), (nb, b), (nc, c))]
    mesh_id = np.concatenate((np.zeros(nn, np.int64), ids)).astype(np.int32)
    # mesh 0 refractive, the others mirrors and terminators
    return (su._rows(v[0]), su._rows(v[1]), su._rows(v[2]), mesh_id) + su.materials(K, mats=((0, 1.5, 0.0, 0.02),
                                                                                            (1, 1.0, 0.9, 0.0),
                                                                                            (2, 1.0, 0.0, 0.0)))


@pytest.mark.parametrize("kind,pieces", PIECES, ids=[f"{k}-{p}" for k, p in PIECES])
def test_piece_tables_at_the_lds_edges(checker, capfd, kind, pieces):
    """S = ceil(pieces / 64) goes 1 -> 2 -> 3 at 64 / 65 and 128 / 129, the table
    takes a second batch at 1 025; the records' LDS is sized by each.  The launch
    reports its table (LPC_HOSTPROF), so the case is the one it says it is."""
    arrs = _piece_scene(kind, pieces)
    o4, d4, pw = su.aimed_rays(arrs, N_PIECE_RAYS, seed=3, sigmas=(5.0, 30.0), lengths=(1.0,))
    z, pm = np.zeros(N_PIECE_RAYS, np.int32), np.full(N_PIECE_RAYS, -2, np.int32)
    e = _open({"LPC_HOSTPROF": "1"})
    try:
        e.upload_arrays(*arrs)
        capfd.readouterr()
        g = e.bounce(o4, d4, pw, z, pm, MRL, 1.0)
        err = capfd.readouterr().err
    finally:
        e.close()
    m = re.search(r"roots: n (\d+) packets (\d+) pieces (\d+) groups (\d+) S (\d+)", err)
    assert m, err
    got = tuple(int(x) for x in m.groups())
    want_groups = 1 if kind == "gated" else 0
    assert got == (N_PIECE_RAYS, 20, pieces, want_groups, -(-min(pieces, 1024) // 64)), got
    o = checker[0](su.oracle_scene(arrs), o4, d4, pw, z, pm, MRL, 1.0)
    hit = o["isects_count"].max(axis=1) > 0
    assert hit.sum() >= 0.25 * hit.size, int(hit.sum())
    assert np.sum(o["isect_idx"][o["isect_mid"] >= 0] < 24) > 0, "no ray ends on a needle"
    _cmp_bounce(g, o, checker[1])


# ---------------------------------------------------------------------------
# (c) a device-sized iteration that outgrows its prediction.  A trace of N rays of
# which one keeps one child predicts an iteration 2 of one ray; the next trace, N
# rays again, keeps `children` of them: its iteration 2 is launched for one ray
# (one block of k_roots_s, of k_shade_stage and of k_stage_move, one block of
# packet bounds) and runs on `children`, so each block strides over the tiles.
CHILDREN = (255, 256, 257, 65537)


def _fates(n, matched, mirror):
    f = np.full(n, fu.FATES.index("terminator"), np.int32)
    step = n // (matched + mirror)
    at = np.arange(matched + mirror) * step
    f[at[:matched]] = fu.FATES.index("matched")
    f[at[matched:]] = fu.FATES.index("mirror")
    return f


@pytest.mark.parametrize("children", CHILDREN)
def test_device_sized_iteration_beyond_its_prediction(oracle_mod, checker, children):
    matched, mirror = children // 2, children % 2
    n = 2 * (matched + mirror) + 7                  # terminators between the rays that keep children
    sc = fu.layout(4)                               # ceiling and floor measure every child
    big = fu.rays(sc, _fates(n, matched, mirror))
    small = fu.rays(sc, _fates(n, 0, 1))
    T = _ref_trace(oracle_mod, checker, ("iter_launches", children), sc, big)
    assert T["agg"][0] == [n, children], T["agg"][0]
    ek = fu.ray_key(big[0][:, :2])
    a = _open({"LPC_SPEC": "0"})
    try:
        L = _read_layout(a, sc, big)                # the population of iteration 2, host-sized
        pop = fu.parents_of(fu.ray_key(L.origin[:, :2]), ek)
        _setup(a, sc, big)
        first, agg, rec = _run(a)
    finally:
        a.close()
    assert len(pop) == children
    _assert_agg(agg, T, checker[1], f"host-sized, {children} children")
    b = _open({"LPC_SPEC": "1"})
    try:
        _setup(b, sc, small)
        st, _, _ = _run(b)
        assert [s[0] for s in st] == [n, 1], st     # the prediction: iteration 2 holds one ray
        _setup(b, sc, big)
        got, aggb, recb = _run(b)
    finally:
        b.close()
    assert got == first, (got, first)
    _assert_agg(aggb, T, checker[1], f"device-sized, {children} children")
    for x, y in zip(recb, rec):
        np.testing.assert_array_equal(x, y)
    # iteration 2's part of the record lists the parents in the population's order,
    # reflected children (ceiling) before refracted ones (floor)
    m1 = first[0][3]
    assert first[1][3] == children and len(recb[1]) == m1 + children
    np.testing.assert_array_equal(fu.parents_of(fu.ray_key(recb[0][m1:, :2]), ek), pop)
    np.testing.assert_array_equal(recb[2][m1:], np.where(np.arange(children) < first[0][1], sc.ceiling, sc.floor))
