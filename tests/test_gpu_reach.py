"""The direction-length bounds on scenes whose hits depend on them (reach_util.py).

Two pruning decisions rest on one number per ray population, its largest |D|^2:
filter_record's tiny-triangle drop ("never a candidate" while |D| <= Dcap; the
records are rebuilt with Dcap = inf when a population exceeds the cap) and the
sliver reach cull (a sliver, or a whole piece, is skipped when its dmin exceeds
the population's max |D|).  The number is computed by host_dmax2 (bounce),
k_ray_scan (set_rays, and on the copy stream for a staged batch), k_count (the
plain compaction), the tile maxima of k_shade_stage reduced in k_stage_move
(with the chunk combine), and read by sliver_launch_size and the device's Dcap
stop rule.  One ray too short in any of them and a hit of the reference is
silently missed: every case below has hits that exist only through the bound.

  1  bounce: one long ray among short ones decides the host bound
  2  set_rays + run_local: the long ray at the indices where k_ray_scan's
     reductions change hands, unsorted and sorted; a NaN component; the
     grid-stride loop's second round
  3  a staged batch behind a short one (the copy-stream scan, the hand-over)
  4  transmitted children three times as long as their parents reach tiny
     triangles: k_count, the traced path, the chunk combine, the speculated
     device-sized iteration that meets a Dcap overflow
  5  the same children reach needles: the sliver cull with a device-side bound,
     merged and separate sliver launches
  6  case 4 under a lowered cap (LPC_DCAP_MILLI) with larger triangles

Every comparison is the project's own: test_gpu_parity._cmp_bounce against the
`checker` fixture for a bounce; for a trace the reference host loop over the
checker's bounce (parity_util.ref_aggregate) -- per-iteration counts equal, the
measured rows bit for bit as a set, per-mesh power within rtol = atol = 1e-12.
Before it compares, each case asserts on the reference's output that the long
rays' cluster hits are there (at least 90 % of them; tests/test_reach_host.py
proves the constructions on the CPU oracle).

Engine.upload_arrays skips an upload of the bytes it holds, and a rebuilt scene
keeps Dcap = inf until the next upload: `_fresh` forces one, so every case
starts from the capped records.

set_rays_dev has no case of its own: it runs the same ray_scan and emitted_rays
as case 2, and the device emitters only make unit directions.
"""
import numpy as np
import pytest

import reach_util as ru
from parity_util import assert_aggregate_equal, lib_aggregate, measured_rows, ref_aggregate
from test_gpu_parity import _cmp_bounce

pytestmark = pytest.mark.gpu

MRL = ru.MAX_RAY_LEN
ITER, TAU = 6, 0.99
SHARE = 0.9
# cluster -> (control length, special length) of the emitted rays of cases 1-3
LENGTHS = dict(tiny=(12.0, 40.0), needle=(40.0, 100.0))
N_UNSORTED, N_SORTED = 4095, 4096 + 63          # below / above kSortMin
N_SECOND_ROUND = 2048 * 256 + 1                 # k_ray_scan's grid covers 2048 x 256 rays at a time

_scenes = {}


def _scene(cluster, plate=False, leg=None):
    key = (cluster, plate, leg)
    if key not in _scenes:
        sc = ru.scene(cluster, plate=plate, leg=leg)
        sc.meshes = ru.meshes_of(sc.arrs)
        sc.oracle = ru.oracle_scene(sc.arrs)
        _scenes[key] = sc
    return _scenes[key]


def _fresh(e, sc):
    """Upload the scene even if the engine holds its bytes: Dcap back to its cap."""
    e._scene_last = None
    e.upload_arrays(*sc.arrs)


def _thr(pw):
    return (1.0 - TAU) * float(np.sum(pw, dtype=np.float64))


_refs = {}


def _ref(key, oracle_mod, checker, sc, rays):
    """The reference trace of a population, computed once per module run."""
    if key not in _refs:
        _refs[key] = ref_aggregate(oracle_mod, checker[0], sc.meshes, rays[0], rays[1], rays[2], ITER, TAU, MRL,
                                   sc.ior_env)
    return _refs[key]


def _cluster_rows(sc, agg):
    rows = agg[2]
    return int(np.sum(rows[:, 4] == sc.mesh["cluster"])) if len(rows) else 0


def _same_trace(lib, ref, what):
    assert_aggregate_equal(lib, ref, what)
    np.testing.assert_allclose(lib[1], ref[1], rtol=1e-12, atol=1e-12, err_msg=what)


def _trace(e, sc, rays, reps=2):
    e.set_rays(rays[0], rays[1], rays[2], MRL, sc.ior_env)
    return lib_aggregate(e, ITER, _thr(rays[2]), reps=reps)


# ---------------------------------------------------------------------------
# 1. bounce: the host bound
@pytest.mark.parametrize("n", [300, N_SORTED])
@pytest.mark.parametrize("cluster", ["tiny", "needle"])
def test_bounce_one_long_ray_decides_the_bound(engine, checker, cluster, n):
    sc = _scene(cluster)
    short, long_ = LENGTHS[cluster]
    o4, d4, pw, ix = ru.population(sc, n, special_at=(n // 2 + 1,), special_len=long_, control_len=short)
    _fresh(engine, sc)
    z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
    g = engine.bounce(o4, d4, pw, z, pm, MRL, sc.ior_env)
    o = checker[0](sc.oracle, o4, d4, pw, z, pm, MRL, sc.ior_env)
    assert ru.cluster_hits(sc, o, ix.special) == 1 and ru.cluster_hits(sc, o) == 1
    assert np.all(o["isect_mid"][ix.control] == sc.mesh["back"])
    _cmp_bounce(g, o, checker[1])


# ---------------------------------------------------------------------------
# 2. set_rays: k_ray_scan
def _at(n):
    return [0, 63, 64, 255, 256, n - 1]


@pytest.mark.parametrize("where", range(6), ids=["first", "63", "64", "255", "256", "last"])
@pytest.mark.parametrize("n", [N_UNSORTED, N_SORTED])
@pytest.mark.parametrize("cluster", ["tiny", "needle"])
def test_set_rays_one_long_ray_at_an_index(engine, oracle_mod, checker, cluster, n, where):
    sc = _scene(cluster)
    short, long_ = LENGTHS[cluster]
    at = _at(n)[where]
    o4, d4, pw, ix = ru.population(sc, n, special_at=(at,), special_len=long_, control_len=short)
    assert ix.special.tolist() == [at]
    ref = _ref(("scan", cluster, n, at), oracle_mod, checker, sc, (o4, d4, pw))
    assert _cluster_rows(sc, ref) == 1 and ref[1][sc.mesh["cluster"]] > 0.0 and ref[1][sc.mesh["back"]] > 0.0
    _fresh(engine, sc)
    _same_trace(_trace(engine, sc, (o4, d4, pw)), ref, f"{cluster} n {n} long ray at {at}")


@pytest.mark.parametrize("cluster", ["tiny", "needle"])
def test_set_rays_nan_component_counts_as_infinite(engine, oracle_mod, checker, cluster):
    """No long ray; one bulk ray with a NaN direction component.  Its |D|^2 counts
    as +inf: the records are rebuilt and no sliver piece is culled.  The NaN ray
    itself hits nothing on either side."""
    sc = _scene(cluster)
    n = N_SORTED
    o4, d4, pw, ix = ru.population(sc, n, control_len=LENGTHS[cluster][0])
    bad = int(ix.away[len(ix.away) // 2])
    d4[bad, 1] = np.nan
    ref = _ref(("nan", cluster), oracle_mod, checker, sc, (o4, d4, pw))
    assert ref[0] == [n] and _cluster_rows(sc, ref) == 0 and ref[1][sc.mesh["back"]] > 0.0
    assert not np.any(np.isnan(ref[2]))
    _fresh(engine, sc)
    _same_trace(_trace(engine, sc, (o4, d4, pw)), ref, f"{cluster} NaN")


@pytest.mark.parametrize("cluster", ["tiny", "needle"])
def test_set_rays_long_ray_in_the_scans_second_round(engine, oracle_mod, checker, cluster):
    """n = 2048 * 256 + 1: the last ray is the only one of the grid-stride loop's
    second round, and the only long one.  The others travel inside the plane
    z = 2 and hit nothing; rays are independent, so the expected per-mesh power
    and measured rows are the reference's on the long ray plus a 1 000-ray
    sample of the others."""
    sc = _scene(cluster)
    n = N_SECOND_ROUND
    o4, d4, pw = ru.away_population(n, length=1.0)
    so, sd = ru._along_z(ru.aim_points(sc, [5]), LENGTHS[cluster][1])
    o4[n - 1, :3], d4[n - 1, :3] = so[0], sd[0]
    sample = np.concatenate([np.arange(0, n - 1, (n - 1) // 1000)[:1000], [n - 1]])
    ref = _ref(("round2", cluster), oracle_mod, checker, sc, (o4[sample], d4[sample], pw[sample]))
    assert ref[0] == [len(sample)] and len(ref[2]) == 1 and _cluster_rows(sc, ref) == 1
    _fresh(engine, sc)
    engine.set_rays(o4, d4, pw, MRL, sc.ior_env)
    lib = lib_aggregate(engine, ITER, _thr(pw), reps=1)
    assert lib[0] == [n]
    np.testing.assert_array_equal(lib[2], ref[2])
    np.testing.assert_allclose(lib[1], ref[1], rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------
# 3. a staged batch
@pytest.mark.parametrize("cluster", ["tiny", "needle"])
def test_staged_batch_with_the_long_ray_last(oracle_mod, checker, cluster):
    from lightpycl_amd.engine import Engine
    sc = _scene(cluster)
    short, long_ = LENGTHS[cluster]
    n = N_SORTED
    first = ru.population(sc, 2000, control_len=1.0, seed=1)[:3]
    second = ru.population(sc, n, special_at=(n - 1,), special_len=long_, control_len=short)[:3]
    ref1 = _ref(("stage1", cluster), oracle_mod, checker, sc, first)
    ref2 = _ref(("scan", cluster, n, n - 1), oracle_mod, checker, sc, second)
    assert _cluster_rows(sc, ref1) == 0 and _cluster_rows(sc, ref2) == 1
    e = Engine(0)
    try:
        e.upload_arrays(*sc.arrs)
        e.stage_rays(*first, MRL, sc.ior_env)
        e.stage_rays(*second, MRL, sc.ior_env)         # scanned on the copy stream, under the capped records
        for rays, ref in ((first, ref1), (second, ref2)):
            st, (c, mp) = e.run_staged(ITER, _thr(rays[2]))
            e.sync()
            lib = ([int(s.n_in) for s in st], np.asarray(mp, np.float64), measured_rows(*e.fetch_measured()))
            assert c == len(lib[2])
            _same_trace(lib, ref, f"{cluster} staged")
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 4-6. children longer than their parents
N_PLATE, CHUNK = 3000, 1000
PATHS = {
    "count": dict(env=dict(LPC_TRACED="0")),
    "traced": dict(env={}),
    "chunk-first": dict(env={}, chunk=CHUNK, at="first"),
    "chunk-last": dict(env={}, chunk=CHUNK, at="last"),
    "spec": dict(env=dict(LPC_SPEC="1"), respec=True),
    # a device-sized iteration holds at most a chunk: two chunks of 2000 and 1000, 1596 children
    "spec-chunk-first": dict(env=dict(LPC_SPEC="1"), respec=True, chunk=2 * CHUNK, at="first"),
    "slivers-side": dict(env=dict(LPC_SLIVER_MERGE="-1")),
    "slivers-side-small": dict(env=dict(LPC_SLIVER_MERGE="4000000")),
}


def _children_case(monkeypatch, oracle_mod, checker, cluster, leg, length, long_, path, what):
    """One plate scene at one emitted length on one path -> after the comparisons,
    (reference, liblpc) aggregates."""
    from lightpycl_amd.engine import Engine
    cfg = PATHS[path]
    sc = _scene(cluster, plate=True, leg=leg)
    at = range(N_PLATE - 64, N_PLATE) if cfg.get("at") == "last" else range(64)
    rays = ru.plate_population(sc, N_PLATE, at, length)
    ix = rays[3]
    if "chunk" in cfg:          # n < kSortMin: the emitted rays keep their order, chunks are index ranges
        assert (ix.plate.max() < CHUNK) if cfg["at"] == "first" else (ix.plate.min() >= N_PLATE - CHUNK)
    ref = _ref(("plate", cluster, leg, length, cfg.get("at", "first")), oracle_mod, checker, sc, rays[:3])
    assert ref[0] == [N_PLATE, len(ix.mirror) + 2 * len(ix.plate)]
    if long_:
        assert _cluster_rows(sc, ref) >= SHARE * len(ix.plate) and ref[1][sc.mesh["cluster"]] > 0.0
    else:
        assert _cluster_rows(sc, ref) == 0 and ref[1][sc.mesh["cluster"]] == 0.0
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    e = Engine(0)
    try:
        if "chunk" in cfg:
            e.set_chunk(cfg["chunk"])
        e.upload_arrays(*sc.arrs)
        lib = _trace(e, sc, rays[:3], reps=3)          # the later traces take the first's prediction
        _same_trace(lib, ref, what)
        if cfg.get("respec"):
            # the prediction is there and Dcap is back at its cap: the speculated
            # device-sized iteration meets the overflow and re-runs host-sized
            for rep in range(2):
                _fresh(e, sc)
                _same_trace(_trace(e, sc, rays[:3], reps=1), ref, f"{what} re-uploaded {rep}")
    finally:
        e.close()
    if not long_:
        assert lib[1][sc.mesh["cluster"]] == 0.0 and _cluster_rows(sc, lib) == 0
    return ref, lib


_TINY_PATHS = ["count", "traced", "chunk-first", "chunk-last", "spec", "spec-chunk-first"]


@pytest.mark.parametrize("length", [12.0, 5.0], ids=["long", "control"])
@pytest.mark.parametrize("path", _TINY_PATHS)
def test_children_reach_tiny_triangles(monkeypatch, oracle_mod, checker, path, length):
    """Emitted |D| = 12 < Dcap = 16; the plate's transmitted children are 35.9 long,
    above both the cap and L_tiny = 25, among reflected children of 12.  Control:
    emitted 5, children 14.7: the tiny mesh measures exactly 0 on both sides."""
    assert 12.0 < 16.0 < ru.child_length(12.0) and ru.child_length(5.0) < 16.0
    _children_case(monkeypatch, oracle_mod, checker, "tiny", None, length, length == 12.0, path, f"tiny {path} {length}")


_NEEDLE_PATHS = ["traced", "spec", "slivers-side", "slivers-side-small", "count"]


@pytest.mark.parametrize("length", [40.0, 20.0], ids=["long", "control"])
@pytest.mark.parametrize("path", _NEEDLE_PATHS)
def test_children_reach_needles(monkeypatch, oracle_mod, checker, path, length):
    """Emitted |D| = 40 (above Dcap: the records are rebuilt at set_rays, as
    intended) and reflected children of 40 stay below the needles' sliver_dmin =
    65.4; only the transmitted children of 120 exceed it.  The sliver cull of the
    second iteration takes its bound from the host (the first trace) and from
    the device (the speculated iterations of the later traces).  Control: emitted
    20, children 59.9."""
    assert 40.0 < 65.0 < ru.child_length(40.0) and ru.child_length(20.0) < 65.0
    _children_case(monkeypatch, oracle_mod, checker, "needle", None, length, length == 40.0, path,
                   f"needle {path} {length}")


@pytest.mark.parametrize("length", [3.0, 1.2], ids=["long", "control"])
@pytest.mark.parametrize("path", ["traced", "spec"])
def test_children_reach_tiny_triangles_under_a_lowered_cap(monkeypatch, oracle_mod, checker, path, length):
    """LPC_DCAP_MILLI = 4000: triangles with legs 4e-4 (L = 6.25; not tiny at a cap
    of 16), emitted 3 < 4, children 8.5; control emitted 1.2, children 2.2."""
    assert 3.0 < 4.0 < 6.25 < ru.child_length(3.0) and ru.child_length(1.2) < 4.0
    monkeypatch.setenv("LPC_DCAP_MILLI", "4000")
    _children_case(monkeypatch, oracle_mod, checker, "tiny", 4e-4, length, length == 3.0, path, f"cap 4 {path} {length}")
