"""The constructions of reach_util.py proved on the reference alone (the CPU
oracle and the host build of the filter records): no GPU.  What the GPU cases of
tests/test_gpu_reach.py rely on -- that a special ray's hit exists only because
of its length, that the triangle it hits is one the direction-length bounds
decide about -- holds here, so none of them can go vacuous.

Shares, not exact counts: at least 90 % of the special rays hit their cluster
(the oracle gives 100 %), and no control ray does.
"""
import numpy as np
import pytest

import reach_util as ru
from test_build_host import DCAP, THIN_K, Records, _p, lib  # noqa: F401  (lib: a fixture)

SHARE = 0.9
# (cluster, leg, Dcap, control length, special length): the lengths the GPU cases use
CLUSTERS = [("tiny", None, 16.0, 12.0, 40.0), ("needle", None, 16.0, 40.0, 100.0), ("tiny", 4e-4, 4.0, 3.0, 9.0)]
# (cluster, leg, Dcap, control emitted length, emitted length) of the plate scenes
PLATES = [("tiny", None, 16.0, 5.0, 12.0), ("needle", None, 16.0, 20.0, 40.0), ("tiny", 4e-4, 4.0, 1.2, 3.0)]


def _bounce(oracle_mod, sc, o4, d4):
    n = o4.shape[0]
    return oracle_mod.bounce(ru.oracle_scene(sc.arrs), o4, d4, np.ones(n, np.float32), np.zeros(n, np.int32),
                             np.full(n, -2, np.int32), ru.MAX_RAY_LEN, sc.ior_env)


def _classify(L, sc, dcap):
    from soup_util import scene_scale
    v0, v1, v2 = sc.arrs[:3]
    cls = np.zeros(v0.shape[0], np.int32)
    L.bh_classify(v0.shape[0], _p(v0), _p(v1), _p(v2), dcap, scene_scale(sc.arrs), THIN_K, _p(cls))
    return cls


@pytest.mark.parametrize("cluster,leg,dcap,short,long_", CLUSTERS)
def test_special_rays_hit_and_control_rays_do_not(oracle_mod, cluster, leg, dcap, short, long_):
    sc = ru.scene(cluster, leg=leg)
    assert short < sc.L[0] and sc.L[1] < long_
    for n, at in ((300, (17,)), (4159, (0, 63, 64, 255, 256, 4158))):
        o4, d4, pw, ix = ru.population(sc, n, special_at=at, special_len=long_, control_len=short)
        out = _bounce(oracle_mod, sc, o4, d4)
        assert ru.cluster_hits(sc, out, ix.special) >= SHARE * len(ix.special)
        assert ru.cluster_hits(sc, out) == ru.cluster_hits(sc, out, ix.special)        # no control, no bulk ray
        assert len(ix.control) == 32 and np.all(out["isect_mid"][ix.control] == sc.mesh["back"])
        assert np.all(out["isect_mid"][ix.away] == -1) and len(ix.away) > n // 8
        # one ray decides the bound: every other direction is shorter than the control length
        dl = np.linalg.norm(np.float64(d4[:, :3]), axis=1)
        assert np.all(np.delete(dl, ix.special) <= short * (1 + 1e-6))
        assert cluster == "needle" or short <= dcap * 0.999
    # all 64 triangles, at the two lengths and just around the threshold
    for length, want in ((short, 0), (0.97 * sc.L[0], 0), (1.03 * sc.L[1], 64), (long_, 64)):
        o, d = ru._along_z(ru.aim_points(sc, np.arange(64)), length)
        hits = ru.cluster_hits(sc, _bounce(oracle_mod, sc, ru._rows(o), ru._rows(d)))
        assert (hits == 0) if want == 0 else (hits >= SHARE * 64), (length, hits)


@pytest.mark.parametrize("leg,dcap", [(None, 16.0), (4e-4, 4.0)])
def test_tiny_triangles_are_never_under_the_cap_only(lib, leg, dcap):  # noqa: F811
    for plate in (False, True):
        sc = ru.scene("tiny", plate=plate, leg=leg)
        capped, free = _classify(lib, sc, dcap), _classify(lib, sc, np.inf)
        assert np.all(capped[sc.tris] == 1), "never a candidate while |D| <= Dcap"
        assert np.all(free[sc.tris] != 1), "a candidate once the records are rebuilt"
        others = np.setdiff1d(np.arange(len(capped)), sc.tris)
        assert np.all(capped[others] == 0) and np.all(free[others] == 0)      # the large surfaces: hierarchy triangles
        if dcap != DCAP:
            assert np.all(_classify(lib, sc, DCAP)[sc.tris] != 1)             # too large for the default cap's rule
        assert dcap < sc.L[0]


@pytest.mark.parametrize("plate,short,long_", [(False, 40.0, 100.0), (True, 40.0, ru.child_length(40.0))])
def test_needles_are_slivers_between_the_two_lengths(lib, plate, short, long_):  # noqa: F811
    sc = ru.scene("needle", plate=plate)
    for dcap in (DCAP, np.inf):
        assert np.all(_classify(lib, sc, dcap)[sc.tris] == 2)
    R = Records(lib, sc.arrs, dcap=np.inf)
    try:
        assert R.err == ""
        sl = R.slivers[np.isin(R.slivers["idx"], sc.tris)]
        assert len(sl) == len(sc.tris)
        # sliver_dmin: above every short length of the GPU cases, below the threshold the
        # reference has (1e-6 / |E1 x E2|), itself below the special length
        assert short < sl["dmin"].min() and sl["dmin"].max() < sc.L[0] and sc.L[1] < long_
        assert sl["dmin"].min() > 0.97 * sc.L[0]                               # and tight: a cull the lengths can reach
    finally:
        R.close()


@pytest.mark.parametrize("cluster,leg,dcap,short,long_", PLATES)
def test_plate_children_reach_the_cluster_by_their_length(oracle_mod, cluster, leg, dcap, short, long_):
    sc = ru.scene(cluster, plate=True, leg=leg)
    got = {}
    for length in (short, long_):
        o4, d4, pw, ix = ru.plate_population(sc, 3000, range(64), length)
        assert ru.cluster_hits(sc, _bounce(oracle_mod, sc, o4, d4)) == 0          # the emitted rays meet the plate first
        meas = []
        _, info = oracle_mod.trace_rays(o4, d4, pw, ru.meshes_of(sc.arrs), 6, 0.99, ru.MAX_RAY_LEN, sc.ior_env,
                                        keep_results=False, measured_out=meas)
        assert info["counts"] == [3000, len(ix.mirror) + 2 * len(ix.plate)]
        got[length] = ([int(np.sum(m[2] == sc.mesh["cluster"])) for m in meas], info["mesh_power"][sc.mesh["cluster"]])
    assert got[short] == ([0, 0], 0.0)
    assert got[long_][0][0] == 0 and got[long_][0][1] >= SHARE * 64 and got[long_][1] > 0.0
    # emitted rays and reflected children below the bound's subject, transmitted children above it
    assert ru.child_length(short) < sc.L[0] and long_ < sc.L[0] < sc.L[1] < ru.child_length(long_)
    if cluster == "tiny":
        assert ru.child_length(short) < dcap * 0.999 and long_ < dcap * 0.999 < dcap < ru.child_length(long_)
