"""The fate scene (tests/fate_util.py) means what it says: the CPU oracle's
bounce of the emitted beam gives every ray exactly its intended fate (meas,
r_meas, t_meas, isect_mid), children start at their parent's x and y bit for
bit, a mirror child carries its parent's power, a matched parent's reflected
child exactly 0 and its refracted child the parent's power.  Every pattern at
n = 65 537, every measure-mesh count, with and without filler meshes; no ray is
excluded.  tests/test_gpu_compaction.py rests on this."""
import numpy as np
import pytest

import fate_util as fu
from soup_util import meshes_of, oracle_scene

N = 65537


def _patterns(sc):
    return [p for p in fu.all_patterns() if all(k in sc.kinds for k in p.needs)]


@pytest.mark.parametrize("n_measure,K", [(0, None), (1, None), (2, None), (4, None), (5, None), (2, 33), (5, 70)])
def test_every_ray_gets_its_fate(oracle_mod, n_measure, K):
    sc = fu.layout(n_measure, K)
    assert sc.n_measure_meshes == n_measure and (K is None or sc.K == K)
    assert np.all(np.diff(sc.arrs[3]) >= 0), "mesh_id sorted"
    S = oracle_scene(sc.arrs)
    pats = _patterns(sc)
    assert len(pats) == (11 if n_measure else 10)
    for pat in pats:
        fates = pat(N, sc.kinds)
        o, d, p = fu.rays(sc, fates)
        assert np.all(p == np.arange(1, N + 1)) and len(np.unique(o[:, :2], axis=0)) == N
        out = oracle_mod.bounce(S, o, d, p, np.zeros(N, np.int32), np.full(N, -2, np.int32), fu.MAX_RAY_LEN, fu.IOR_ENV)
        fu.check_fates(sc, fates, o, p, out)


def test_all_matched_scene_keeps_the_geometry(oracle_mod):
    """The order probe of the GPU tests: the same triangles, every patch matched,
    so every ray aimed at a patch keeps both children."""
    a, b = fu.layout(2), fu.layout(2, all_matched=True)
    for x, y in zip(a.arrs[:4], b.arrs[:4]):
        np.testing.assert_array_equal(x, y)
    fates = fu.halves("matched", "terminator")(4097, a.kinds)
    o, d, p = fu.rays(b, fates)
    out = oracle_mod.bounce(oracle_scene(b.arrs), o, d, p, np.zeros(4097, np.int32), np.full(4097, -2, np.int32),
                            fu.MAX_RAY_LEN, fu.IOR_ENV)
    assert np.all(out["r_meas"] == 0) and np.all(out["t_meas"] == 0)
    np.testing.assert_array_equal(out["t_pow"], p)


def test_second_iteration_ends_on_ceiling_and_floor(oracle_mod):
    """Chained population: reflected children end on the ceiling, refracted ones
    on the floor, each with its parent's x and y; with both of measure type every
    kept child is measured in iteration 2 and nothing is left for a third."""
    sc = fu.layout(4)
    n = 4099
    fates = fu.cycle()(n, sc.kinds)
    o, d, p = fu.rays(sc, fates)
    meas = []
    _, info = oracle_mod.trace_rays(o, d, p, meshes_of(sc.arrs), 3, 1.0, fu.MAX_RAY_LEN, fu.IOR_ENV,
                                    keep_results=False, measured_out=meas)
    want = fu.intended(sc, fates)
    kept = int((want["r_meas"] == 0).sum() + (want["t_meas"] == 0).sum())
    assert info["counts"] == [n, kept]
    pos2, _, mesh2 = meas[1]
    assert len(mesh2) == kept
    nr = int((want["r_meas"] == 0).sum())
    assert np.all(mesh2[:nr] == sc.ceiling) and np.all(mesh2[nr:] == sc.floor)
    par = fu.parents_of(fu.ray_key(pos2[:, :2]), fu.ray_key(o[:, :2]))
    np.testing.assert_array_equal(par[:nr], np.flatnonzero(want["r_meas"] == 0))
    np.testing.assert_array_equal(par[nr:], np.flatnonzero(want["t_meas"] == 0))


@pytest.mark.parametrize("n_measure", [2, 4])
def test_nothing_dissipates_in_the_second_iteration(oracle_mod, n_measure):
    """Every child crosses one triangle of the ceiling or the floor (the rays keep
    clear of their diagonal), so none is taken as inside its parent's patch: the
    power iteration 2 records is the population's, bit for bit."""
    sc = fu.layout(n_measure)
    fates = fu.random(1)(N, sc.kinds)
    o, d, p = fu.rays(sc, fates)
    res, _ = oracle_mod.trace_rays(o, d, p, meshes_of(sc.arrs), 3, 1.0, fu.MAX_RAY_LEN, fu.IOR_ENV)
    out = oracle_mod.bounce(oracle_scene(sc.arrs), o, d, p, np.zeros(N, np.int32), np.full(N, -2, np.int32),
                            fu.MAX_RAY_LEN, fu.IOR_ENV)
    pop = np.concatenate((out["r_pow"][out["r_meas"] == 0], out["t_pow"][out["t_meas"] == 0]))
    assert len(res) == 2
    np.testing.assert_array_equal(res[1][2], pop)
