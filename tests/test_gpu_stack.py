"""Nested, adjacent and coincident media through the device's shading paths: the
layer-stack scene of tests/stack_util.py (tests/test_stack_host.py shows that the
reference realises every column's situation) at the mesh counts where the
shading loads a ray's slots differently:

  4 (reduced), 8, 12, 16   slots in registers, postproc<4 / 8 / 12 / 16>
  17, 33                   slots from memory (17: written-slot masks; 33: none)
  70                       and the re-read of slots 64 and up

Populations cycle through the columns, so every wave mixes rays that wrote one
slot (their single-slot shortcut) with rays that wrote up to five.  The drop-in
bounce (k_shade) of two levels and four traced iterations (k_shade_stage) are
compared with the reference's kernels, or with the CPU oracle under
test_gpu_parity._cmp_bounce's rule when the reference code object is absent.
"""
import types

import numpy as np
import pytest

import stack_util as su
from soup_util import kept_children, meshes_of, oracle_scene
from test_gpu_compaction import _pow_equal
from test_gpu_parity import _cmp_bounce
from test_gpu_shade_paths import OFF, _open

pytestmark = pytest.mark.gpu

CONFIGS = [("reduced", 4), ("full", 8), ("full", 12), ("full", 16), ("full", 17), ("full", 33), ("full", 70)]
SIZES = (1, 64, 65, 257)
ITERATIONS = 4
TRACE_RAYS = 257                        # at most 257 * 2^3 rays in the fourth iteration: populations keep their order


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"{c[0]}-K{c[1]}")
def stack(request):
    kind, K = request.param
    sc = su.scene(su.REDUCED if kind == "reduced" else su.FULL, K)
    assert sc.K == K
    return types.SimpleNamespace(sc=sc, K=K, ref=oracle_scene(sc.arrs), meshes=meshes_of(sc.arrs))


def _cols(sc, n):
    """n rays cycling through the columns, starting at column n (one ray: not
    always the first column)."""
    return (np.arange(n) + n) % len(sc.cols)


@pytest.mark.parametrize("n", SIZES)
def test_bounce_two_levels(engine, checker, stack, n):
    sc = stack.sc
    engine.upload_arrays(*sc.arrs)
    cols = _cols(sc, n)
    o4, d4, pw = su.rays(cols)
    z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
    ref = checker[0](stack.ref, o4, d4, pw, z, pm, su.MAX_RAY_LEN, su.IOR_ENV)
    su.check_declared(sc, cols, ref)
    _cmp_bounce(engine.bounce(o4, d4, pw, z, pm, su.MAX_RAY_LEN, su.IOR_ENV), ref, checker[1])
    # second level: the judge's kept children, started on the surfaces with prev >= 0
    o2, d2, p2, m2 = kept_children(ref)
    assert len(p2) >= n // 2 or n == 1
    if len(p2) == 0:
        return
    z2 = np.zeros(len(p2), np.int32)
    ref2 = checker[0](stack.ref, o2, d2, p2, z2, m2, su.MAX_RAY_LEN, su.IOR_ENV)
    _cmp_bounce(engine.bounce(o2, d2, p2, z2, m2, su.MAX_RAY_LEN, su.IOR_ENV), ref2, checker[1])


def _trace(e, rays):
    """ITERATIONS traced iterations from the emitted rays: per iteration the stats,
    the exported rows and the measured record so far."""
    e.set_rays(*rays, su.MAX_RAY_LEN, su.IOR_ENV)
    out = []
    for _ in range(ITERATIONS):
        if e.population() == 0:
            break
        st, ex = e.iterate(export=True)
        rec = [x.copy() for x in e.fetch_measured()]
        out.append(((int(st.n_in), int(st.n_reflect), int(st.n_refract), int(st.n_measured)),
                    {k: v.copy() for k, v in ex.items()}, rec))
    return out


def _against_host_loop(oracle_mod, checker, stack, rays, got, what):
    """The reference's host loop over the judge's bounce: every iteration's counts
    and rows, and the measured record as it grows."""
    measured = []
    results, info = oracle_mod.trace_rays(*rays, stack.meshes, ITERATIONS, 1.0, su.MAX_RAY_LEN, su.IOR_ENV,
                                          bounce_fn=checker[0], measured_out=measured)
    assert [g[0][0] for g in got] == info["counts"], (what, [g[0] for g in got], info["counts"])
    assert len(got) == ITERATIONS, (what, "the stacks keep rays alive for every iteration")
    exact = checker[1]
    for i, ((st, ex, rec), (org, dst, pw, ms)) in enumerate(zip(got, results)):
        w = f"{what}, iteration {i}"
        np.testing.assert_array_equal(ex["origin"][:, :3], org[:, :3], err_msg=w)
        np.testing.assert_array_equal(ex["dest"][:, :3], dst[:, :3], err_msg=w)
        np.testing.assert_array_equal(ex["meas"], ms, err_msg=w)
        _pow_equal(ex["pow"], pw, exact, w)
        assert st[3] == int((ms == 1).sum()), (w, st)
        if i + 1 < len(results):
            assert st[1] + st[2] == len(results[i + 1][2].reshape(-1)) == len(ex["next_pow"]), (w, st)
        pos = np.concatenate([m[0] for m in measured[: i + 1]])
        np.testing.assert_array_equal(rec[0][:, :3], pos[:, :3], err_msg=w)
        _pow_equal(rec[1], np.concatenate([m[1] for m in measured[: i + 1]]), exact, w)
        np.testing.assert_array_equal(rec[2], np.concatenate([m[2] for m in measured[: i + 1]]), err_msg=w)


def _same_trace(a, b, what):
    assert len(a) == len(b), what
    for i, ((sa, xa, ra), (sb, xb, rb)) in enumerate(zip(a, b)):
        assert sa == sb, (what, i, sa, sb)
        for k in xa:
            assert xa[k].tobytes() == xb[k].tobytes(), f"{what}: iteration {i}, {k}"
        for x, y, k in zip(ra, rb, ("position", "power", "mesh")):
            assert x.tobytes() == y.tobytes(), f"{what}: iteration {i}, measured {k}"


def _policies(K):
    return [("default", {})] + ([("LPC_SHADE_FAST=0", OFF)] if K in (8, 17) else [])


def test_trace_against_host_loop(oracle_mod, checker, stack):
    sc = stack.sc
    cols = _cols(sc, TRACE_RAYS)
    rays = su.rays(cols)
    first = None
    for name, cfg in _policies(stack.K):
        e = _open(cfg)
        try:
            e.upload_arrays(*sc.arrs)
            got = _trace(e, rays)
            _against_host_loop(oracle_mod, checker, stack, rays, got, f"K {stack.K}, {name}")
            # the slots of many-slot rays went back to the clean state: a second trace
            # on the same engine gives the first one's rows
            e.reset()
            _same_trace(_trace(e, rays), got, f"K {stack.K}, {name}: second trace")
            if first is None:
                first = got
            else:
                _same_trace(got, first, f"K {stack.K}: {name} against the default policy")
        finally:
            e.close()


# -- fewer meshes than register slots -----------------------------------------------------
def _edge_scene(K):
    """Column 0: glass (mesh 0) 4e-6 short of max_ray_len under the beam; a measuring
    ceiling (mesh 1); never-hit GLASS fillers up to K meshes, so the last mesh is
    refractive.  The reference's max-min rule hands the hit to the LAST clean
    refractive slot (t = max_ray_len is inside EPSILON of the hit): n2 = K - 1."""
    from soup_util import _rows
    import fate_util as fu
    z_edge = 1.0 - (float(su.MAX_RAY_LEN) - su.NEAR)
    tris = fu._quad(0, 1, z_edge) + fu._quad(0, 1, 2)
    ids, mats = [0, 0, 1, 1], [su.MATERIALS["A"], su.MATERIALS["CEIL"]]
    for j in range(2, K):
        x = 64 + 2 * j
        tris.append(((x, 64, 32), (x + 1, 64, 32), (x, 65, 32)))
        ids.append(j)
        mats.append(su.MATERIALS["C"])
    t, m = np.asarray(tris, np.float64), np.asarray(mats, np.float64)
    return (_rows(t[:, 0]), _rows(t[:, 1]), _rows(t[:, 2]), np.asarray(ids, np.int32), m[:, 0].astype(np.int32),
            m[:, 1].astype(np.float32), m[:, 2].astype(np.float32), m[:, 3].astype(np.float32))


@pytest.mark.parametrize("K", (3, 6, 9, 13))
def test_fewer_meshes_than_register_slots(engine, checker, K):
    """K below the register slot count KU (4, 8, 12, 16): postproc<KU> walks KU
    slots, and the ones from K up are no meshes.  A hit inside EPSILON of
    max_ray_len is the case where a clean slot takes the hit over, so a slot from
    K up that counted as a mesh would take it instead of mesh K - 1."""
    arrs = _edge_scene(K)
    engine.upload_arrays(*arrs)
    n = 65
    o4, d4, pw = su.rays(np.zeros(n, np.int64))
    z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
    ref = checker[0](oracle_scene(arrs), o4, d4, pw, z, pm, su.MAX_RAY_LEN, su.IOR_ENV)
    assert np.all(ref["isect_mid"] == 0) and np.all(ref["n2"] == K - 1), (ref["isect_mid"], ref["n2"])
    _cmp_bounce(engine.bounce(o4, d4, pw, z, pm, su.MAX_RAY_LEN, su.IOR_ENV), ref, checker[1])
    e = _open({})
    try:                                # the traced path's shade_post<KU>
        e.upload_arrays(*arrs)
        e.set_rays(o4, d4, pw, su.MAX_RAY_LEN, su.IOR_ENV)
        st, ex = e.iterate(export=True)
        np.testing.assert_array_equal(ex["dest"][:, :3], ref["dest"][:, :3])
        _pow_equal(ex["pow"], ref["pow"], checker[1], "traced iteration")
        assert (int(st.n_reflect), int(st.n_refract)) == (int((ref["r_meas"] == 0).sum()), int((ref["t_meas"] == 0).sum()))
        kept = np.concatenate((ref["r_pow"][ref["r_meas"] == 0], ref["t_pow"][ref["t_meas"] == 0]))
        _pow_equal(ex["next_pow"], kept, checker[1], "traced iteration: children")
    finally:
        e.close()
