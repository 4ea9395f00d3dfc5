"""The drop-in CL_Tracer on the GPU against the REFERENCE's own host loop
(``tests/golden/ref_host/trace_*.npz``: the reference's ``iterative_tracer.py`` run
by ``oracle/ref_host.py`` over the CPU oracle's kernels).  Fixtures only: nothing
here reads the reference.

The scene is rebuilt from the arrays the fixture stores in full (the rays, the
cubes); what does not fit its file and is stored as a digest (the hemisphere,
the lens) comes from the builders after the digest is checked.

Not bit for bit: the fixture's kernels ran with the C library's sqrt / exp, which
differ from gfx950's rsqrt and exp by ulps.  The tolerances are the project's own
for oracle against hardware (tests/test_golden.py):
iteration count equal, per-iteration counts within 1e-3, per-mesh and total
measured power within rtol 1e-4, angular histogram relative L1 <= 1e-3; results
tuples have the fixture's shapes and dtypes; iteration 0's origins are an input
and equal bit for bit.  Where the reference's own kernels are built
(``exact_ref``) the restated loop also drives them from the same inputs, and the
tracer equals that element for element."""
import functools
import json
import os
import types

import numpy as np
import pytest

import ref_host as rh
from lightpycl_amd import geo_optical_elements as goe
from lightpycl_amd import scenes
from parity_util import COUNT_RTOL, HIST_L1, POWER_RTOL, hist_l1

pytestmark = pytest.mark.gpu
CASES = ["cube", "nested_cubes", "lens"]


def fixture(name):
    path = os.path.join(rh.FIXTURE_DIR, name + ".npz")
    assert os.path.isfile(path), "fixture %s is missing" % path
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def scene_from_fixture(name):
    """(source, meshes, constants): stored arrays where the fixture has them in full, the builders'
    (checked against the fixture's digest) where it does not."""
    fix = fixture("scene_" + name)
    n, seed = rh.SCENE_SIZES[name]
    sc = scenes.BUILDERS[name](n=n, seed=seed)
    rays = {}
    for k in ("rays_origin", "rays_dir", "rays_power"):
        key = "%s/s0_%s" % (name, k)
        rh.check(fix, key, np.asarray(getattr(sc.sources[0], k)), what=name)
        rays[k] = fix[key]                     # the reference-made rays: stored in full for all three cases
    mats = fix[name + "/materials"]
    types_ = json.loads(str(fix[name + "/matTypes"]))
    meshes, stored = [], 0
    for j, m in enumerate(sc.meshes):
        keys = ["%s/m%d_v%d" % (name, j, k) for k in range(3)]
        tb = m.tribuf()
        for k in range(3):
            rh.check(fix, keys[k], np.asarray(tb[k]), what=name)
        if all(k in fix for k in keys):
            v = [fix[k] for k in keys]
            T = v[0].shape[0]
            g = goe.GeoObject(np.concatenate(v), np.arange(3 * T).reshape(3, T).T, mat_type=types_[j],
                              IOR=float(mats[j][1]), dissipation=float(mats[j][3]))
            stored += 1
        else:
            g = m
        np.testing.assert_array_equal(rh.material_row(g), mats[j])
        meshes.append(g)
    assert stored == dict(cube=1, nested_cubes=4, lens=0)[name]    # the cubes; the revolved meshes do not fit
    c = {k: fix["%s/%s" % (name, k)] for k in ("max_ray_len", "ior_env", "iterations", "tau", "hist_limits",
                                               "hist_points")}
    return types.SimpleNamespace(**rays), meshes, c


@functools.lru_cache(maxsize=None)
def trace_case(name):
    """The drop-in tracer over a case's fixture scene, traced once per session."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    src, meshes, c = scene_from_fixture(name)
    tr = CL_Tracer(device=0)
    res = tr.iterative_tracer(light_source=[src], meshes=meshes, trace_iterations=int(c["iterations"]),
                              trace_until_dissipated=float(c["tau"]), max_ray_len=c["max_ray_len"],
                              ior_env=c["ior_env"])
    return types.SimpleNamespace(name=name, tr=tr, res=res, src=src, meshes=meshes, c=c,
                                 fix=fixture("trace_" + name))


def recorded(fix, key):
    """(shape, dtype) of an array of the fixture, stored in full or as a digest."""
    if key in fix:
        return fix[key].shape, fix[key].dtype
    return tuple(fix[key + "__shape"]), np.dtype(str(fix[key + "__dtype"]))


@pytest.mark.parametrize("name", CASES)
def test_trace_vs_the_references_host_loop(name):
    traced = trace_case(name)
    fix, res, tr = traced.fix, traced.res, traced.tr
    want = list(fix["counts"])
    got = [len(r[3]) for r in res]
    print(traced.name, "counts", got, "reference", want)
    assert len(res) == int(fix["iterations"]) == len(want)
    assert all(abs(a - b) <= COUNT_RTOL * b for a, b in zip(got, want)), (got, want)
    assert got[0] == want[0]
    rh.check(fix, "it00_origin", res[0][0], what=traced.name)           # an input: bit for bit
    for i, r in enumerate(res):
        for k, key in enumerate(("origin", "dest", "pow", "meas")):
            shape, dtype = recorded(fix, "it%02d_%s" % (i, key))
            assert r[k].dtype == dtype, (i, key, r[k].dtype, dtype)
            assert r[k].shape[1:] == shape[1:] and r[k].ndim == len(shape), (i, key, r[k].shape, shape)
            if got[i] == want[i]:
                assert r[k].shape == shape, (i, key, r[k].shape, shape)
    mp = np.asarray(tr.measured_power(), np.float64)
    print(traced.name, "mesh power", mp, "reference", fix["mesh_power"])
    np.testing.assert_allclose(mp, fix["mesh_power"], rtol=POWER_RTOL, atol=1e-12)
    np.testing.assert_allclose(mp.sum(), fix["mesh_power"].sum(), rtol=POWER_RTOL, atol=1e-12)
    pos, pwr = tr.get_measured_rays()
    np.testing.assert_allclose(np.sum(np.float64(pwr)), fix["mesh_power"].sum(), rtol=POWER_RTOL, atol=1e-12)
    assert abs(pos.shape[0] - int(fix["measured_count"])) <= COUNT_RTOL * max(int(fix["measured_count"]), 1)


@pytest.mark.parametrize("name", CASES)
def test_trace_vs_the_reference_kernels_under_the_restated_loop(name, oracle_mod, exact_ref):
    """The loop the CPU tests hold against the reference's, over the reference's own kernels on the
    same fixture inputs: the tracer's results tuples element for element."""
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    traced = trace_case(name)
    c, src = traced.c, traced.src
    ref, info = oracle_mod.trace_rays(np.asarray(src.rays_origin, np.float32), np.asarray(src.rays_dir, np.float32),
                                      np.asarray(src.rays_power, np.float32), traced.meshes, int(c["iterations"]),
                                      float(c["tau"]), c["max_ray_len"], c["ior_env"], bounce_fn=exact_ref.bounce)
    res = traced.res
    assert [len(r[3]) for r in res] == info["counts"]
    for it, (a, b) in enumerate(zip(res, ref)):
        np.testing.assert_array_equal(a[0][:, :3], b[0][:, :3], err_msg=f"origin it{it}")
        np.testing.assert_array_equal(a[1][:, :3], b[1][:, :3], err_msg=f"dest it{it}")
        assert a[2].shape == b[2].shape and a[2].dtype == b[2].dtype and a[3].dtype == b[3].dtype == np.int32
        np.testing.assert_array_equal(a[2], b[2], err_msg=f"pow it{it}")
        np.testing.assert_array_equal(a[3], b[3], err_msg=f"meas it{it}")
    pos, pwr = traced.tr.get_measured_rays()
    rpos, rpwr = oracle_mod.measured_rays(ref)
    np.testing.assert_array_equal(pos[:, :3], rpos[:, :3])
    np.testing.assert_array_equal(np.asarray(pwr).reshape(-1), np.asarray(rpwr).reshape(-1))
    # and the fixture's loop (CPU kernels) against this one (reference kernels): the same tolerances
    want = list(traced.fix["counts"])
    assert len(want) == len(info["counts"])
    assert all(abs(a - b) <= COUNT_RTOL * b for a, b in zip(info["counts"], want))
    np.testing.assert_allclose(info["mesh_power"], traced.fix["mesh_power"], rtol=POWER_RTOL, atol=1e-12)


def test_angular_histogram_of_the_lens_vs_the_references():
    traced = trace_case("lens")
    c = traced.c
    ana = fixture("analyses_lens")
    lim = tuple(tuple(float(v) for v in r) for r in c["hist_limits"])
    H, xe, ye = traced.tr.get_binned_data_angular(limits=lim, points=int(c["hist_points"]))
    l1 = hist_l1(H, ana["angular_H"])
    print("lens angular histogram relative L1", l1)
    assert H.shape == ana["angular_H"].shape and ana["angular_H"].sum() > 0
    np.testing.assert_array_equal(xe, ana["angular_xe"])
    np.testing.assert_array_equal(ye, ana["angular_ye"])
    assert l1 <= HIST_L1
