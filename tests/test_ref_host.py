"""The drop-in Python layer against the REFERENCE's own Python output.

``oracle/ref_host.py`` runs the reference's ``light_source.py``,
``geo_optical_elements.py`` and ``iterative_tracer.py`` (translated with lib2to3,
over a stand-in PyOpenCL whose kernels are the CPU oracle's) and recorded what
they compute in ``tests/golden/ref_host/*.npz``.  Held against it here:

* ``lightpycl_amd.light_source`` / ``geo_optical_elements``: rays and meshes;
* ``lightpycl_amd.scenes.BUILDERS``: the example scenes and their constants;
* ``oracle.trace`` / ``trace_rays`` / ``measured_rays`` / ``binned_angular``: the
  host loop (both sides run the same CPU kernels, so equality tests the loop);
* the host paths of ``CL_Tracer.plot_elevation_histogram``,
  ``get_beam_width_half_power`` and ``get_beam_HWHM``.

Fixture mode runs everywhere (a missing fixture is a failure).  Live mode runs
where the reference is (``ref_host.available()``): the reference modules are
called in-process beside ours under the same seed, everything is exact, the
generators also take 20 randomised argument sets each, and the committed
fixtures are checked against what the recipe computes now.  If live mode
passes while fixture mode fails, the fixtures are stale (regenerate them with
``python oracle/ref_host.py``) or the recipe is not deterministic.

Comparison rules: float32 arrays, integers, shapes and dtypes are equal bit for
bit (arrays too large to store are compared by their sampled rows, then by
SHA-256); the float64 analysis outputs of fixture mode take the two tolerances
``tests/test_gpu_beam.py`` derives (kept in ``tests/beam_ref.py``): elevations
and angles ``ELEV_TOL``, sums ``SUM_RTOL``.

Not pinned, because the reference cannot run them here (``ref_host.CANNOT_RUN``):
``optical_elements.curve_to_mesh`` and ``extrude_by_vector(capped=True)`` (need
``triangle``); ``GeoObject.write_dxf``, ``light_source.save_dxf``,
``CL_Tracer.save_traced_scene`` (need ``dxfwrite``);
``CL_Tracer.replicate_lightsources_and_plot``, ``plot_binned_data``,
``pickle_results`` and ``load_pickle_results``.  ``setMaterial`` with an unknown
type raises NameError in the reference after it has set the fallback type; the
drop-in warns and goes on, and the state both leave is compared.
"""
import functools
import json
import os

import numpy as np
import pytest

import ref_host as rh
from lightpycl_amd import scenes
from beam_ref import ELEV_TOL, SUM_RTOL, no_pdf  # noqa: F401  (no_pdf: a fixture)

OURS = rh.ours()
LIVE, WHY = rh.available()
live = pytest.mark.skipif(not LIVE, reason="live mode needs the reference: " + WHY)
CANNOT_RUN = ("optical_elements.curve_to_mesh", "optical_elements.extrude_by_vector(capped=True)",
              "GeoObject.write_dxf", "light_source.save_dxf", "CL_Tracer.save_traced_scene",
              "CL_Tracer.replicate_lightsources_and_plot", "CL_Tracer.plot_binned_data",
              "CL_Tracer.pickle_results", "CL_Tracer.load_pickle_results")
ANGLE_TOL = ELEV_TOL * 180.0 / np.pi


@functools.lru_cache(maxsize=None)
def fixture(name):
    path = os.path.join(rh.FIXTURE_DIR, name + ".npz")
    assert os.path.isfile(path), "fixture %s is missing (python oracle/ref_host.py writes it)" % path
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def file_of(groups, case):
    return next(f for f, names in groups.items() if case in names)


def check_record(fix, prefix, got, skip=()):
    """Every array the reference recorded under prefix/ is reproduced, and nothing else is claimed."""
    assert set(rh.unpacked_keys(fix, prefix)) == set(got), (prefix, sorted(got))
    for k, v in got.items():
        if k not in skip:
            rh.check(fix, prefix + "/" + k, v, what=prefix)


def same_record(got, want, what, skip=()):
    """Live mode: two records of the same case, bit for bit, shapes and dtypes included."""
    assert set(got) == set(want), what
    for k in want:
        if k in skip:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, a.dtype, b.shape, b.dtype)
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, k))


def test_the_list_of_what_cannot_run_is_the_recipes():
    assert tuple(rh.CANNOT_RUN) == CANNOT_RUN
    for name in ("curve_to_mesh", "replicate_lightsources_and_plot"):
        assert name in rh.__doc__ and name in __doc__


# -- fixture mode ----------------------------------------------------------------------------
def _expected_args(name):
    if name.startswith("rays_"):
        return {n: rh.RAY_CASES[n] for n in rh.ray_groups()[name]}
    if name.startswith("geometry_"):
        return {n: rh.GEO_CASES[n] for n in rh.geo_groups()[name]}
    if name == "curves":
        return rh.CURVE_CASES
    if name.startswith("scene_"):
        n, seed = rh.SCENE_SIZES[name[6:]]
        return dict(n=n, seed=seed)
    return rh.TRACE_CASES[name.split("_", 1)[1]]


def test_fixture_directory_holds_the_catalogues_files_and_no_other():
    assert sorted(os.listdir(rh.FIXTURE_DIR)) == sorted(f + ".npz" for f in rh.FIXTURE_FILES)


@pytest.mark.parametrize("name", rh.FIXTURE_FILES)
def test_fixture_file_records_the_catalogues_calls(name):
    fix = fixture(name)
    assert str(fix["source"]) == rh.SOURCE and str(fix["numpy"])
    assert json.loads(str(fix["args"])) == json.loads(json.dumps(_expected_args(name)))
    assert os.path.getsize(os.path.join(rh.FIXTURE_DIR, name + ".npz")) <= 128 * 1024


@pytest.mark.parametrize("case", list(rh.RAY_CASES))
def test_rays_reproduce_the_reference(case):
    check_record(fixture(file_of(rh.ray_groups(), case)), case, rh.run_ray_case(OURS, rh.RAY_CASES[case]))


@pytest.mark.parametrize("case", list(rh.GEO_CASES))
def test_geometry_reproduces_the_reference(case):
    got = rh.run_geo_case(OURS, rh.GEO_CASES[case])
    assert json.loads(str(got["raised"])) == []
    fix = fixture(file_of(rh.geo_groups(), case))
    assert json.loads(str(fix[case + "/raised"])) == (["setMaterial: NameError"] if case == "material_unknown" else [])
    check_record(fix, case, got, skip=("raised",))


@pytest.mark.parametrize("case", list(rh.CURVE_CASES))
def test_curves_reproduce_the_reference(case):
    check_record(fixture("curves"), case, rh.run_curve_case(OURS, rh.CURVE_CASES[case]))


def _builder_record(name, n, seed):
    sc = scenes.BUILDERS[name](n=n, seed=seed)
    rec = rh.scene_record(sc.sources, sc.meshes)
    rec.update(rh.constants_record(dict(max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, iterations=sc.iterations,
                                        tau=sc.tau, hist_limits=sc.hist_limits, hist_points=sc.hist_points)))
    assert type(sc.max_ray_len) is np.float32 and type(sc.ior_env) is np.float32
    return rec


@pytest.mark.parametrize("name", list(rh.SCENE_SIZES))
def test_scene_builders_reproduce_the_example_scripts(name):
    check_record(fixture("scene_" + name), name, _builder_record(name, *rh.SCENE_SIZES[name]))


@functools.lru_cache(maxsize=None)
def our_trace(name):
    """oracle.trace over the drop-in's scene of a trace case, computed once and left unchanged."""
    import oracle
    oracle.build()
    case = rh.TRACE_CASES[name]
    c = rh.trace_settings(case)
    sources, meshes = rh.build_scene(OURS, case["scene"], case["n"], case["seed"], case.get("extra_sources", ()))
    results, info = oracle.trace(sources, meshes, c["iterations"], c["tau"], np.float32(c["max_ray_len"]),
                                 np.float32(c["ior_env"]))
    for r in results:
        for a in r:
            a.flags.writeable = False
    return results, info, c


def _loop_record(results, info):
    out = dict(iterations=np.int64(len(results)), counts=np.array(info["counts"], np.int64),
               mesh_power=info["mesh_power"])
    for i, r in enumerate(results):
        for k, key in enumerate(("origin", "dest", "pow", "meas")):
            out["it%02d_%s" % (i, key)] = r[k]
    return out


@pytest.mark.parametrize("name", list(rh.TRACE_CASES))
def test_host_loop_reproduces_the_reference(name):
    """Results tuples element for element, per-iteration counts and the measured rays."""
    import oracle
    results, info, _ = our_trace(name)
    fix = fixture("trace_" + name)
    assert [len(r[3]) for r in results] == info["counts"] == list(fix["counts"])
    for k, v in _loop_record(results, info).items():
        rh.check(fix, k, v, what=name)
    pos, pwr = oracle.measured_rays(results)
    assert int(fix["measured_count"]) == pos.shape[0]
    if pos.shape[0]:
        rh.check(fix, "measured_pos", pos, what=name)
        rh.check(fix, "measured_pwr", pwr, what=name)
    # the same loop from the concatenated arrays (trace_rays, what the GPU tests drive)
    case = rh.TRACE_CASES[name]
    sources, meshes = rh.build_scene(OURS, case["scene"], case["n"], case["seed"], case.get("extra_sources", ()))
    c = rh.trace_settings(case)
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32) for s in sources])
    if name in ("nested_cubes", "lens_two_sources", "lens_four_iterations"):
        again, info2 = oracle.trace_rays(o, d, p, meshes, c["iterations"], c["tau"], c["max_ray_len"], c["ior_env"])
        assert info2["counts"] == info["counts"]
        for a, b in zip(again, results):
            for x, y in zip(a, b):
                assert x.shape == y.shape and x.dtype == y.dtype
                np.testing.assert_array_equal(x, y)


def stereo_hist(oracle, pos, pwr, limits, points):
    """get_binned_data_stereographic (iterative_tracer.py:503-531) over the oracle's kernel."""
    x, y, pc = oracle.stereograph_project(pos, pwr)
    dx = np.float64(limits[0][1] - limits[0][0]) / np.float64(points)
    dy = np.float64(limits[1][1] - limits[1][0]) / np.float64(points)
    return np.histogram2d(x=x.flatten(), y=y.flatten(), bins=points, range=limits,
                          weights=(np.float64(pc) / (dx * dy)).flatten())


def _our_histograms(name):
    import oracle
    results, _, c = our_trace(name)
    pos, pwr = oracle.measured_rays(results)
    lim = tuple(tuple(r) for r in c["hist_limits"])
    return dict(angular=oracle.binned_angular(pos, pwr, lim, c["hist_points"]),
                stereo=stereo_hist(oracle, pos, pwr, rh.STEREO_LIMITS, c["hist_points"]))


def host_tracer(results):
    """A CL_Tracer holding results, without a device: the host paths of the analyses need none."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    tr = CL_Tracer.__new__(CL_Tracer)
    tr.results, tr._aggregate = results, False
    return tr


def _our_beam(tr):
    """{fixture key: value} of the three beam functions' host paths, named as the recipe names them."""
    out = {}
    for p, pole in enumerate(rh.POLES):
        for npts in rh.BEAM_POINTS:
            H, x = tr.plot_elevation_histogram(points=npts, pole=pole)
            t, a, c = tr.get_beam_width_half_power(points=npts, pole=pole)
            u, b, w = tr.get_beam_HWHM(points=npts, pole=pole)
            tag = "_p%d_n%d_" % (p, npts)
            out.update({"hist" + tag + "H": H, "hist" + tag + "x": x,
                        "half" + tag + "total": t, "half" + tag + "angle": a, "half" + tag + "percent": c,
                        "hwhm" + tag + "total": u, "hwhm" + tag + "angle": b,
                        "hwhm" + tag + "percent": np.asarray(w, np.float64).reshape(-1)})
    return out


def _ref_beam(rec):
    """The same keys from the reference's recorded quantities: it prints elevation / pi * 180 and
    power / total * 100 (iterative_tracer.py:464-466, :499-501)."""
    out = {}
    for k, v in rec.items():
        kind, rest = k.split("_", 1)
        if kind == "hist":
            out[k] = v
        elif kind in ("half", "hwhm"):
            tag, what = rest.rsplit("_", 1)
            total = rec["%s_%s_total" % (kind, tag)]
            if what == "total":
                out[k] = v
            elif what == "elevation":
                out["%s_%s_angle" % (kind, tag)] = v / np.pi * 180.0
            else:
                out["%s_%s_percent" % (kind, tag)] = v / total * 100.0
    return out


MEASURING = [n for n in rh.TRACE_CASES if n != "nested_cubes"]


def test_a_trace_without_measured_rays_records_no_analysis():
    assert int(fixture("trace_nested_cubes")["measured_count"]) == 0
    assert not [k for k in fixture("analyses_nested_cubes") if rh.is_analysis_key(k)]


@pytest.mark.parametrize("name", MEASURING)
def test_histograms_reproduce_the_reference(name):
    fix = fixture("analyses_" + name)
    for mode, (H, xe, ye) in _our_histograms(name).items():
        want = fix[mode + "_H"]
        assert H.shape == want.shape and H.dtype == want.dtype and want.sum() > 0
        np.testing.assert_allclose(H, want, rtol=SUM_RTOL, atol=SUM_RTOL * want.max(), err_msg=mode)
        np.testing.assert_allclose(xe, fix[mode + "_xe"], rtol=0, atol=ELEV_TOL)
        np.testing.assert_allclose(ye, fix[mode + "_ye"], rtol=0, atol=ELEV_TOL)


@pytest.mark.parametrize("name", MEASURING)
def test_beam_host_paths_reproduce_the_reference(no_pdf, name):
    fix = fixture("analyses_" + name)
    want = _ref_beam({k: v for k, v in fix.items() if k.split("_")[0] in ("hist", "half", "hwhm")})
    got = _our_beam(host_tracer(our_trace(name)[0]))
    assert set(got) == set(want) and len(want) == 2 * 2 * 8
    for k, w in want.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == np.shape(w), (k, g.shape, np.shape(w))
        if k.endswith("_x"):
            np.testing.assert_allclose(g, w, rtol=0, atol=ELEV_TOL, err_msg=k)
        elif k.endswith("_angle"):
            np.testing.assert_allclose(g, w, rtol=0, atol=ANGLE_TOL, err_msg=k)
        elif k.endswith("_H"):
            np.testing.assert_allclose(g, w, rtol=SUM_RTOL, atol=SUM_RTOL * np.abs(w).max(), err_msg=k)
        else:
            np.testing.assert_allclose(g, w, rtol=SUM_RTOL, err_msg=k)


# -- live mode -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def REF():
    return rh.load()


@functools.lru_cache(maxsize=None)
def ref_trace(name):
    rec, stop, _ = rh.run_trace_case(rh.load(), rh.TRACE_CASES[name])
    return rec, stop


@live
def test_live_nothing_of_the_reference_is_left_in_sys_modules(REF):
    import sys
    for m in rh.MODULES + ("pyopencl", "dxfwrite", "triangle"):
        assert m not in sys.modules or not (getattr(sys.modules[m], "__file__", None) or "").startswith(rh.PY_DIR)
    assert REF.ls.__file__.startswith(rh.PY_DIR) and REF.ls.light_source is not OURS.ls.light_source


@live
@pytest.mark.parametrize("case", list(rh.RAY_CASES))
def test_live_rays(REF, case):
    want = rh.run_ray_case(REF, rh.RAY_CASES[case])
    same_record(rh.run_ray_case(OURS, rh.RAY_CASES[case]), want, case)
    check_record(fixture(file_of(rh.ray_groups(), case)), case, want)          # the fixture is current


@live
@pytest.mark.parametrize("case", list(rh.GEO_CASES))
def test_live_geometry(REF, case):
    want = rh.run_geo_case(REF, rh.GEO_CASES[case])
    same_record(rh.run_geo_case(OURS, rh.GEO_CASES[case]), want, case, skip=("raised",))
    check_record(fixture(file_of(rh.geo_groups(), case)), case, want)


@live
@pytest.mark.parametrize("case", list(rh.CURVE_CASES))
def test_live_curves(REF, case):
    want = rh.run_curve_case(REF, rh.CURVE_CASES[case])
    same_record(rh.run_curve_case(OURS, rh.CURVE_CASES[case]), want, case)
    check_record(fixture("curves"), case, want)


@live
def test_live_randomised_arguments(REF):
    """20 argument sets per generator from a seeded default_rng (radii, centres, ang_pts in 3..12,
    ray counts in 1..300, ...), the reference beside the drop-in."""
    rays, geo, curves = rh.random_cases(seed=2024, count=20)
    per_generator = {}
    for cases in (rays, geo, curves):
        for name in cases:
            per_generator[name.rsplit("_", 1)[0]] = per_generator.get(name.rsplit("_", 1)[0], 0) + 1
    assert per_generator == {g: 20 for g in (
        "random", "grid", "collimated", "rotate", "cube", "revolve", "translate_rotate", "extrude", "sphere",
        "hemisphere", "parabolic_mirror", "topless_cylinder", "spherical_lens_nofoc", "lens_spherical_biconcave",
        "lens_spherical_2r", "curve_lens_spherical", "curve_lens_spherical_biconcave")}
    for name, case in rays.items():
        same_record(rh.run_ray_case(OURS, case), rh.run_ray_case(REF, case), name)
    for name, case in geo.items():
        same_record(rh.run_geo_case(OURS, case), rh.run_geo_case(REF, case), name)
    for name, case in curves.items():
        same_record(rh.run_curve_case(OURS, case), rh.run_curve_case(REF, case), name)


@live
@pytest.mark.parametrize("name", list(rh.SCENE_SIZES))
def test_live_scenes(REF, name):
    n, seed = rh.SCENE_SIZES[name]
    want = rh.scene_record(*rh.build_scene(REF, name, n, seed))
    want.update(rh.constants_record(rh.SCENE_CONSTANTS[name]))
    same_record(_builder_record(name, n, seed), want, name)
    check_record(fixture("scene_" + name), name, want)


@live
@pytest.mark.parametrize("name", list(rh.TRACE_CASES))
def test_live_host_loop_and_analyses(REF, no_pdf, name):
    """The reference's CL_Tracer (its loop, get_measured_rays, both binned histograms and the three
    beam functions) beside oracle.trace and the drop-in's host paths: everything exact."""
    import oracle
    rec, stop = ref_trace(name)
    results, info, _ = our_trace(name)
    want_loop = {k: v for k, v in rec.items() if k in ("iterations", "counts", "mesh_power") or k.startswith("it")}
    same_record(_loop_record(results, info), want_loop, name)
    pos, pwr = oracle.measured_rays(results)
    assert int(rec["measured_count"]) == pos.shape[0]
    if name == "nested_cubes":
        assert pos.shape[0] == 0
        return
    same_record(dict(pos=pos, pwr=pwr), dict(pos=rec["measured_pos"], pwr=rec["measured_pwr"]), name)
    for mode, (H, xe, ye) in _our_histograms(name).items():
        same_record(dict(H=H, xe=xe, ye=ye), {k: rec["%s_%s" % (mode, k)] for k in ("H", "xe", "ye")}, name + mode)
    want = _ref_beam({k: v for k, v in rec.items() if k.split("_")[0] in ("hist", "half", "hwhm")})
    got = _our_beam(host_tracer(results))
    assert set(got) == set(want)
    for k, w in want.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == np.shape(w), k
        np.testing.assert_array_equal(g, w, err_msg=k)


@live
def test_live_the_loop_reaches_both_breaks_and_the_cap():
    stops = {n: ref_trace(n)[1] for n in rh.TRACE_CASES}
    assert {"threshold", "empty", "iterations"} <= set(stops.values()), stops
    assert {n: str(fixture("trace_" + n)["stop"]) for n in rh.TRACE_CASES} == stops


@live
@pytest.mark.parametrize("name", list(rh.TRACE_CASES))
def test_live_trace_fixtures_are_current(name):
    rec, _ = ref_trace(name)
    loop, ana = fixture("trace_" + name), fixture("analyses_" + name)
    for k, v in rec.items():
        rh.check(ana if rh.is_analysis_key(k) else loop, k, v, what=name)
