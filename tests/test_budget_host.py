"""CPU tests of the power budget: the host reference helper (tests/budget_ref.py)
over the CPU oracle -- its identities on the five cases of the GPU tests -- and
the library surface as far as it runs without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import budget_ref
from lightpycl_amd import geo_optical_elements as goe
from lightpycl_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["cube", "nested_cubes", "eye", "cube_field", "mixed"]


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


def mixed_scene():
    """Every category at once: the dissipative cube scene with its cube made a
    denser, weakly absorbing glass, a mirror of reflectivity 0.9 and a terminator."""
    sc = scenes.cube(n=2000)
    sc.meshes[1].setMaterial(mat_type="refractive", IOR=1.5, dissipation=0.05)
    oe = goe.optical_elements()
    mirror = oe.cube(center=(20, 0, 20, 0), size=[10, 10, 10, 0])
    mirror.setMaterial(mat_type="mirror")
    mirror.reflectivity = 0.9                   # setMaterial does not store a mirror's reflectivity
    term = oe.cube(center=(-20, 0, 20, 0), size=[10, 10, 10, 0])
    term.setMaterial(mat_type="terminator")
    sc.meshes = list(sc.meshes) + [mirror, term]
    sc.name = "mixed"
    return sc


_SCENES = {}


def case_scene(name):
    """The five cases: the smallest that span tiles, several iterations and every
    category (built once per session)."""
    if name not in _SCENES:
        if name == "mixed":
            sc = mixed_scene()
        elif name == "cube_field":
            sc = scenes.cube_field(n=2000, count=300)
        elif name == "eye":
            sc = scenes.eye(n=400)
        else:
            sc = scenes.BUILDERS[name](n=2000)
        _SCENES[name] = sc
    return _SCENES[name]


def assert_case_claims(name, ref):
    """The reference's side of a case exercises what the case is there for."""
    t = budget_ref.totals(ref)
    n_it = len(ref["iters"])
    if name == "cube":
        assert t["dissipated"] > 0 and t["escaped"] > 0 and t["measured"] > 0
    elif name == "nested_cubes":
        assert t["measured"] == 0 and t["escaped"] > 0 and t["absorbed"] > 0 and n_it >= 3
        assert any((it["kept"][0] < 0).any() for it in ref["iters"]), "negative powers"
    elif name == "eye":
        assert n_it >= 3 and max(ref["counts"]) > 2 * 1024 and t["absorbed"] > 0 and t["measured"] > 0
    elif name == "cube_field":
        assert ref["K"] == 301 and t["dissipated"] > 0 and t["escaped"] > 0 and t["measured"] > 0
    elif name == "mixed":
        for c in ("dissipated", "escaped", "terminated", "measured", "absorbed"):
            assert t[c] > 0, c
        absorbed = sum(float(it["absorbed"][0].sum()) for it in ref["iters"])
        assert absorbed > 1.0, absorbed                 # the mirror's (1 - R) p, not only rounding residue
    assert not any(np.isnan(it[c][0]).any() for it in ref["iters"] for c in budget_ref.SUMS)


_REFS = {}


def cpu_reference(oracle_mod, name):
    if name not in _REFS:
        sc = case_scene(name)
        o, d, p = rays_of(sc)
        _REFS[name] = budget_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                       sc.ior_env)
    return _REFS[name]


@pytest.mark.parametrize("name", CASES)
def test_helper_identities(oracle_mod, name):
    """power_in = dissipated + escaped + terminated + measured + absorbed + kept per
    iteration and kept_i - culled_i = power_in_{i+1}, on exactly rounded sums of
    the helper's terms, each within n 2^-52 sum|terms|."""
    ref = cpu_reference(oracle_mod, name)
    assert_case_claims(name, ref)
    per, between = budget_ref.residues(ref)
    assert len(per) == len(ref["iters"]) and len(between) == len(per) - 1
    for i, (r, bound) in enumerate(per):
        print(name, "iteration", i, "residue", r, "bound", bound)
        assert abs(r) <= bound, (name, i, r, bound)
    for i, (r, bound) in enumerate(between):
        print(name, "between", i, "residue", r, "bound", bound)
        assert abs(r) <= bound, (name, i, r, bound)
    # the measured column is the loop's own per-mesh measured power
    for m in range(ref["K"]):
        budget_ref.assert_sum(ref["mesh_power"][m], budget_ref.mesh_terms(ref, "measured", m), (name, "mesh", m))
    # every ray is in exactly one of the hit categories
    for it in ref["iters"]:
        n = len(it["power_in"][0])
        assert n == sum(len(it[c][0]) for c in ("escaped", "terminated", "measured", "absorbed"))
        assert len(it["kept"][0]) == n and len(it["dissipated"][0]) <= n


def test_helper_with_cutoff(oracle_mod):
    """With a cutoff the culled children leave between the iterations."""
    import cutoff_ref
    sc = case_scene("nested_cubes")
    o, d, p = rays_of(sc)
    ref = budget_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env,
                           cut=cutoff_ref.cut_of(p, 1e-3))
    assert sum(len(c) for c in ref["culled"]) > 0
    per, between = budget_ref.residues(ref)
    for r, bound in per + between:
        assert abs(r) <= bound


def test_host_api():
    """The library exports the entry points, lpc.h declares them, the ABI version
    stays, _lib.py binds them and the Python layers take the keyword."""
    from lightpycl_amd import _lib
    from lightpycl_amd.build import build
    build(verbose=False)
    L = _lib.load()
    assert L.lpc_abi_version() == 4
    for name in ("lpc_trace_set_budget", "lpc_trace_budget"):
        assert name in _lib.EXPORTED
        getattr(L, name)
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib._PROTOS["lpc_trace_set_budget"] == [P, ctypes.c_int]
    assert _lib._PROTOS["lpc_trace_budget"] == [P, P, I32, P, P, P, I32]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lpc.h")).read())
    assert "int lpc_trace_set_budget(lpc_handle *h, int on);" in hdr
    assert ("int lpc_trace_budget(lpc_handle *h, lpc_budget_iter *per_iter, int32_t iter_cap, int32_t *n_iter, "
            "double *mesh_power, int64_t *mesh_count, int32_t mesh_cap);") in hdr
    assert "#define LPC_ABI_VERSION 4" in hdr
    # lpc_budget_iter: seven doubles, six int64, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} lpc_budget_iter;", hdr).group(1)
    names = re.findall(r"\b(power_in|dissipated|escaped|terminated|measured|absorbed|kept|n_\w+)\b",
                       re.sub(r"/\*.*?\*/", "", body))
    assert tuple(names) == _lib.BUDGET_SUMS + _lib.BUDGET_COUNTS
    assert ctypes.sizeof(_lib.BudgetIter) == 13 * 8
    assert [f[0] for f in _lib.BudgetIter._fields_] == names
    # a null handle is refused
    n = ctypes.c_int32(7)
    assert L.lpc_trace_set_budget(None, 1) == -1
    assert L.lpc_trace_budget(None, None, 0, ctypes.byref(n), None, None, 0) == -1
    # the Python surface
    from lightpycl_amd.distributed import ShardedTrace  # noqa: F401
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import CL_Tracer
    from lightpycl_amd.pool import TracePool
    assert callable(Engine.set_budget) and callable(Engine.budget) and callable(CL_Tracer.power_budget)
    for fn in (CL_Tracer.iterative_tracer, TracePool.submit):
        assert inspect.signature(fn).parameters["power_budget"].default is False
