"""GPU tests of the per-ray power cutoff (lpc_trace_set_min_power) and its
culled-power ledger (lpc_trace_culled) on every trace path, against the
reference's host loop with the rule (tests/cutoff_ref.py) over the reference's
OWN kernels (oracle/_ref, tests/ref_gpu.py): results tuples element for
element, aggregate traces as in parity_util.assert_aggregate_equal, the ledger's
counts exactly and its float64 powers within the summation bound.

The shapes (eye 400, lens / nested_cubes / synthetic_dense 2 000) are the
smallest at which the populations still span tiles, chunks (set_chunk(1000))
and several iterations.  The reference traces are computed once per case."""
import json
import os
import socket
import sys

import numpy as np
import pytest

import cutoff_ref
from lightpycl_amd import scenes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# scene, rays, cutoff as a fraction of the mean emitted ray's power
RESULT_CASES = [("eye", 400, 1e-6), ("lens", 2000, 1e-4), ("nested_cubes", 2000, 1e-3)]
AGG_CASES = RESULT_CASES + [("synthetic_dense", 2000, 1e-6)]


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


_SCENES, _REFS = {}, {}


def _scene(name, n):
    if (name, n) not in _SCENES:
        _SCENES[(name, n)] = scenes.BUILDERS[name](n=n)
    return _SCENES[(name, n)]


def _reference(oracle_mod, exact_ref, sc, o, d, p, cut, key):
    """The helper over the reference's kernels, once per case: results tuples, the
    aggregate triple (counts, per-mesh power, sorted measured rows), culled powers."""
    from parity_util import measured_rows
    if key not in _REFS:
        meas = []
        res, info = cutoff_ref.trace_rays(oracle_mod, o, d, p, sc.meshes, sc.iterations, sc.tau, sc.max_ray_len,
                                          sc.ior_env, cut=cut, keep_results=True, bounce_fn=exact_ref.bounce,
                                          measured_out=meas)
        pos = np.concatenate([m[0] for m in meas])
        pw = np.concatenate([m[1] for m in meas])
        mm = np.concatenate([m[2] for m in meas])
        _REFS[key] = dict(results=res, culled=info["culled"],
                          agg=(list(info["counts"]), np.asarray(info["mesh_power"]), measured_rows(pos, pw, mm)))
    return _REFS[key]


def _case(oracle_mod, exact_ref, name, n, f):
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    sc = _scene(name, n)
    o, d, p = rays_of(sc)
    cut = cutoff_ref.cut_of(p, f) if f else np.float32(0.0)
    # the reference loop keeps the source's own power shape in iteration 0's tuple (:116, :347)
    p_ref = np.float32(sc.sources[0].rays_power) if len(sc.sources) == 1 else p
    ref = _reference(oracle_mod, exact_ref, sc, o, d, p_ref, cut, (name, n, f))
    if f:
        assert sum(len(c) for c in ref["culled"]) > 0 and len(ref["agg"][0]) >= 3, "the case must cull"
    return sc, (o, d, p), cut, ref


def _tracer_aggregate(tr):
    from parity_util import measured_rows
    pos, p, mm = tr.engine.fetch_measured()
    return list(tr.iteration_counts), np.asarray(tr.measured_power()), measured_rows(pos, p, mm)


def _engine_trace(e, sc, thr, reps=3):
    """parity_util.lib_aggregate (reset + lpc_trace_run, `reps` back-to-back traces
    with identical bits) with the ledger: it must repeat bit for bit as well."""
    from parity_util import lib_aggregate
    first = None
    for _ in range(reps):
        agg = lib_aggregate(e, sc.iterations, thr, reps=1)
        cc, cp = e.culled()
        got = (agg[0], agg[1].tolist(), cc.tolist(), cp.view(np.int64).tolist())
        assert first is None or got == first[0], "back-to-back traces differ"
        assert first is None or np.array_equal(agg[2], first[1][2])
        first = first or (got, agg, cc, cp)
    return first[1], first[2], first[3]


def _thr(sc, p):
    return (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))


# -- 1. results mode -----------------------------------------------------------------
@pytest.mark.parametrize("name,n,f,chunk", [c + (0,) for c in RESULT_CASES] + [("eye", 400, 1e-6, 1000)])
def test_results_mode(oracle_mod, exact_ref, monkeypatch, name, n, f, chunk):
    """keep_results=True (k_count / k_scatter), also in several chunks per
    iteration (LPC_CHUNK=1000 below the eye's populations)."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, cut, ref = _case(oracle_mod, exact_ref, name, n, f)
    if chunk:
        monkeypatch.setenv("LPC_CHUNK", str(chunk))
        assert max(ref["agg"][0]) > chunk
    tr = CL_Tracer(device=0)
    try:
        res = tr.iterative_tracer(light_source=sc.sources, meshes=sc.meshes, trace_iterations=sc.iterations,
                                  trace_until_dissipated=sc.tau, max_ray_len=sc.max_ray_len, ior_env=sc.ior_env,
                                  keep_results=True, min_ray_power=cut)
        assert [len(r[3]) for r in res] == ref["agg"][0]
        for it, (a, b) in enumerate(zip(res, ref["results"])):
            np.testing.assert_array_equal(a[0][:, :3], b[0][:, :3], err_msg=f"origin it{it}")
            np.testing.assert_array_equal(a[1][:, :3], b[1][:, :3], err_msg=f"dest it{it}")
            assert a[2].shape == b[2].shape
            np.testing.assert_array_equal(a[2], b[2], err_msg=f"pow it{it}")
            np.testing.assert_array_equal(a[3], b[3], err_msg=f"meas it{it}")
        cutoff_ref.assert_ledger(tr.culled_counts, tr.culled_power, ref["culled"], f"{name} results")
        assert tr.power_culled() == pytest.approx(sum(float(v) for c in ref["culled"] for v in c), rel=1e-12)
    finally:
        tr.engine.close()


# -- 2. aggregate mode ---------------------------------------------------------------
@pytest.mark.parametrize("name,n,f", AGG_CASES)
def test_aggregate_mode(oracle_mod, exact_ref, name, n, f):
    from parity_util import assert_aggregate_equal
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, cut, ref = _case(oracle_mod, exact_ref, name, n, f)
    tr = CL_Tracer(device=0)
    try:
        runs = []
        for rep in range(3):                                       # back to back: identical bits, ledger included
            tr.iterative_tracer(light_source=sc.sources, meshes=sc.meshes, trace_iterations=sc.iterations,
                                trace_until_dissipated=sc.tau, max_ray_len=sc.max_ray_len, ior_env=sc.ior_env,
                                keep_results=False, min_ray_power=cut)
            agg = _tracer_aggregate(tr)
            runs.append((agg, list(tr.culled_counts), list(tr.culled_power)))
        agg, cc, cp = runs[0]
        assert_aggregate_equal(agg, ref["agg"], f"{name} aggregate cut {cut}")
        cutoff_ref.assert_ledger(cc, cp, ref["culled"], f"{name} aggregate")
        for other, oc, op in runs[1:]:
            assert other[0] == agg[0] and oc == cc
            assert np.array_equal(other[1], agg[1]) and np.array_equal(other[2], agg[2])
            assert np.array_equal(np.float64(op).view(np.int64), np.float64(cp).view(np.int64))
    finally:
        tr.engine.close()


# -- 3. paths ------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["chunks", "resort", "traced0", "staged"])
@pytest.mark.parametrize("name,n,f", AGG_CASES)
def test_paths(oracle_mod, exact_ref, monkeypatch, name, n, f, path):
    """Several chunks per iteration (set_chunk(1000)), re-sorted populations
    (LPC_RESORT_MIN=1000), LPC_TRACED=0, and streamed staged batches; the
    environment cases on a fresh Engine, as test_population_paths_match_reference."""
    from parity_util import assert_aggregate_equal, measured_rows
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), cut, ref = _case(oracle_mod, exact_ref, name, n, f)
    if path == "resort":
        monkeypatch.setenv("LPC_RESORT_MIN", "1000")
    if path == "traced0":
        monkeypatch.setenv("LPC_TRACED", "0")
    thr = _thr(sc, p)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        if path == "chunks":
            e.set_chunk(1000)
            assert max(ref["agg"][0]) > 1000
        e.set_min_power(cut)
        if path == "staged":
            first = None
            for rep in range(3):
                e.stage_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, (cnt, mp) = e.run_staged(sc.iterations, thr)
                cc, cp = e.culled()
                agg = ([int(s.n_in) for s in stats], np.asarray(mp), measured_rows(*e.fetch_measured()))
                got = (agg[0], agg[1].tolist(), cc.tolist(), cp.view(np.int64).tolist())
                assert first is None or got == first
                first = first or got
        else:
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            agg, cc, cp = _engine_trace(e, sc, thr)
    finally:
        e.close()
    assert_aggregate_equal(agg, ref["agg"], f"{name} {path}")
    cutoff_ref.assert_ledger(cc, cp, ref["culled"], f"{name} {path}")


def test_device_source(oracle_mod, exact_ref):
    """An on_device=True source (lpc_trace_set_rays_dev): the trace with a cutoff
    equals the helper's over the source's fetched rays."""
    from parity_util import assert_aggregate_equal
    from lightpycl_amd import light_source as lsrc
    from lightpycl_amd.iterative_tracer import CL_Tracer
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    sc = _scene("lens", 2000)
    np.random.seed(1)
    src = lsrc.light_source(center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1), power=1000.,
                            ray_count=2000, on_device=True)
    tr = CL_Tracer(device=0)
    try:
        p = np.asarray(src.__dict__["_dev"].fetch(origin=False, dirs=False)[2], np.float32)
        cut = cutoff_ref.cut_of(p, 1e-4)
        tr.iterative_tracer([src], sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                            max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False, min_ray_power=cut)
        assert "sources" not in tr.phase_s and src.__dict__.get("_dev") is not None
        agg = _tracer_aggregate(tr)
        cc, cp = list(tr.culled_counts), list(tr.culled_power)
        o, d, p = src.__dict__["_dev"].fetch()
    finally:
        tr.engine.close()
    ref = _reference(oracle_mod, exact_ref, sc, o, d, p, cut, ("lens-device", 2000, 1e-4))
    assert sum(len(c) for c in ref["culled"]) > 0
    assert_aggregate_equal(agg, ref["agg"], "device source")
    cutoff_ref.assert_ledger(cc, cp, ref["culled"], "device source")


# -- 4. speculation ------------------------------------------------------------------
@pytest.mark.parametrize("name,n,f", [("eye", 400, 1e-6), ("synthetic_dense", 2000, 1e-6)])
def test_cut_changes_on_one_handle(oracle_mod, exact_ref, name, n, f):
    """cut 0, c, c, 0 on one handle (the third trace runs on the second's
    speculation history, the others after the history was dropped): each trace
    equals a fresh handle's trace with that cut, the reference's included."""
    from parity_util import assert_aggregate_equal, lib_aggregate
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), cut, ref = _case(oracle_mod, exact_ref, name, n, f)
    _, _, _, ref0 = _case(oracle_mod, exact_ref, name, n, 0.0)
    thr = _thr(sc, p)

    def one(e, c):
        e.set_min_power(c)
        e.reset()
        stats, (cnt, mp) = e.run_local(sc.iterations, thr)
        cc, cp = e.culled()
        from parity_util import measured_rows
        return ([(s.n_in, s.n_reflect, s.n_refract, s.n_measured, s.power_next) for s in stats], int(cnt),
                mp.tolist(), cc.tolist(), cp.view(np.int64).tolist(), measured_rows(*e.fetch_measured()))

    fresh = {}
    for c in (np.float32(0.0), cut):
        e = Engine(0)
        try:
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            fresh[float(c)] = one(e, c)
        finally:
            e.close()
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        for k, c in enumerate((np.float32(0.0), cut, cut, np.float32(0.0))):
            got, want = one(e, c), fresh[float(c)]
            assert got[:5] == want[:5], (k, float(c))
            np.testing.assert_array_equal(got[5], want[5], err_msg=f"trace {k}")
    finally:
        e.close()
    for c, r in ((0.0, ref0), (float(cut), ref)):
        w = fresh[c]
        assert_aggregate_equal(([s[0] for s in w[0]], np.asarray(w[2]), w[5]), r["agg"], f"{name} cut {c}")
        cutoff_ref.assert_ledger(w[3], np.asarray(w[4], np.int64).view(np.float64), r["culled"], f"{name} cut {c}")


# -- 5. off is off -------------------------------------------------------------------
@pytest.mark.parametrize("keep", [True, False])
def test_off_is_off(keep):
    """min_ray_power=0.0 and no keyword: identical stats and measured record, a
    ledger of zeros."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc = _scene("eye", 400)
    out = []
    for kw in (dict(), dict(min_ray_power=0.0)):
        tr = CL_Tracer(device=0)
        try:
            res = tr.iterative_tracer(light_source=sc.sources, meshes=sc.meshes, trace_iterations=sc.iterations,
                                      trace_until_dissipated=sc.tau, max_ray_len=sc.max_ray_len,
                                      ior_env=sc.ior_env, keep_results=keep, **kw)
            pos, pw = tr.get_measured_rays()
            out.append((list(tr.iteration_counts), list(tr.power_left), np.asarray(pos), np.asarray(pw),
                        np.asarray(tr.measured_power()), res))
            n = len(tr.iteration_counts)
            assert n >= 3 and tr.culled_counts == [0] * n and tr.culled_power == [0.0] * n
            assert tr.power_culled() == 0.0
            cc, cp = tr.engine.culled()
            assert len(cc) == n and not cc.any() and not cp.any()
        finally:
            tr.engine.close()
    a, b = out
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:5], b[2:5]):
        assert np.array_equal(x, y)
    assert len(a[5]) == len(b[5])
    for x, y in zip(a[5], b[5]):
        for u, v in zip(x, y):
            assert np.array_equal(np.asarray(u), np.asarray(v))


def test_engine_argument_checks(engine):
    from lightpycl_amd._lib import LpcError
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(LpcError):
            engine.set_min_power(bad)
    engine.set_min_power(0.0)


# -- 6. TracePool --------------------------------------------------------------------
def test_pool_submit_with_cutoff(oracle_mod, exact_ref):
    from parity_util import assert_aggregate_equal, measured_rows
    from lightpycl_amd.pool import TracePool
    sc, (o, d, p), cut, ref = _case(oracle_mod, exact_ref, "eye", 400, 1e-6)
    _, _, _, ref0 = _case(oracle_mod, exact_ref, "eye", 400, 0.0)
    with TracePool(sc.meshes, engines=2) as pool:
        # with, without, with: every batch sets its own cutoff (omitted = off)
        futs = [pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, measured=True,
                            min_ray_power=cut),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, measured=True),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, measured=True),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, measured=True,
                            min_ray_power=cut)]
        got = [f.result(timeout=120) for f in futs]
    for g, r, with_cut in zip(got, (ref, ref0, ref0, ref), (True, False, False, True)):
        assert_aggregate_equal((g["counts"], g["mesh_power"], measured_rows(*g["measured"])), r["agg"], "pool")
        if with_cut:
            cutoff_ref.assert_ledger(g["culled_counts"], g["culled_power"], r["culled"], "pool")
        else:
            assert "culled_counts" not in g


# -- 7. two ranks --------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _child(rank, world, port, name, n, f, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lightpycl_amd.distributed import ShardedTrace, ShmComm, TorchComm, shard_bounds
    from lightpycl_amd.engine import Engine
    sc = scenes.BUILDERS[name](n=n)
    o, d, p = rays_of(sc)
    cut = cutoff_ref.cut_of(p, f)
    lo, hi = shard_bounds(len(p), rank, world)
    eng = Engine(0)
    eng.upload_meshes(sc.meshes)
    eng.set_min_power(cut)
    eng.set_rays(o[lo:hi], d[lo:hi], p[lo:hi], sc.max_ray_len, sc.ior_env)
    comm = TorchComm(dist)
    iter_comm = ShmComm.from_dist(dist)
    tr = ShardedTrace(eng, comm, iter_comm=iter_comm)
    in_pow = float(np.sum(p[lo:hi], dtype=np.float64))
    runs = []
    for rep in range(2):                            # the second on the first's speculation history
        eng.reset()
        r = tr.run(sc.iterations, sc.tau, in_pow)
        runs.append(dict(counts=r["global_counts"], mesh_power=list(map(float, r["mesh_power"])),
                         culled_counts=r["culled_counts"], culled_power=r["culled_power"]))
    if rank == 0:
        with open(out_path, "w") as fh:
            json.dump(runs, fh)
    tr.close()
    iter_comm.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_two_processes(oracle_mod, exact_ref, tmp_path):
    """Two processes, each tracing its shard with the cutoff: the rank-summed
    ledger equals the single-device trace's counts exactly, its powers within
    the summation order; global counts and per-mesh power as the single device's."""
    import torch.multiprocessing as mp
    from lightpycl_amd.engine import Engine
    name, n, f = "eye", 400, 1e-6
    sc, (o, d, p), cut, ref = _case(oracle_mod, exact_ref, name, n, f)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_min_power(cut)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        single, scc, scp = _engine_trace(e, sc, _thr(sc, p), reps=1)
    finally:
        e.close()
    out = str(tmp_path / "r.json")
    mp.spawn(_child, args=(2, _free_port(), name, n, f, out), nprocs=2, join=True)
    runs = json.load(open(out))
    for r in runs:
        assert r["counts"] == single[0] == ref["agg"][0]
        np.testing.assert_allclose(r["mesh_power"], single[1], rtol=1e-12, atol=1e-300)
        assert r["culled_counts"] == scc.tolist()
        cutoff_ref.assert_ledger(r["culled_counts"], r["culled_power"], ref["culled"], "two ranks")
    cutoff_ref.assert_ledger(scc, scp, ref["culled"], "single device")
    assert runs[0] == runs[1]
