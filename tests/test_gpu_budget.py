"""GPU tests of the power budget (lpc_trace_set_budget / lpc_trace_budget) on
every trace path, against the host helper (tests/budget_ref.py) over the
reference's OWN kernels (oracle/_ref, tests/ref_gpu.py) when they are built, else
over the CPU oracle: counts exactly, every float64 sum within (n - 1) 2^-53
sum|terms| of the exactly rounded sum of the helper's terms (the bound of any
summation order of identical terms).

The cases (tests/test_budget_host.py) are the smallest that span tiles, chunks
(set_chunk(1000)), several iterations and every category; each reference trace
is computed once."""
import ctypes
import json
import os
import socket
import sys

import numpy as np
import pytest

import budget_ref
import cutoff_ref
from test_budget_host import CASES, assert_case_claims, case_scene, rays_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_REFS = {}


def _case(oracle_mod, checker, name, f=0.0):
    """(scene, rays, cut, helper's reference), the reference once per (case, cutoff)."""
    sc = case_scene(name)
    o, d, p = rays_of(sc)
    cut = cutoff_ref.cut_of(p, f) if f else np.float32(0.0)
    key = (name, f)
    if key not in _REFS:
        _REFS[key] = budget_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len,
                                      sc.ior_env, cut=cut, bounce_fn=checker[0])
    ref = _REFS[key]
    assert_case_claims(name, ref)
    if f:
        assert sum(len(c) for c in ref["culled"]) > 0 and len(ref["iters"]) >= 3, "the case must cull"
    return sc, (o, d, p), cut, ref


def _thr(sc, p):
    return (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))


def _trace_kw(sc, **kw):
    return dict(light_source=sc.sources, meshes=sc.meshes, trace_iterations=sc.iterations,
                trace_until_dissipated=sc.tau, max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, **kw)


def _bits(b):
    """A ledger's exact part and its sums (the sums may differ in their last bits
    from run to run: atomics)."""
    mc = b["mesh_count"]
    if isinstance(mc, dict):
        mc = np.stack([mc[c] for c in budget_ref.MESH_CATS], axis=1)
    return {k: np.asarray(b[k]).tolist() for k in budget_ref.COUNTS}, np.asarray(mc).tolist()


def _engine_trace(e, sc, thr):
    e.reset()
    stats, (cnt, mp) = e.run_local(sc.iterations, thr)
    return stats, cnt, mp


def _stats_bits(stats):
    return [(s.n_in, s.n_reflect, s.n_refract, s.n_measured, np.float64(s.power_next).view(np.int64).item())
            for s in stats]


def _assert_closure(b, ref, what):
    tol = budget_ref.closure_tol(ref)
    print(what, "closure", b["closure"], "tol", tol, "left", b["left"])
    assert abs(b["closure"]) <= tol, (what, b["closure"], tol)


# -- 1. aggregate mode ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_aggregate_mode(oracle_mod, checker, name):
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, _, ref = _case(oracle_mod, checker, name)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=False, power_budget=True))
        b = tr.power_budget()
        assert b is not None
        budget_ref.assert_budget(b, ref, f"{name} aggregate")
        assert [int(v) for v in b["n_in"]] == list(tr.iteration_counts)
        mp = np.asarray(tr.measured_power())
        for m in range(ref["K"]):
            budget_ref.assert_sum(mp[m], budget_ref.mesh_terms(ref, "measured", m), (name, "measured_power", m))
            assert abs(b["mesh"]["measured"][m] - mp[m]) <= 2 * budget_ref.sum_tol(
                budget_ref.mesh_terms(ref, "measured", m))
        assert not b["culled"].any() and not b["n_culled"].any()
        _assert_closure(b, ref, name)
        if name == "nested_cubes":
            assert b["left"] < 0                          # the identities hold with negative terms
        # a second trace on the same tracer: the ledger was cleared, not accumulated
        tr.iterative_tracer(**_trace_kw(sc, keep_results=False, power_budget=True))
        b2 = tr.power_budget()
        budget_ref.assert_budget(b2, ref, f"{name} aggregate, second trace")
        assert _bits(b2) == _bits(b)
    finally:
        tr.engine.close()


# -- 2. results mode -----------------------------------------------------------------
@pytest.mark.parametrize("name,chunk", [("cube", 0), ("mixed", 0), ("eye", 0), ("eye", 1000)])
def test_results_mode(oracle_mod, checker, monkeypatch, name, chunk):
    """keep_results=True (k_shade + k_count / k_scatter), also in several chunks per
    iteration: the ledger equals the helper's and the results tuples are
    bit-equal to a run with the ledger off."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, _, ref = _case(oracle_mod, checker, name)
    if chunk:
        monkeypatch.setenv("LPC_CHUNK", str(chunk))
        assert max(ref["counts"]) > chunk
    out = []
    for on in (True, False):
        tr = CL_Tracer(device=0)
        try:
            res = tr.iterative_tracer(**_trace_kw(sc, keep_results=True, power_budget=on))
            res = [tuple(np.array(a) for a in r) for r in res]
            out.append((res, list(tr.iteration_counts), list(tr.power_left), tr.power_budget()))
        finally:
            tr.engine.close()
    (ra, ca, pa, b), (rb, cb, pb, none) = out
    assert none is None
    assert ca == cb == ref["counts"] and pa == pb and len(ra) == len(rb)
    for x, y in zip(ra, rb):
        for u, v in zip(x, y):
            assert u.shape == v.shape and u.dtype == v.dtype
            assert np.array_equal(u.view(np.int32), v.view(np.int32))
    budget_ref.assert_budget(b, ref, f"{name} results chunk {chunk}")
    _assert_closure(b, ref, name)


# -- 3. paths ------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["chunks", "resort", "traced0", "staged", "rerun"])
@pytest.mark.parametrize("name", ["eye", "mixed"])
def test_paths(oracle_mod, checker, monkeypatch, name, path):
    """Several chunks per iteration (set_chunk(1000)), re-sorted populations
    (LPC_RESORT_MIN=1000), LPC_TRACED=0, streamed staged batches and rerun (the
    trace and its reset in one call); the environment cases on a fresh Engine."""
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, name)
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
            assert max(ref["counts"]) > 1000
        e.set_budget(True)
        first = None
        for rep in range(3):                    # the later traces on the first's speculation history
            if path == "staged":
                e.stage_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _ = e.run_staged(sc.iterations, thr)
            elif path == "rerun":
                if rep == 0:
                    e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _ = e.run_local(sc.iterations, thr, reset=True)
            else:
                if rep == 0:
                    e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
                stats, _, _ = _engine_trace(e, sc, thr)
            b = e.budget()
            assert [int(s.n_in) for s in stats] == ref["counts"]
            budget_ref.assert_budget(b, ref, f"{name} {path} trace {rep}")
            assert first is None or _bits(b) == first
            first = first or _bits(b)
    finally:
        e.close()


def test_device_source(oracle_mod, checker):
    """An on_device=True source (lpc_trace_set_rays_dev): the ledger equals the
    helper's over the source's fetched rays."""
    from lightpycl_amd import light_source as lsrc
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc = case_scene("mixed")
    np.random.seed(1)
    src = lsrc.light_source(center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1), power=1000.,
                            ray_count=2000, on_device=True)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer([src], sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                            max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False, power_budget=True)
        assert "sources" not in tr.phase_s and src.__dict__.get("_dev") is not None
        b = tr.power_budget()
        o, d, p = src.__dict__["_dev"].fetch()
    finally:
        tr.engine.close()
    ref = budget_ref.trace(oracle_mod, sc.meshes, o, d, p, sc.iterations, sc.tau, sc.max_ray_len, sc.ior_env,
                           bounce_fn=checker[0])
    t = budget_ref.totals(ref)
    assert t["dissipated"] > 0 and t["measured"] > 0 and t["absorbed"] > 0 and len(ref["iters"]) >= 2
    budget_ref.assert_budget(b, ref, "device source")
    _assert_closure(b, ref, "device source")


# -- 4. with the cutoff --------------------------------------------------------------
@pytest.mark.parametrize("name,f", [("eye", 1e-6), ("nested_cubes", 1e-3)])
@pytest.mark.parametrize("keep", [False, True])
def test_with_cutoff(oracle_mod, checker, name, f, keep):
    """Both ledgers on: each equals the helper's (over cutoff_ref.trace_rays), kept
    is taken before the cutoff, and kept_i - culled_i = power_in_{i+1}."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, _, cut, ref = _case(oracle_mod, checker, name, f)
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, min_ray_power=cut, power_budget=True))
        b = tr.power_budget()
        cc, cp = list(tr.culled_counts), list(tr.culled_power)
    finally:
        tr.engine.close()
    budget_ref.assert_budget(b, ref, f"{name} cut")
    cutoff_ref.assert_ledger(cc, cp, ref["culled"], f"{name} cut")
    assert b["n_culled"].tolist() == cc and b["culled"].tolist() == cp
    between = budget_ref.residues(ref)[1]
    for i in range(len(ref["iters"]) - 1):
        terms = ([float(v) for v in ref["iters"][i]["kept"][0]] + [float(v) for v in ref["culled"][i]] +
                 [float(v) for v in ref["iters"][i + 1]["power_in"][0]])
        tol = budget_ref.sum_tol(terms) + abs(between[i][0]) + 2.0 ** -52 * sum(abs(float(b[k][j])) for k, j in
                                                          (("kept", i), ("culled", i), ("power_in", i + 1)))
        r = (b["kept"][i] - b["culled"][i]) - b["power_in"][i + 1]
        print(name, "between", i, "residue", r, "tol", tol)
        assert abs(r) <= tol, (name, i, r, tol)
    _assert_closure(b, ref, f"{name} cut")


# -- 5. speculation and reuse --------------------------------------------------------
@pytest.mark.parametrize("name", ["eye", "mixed"])
def test_budget_changes_on_one_handle(oracle_mod, checker, name):
    """off, on, on, off on one handle (the later traces run on the earlier ones'
    speculation history, device-sized iterations included): each "on" trace's
    ledger equals a fresh handle's and the helper's -- every ray counted once --
    and each "off" trace is bit-equal, in stats and measured record, to a handle
    that never had the ledger on."""
    from parity_util import measured_rows
    from lightpycl_amd.engine import Engine
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, name)
    thr = _thr(sc, p)

    def one(e, on):
        e.set_budget(on)
        stats, cnt, mp = _engine_trace(e, sc, thr)
        return (_stats_bits(stats), int(cnt), np.asarray(mp).tolist(), measured_rows(*e.fetch_measured()),
                e.budget())

    fresh = {}
    for on in (False, True):
        e = Engine(0)
        try:
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            if not on:                          # never had the ledger on
                stats, cnt, mp = _engine_trace(e, sc, thr)
                fresh[on] = (_stats_bits(stats), int(cnt), np.asarray(mp).tolist(),
                             measured_rows(*e.fetch_measured()), e.budget())
            else:
                fresh[on] = one(e, True)
        finally:
            e.close()
    assert len(fresh[False][4]["n_in"]) == 0
    budget_ref.assert_budget(fresh[True][4], ref, f"{name} fresh")
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        for k, on in enumerate((False, True, True, False)):
            got, want = one(e, on), fresh[on]
            assert got[:3] == want[:3] == fresh[False][:3], (k, on)
            np.testing.assert_array_equal(got[3], fresh[False][3], err_msg=f"trace {k}")
            if on:
                budget_ref.assert_budget(got[4], ref, f"{name} trace {k}")
                assert _bits(got[4]) == _bits(want[4])
            else:
                assert len(got[4]["n_in"]) == 0 and not got[4]["mesh_count"].any()
    finally:
        e.close()


# -- 6. off is off -------------------------------------------------------------------
def _live_bytes():
    from lightpycl_amd import _lib
    d, p = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().lpc_debug_live_bytes(ctypes.byref(d), ctypes.byref(p)))
    return d.value, p.value


@pytest.mark.parametrize("keep", [True, False])
def test_off_is_off(keep):
    """No keyword and power_budget=False: identical stats and measured record, no
    ledger rows; and the library's buffers balance over open, trace with the
    ledger, close."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc = case_scene("eye")
    out = []
    for kw in (dict(), dict(power_budget=False)):
        tr = CL_Tracer(device=0)
        try:
            res = tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, **kw))
            res = [tuple(np.array(a) for a in r) for r in res]
            pos, pw = tr.get_measured_rays()
            out.append((list(tr.iteration_counts), list(tr.power_left), np.asarray(pos), np.asarray(pw),
                        np.asarray(tr.measured_power()), res))
            assert len(tr.iteration_counts) >= 3 and tr.power_budget() is None
            b = tr.engine.budget()
            assert len(b["n_in"]) == 0 and len(b["power_in"]) == 0
            assert not b["mesh_power"].any() and not b["mesh_count"].any()
        finally:
            tr.engine.close()
    a, b = out
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:5], b[2:5]):
        assert np.array_equal(x, y)
    assert len(a[5]) == len(b[5])
    for x, y in zip(a[5], b[5]):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    before = _live_bytes()
    tr = CL_Tracer(device=0)
    try:
        tr.iterative_tracer(**_trace_kw(sc, keep_results=keep, power_budget=True))
        assert len(tr.power_budget()["n_in"]) == len(a[0])
        assert _live_bytes()[0] > before[0]
    finally:
        tr.engine.close()
    assert _live_bytes() == before


# -- 7. argument checks --------------------------------------------------------------
def test_argument_checks():
    from lightpycl_amd import _lib
    from lightpycl_amd.engine import Engine
    sc = case_scene("mixed")
    o, d, p = rays_of(sc)
    K = len(sc.meshes)
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_budget(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        stats, _, _ = _engine_trace(e, sc, _thr(sc, p))
        L, n = e.L, ctypes.c_int32(-1)
        # NULL buffers with a zero cap: only n_iter
        assert L.lpc_trace_budget(e.h, None, 0, ctypes.byref(n), None, None, 0) == 0
        assert n.value == len(stats) >= 2
        # mesh_cap < K: LPC_E_ARG, nothing written
        rows = (_lib.BudgetIter * n.value)()
        ctypes.memset(rows, 0x5a, ctypes.sizeof(rows))
        mp = np.full((K, 4), 7.5, np.float64)
        mc = np.full((K, 4), 7, np.int64)
        n2 = ctypes.c_int32(-1)
        rc = L.lpc_trace_budget(e.h, ctypes.cast(rows, ctypes.c_void_p), n.value, ctypes.byref(n2), _lib.ptr(mp),
                                _lib.ptr(mc), K - 1)
        assert rc == -1 and b"mesh" in L.lpc_last_error(e.h)
        assert n2.value == -1 and (mp == 7.5).all() and (mc == 7).all()
        assert bytes(rows) == b"\x5a" * ctypes.sizeof(rows)
        # a missing row buffer with a positive cap
        assert L.lpc_trace_budget(e.h, None, 1, ctypes.byref(n2), None, None, 0) == -1
        # fewer rows than iterations: only those are written
        assert L.lpc_trace_budget(e.h, ctypes.cast(rows, ctypes.c_void_p), 1, ctypes.byref(n2), None, None, 0) == 0
        assert n2.value == n.value and rows[0].n_in == len(p)
        assert bytes(rows)[ctypes.sizeof(_lib.BudgetIter):] == b"\x5a" * (ctypes.sizeof(rows) - 13 * 8)
        # the ledger is cleared with the measured record
        e.reset()
        assert L.lpc_trace_budget(e.h, None, 0, ctypes.byref(n2), None, None, 0) == 0 and n2.value == 0
        assert not e.budget()["mesh_count"].any()
    finally:
        e.close()


# -- 8. TracePool --------------------------------------------------------------------
def test_pool_submit_with_budget(oracle_mod, checker):
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import budget_dict
    from lightpycl_amd.pool import TracePool
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "eye")
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_budget(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _engine_trace(e, sc, _thr(sc, p))
        single = budget_dict(e.budget())
    finally:
        e.close()
    with TracePool(sc.meshes, engines=2) as pool:
        # with, without, without, with: every batch sets its own switch (omitted = off)
        futs = [pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, power_budget=True),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau),
                pool.submit(o, d, p, sc.max_ray_len, sc.ior_env, sc.iterations, sc.tau, power_budget=True)]
        got = [f.result(timeout=120) for f in futs]
    for g, on in zip(got, (True, False, False, True)):
        assert g["counts"] == ref["counts"]
        if on:
            b = g["power_budget"]
            budget_ref.assert_budget(b, ref, "pool")
            assert {k: b[k].tolist() for k in budget_ref.COUNTS} == {k: single[k].tolist() for k in budget_ref.COUNTS}
            assert all(np.array_equal(b["mesh_count"][c], single["mesh_count"][c]) for c in budget_ref.MESH_CATS)
            _assert_closure(b, ref, "pool")
        else:
            assert "power_budget" not in g


# -- 9. two ranks --------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _child(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lightpycl_amd.distributed import ShardedTrace, ShmComm, TorchComm, shard_bounds
    from lightpycl_amd.engine import Engine
    from test_budget_host import mixed_scene
    sc = mixed_scene()
    o, d, p = rays_of(sc)
    lo, hi = shard_bounds(len(p), rank, world)
    eng = Engine(0)
    eng.upload_meshes(sc.meshes)
    eng.set_budget(True)
    eng.set_rays(o[lo:hi], d[lo:hi], p[lo:hi], sc.max_ray_len, sc.ior_env)
    comm = TorchComm(dist)
    iter_comm = ShmComm.from_dist(dist)
    tr = ShardedTrace(eng, comm, iter_comm=iter_comm)
    in_pow = float(np.sum(p[lo:hi], dtype=np.float64))
    runs = []
    for rep in range(2):                            # the second on the first's speculation history
        eng.reset()
        r = tr.run(sc.iterations, sc.tau, in_pow)
        b = r["power_budget"]
        runs.append(dict(counts=r["global_counts"],
                         rows={k: np.asarray(b[k]).tolist() for k in budget_ref.SUMS + tuple(budget_ref.COUNTS)},
                         mesh={c: b["mesh"][c].tolist() for c in budget_ref.MESH_CATS},
                         mesh_count={c: b["mesh_count"][c].tolist() for c in budget_ref.MESH_CATS},
                         left=b["left"], closure=b["closure"]))
    if rank == 0:
        with open(out_path, "w") as fh:
            json.dump(runs, fh)
    tr.close()
    iter_comm.close()
    eng.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_two_processes(oracle_mod, checker, tmp_path):
    """Two processes, each tracing its shard of `mixed` with the ledger on: the
    rank-summed counts are exactly the single device's (a speculative iteration a
    rank drops is not counted), the sums within the bound of the helper's."""
    import torch.multiprocessing as mp
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import budget_dict
    sc, (o, d, p), _, ref = _case(oracle_mod, checker, "mixed")
    e = Engine(0)
    try:
        e.upload_meshes(sc.meshes)
        e.set_budget(True)
        e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
        _engine_trace(e, sc, _thr(sc, p))
        single = budget_dict(e.budget())
    finally:
        e.close()
    budget_ref.assert_budget(single, ref, "single device")
    out = str(tmp_path / "r.json")
    mp.spawn(_child, args=(2, _free_port(), out), nprocs=2, join=True)
    runs = json.load(open(out))
    for r in runs:
        assert r["counts"] == ref["counts"]
        b = {k: np.asarray(v) for k, v in r["rows"].items()}
        b["mesh"] = {c: np.asarray(v) for c, v in r["mesh"].items()}
        b["mesh_count"] = {c: np.asarray(v) for c, v in r["mesh_count"].items()}
        for k in budget_ref.COUNTS:
            assert b[k].tolist() == single[k].tolist(), k
        for c in budget_ref.MESH_CATS:
            assert b["mesh_count"][c].tolist() == single["mesh_count"][c].tolist(), c
        budget_ref.assert_budget(b, ref, "two ranks")
        assert abs(r["closure"]) <= budget_ref.closure_tol(ref)
