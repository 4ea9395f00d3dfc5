"""GPU tests of the device-born light sources: numpy's generator continued on the
device bit for bit, light_source(on_device=True) against the host source at the
same seed (the criteria of tests/test_emit_host.py, through the public
attributes), np.random's state afterwards, shards, and traces of device sources
against traces of their fetched host copies."""
import emit_util as eu
import numpy as np
import parity_util as pu
import pytest

from lightpycl_amd import _lib, scenes
from lightpycl_amd import light_source as lsrc
from lightpycl_amd.iterative_tracer import CL_Tracer

pytestmark = pytest.mark.gpu


def _state():
    st = np.random.get_state()
    return st[1].copy(), int(st[2])


def _same_state(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def _device_source(n, direction, power, **kw):
    np.random.seed(eu.SEED)
    s = lsrc.light_source(center=eu.center(), direction=direction, power=power, ray_count=n, on_device=True, **kw)
    assert s.__dict__.get("_dev") is not None
    return s


# -- the generator ---------------------------------------------------------------
@pytest.mark.parametrize("n", eu.GEN_COUNTS)
def test_generator_on_the_device_is_numpys_bit_for_bit(engine, n):
    for name, key, pos in eu.generator_states():
        ref, rkey, rpos = eu.numpy_stream(key, pos, n)
        got, gkey, gpos = engine.rng_mt19937(key, pos, n)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (name, n)
        assert gpos == rpos and np.array_equal(gkey, rkey), (name, n, gpos, rpos)
        # a skip of n, then a fill: the tail of one fill
        none, skey, spos = engine.rng_mt19937(key, pos, n, skip=True)
        assert none is None and spos == rpos and np.array_equal(skey, rkey), (name, n)
        tail, _, _ = engine.rng_mt19937(skey, spos, 700)
        whole, _, _ = engine.rng_mt19937(key, pos, n + 700)
        assert np.array_equal(tail.view(np.uint64), whole[n:].view(np.uint64)), (name, n)


# -- light_source(on_device=True) against the host source -------------------------------
@pytest.mark.parametrize("power", eu.POWERS)
@pytest.mark.parametrize("direction", eu.DIRECTIONS)
@pytest.mark.parametrize("n", eu.SIZES)
def test_on_device_source_matches_the_host_source(n, direction, power):
    # the host-only sequence: constructor, collimated, then another source
    ref = eu.host_source(n, direction, power)
    ref_o, ref_d, ref_p = ref.rays_origin, ref.rays_dir, ref.rays_power
    st_ctor = _state()
    ref.random_collimated_rays(diameter=eu.DIAMETER)
    st_coll = _state()
    ref_next = lsrc.light_source(ray_count=33)

    what = f"n={n} dir={direction} power={power}"
    dev = _device_source(n, direction, power)
    assert _same_state(_state(), st_ctor), what
    assert np.array_equal(dev.rays_origin, np.asarray(ref_o)), what
    eu.check_rows(dev.rays_dir, np.asarray(ref_d), 1.0, what + " hemisphere dir")
    eu.check_power(dev.rays_power, ref_p, n, power, what + " hemisphere")        # (n, 1), as the host's
    assert dev.rays_dest.shape == (n, 4) and dev.rays_dest.dtype == np.float32

    dev.random_collimated_rays(diameter=eu.DIAMETER)
    assert _same_state(_state(), st_coll), what
    eu.check_rows(dev.rays_origin, np.asarray(ref.rays_origin), eu.origin_scale(False), what + " collimated origin")
    eu.check_rows(dev.rays_dir, np.asarray(ref.rays_dir), 1.0, what + " collimated dir")
    eu.check_power(dev.rays_power, ref.rays_power, n, power, what + " collimated")   # (n,)
    assert np.array_equal(dev.rays_power, ref.rays_power), what

    nxt = lsrc.light_source(ray_count=33)                           # a host source continues the sequence
    for k in ("rays_origin", "rays_dir", "rays_power"):
        assert np.array_equal(np.asarray(getattr(nxt, k)), np.asarray(getattr(ref_next, k))), (what, k)


@pytest.mark.parametrize("collimated", [False, True])
@pytest.mark.parametrize("axis", ["x", "y", "z"])
@pytest.mark.parametrize("direction", eu.DIRECTIONS)
@pytest.mark.parametrize("n", eu.SIZES)
def test_rotate_on_the_device_matches_the_host(n, direction, axis, collimated):
    """rotate_rays on the device source against the host's rotate_rays of that
    source's own fetched rays (identical inputs)."""
    dev = _device_source(n, direction, 1)
    if collimated:
        dev.random_collimated_rays(diameter=eu.DIAMETER)
    ref = lsrc.light_source(ray_count=1)
    ref.rays_origin, ref.rays_dir = dev.rays_origin, dev.rays_dir
    ref.rotate_rays(axis=axis, pivot=list(eu.PIVOT), ang=eu.ROT_ANGLE)
    dev.rotate_rays(axis=axis, pivot=list(eu.PIVOT), ang=eu.ROT_ANGLE)
    assert dev.__dict__.get("_dev") is not None
    what = f"rotate {axis} n={n} dir={direction} collimated={collimated}"
    eu.check_rows(dev.rays_origin, ref.rays_origin, eu.origin_scale(True), what + " origin")
    eu.check_rows(dev.rays_dir, ref.rays_dir, 1.0, what + " dir")


def test_cos_power_family_and_host_conversion():
    n = 1000
    for m in (0, 1, 2, 3.5):
        np.random.seed(eu.SEED)
        ref = lsrc.light_source(center=eu.center(), direction=(1, 2, 3), power=10, ray_count=n,
                                directivity=lsrc.cos_power(m))
        np.random.seed(eu.SEED)
        dev = lsrc.light_source(center=eu.center(), direction=(1, 2, 3), power=10, ray_count=n,
                                directivity=lsrc.cos_power(m), on_device=True)
        eu.check_power(dev.rays_power, ref.rays_power, n, 10, f"cos_power({m})")
    # an assignment, or grid_rays, makes it an ordinary host source
    fetched = dev.rays_dir
    dev.rays_power = dev.rays_power * 2
    assert dev.__dict__.get("_dev") is None and np.array_equal(dev.rays_dir, fetched)
    dev = _device_source(100, (0, 0, 1), 1)
    dev.grid_rays()
    assert dev.__dict__.get("_dev") is None and dev.rays_dir.shape == (100, 4)


# -- shards ----------------------------------------------------------------------
@pytest.mark.parametrize("collimated", [False, True])
def test_shards_concatenate_to_the_whole_and_runs_repeat(collimated):
    n = 4099

    def emit(**kw):
        s = _device_source(n, (1, 2, 3), 1000, **kw)
        if collimated:
            s.random_collimated_rays(diameter=eu.DIAMETER)
        return s.rays_origin, s.rays_dir, s.rays_power, _state()

    whole, again = emit(), emit()
    parts = [emit(shard=(a, b - a)) for a, b in ((0, 1000), (1000, 1063), (1063, n))]
    for k in range(3):
        assert whole[k].shape[0] == n
        assert np.array_equal(whole[k], again[k]), (collimated, k)   # the sum's order is fixed
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (collimated, k)
    for p in parts:                                                  # every shard advances over all draws
        assert _same_state(p[3], whole[3])
    from lightpycl_amd.distributed import emit_shard, shard_bounds
    assert [emit_shard(n, r, 3) for r in range(3)] == [(lo, hi - lo) for lo, hi in
                                                       (shard_bounds(n, r, 3) for r in range(3))]


# -- traces ------------------------------------------------------------------------
def _host_copy(dev):
    s = lsrc.light_source(ray_count=1)
    s.rays_origin, s.rays_dir, s.rays_power = dev.rays_origin, dev.rays_dir, dev.rays_power
    return s


def _aggregate(tr):
    pos, p, mm = tr.engine.fetch_measured()
    return list(tr.iteration_counts), np.asarray(tr.measured_power()), pu.measured_rows(pos, p, mm)


@pytest.fixture(scope="module")
def lens_scene():
    return scenes.lens(n=10, seed=1)


def _lens_source(n=1000, **kw):
    np.random.seed(1)
    return lsrc.light_source(center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1), power=1000.,
                             ray_count=n, on_device=True, **kw)


def test_trace_of_device_sources_equals_trace_of_their_host_copies(lens_scene):
    sc = lens_scene
    one = _lens_source()
    two = [_lens_source(shard=(0, 600)), _lens_source(700, directivity=lsrc.cos_power(2))]
    for sources in ([one], two):
        a = CL_Tracer(device=0)
        a.iterative_tracer(sources, sc.meshes, trace_iterations=4, max_ray_len=sc.max_ray_len, keep_results=False)
        assert "sources" not in a.phase_s                            # no host arrays were built
        assert all(s.__dict__.get("_dev") is not None for s in sources)
        b = CL_Tracer(device=0)
        b.iterative_tracer([_host_copy(s) for s in sources], sc.meshes, trace_iterations=4,
                           max_ray_len=sc.max_ray_len, keep_results=False)
        assert "sources" in b.phase_s
        A, B = _aggregate(a), _aggregate(b)
        assert A[0][0] == sum(s.__dict__["_dev"].n for s in sources) and len(A[2]) > 0
        pu.assert_aggregate_equal(A, B, "device sources against host copies")
        assert np.array_equal(A[1], B[1])                            # per-mesh power: the same rays, the same order
        # reset + re-run reproduces the trace (the emitted rays' copy is kept)
        thr = (1.0 - 0.99) * sum(s.__dict__["_dev"].power_sum for s in sources)
        again = pu.lib_aggregate(a.engine, 4, thr, reps=2)
        pu.assert_aggregate_equal(again, A, "reset + re-run")
        a.engine.close()
        b.engine.close()


def test_results_mode_fetches_the_device_source(lens_scene):
    sc = lens_scene
    src = _lens_source()
    a = CL_Tracer(device=0)
    ra = a.iterative_tracer([src], sc.meshes, trace_iterations=4, max_ray_len=sc.max_ray_len, keep_results=True)
    b = CL_Tracer(device=0)
    rb = b.iterative_tracer([_host_copy(src)], sc.meshes, trace_iterations=4, max_ray_len=sc.max_ray_len,
                            keep_results=True)
    assert len(ra) == len(rb) > 0 and a.iteration_counts == b.iteration_counts
    for x, y in zip(ra, rb):
        for u, v in zip(x, y):
            assert np.array_equal(np.asarray(u), np.asarray(v))
    a.engine.close()
    b.engine.close()


# -- errors ------------------------------------------------------------------------
def test_errors(engine):
    st = _state()
    with pytest.raises(TypeError, match="cos_power"):
        lsrc.light_source(ray_count=10, directivity=lambda az, el: np.cos(el), on_device=True)
    for shard in ((0, 11), (11, 0), (-1, 2), (5, 6)):
        with pytest.raises(ValueError):
            lsrc.light_source(ray_count=10, on_device=True, shard=shard)
    assert _same_state(_state(), st)
    key, pos = st
    eye = np.eye(3)
    for kw in (dict(n=0), dict(n=10, first=0, count=11), dict(n=10, first=11, count=0), dict(n=10, first=-1, count=1),
               dict(n=10, m=-0.5)):
        args = dict(n=10, first=0, count=None, m=1.0)
        args.update(kw)
        with pytest.raises(_lib.LpcError):
            engine.emit_hemisphere(key, pos, args["n"], eu.center(), eye, eye, m=args["m"], first=args["first"],
                                   count=args["count"])
    with pytest.raises(_lib.LpcError):
        engine.emit_collimated(key, pos, 10, 1.0, eu.center(), eye, eye, [0, 0, 1], first=4, count=7)
    rays, _, _ = engine.emit_hemisphere(key, pos, 10, eu.center(), eye, eye, first=10, count=0)   # an empty shard
    assert rays.n == 0 and rays.power_sum == 0.0


def test_source_of_another_device_falls_back_to_the_fetch_path(lens_scene):
    if _lib.device_count() < 2:
        pytest.skip("needs two GPUs")
    sc = lens_scene
    np.random.seed(1)
    src = lsrc.light_source(power=1000., ray_count=1000, on_device=True, device=1)
    a = CL_Tracer(device=0)
    a.iterative_tracer([src], sc.meshes, trace_iterations=4, max_ray_len=sc.max_ray_len, keep_results=False)
    assert "sources" in a.phase_s                                    # the host path ran on the fetched arrays
    b = CL_Tracer(device=0)
    b.iterative_tracer([_host_copy(src)], sc.meshes, trace_iterations=4, max_ray_len=sc.max_ray_len,
                       keep_results=False)
    pu.assert_aggregate_equal(_aggregate(a), _aggregate(b), "another device's source")
    with pytest.raises(_lib.LpcError):
        a.engine.set_rays_dev([src.__dict__["_dev"]])
    a.engine.close()
    b.engine.close()
