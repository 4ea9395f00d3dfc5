"""The compaction of a bounce -- k_shade_stage + k_stage_move (traced
iterations) and k_shade + k_count / k_scan / k_scatter / k_append (per-ray
export, chunks) -- on populations whose ray fates are constructed
(tests/fate_util.py; tests/test_fate_host.py shows that every ray gets its
intended fate).  A ray's (x, y) names it in every block of the next population
and in the measured record, so the tests see where each row lands:

  (a) layout of a traced iteration: counts, [reflected ; refracted] blocks as
      sets against the reference's children, each block in parent order;
  (b) the reference-order paths, element for element, position included;
  (c) both with chunk sizes that are and are not multiples of the 256-ray tile;
  (d) whole traces: measure-mesh counts 0, 1, 4, 5 (LPC_MP_MAX is 4), K up to 70
      meshes, host-sized, speculative, asynchronous, after a smaller trace;
  (e) the CUT instantiation with children of power exactly 0.

Expected per-ray values come from the `checker` fixture: the reference's own
kernels (bit for bit) or the CPU oracle (the bars of test_gpu_parity._cmp_bounce).
The layout checks are discrete and hold under both.
"""
import math
import types

import numpy as np
import pytest

import cutoff_ref
import fate_util as fu
from parity_util import assert_aggregate_equal, measured_rows
from soup_util import meshes_of, oracle_scene
from test_gpu_parity import _ulps

pytestmark = pytest.mark.gpu

TILE, GROUP = 256, 256 * 256
SMALL = (1, 255, 256, 257, 1023, 1025)
LARGE = (65535, 65536, 65537, 131073)
LARGE_PATTERNS = [fu.uniform("matched"), fu.uniform("terminator"), fu.halves("matched", "terminator"),
                  fu.halves("terminator", "matched"), fu.random(1)]
CHUNKS = (256, 257, 1000, 65536, 70001)
U = 2.0 ** -53


def _id(v):
    return getattr(v, "label", None)


# -- shared inputs and references, computed once -------------------------------------------
_CASES, _BOUNCES, _TRACES = {}, {}, {}


def _case(n_measure, K, pat, n):
    """(scene, fates, (o, d, p)) of one population."""
    key = (n_measure, K, pat.label, n)
    if key not in _CASES:
        sc = fu.layout(n_measure, K)
        fates = pat(n, sc.kinds)
        _CASES[key] = (sc, fates, fu.rays(sc, fates))
    return _CASES[key]


def _bounce(checker, key, sc, rays):
    """The reference's bounce of the emitted rays (the fields the tests read)."""
    if key not in _BOUNCES:
        o, d, p = rays
        n = len(p)
        out = checker[0](oracle_scene(sc.arrs), o, d, p, np.zeros(n, np.int32), np.full(n, -2, np.int32),
                         fu.MAX_RAY_LEN, fu.IOR_ENV)
        _BOUNCES[key] = {k: np.array(out[k]) for k in ("dest", "pow", "meas", "isect_mid", "r_origin", "r_pow",
                                                       "r_meas", "t_origin", "t_pow", "t_meas")}
    return _BOUNCES[key]


def _ref_trace(oracle_mod, checker, key, sc, rays, cut=0.0):
    """The reference's host loop (three iterations, no power stop) with its
    results tuples, the aggregate triple and the culled powers."""
    key = key + (float(cut),)
    if key not in _TRACES:
        o, d, p = rays
        meas = []
        res, info = cutoff_ref.trace_rays(oracle_mod, o, d, p, meshes_of(sc.arrs), 3, 1.0, fu.MAX_RAY_LEN, fu.IOR_ENV,
                                          cut=cut, keep_results=True, bounce_fn=checker[0], measured_out=meas)
        pos = np.concatenate([m[0] for m in meas])
        pw = np.concatenate([m[1] for m in meas])
        mm = np.concatenate([m[2] for m in meas])
        _TRACES[key] = dict(results=res, culled=info["culled"], meas=meas,
                            agg=(list(info["counts"]), np.asarray(info["mesh_power"]), measured_rows(pos, pw, mm)))
    return _TRACES[key]


def _pow_equal(a, b, exact, what):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if exact:
        np.testing.assert_array_equal(a, b, err_msg=what)
    elif a.size:        # test_gpu_parity._cmp_bounce's bar for the CPU oracle
        assert np.all((_ulps(a, b) <= 64) | (np.abs(np.float64(a) - b) <= 1e-6 * np.abs(b).max())), what


def _sum_within(got, terms, exact, what):
    """A float64 sum of non-negative float32 terms in another order: the bound
    parity_util.assert_aggregate_equal states."""
    want = math.fsum(float(v) for v in terms)
    tol = max(1e-12, (len(terms) - 1) * U) + (0.0 if exact else 1e-6)
    assert abs(got - want) <= tol * abs(want) + 1e-300, (what, got, want, len(terms))


def _setup(e, sc, rays, chunk=0, cut=0.0):
    e.upload_arrays(*sc.arrs)
    e.set_chunk(chunk)
    e.set_min_power(cut)
    e.set_rays(*rays, fu.MAX_RAY_LEN, fu.IOR_ENV)


def _read_layout(e, sc, rays, chunk=0, cut=0.0):
    """set_rays, one traced iterate(), then iterate(export=True): the second
    call's origin / pow rows are the population the first call built, in
    population order."""
    _setup(e, sc, rays, chunk, cut)
    st1, _ = e.iterate()
    rec = e.fetch_measured()
    mcount, mpow = e.measured()
    pp = e.population_power()
    cul = e.culled()
    st2, ex = e.iterate(export=True)
    return types.SimpleNamespace(st=st1, st2=st2, origin=ex["origin"], pow=ex["pow"], pp=pp, rec=rec, mcount=mcount,
                                 mpow=np.array(mpow), culled=cul)


def _traced_order(e, n_measure, K, rays, chunk=0):
    """The launch's order of the emitted rays: the same rays over the same
    triangles with every patch matched (the coherence key reads origins,
    directions and the scene box, never a material), where every ray aimed at a
    patch keeps a refracted child.  -> parent index per traced position."""
    L = _read_layout(e, fu.layout(n_measure, K, all_matched=True), rays, chunk)
    ek = fu.ray_key(rays[0][:, :2])
    nR = int(L.st.n_reflect)
    perm = fu.parents_of(fu.ray_key(L.origin[nR:, :2]), ek)
    np.testing.assert_array_equal(fu.parents_of(fu.ray_key(L.origin[:nR, :2]), ek), perm)
    return perm


def _check_layout(L, sc, fates, rays, ref, exact, cut=0.0, perm=None, what=""):
    """The assertions of (a) on one read layout.  -> the parent sequences of the
    reflected block, the refracted block and the measured record."""
    o, d, p = rays
    n = len(p)
    want = fu.intended(sc, fates)
    with np.errstate(invalid="ignore"):
        keepR = (ref["r_meas"] == 0) & ~(np.abs(ref["r_pow"]) < np.float32(cut))
        keepT = (ref["t_meas"] == 0) & ~(np.abs(ref["t_pow"]) < np.float32(cut))
    isM = ref["meas"] == 1
    if cut == 0.0:      # the counts of intended fates
        assert (int(keepR.sum()), int(keepT.sum()), int(isM.sum())) == \
            (int((want["r_meas"] == 0).sum()), int((want["t_meas"] == 0).sum()), int((want["meas"] == 1).sum()))
    nR, nT, nM = int(L.st.n_reflect), int(L.st.n_refract), int(L.st.n_measured)
    assert (int(L.st.n_in), nR, nT, nM) == (n, int(keepR.sum()), int(keepT.sum()), int(isM.sum())), what
    assert L.origin.shape == (nR + nT, 4) and int(L.st2.n_in) == nR + nT, what
    ek = fu.ray_key(o[:, :2])
    par = []
    for name, lo, hi, keep, c in (("reflected", 0, nR, keepR, "r"), ("refracted", nR, nR + nT, keepT, "t")):
        rows, pw = L.origin[lo:hi], L.pow[lo:hi]
        pa = fu.parents_of(fu.ray_key(rows[:, :2]), ek)
        # as a set: every reference child once, none else (the keys are unique per parent)
        np.testing.assert_array_equal(np.sort(pa), np.flatnonzero(keep), err_msg=f"{name} block {what}")
        np.testing.assert_array_equal(rows[:, :3], ref[c + "_origin"][pa, :3], err_msg=f"{name} origins {what}")
        _pow_equal(pw, ref[c + "_pow"][pa], exact, f"{name} power {what}")
        par.append(pa)
    # each block in parent order: parents with both children in the same relative order
    both = keepR & keepT
    np.testing.assert_array_equal(par[0][both[par[0]]], par[1][both[par[1]]], err_msg=f"parent order {what}")
    # the measured record of the iteration
    assert int(L.mcount) == nM and len(L.rec[1]) == nM
    pm = fu.parents_of(fu.ray_key(L.rec[0][:, :2]), ek)
    np.testing.assert_array_equal(np.sort(pm), np.flatnonzero(isM), err_msg=f"measured record {what}")
    np.testing.assert_array_equal(L.rec[0][:, :3], ref["dest"][pm, :3])
    np.testing.assert_array_equal(L.rec[1], ref["pow"].reshape(-1)[pm])       # a measured ray's power is its parent's
    np.testing.assert_array_equal(L.rec[2], ref["isect_mid"][pm])
    # population_power() is the next call's exported power, element for element
    np.testing.assert_array_equal(L.pp, L.pow, err_msg=f"population power {what}")
    # power_next and the per-mesh measured power within the float64 summation bound
    _sum_within(float(L.st.power_next), np.concatenate((ref["r_pow"][keepR], ref["t_pow"][keepT])), exact,
                f"power_next {what}")
    mp_ref = np.zeros(sc.K, np.float64)
    np.add.at(mp_ref, ref["isect_mid"][isM], ref["pow"].reshape(-1)[isM].astype(np.float64))
    assert_aggregate_equal(([n], L.mpow, measured_rows(*L.rec)),
                           ([n], mp_ref, measured_rows(ref["dest"][isM], ref["pow"].reshape(-1)[isM],
                                                       ref["isect_mid"][isM])), what)
    if perm is not None:    # the blocks and the record are the launch's order, filtered
        np.testing.assert_array_equal(par[0], perm[keepR[perm]], err_msg=f"reflected block order {what}")
        np.testing.assert_array_equal(par[1], perm[keepT[perm]], err_msg=f"refracted block order {what}")
        np.testing.assert_array_equal(pm, perm[isM[perm]], err_msg=f"measured record order {what}")
    return par[0], par[1], pm


def _occupancy(perm, keepR, keepT, isM):
    """Per 256-ray tile of the launch's order: (cR, cT, cM)."""
    n = len(perm)
    pad = (-n) % TILE
    c = [np.concatenate((f[perm].astype(np.int64), np.zeros(pad, np.int64))).reshape(-1, TILE).sum(1)
         for f in (keepR, keepT, isM)]
    return np.stack(c, axis=1)


def _groups_empty(occ):
    """Which 256-tile groups keep and measure nothing."""
    t = occ.sum(1)
    pad = (-len(t)) % (GROUP // TILE)
    return np.concatenate((t, np.zeros(pad, np.int64))).reshape(-1, GROUP // TILE).sum(1) == 0


# -- (a) layout of a traced iteration --------------------------------------------------
def _layout_case(engine, checker, n, pat, chunk=0):
    sc, fates, rays = _case(2, None, pat, n)
    key = (2, None, pat.label, n)
    ref = _bounce(checker, key, sc, rays)
    what = f"{pat.label} n {n} chunk {chunk}"
    try:
        # the launch's order of all rays (a chunk sorts its own rays: the same per chunk)
        perm = _traced_order(engine, 2, None, rays, chunk)
        gap = fates == fu.FATES.index("gap")
        np.testing.assert_array_equal(np.sort(perm), np.flatnonzero(~gap))
        L = _read_layout(engine, sc, rays, chunk)
    finally:
        engine.set_chunk(0)
    pR, pT, pM = _check_layout(L, sc, fates, rays, ref, checker[1], perm=perm, what=what)
    occ = None
    if not gap.any() and (chunk == 0 or chunk % TILE == 0 or chunk >= n):
        # no ray without a place in the order: the occupancy of every tile
        # (chunks that are multiples of the tile keep the tiles' borders)
        occ = _occupancy(perm, ref["r_meas"] == 0, ref["t_meas"] == 0, ref["meas"] == 1)
    return sc, fates, rays, L, (pR, pT, pM), occ


@pytest.mark.parametrize("pat", fu.all_patterns(), ids=_id)
@pytest.mark.parametrize("n", SMALL)
def test_layout_small(engine, checker, n, pat):
    sc, fates, rays, L, (pR, pT, pM), occ = _layout_case(engine, checker, n, pat)
    if pat.label == "uniform-matched":
        np.testing.assert_array_equal(pR, pT)
        np.testing.assert_array_equal(np.sort(pR), np.arange(n))
        if n >= TILE:
            assert np.any((occ[:, 0] == TILE) & (occ[:, 1] == TILE)), "a tile with cR = cT = 256"
    if pat.label == "uniform-measure":
        np.testing.assert_array_equal(np.sort(pM), np.arange(n))
        if n >= TILE:
            assert np.any(occ[:, 2] == TILE)


@pytest.mark.parametrize("pat", LARGE_PATTERNS, ids=_id)
@pytest.mark.parametrize("n", LARGE)
def test_layout_large(engine, checker, n, pat):
    sc, fates, rays, L, (pR, pT, pM), occ = _layout_case(engine, checker, n, pat)
    if occ is None:         # rays aimed at the gap have no place in the recovered order
        return
    full = int(np.sum((occ[:, 0] == TILE) & (occ[:, 1] == TILE)))
    empty = _groups_empty(occ)
    print(f"occupancy {pat.label} n {n}: tiles {len(occ)} full {full} empty tiles {int((occ.sum(1) == 0).sum())} "
          f"groups {len(empty)} empty groups {int(empty.sum())}")
    if pat.label == "uniform-matched":
        np.testing.assert_array_equal(pR, pT)
        np.testing.assert_array_equal(np.sort(pR), np.arange(n))
        assert full == n // TILE and not empty.any()            # every whole tile: cR = cT = 256
    if pat.label == "uniform-terminator":
        assert L.origin.shape[0] == 0 and empty.all() and len(empty) == -(-n // GROUP)   # whole groups keep nothing
    if pat.label.startswith("halves"):
        # derived from the recovered order: the beam's coherence order keeps a
        # patch's rays together, so one launch holds full tiles (cR = cT = 256),
        # tiles that keep nothing and, past 65 536 rays, a group that keeps nothing
        # (its count word is never added to)
        assert full >= (n // 2) // TILE - 1 and int((occ.sum(1) == 0).sum()) >= (n // 2) // TILE - 2
        assert n <= GROUP or empty.any()


# -- (b) the paths that keep the reference's order -----------------------------------------
def _export_trace(e, sc, rays, chunk=0, cut=0.0):
    """iterate(export=True) from the first iteration on."""
    _setup(e, sc, rays, chunk, cut)
    out = []
    for _ in range(3):
        st, ex = e.iterate(export=True)
        out.append((st, ex))
        if st.n_reflect + st.n_refract == 0:
            break
    return out


def _assert_results(res, ref, exact, what):
    """Results tuples (origin, dest, pow, meas) against the reference host loop's."""
    assert len(res) == len(ref), (what, len(res), len(ref))
    for it, (a, b) in enumerate(zip(res, ref)):
        np.testing.assert_array_equal(a[0][:, :3], b[0][:, :3], err_msg=f"origin it{it} {what}")
        np.testing.assert_array_equal(a[1][:, :3], b[1][:, :3], err_msg=f"dest it{it} {what}")
        np.testing.assert_array_equal(a[3], b[3], err_msg=f"meas it{it} {what}")
        _pow_equal(a[2], b[2], exact, f"pow it{it} {what}")


def _assert_export(got, T, exact, what):
    ref = T["results"]
    _assert_results([(ex["origin"], ex["dest"], ex["pow"], ex["meas"]) for _, ex in got], ref, exact, what)
    assert [int(st.n_in) for st, _ in got] == T["agg"][0], what
    for it, (st, ex) in enumerate(got):
        assert int(st.n_measured) == len(T["meas"][it][1]), (what, it)
        if it + 1 < len(ref):
            # the next population: iteration 2 ends on the ceiling and the floor, where
            # nothing dissipates, so its recorded power is the population's
            nxt = ref[it + 1][2].reshape(-1)
            assert int(st.n_reflect + st.n_refract) == len(nxt), (what, it)
            _pow_equal(ex["next_pow"], nxt, exact, f"next_pow it{it} {what}")
        else:
            assert int(st.n_reflect + st.n_refract) == 0 or it == 2, (what, it)


@pytest.mark.parametrize("pat", [fu.cycle(), fu.random(1)], ids=_id)
@pytest.mark.parametrize("n", SMALL + LARGE)
def test_reference_order_export(engine, oracle_mod, checker, n, pat):
    sc, fates, rays = _case(2, None, pat, n)
    T = _ref_trace(oracle_mod, checker, (2, None, pat.label, n), sc, rays)
    got = _export_trace(engine, sc, rays)
    _assert_export(got, T, checker[1], f"{pat.label} n {n}")
    pos, pw, mm = engine.fetch_measured()       # the measured record in the reference's order
    np.testing.assert_array_equal(pos[:, :3], np.concatenate([m[0] for m in T["meas"]])[:, :3])
    _pow_equal(pw, np.concatenate([m[1] for m in T["meas"]]), checker[1], "measured power")
    np.testing.assert_array_equal(mm, np.concatenate([m[2] for m in T["meas"]]))


@pytest.mark.parametrize("pat", [fu.cycle(), fu.random(1)], ids=_id)
@pytest.mark.parametrize("n", SMALL + LARGE)
def test_reference_order_tracer(oracle_mod, checker, n, pat):
    from lightpycl_amd.iterative_tracer import CL_Tracer
    sc, fates, (o, d, p) = _case(2, None, pat, n)
    T = _ref_trace(oracle_mod, checker, (2, None, pat.label, n), sc, (o, d, p))
    src = types.SimpleNamespace(rays_origin=o, rays_dir=d, rays_power=p)
    tr = CL_Tracer(device=0)
    try:
        res = tr.iterative_tracer(light_source=[src], meshes=meshes_of(sc.arrs), trace_iterations=3,
                                  trace_until_dissipated=1.0, max_ray_len=fu.MAX_RAY_LEN, ior_env=fu.IOR_ENV,
                                  keep_results=True)
        assert [len(r[3]) for r in res] == T["agg"][0]
        _assert_results(res, T["results"], checker[1], f"tracer {pat.label} n {n}")
    finally:
        tr.engine.close()


# -- (c) chunks ------------------------------------------------------------------------------
CHUNK_PATTERNS = [fu.halves("matched", "terminator"), fu.random(1)]


@pytest.mark.parametrize("pat", CHUNK_PATTERNS, ids=_id)
@pytest.mark.parametrize("n", (65537, 131073))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_layout_chunked(engine, checker, chunk, n, pat):
    """(a) in several chunks per iteration: running row bases, the refracted
    rows staged and appended (k_append), chunk borders inside a tile.  The
    runtime takes the chunk size as given (no rounding); 70 001 exceeds 65 537
    rays and their children, so that pair runs as one chunk (its nearest
    chunked neighbour is 65 536) and only 131 073 rays split at 70 001."""
    assert chunk < n or (chunk, n) == (70001, 65537)
    _layout_case(engine, checker, n, pat, chunk)


_UNCHUNKED = {}


@pytest.mark.parametrize("pat", CHUNK_PATTERNS, ids=_id)
@pytest.mark.parametrize("n", (65537, 131073))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_reference_order_chunked(engine, oracle_mod, checker, chunk, n, pat):
    """(b) in several chunks: equal to the unchunked export, element for element,
    and to the reference's host loop."""
    sc, fates, rays = _case(2, None, pat, n)
    T = _ref_trace(oracle_mod, checker, (2, None, pat.label, n), sc, rays)
    try:
        if (pat.label, n) not in _UNCHUNKED:
            _UNCHUNKED[(pat.label, n)] = _export_trace(engine, sc, rays, 0)
        got = _export_trace(engine, sc, rays, chunk)
    finally:
        engine.set_chunk(0)
    whole = _UNCHUNKED[(pat.label, n)]
    assert len(got) == len(whole)
    for (sa, a), (sb, b) in zip(got, whole):
        assert (sa.n_in, sa.n_reflect, sa.n_refract, sa.n_measured) == (sb.n_in, sb.n_reflect, sb.n_refract, sb.n_measured)
        for k in ("origin", "dest", "pow", "meas", "next_pow"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k} chunk {chunk}")
    _assert_export(got, T, checker[1], f"{pat.label} n {n} chunk {chunk}")


# -- (d) whole traces ------------------------------------------------------------------------
def _assert_agg(lib, T, exact, what):
    ref = T["agg"]
    if exact:
        assert_aggregate_equal(lib, ref, what)
        return
    # the CPU oracle: the same rays (position and mesh exactly), powers within its bar
    assert lib[0] == ref[0], (what, lib[0], ref[0])
    a, b = lib[2], ref[2]
    ia, ib = np.lexsort(a[:, [4, 2, 1, 0]].T[::-1]), np.lexsort(b[:, [4, 2, 1, 0]].T[::-1])
    np.testing.assert_array_equal(a[ia][:, [0, 1, 2, 4]], b[ib][:, [0, 1, 2, 4]], err_msg=what)
    _pow_equal(a[ia][:, 3], b[ib][:, 3], False, what)
    np.testing.assert_allclose(lib[1], ref[1], rtol=1e-6, err_msg=what)


def _run(e, wait=True, reset=False):
    """One aggregate trace of the rays set on ``e`` (three iterations, no power
    stop) -> (stats tuple list, aggregate triple)."""
    if not reset:
        e.reset()
    stats, (cnt, mp) = e.run_local(3, 0.0, wait=wait, reset=reset)
    rec = e.fetch_measured()
    assert int(cnt) == len(rec[1])
    return ([(int(s.n_in), int(s.n_reflect), int(s.n_refract), int(s.n_measured), float(s.power_next)) for s in stats],
            ([int(s.n_in) for s in stats], np.array(mp), measured_rows(*rec)), rec)


@pytest.mark.parametrize("n,pat", [(65537, fu.random(1)), (131073, fu.halves("matched", "terminator"))],
                         ids=["random-65537", "halves-131073"])
@pytest.mark.parametrize("K", [None, 33, 70])
@pytest.mark.parametrize("n_measure", [0, 1, 4, 5])
def test_whole_traces(oracle_mod, checker, monkeypatch, n_measure, K, n, pat):
    """run_local on every measure-mesh count and K (masks on, off, beyond 64
    slots): host-sized twice back to back, asynchronous, after a smaller trace,
    and the speculative device-sized path, all equal to the reference's trace."""
    from lightpycl_amd.engine import Engine
    sc, fates, rays = _case(n_measure, K, pat, n)
    key = (n_measure, K, pat.label, n)
    T = _ref_trace(oracle_mod, checker, key, sc, rays)
    ssc, sfates, srays = _case(n_measure, K, fu.random(2), 257)
    sT = _ref_trace(oracle_mod, checker, (n_measure, K, "random2", 257), ssc, srays)
    exact = checker[1]
    what = f"measure meshes {n_measure} K {sc.K} {pat.label} n {n}"
    ek = fu.ray_key(rays[0][:, :2])
    monkeypatch.setenv("LPC_SPEC", "0")
    a = Engine(0)
    try:
        # the population order of iteration 2, as (a) reads it
        L = _read_layout(a, sc, rays)
        pop = fu.parents_of(fu.ray_key(L.origin[:, :2]), ek)
        _setup(a, sc, rays)
        first, agg, rec = _run(a)
        _assert_agg(agg, T, exact, what)
        if n_measure >= 4:
            # ceiling and floor measure every kept child: iteration 2's part of the
            # record lists the parents in the population's order
            m1 = first[0][3]
            assert first[1][3] == len(pop) and len(rec[1]) == m1 + len(pop)
            np.testing.assert_array_equal(fu.parents_of(fu.ray_key(rec[0][m1:, :2]), ek), pop,
                                          err_msg=f"iteration 2 record order {what}")
            want_mesh = np.where(np.arange(len(pop)) < first[0][1], sc.ceiling, sc.floor)
            np.testing.assert_array_equal(rec[2][m1:], want_mesh)
        again, agg2, rec2 = _run(a)                              # back to back
        assert again == first
        for x, y in zip(rec2, rec):
            np.testing.assert_array_equal(x, y)
        for kw in (dict(wait=False), dict(wait=False, reset=True)):    # lpc_trace_run_async / _rerun_async
            got, agg3, rec3 = _run(a, **kw)
            assert got == first, (what, kw)
            for x, y in zip(rec3, rec):
                np.testing.assert_array_equal(x, y)
        # a smaller trace on the same engine, then the large one again: stale tile
        # counts or group words of the larger trace would show in either
        _setup(a, ssc, srays)
        _, sagg, _ = _run(a)
        _assert_agg(sagg, sT, exact, "small after " + what)
        _setup(a, sc, rays)
        got, agg4, rec4 = _run(a)
        assert got == first
        for x, y in zip(rec4, rec):
            np.testing.assert_array_equal(x, y)
    finally:
        a.close()
    # the speculative, device-sized path: the first trace builds the prediction,
    # the others take it; a smaller trace in between mispredicts
    monkeypatch.setenv("LPC_SPEC", "1")
    b = Engine(0)
    try:
        _setup(b, sc, rays)
        for rep in range(3):
            got, _, recb = _run(b)
            assert got == first, (what, "speculative", rep)
            for x, y in zip(recb, rec):
                np.testing.assert_array_equal(x, y)
        _setup(b, ssc, srays)
        for rep in range(2):
            _, sagg, _ = _run(b)
            _assert_agg(sagg, sT, exact, "speculative small after " + what)
        _setup(b, sc, rays)
        for rep in range(2):
            got, _, recb = _run(b, wait=False)
            assert got == first, (what, "speculative after small", rep)
            for x, y in zip(recb, rec):
                np.testing.assert_array_equal(x, y)
    finally:
        b.close()


# -- (e) cutoff ------------------------------------------------------------------------------
ZERO_CUT = np.float32(0.01)         # above 0, below the smallest glass reflection (0.039)


@pytest.mark.parametrize("n", (257, 65537))
def test_cutoff_drops_the_zero_power_children(engine, checker, n):
    """uniform(matched): every reflected child (power exactly 0) is culled, the
    population is the refracted children only, the split at row 0; the ledger
    counts the matched parents and a culled power of exactly 0.0.  Traced and
    export paths."""
    pat = fu.uniform("matched")
    sc, fates, rays = _case(2, None, pat, n)
    ref = _bounce(checker, (2, None, pat.label, n), sc, rays)
    try:
        L = _read_layout(engine, sc, rays, cut=ZERO_CUT)
        pR, pT, _ = _check_layout(L, sc, fates, rays, ref, checker[1], cut=ZERO_CUT, what=f"cut n {n}")
        assert L.st.n_reflect == 0 and L.st.n_refract == n and len(pR) == 0
        np.testing.assert_array_equal(np.sort(pT), np.arange(n))
        cc, cp = L.culled
        assert cc.tolist() == [n] and cp.tolist() == [0.0]
        # the export path's first iteration
        _setup(engine, sc, rays, cut=ZERO_CUT)
        st, ex = engine.iterate(export=True)
        assert (st.n_reflect, st.n_refract) == (0, n)
        np.testing.assert_array_equal(ex["next_pow"], ref["t_pow"])
        cc, cp = engine.culled()
        assert cc.tolist() == [n] and cp.tolist() == [0.0]
    finally:
        engine.set_min_power(0.0)


@pytest.mark.parametrize("pat", [fu.cycle(), fu.random(1)], ids=_id)
@pytest.mark.parametrize("n", (257, 65537))
def test_cutoff_between_glass_reflections(engine, oracle_mod, checker, n, pat):
    """A cut between two glass reflection powers (and above the matched
    children's 0): traced and export paths against tests/cutoff_ref.py."""
    sc, fates, rays = _case(2, None, pat, n)
    key = (2, None, pat.label, n)
    ref = _bounce(checker, key, sc, rays)
    g = np.sort(ref["r_pow"][fates == fu.FATES.index("glass")])
    assert len(g) >= 4 and g[0] > 0.039
    lo, hi = g[len(g) // 2 - 1], g[len(g) // 2]
    cut = np.float32((float(lo) + float(hi)) / 2)
    assert lo < cut < hi
    T = _ref_trace(oracle_mod, checker, key, sc, rays, cut=cut)
    n_glass, n_matched = len(g), int((fates == fu.FATES.index("matched")).sum())
    # culled: every matched reflection, the glass reflections below the cut (and
    # whatever else the low-power parents keep below it)
    assert len(T["culled"][0]) >= n_matched + n_glass // 2
    exact = checker[1]
    try:
        L = _read_layout(engine, sc, rays, cut=cut)
        _check_layout(L, sc, fates, rays, ref, exact, cut=cut, what=f"cut {cut} {pat.label} n {n}")
        assert L.culled[0].tolist() == [len(T["culled"][0])]
        _setup(engine, sc, rays, cut=cut)
        _, agg, _ = _run(engine)
        cc, cp = engine.culled()
        _assert_agg(agg, T, exact, f"traced cut {cut}")
        cutoff_ref.assert_ledger(cc, cp, T["culled"], f"traced cut {cut}")
        got = _export_trace(engine, sc, rays, cut=cut)
        cc, cp = engine.culled()
        _assert_export(got, T, exact, f"export cut {cut}")
        cutoff_ref.assert_ledger(cc, cp, T["culled"], f"export cut {cut}")
    finally:
        engine.set_min_power(0.0)
