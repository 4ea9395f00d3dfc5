"""The drop-in kernels lpc_intersect_postproc (k_postproc_aos) and
lpc_reflect_refract_rays (k_fresnel_aos) on constructed rows, against the
reference's own kernels launched one at a time on the same buffers
(tests/ref_gpu.RefKernels.postproc / reflect_refract), bit for bit.  Without the
reference code object the CPU oracle judges: postproc still bit for bit (no
rsqrt in it), the Fresnel outputs under test_gpu_parity._cmp_bounce's rule for
the oracle, applied per input power so that the infinite and the tiny powers do
not set each other's scale.

Rows: tests/postproc_tables.py (the slot tables of
tests/test_postproc_tables_host.py, under one scene's material pattern at a
time) and tests/shade_rows.py (tests/test_shade_rows_host.py).
"""
import numpy as np
import pytest

import postproc_tables as pt
import shade_rows as sr
from soup_util import _rows, oracle_scene
from test_gpu_parity import _ulps

pytestmark = pytest.mark.gpu

POSTPROC_K = (3, 5, 9, 13, 17, 33, 65)
MAX_ROWS = 100_000
PATTERNS = ("none", "all", "alternating", "first", "last")


def _pattern(name, K):
    j = np.arange(K)
    return {"none": j < 0, "all": j >= 0, "alternating": j % 2 == 0, "first": j == 0, "last": j == K - 1}[name]


def _far_scene(K, refr, p):
    """K one-triangle meshes far apart; mesh j refractive where refr[j], its type
    the (p + j)-th of its class, cycled."""
    j = np.arange(K)
    x = 64.0 + 2 * j
    v0 = np.stack([x, np.full(K, 64.0), np.full(K, 32.0)], axis=1)
    mat = np.where(refr, pt.REFRACTIVE[(p + j) % 2], pt.OTHER[(p + j) % 3]).astype(np.int32)
    return (_rows(v0), _rows(v0 + [1.0, 0.0, 0.0]), _rows(v0 + [0.0, 1.0, 0.0]), j.astype(np.int32), mat,
            np.full(K, 1.5, np.float32), np.full(K, 0.9, np.float32), np.zeros(K, np.float32))


def _part1_rows(K, mrl):
    """At most MAX_ROWS of the host test's rows for K."""
    if K in pt.EXHAUSTIVE_K:
        parts = [pt.exhaustive_rows(K, mrl, prev) for prev in range(-2, K)]
        n = sum(r.n for r in parts)
        sel = np.unique(np.round(np.linspace(0, n - 1, min(n, MAX_ROWS))).astype(np.int64))
        cat = lambda k: np.concatenate([getattr(r, k) for r in parts])[sel]
        rows = parts[0]
        rows.prev, rows.t, rows.cnt, rows.idx, rows.mat = (np.ascontiguousarray(cat(k)) for k in ("prev", "t", "cnt", "idx", "mat"))
        rows.table = cat("table")
        rows.n = len(sel)
        return rows
    return pt.take(pt.sampled_rows(K, mrl), slice(0, MAX_ROWS))


def _lib_postproc(engine, rows):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: t.data_ptr()
    n = rows.n
    o, d = pt.ray_buffers(n)
    to, td, prev, tmin, cnt, itmp = T(o), T(d), T(rows.prev), T(rows.t), T(rows.cnt), T(rows.idx)
    dest = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    n1, n2, ent, imid, iidx = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(5))
    torch.cuda.synchronize()
    engine._c(engine.L.lpc_intersect_postproc(engine.h, n, P(to), P(td), P(dest), P(prev), P(n1), P(n2), P(ent), P(imid),
                                              P(iidx), P(tmin), P(cnt), P(itmp), np.float32(rows.mrl)))
    h = lambda t: t.cpu().numpy()
    return dict(dest=h(dest), n1=h(n1), n2=h(n2), entering=h(ent), isect_mid=h(imid), isect_idx=h(iidx))


@pytest.mark.parametrize("K", POSTPROC_K)
def test_postproc_tables(engine, oracle_mod, exact_ref, K):
    seen = {}
    for p, name in enumerate(PATTERNS):
        mrl = pt.MAX_RAY_LENS[p % len(pt.MAX_RAY_LENS)]
        arrs = _far_scene(K, _pattern(name, K), p)
        rows = pt.with_materials(_part1_rows(K, mrl), arrs[4])
        assert 0 < rows.n <= MAX_ROWS
        engine.upload_arrays(*arrs)
        got = _lib_postproc(engine, rows)
        judge = pt.oracle_postproc(oracle_mod, rows)
        hit = judge[:, 0] >= 0
        want = dict(isect_mid=judge[:, 0], isect_idx=judge[:, 1], n1=judge[:, 2], n2=judge[:, 3],
                    entering=np.where(hit, judge[:, 4], 0))          # no hit: the zeroed buffer stays
        tx = judge[:, 5].view(np.float32)
        if exact_ref is not None:
            o, d = pt.ray_buffers(rows.n)
            ref = exact_ref.postproc(oracle_scene(arrs), o, d, rows.prev, rows.t, rows.cnt, rows.idx, rows.mrl)
            for k in want:              # the oracle and the reference's kernel agree, so the guards below hold for both
                np.testing.assert_array_equal(ref[k], want[k], err_msg=f"oracle against the reference kernel: {k}")
            assert ref["dest"][:, 0].tobytes() == tx.tobytes()
            want = {k: ref[k] for k in want}
            want_dest = ref["dest"]
        else:
            want_dest = np.zeros((rows.n, 4), np.float32)
            want_dest[:, 0] = tx
        what = f"K={K}, pattern {name}, max_ray_len {mrl}"
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
        assert got["dest"].tobytes() == np.ascontiguousarray(want_dest).tobytes(), f"{what}: dest"
        for k, v in pt.outcomes(rows, judge).items():
            seen[k] = seen.get(k, 0) + int(v.sum())
    for k in ("entering_takeover", "exiting_alone", "n2_other", "tie_first", "tie_second", "exiting_minmax"):
        assert seen[k] > 0, (K, k, seen)


# -- Fresnel ---------------------------------------------------------------------------
def _lib_fresnel(engine, R):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: t.data_ptr()
    n = R.n
    o, e, d, pw, ms = T(R.origin), T(R.dest), T(R.dir), T(R.pow.copy()), T(R.meas.copy())
    n1, n2, imid, iidx = T(R.n1), T(R.n2), T(R.imid), T(R.iidx)
    F4 = lambda: torch.zeros((n, 4), dtype=torch.float32, device=dev)
    I = lambda: torch.zeros(n, dtype=torch.int32, device=dev)
    ro, rd, to, td = F4(), F4(), F4(), F4()
    rp, tp = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    rm, tm = I(), I()
    torch.cuda.synchronize()
    engine._c(engine.L.lpc_reflect_refract_rays(engine.h, n, P(o), P(e), P(d), P(pw), P(ms), P(n1), P(n2), P(ro), P(rd),
                                                P(rp), P(rm), P(to), P(td), P(tp), P(tm), P(imid), P(iidx),
                                                np.float32(sr.IOR_ENV)))
    h = lambda t: t.cpu().numpy()
    return dict(pow=h(pw), meas=h(ms), r_origin=h(ro), r_dir=h(rd), r_pow=h(rp), r_meas=h(rm), t_origin=h(to),
                t_dir=h(td), t_pow=h(tp), t_meas=h(tm))


def _bits_equal(a, b, sel, what):
    a, b = np.ascontiguousarray(a[sel]), np.ascontiguousarray(b[sel])
    bad = np.flatnonzero(np.any((a.view(np.int32) != b.view(np.int32)).reshape(len(a), -1), axis=1))
    assert bad.size == 0, (what, bad.size, int(np.flatnonzero(sel)[bad[0]]), a[bad[0]], b[bad[0]])


def _close(a, b, pw_in, sel, what):
    """_cmp_bounce's bar for the CPU oracle (64 ulp, or 1e-6 of the largest
    magnitude), the largest magnitude taken over the rows of one input power;
    non-finite values must agree as such."""
    a, b = np.float32(a[sel]), np.float32(b[sel])
    p = np.broadcast_to(pw_in[sel].reshape((-1,) + (1,) * (a.ndim - 1)), a.shape)
    a, b, p = a.reshape(-1), b.reshape(-1), p.reshape(-1)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]), what
    for v in np.unique(p[~np.isnan(p)]):       # (an infinite input power still has finite directions)
        m = fin & (p == v)
        if m.any():
            scale = np.abs(np.float64(b[m])).max()
            ok = (_ulps(a[m], b[m]) <= 64) | (np.abs(np.float64(a[m]) - np.float64(b[m])) <= 1e-6 * scale)
            assert ok.all(), (what, float(v), int((~ok).sum()))


def test_fresnel_rows(engine, oracle_mod, exact_ref, capsys):
    sc = sr.scene(True)
    try:
        engine.upload_arrays(*sc.arrs)
    except Exception:                   # the library refuses the 5e9 triangle: the rows without it
        sc = sr.scene(False)
        engine.upload_arrays(*sc.arrs)
    R = sr.rows(sc)
    with capsys.disabled():
        print(f"\n[fresnel rows] {R.n} rows; the 5e9 triangle is {'in' if sc.with_huge else 'LEFT OUT (refused at upload)'}; "
              f"judge: {'the reference kernel' if exact_ref is not None else 'the CPU oracle'}")
    got = _lib_fresnel(engine, R)
    orc = sr.oracle_shade(oracle_mod, sc, R)
    everything = np.ones(R.n, bool)
    # origins of the children: the destination, in every row
    for k in ("r_origin", "t_origin"):
        _bits_equal(got[k][:, :3], R.dest[:, :3], everything, k)
    if exact_ref is not None:
        S = oracle_scene(sc.arrs)
        ref = exact_ref.reflect_refract(S, R.origin, R.dest, R.dir, R.pow, R.meas, np.zeros(R.n, np.int32), R.n1, R.n2,
                                        R.imid, R.iidx, sr.IOR_ENV, sr.MAX_RAY_LEN)
        # the NaN-TIR rows, named by the oracle: there the reference stores uninitialised
        # locals; only what it does define is compared with it
        nan = sr.nan_rows(sc, R, orc)
        judge = {k: np.where((nan if ref[k].ndim == 1 else nan[:, None]), orc[k], ref[k]) for k in sr.OUT}
        seen = sr.check_coverage(sc, R, judge)
        for k in sr.OUT:
            _bits_equal(got[k], ref[k], everything if k in ("pow", "meas") else ~nan, f"{k} against the reference kernel")
    else:
        nan = sr.nan_rows(sc, R, orc)
        seen = sr.check_coverage(sc, R, orc)
        crit = R.group == "critical"
        with capsys.disabled():
            print(f"\n[fresnel rows] no reference code object: {int(crit.sum())} rows of the critical group left out "
                  f"of the decision comparison, {R.n - int(crit.sum())} rows compared")
        for k in ("meas", "r_meas", "t_meas"):
            _bits_equal(got[k], orc[k], ~crit, f"{k} against the oracle")
        for k in ("pow", "r_pow", "t_pow", "r_dir", "t_dir"):
            _close(got[k], orc[k], R.pow, ~crit, f"{k} against the oracle")
    # the documented dead children of the NaN-TIR rows; a mirror's
    # reflected power is still power * R, as the oracle has it
    assert seen["nan"] == int(nan.sum()) > 0
    assert not got["r_dir"][nan].any() and not got["t_dir"][nan].any() and not got["t_pow"][nan].any()
    assert np.all(got["r_meas"][nan] == -1) and np.all(got["t_meas"][nan] == -1)
    _bits_equal(got["r_pow"], orc["r_pow"], nan, "r_pow of the NaN-TIR rows")
    glass_nan = nan & (sc.arrs[4][np.maximum(R.imid, 0)] == 0)
    assert glass_nan.any() and not got["r_pow"][glass_nan].any()
