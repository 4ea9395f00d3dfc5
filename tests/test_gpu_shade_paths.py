"""k_shade_stage's two paths: a wave whose rays wrote at most one slot each reads
that slot alone (postproc_single, LPC_SHADE_FAST, the default); a wave with any
other ray, and every wave under LPC_SHADE_FAST=0, takes postproc over all slots.
tests/test_postproc_single_host.py shows the two equal on the CPU; here whole
traces under both policies are compared, at the populations where a wave changes
path.

Scene: unit-square patches in the plane z = 0, side by side along x, one mesh
each; a beam from z = 1 straight down.  A ray's line meets

  column 0  a mirror; above it a mirror ceiling (its children bounce between the two)
  column 1  glass             (children: up to the measuring ceiling, down to nothing)
  column 2  a terminator
  column 3  a measure mesh
  column 4  glass and, at z = -0.5, a second glass mesh: two written slots
  column 5  glass at z = -11, beyond max_ray_len = 10: a count, no key
  column 6  glass 4e-6 short of max_ray_len, inside EPSILON = 1e-5 of it: postproc's
            max-min rule hands the hit to a clean refractive slot (the single-slot
            path's fallback)

and nothing else, so the rays of columns 0-3, 5 and 6 write one slot and their
children one or none.  Filler meshes, never hit, raise the mesh count: 10 (slots
in registers), 20 (slots read from memory, masks present) and 40 (no masks:
postproc only, under both policies).

Populations below 4 096 rays are traced in the order given, so ray i sits on
lane i % 64 of wave i // 64.  Ray i carries power i + 1.
"""
import os
import types

import numpy as np
import pytest

import fate_util as fu
from soup_util import _rows, oracle_scene
from test_gpu_compaction import _pow_equal
from test_gpu_parity import _cmp_bounce

pytestmark = pytest.mark.gpu

MRL = np.float32(10.0)
IOR_ENV = np.float32(1.0)
ITERATIONS = 5
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
MESH_COUNTS = (10, 20, 40)
SINGLE = (0, 1, 2, 3)               # columns whose rays write one slot
TWO, FAR, EDGE = 4, 5, 6
ON, OFF = {"LPC_SHADE_FAST": "1"}, {"LPC_SHADE_FAST": "0"}
_KNOBS = ("LPC_SHADE_FAST", "LPC_SPEC")

GLASS, GLASS2 = (0, 1.5, 0.0, 0.02), (0, 1.3, 0.0, 0.01)
MIRROR, TERMINATOR, MEASURE = (1, 1.0, 0.9, 0.0), (2, 1.0, 0.0, 0.0), (3, 1.0, 0.0, 0.0)


def _scene(K):
    z_edge = 1.0 - (10.0 - 4e-6)
    parts = [(0, 1, 0.0, MIRROR), (1, 2, 0.0, GLASS), (2, 3, 0.0, TERMINATOR), (3, 4, 0.0, MEASURE),
             (4, 5, 0.0, GLASS), (4, 5, -0.5, GLASS2), (5, 6, -11.0, GLASS), (6, 7, z_edge, GLASS),
             (0, 1, 2.0, MIRROR), (1, 7, 2.0, MEASURE)]
    tris, ids, mats = [], [], []
    for j, (x0, x1, z, mat) in enumerate(parts):
        tris += fu._quad(x0, x1, z)
        ids += [j, j]
        mats.append(mat)
    assert K >= len(parts)
    for j in range(len(parts), K):      # never hit: far from the beam and its children
        x = 64 + 2 * j
        tris.append(((x, 64, 32), (x + 1, 64, 32), (x, 65, 32)))
        ids.append(j)
        mats.append(TERMINATOR)
    t = np.asarray(tris, np.float64)
    m = np.asarray(mats, np.float64)
    return (_rows(t[:, 0]), _rows(t[:, 1]), _rows(t[:, 2]), np.asarray(ids, np.int32), m[:, 0].astype(np.int32),
            m[:, 1].astype(np.float32), m[:, 2].astype(np.float32), m[:, 3].astype(np.float32))


def _rays(cols):
    """One ray per entry of `cols`, aimed at that column from z = 1, each at its own
    point strictly inside the patch's lower triangle."""
    cols = np.asarray(cols, np.int64)
    n = len(cols)
    pts = fu._points()[:n]
    o = np.zeros((n, 4), np.float32)
    o[:, 0] = cols + pts[:, 0] / fu.GRID
    o[:, 1] = pts[:, 1] / fu.GRID
    o[:, 2] = 1.0
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = -1.0
    return o, d, np.arange(1, n + 1, dtype=np.float32)


def _populations(n):
    """name -> column per ray.  The rays of columns 0-3 in turn, and one ray (or
    several) of another column at a chosen lane."""
    base = np.asarray(SINGLE)[np.arange(n) % len(SINGLE)]

    def put(at):
        c = base.copy()
        for i, col in at:
            c[i] = col
        return c
    mid, l63, last = n // 2, min(63, n - 1), n - 1
    return {"single": base, "two-lane0": put([(0, TWO)]), "two-lane63": put([(l63, TWO)]),
            "two-last": put([(last, TWO)]), "far": put([(mid, FAR)]), "edge": put([(mid, EDGE)]),
            "all": put([(mid, FAR), (max(mid - 1, 0), EDGE), (l63, TWO), (last, TWO), (0, TWO)])}


def _open(cfg):
    """A fresh engine under the policy `cfg` (the knobs are read when it opens)."""
    from lightpycl_amd.engine import Engine
    old = {k: os.environ.pop(k, None) for k in _KNOBS}
    try:
        os.environ.update(cfg)
        return Engine(0)
    finally:
        for k in _KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module", params=MESH_COUNTS, ids=lambda k: f"K{k}")
def setup(request):
    """Per mesh count: the scene and one engine per policy for the whole module."""
    arrs = _scene(request.param)
    es = [_open(ON), _open(OFF)]
    try:
        for e in es:
            e.upload_arrays(*arrs)
        yield types.SimpleNamespace(K=request.param, arrs=arrs, ref=oracle_scene(arrs), on=es[0], off=es[1])
    finally:
        for e in es:
            e.close()


def _trace2(e, rays):
    """Two back-to-back traces of the rays on `e` (the second one's chained
    populations are device-sized): each one's per-iteration stats, per-mesh power
    and measured record."""
    e.set_rays(*rays, MRL, IOR_ENV)
    out = []
    for _ in range(2):
        e.reset()
        stats, (cnt, mp) = e.run_local(ITERATIONS, 0.0)
        st = [(int(s.n_in), int(s.n_reflect), int(s.n_refract), int(s.n_measured), float(s.power_next)) for s in stats]
        pos, p, mm = e.fetch_measured()
        assert cnt == len(p)
        out.append((st, np.array(mp), pos.copy(), p.copy(), mm.copy()))
    return out


def _children(e, rays):
    """One traced iteration, then the population it built, in population order,
    and what the measured record holds after it."""
    e.set_rays(*rays, MRL, IOR_ENV)
    st, _ = e.iterate()
    rec = [x.copy() for x in e.fetch_measured()]
    pw = e.population_power()
    st2, ex = e.iterate(export=True)
    return ((int(st.n_in), int(st.n_reflect), int(st.n_refract), int(st.n_measured), float(st.power_next)),
            ex["origin"][:, :3].copy(), pw, ex["dest"][:, :3].copy(), ex["pow"].copy(), ex["meas"].copy(), ex["next_pow"].copy(), rec)


def _assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes(), f"{what}: per-mesh power bits"
    for x, y, k in zip(a[2:], b[2:], ("position", "power", "mesh")):
        assert x.tobytes() == y.tobytes(), f"{what}: measured {k}, in order"


def _assert_children(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for x, y, k in zip(a[1:7], b[1:7], ("origin", "power", "dest", "pow", "meas", "next_pow")):
        assert x.tobytes() == y.tobytes(), f"{what}: children {k}, in order"
    for x, y, k in zip(a[7], b[7], ("position", "power", "mesh")):
        assert x.tobytes() == y.tobytes(), f"{what}: measured {k} after one iteration, in order"


def _against_reference(checker, S, e, cols, rays, ch, what):
    """The reference's bounce of the emitted rays: the drop-in bounce of `e` equals
    it, and the traced iteration's rows are its kept children ([reflected ;
    refracted], each in ray order) and its measured rays."""
    o4, d4, pw = rays
    n = len(pw)
    z, pm = np.zeros(n, np.int32), np.full(n, -2, np.int32)
    o = checker[0](S.ref, o4, d4, pw, z, pm, MRL, IOR_ENV)
    _cmp_bounce(e.bounce(o4, d4, pw, z, pm, MRL, IOR_ENV), o, checker[1])
    mid = np.asarray(o["isect_mid"]).reshape(-1)
    # the scene does what its description says: column c ends on mesh c, the ray
    # beyond max_ray_len nowhere, and the ray inside EPSILON hands n2 to a clean slot
    want = np.where(cols == TWO, 4, np.where(cols == FAR, -1, np.where(cols == EDGE, 7, cols)))
    np.testing.assert_array_equal(mid, want, err_msg=what)
    cnt = np.asarray(o["isects_count"])
    assert np.all(cnt[cols == FAR, 6] == 1) and np.all((cnt[cols == TWO] > 0).sum(axis=1) == 2)
    n2 = np.asarray(o["n2"]).reshape(-1)
    assert np.all(n2[cols == EDGE] != 7) and np.all(n2[cols == EDGE] >= 0), n2[cols == EDGE]
    kr, kt, ms = (np.asarray(o[k]).reshape(-1) for k in ("r_meas", "t_meas", "meas"))
    st, origin, power = ch[0], ch[1], ch[2]
    assert st[:4] == (n, int((kr == 0).sum()), int((kt == 0).sum()), int((ms == 1).sum())), (what, st)
    dest = np.asarray(o["dest"], np.float32)[:, :3]
    np.testing.assert_array_equal(origin[:, :3], np.concatenate((dest[kr == 0], dest[kt == 0])), err_msg=what)
    _pow_equal(power, np.concatenate((np.asarray(o["r_pow"]).reshape(-1)[kr == 0],
                                      np.asarray(o["t_pow"]).reshape(-1)[kt == 0])), checker[1], what)
    rec = ch[7]
    np.testing.assert_array_equal(rec[0][:, :3], dest[ms == 1], err_msg=what)
    _pow_equal(rec[1], np.asarray(o["pow"]).reshape(-1)[ms == 1], checker[1], what)
    np.testing.assert_array_equal(rec[2], mid[ms == 1], err_msg=what)


@pytest.mark.parametrize("n", SIZES)
def test_single_slot_path_equals_postproc(setup, checker, n):
    S = setup
    for name, cols in _populations(n).items():
        what = f"K {S.K}, {n} rays, {name}"
        rays = _rays(cols)
        on, off = _trace2(S.on, rays), _trace2(S.off, rays)
        _assert_same(on[0], off[0], f"{what}: on against off, first trace")
        _assert_same(on[1], off[1], f"{what}: on against off, second trace")
        _assert_same(on[1], on[0], f"{what}: second trace against the first")
        st = on[0][0]
        assert st[0][0] == n and (n < 4 or (len(st) == ITERATIONS and st[-1][0] > 0)), (what, st)   # the mirrors chain
        con, coff = _children(S.on, rays), _children(S.off, rays)
        _assert_children(con, coff, what)
        if name == "all":               # one policy per size against the reference
            k = SIZES.index(n) % 2
            _against_reference(checker, S, (S.on, S.off)[k], cols, rays, (con, coff)[k], what)
    # the slot arrays are clean after each trace: other rays on the same engines
    # give what a fresh engine gives
    other = _rays(np.roll(_populations(n)["all"], 1)[::-1])
    fresh = _open(ON)
    try:
        fresh.upload_arrays(*S.arrs)
        want = _trace2(fresh, other)
    finally:
        fresh.close()
    for e, pol in ((S.on, "on"), (S.off, "off")):
        got = _trace2(e, other)
        _assert_same(got[0], want[0], f"K {S.K}, {n} rays: other rays after the traces, policy {pol}")
        _assert_same(got[1], want[1], f"K {S.K}, {n} rays: other rays after the traces, policy {pol}, second trace")
