"""GPU parity of the walk on the triangle soups of soup_util.py: the shapes the
hand-built scenes of test_gpu_parity.py do not pin -- runs of 1, 8 or 9 triangles,
runs made of slivers only, hundreds of coincident triangles, packets that fill
the walk's LDS queues to their guards, non-monotone mesh-id sequences,
non-finite rays, rays longer than the filter records cover.

Every test uploads flat arrays (Engine.upload_arrays), runs Engine.bounce and
compares with the `checker` fixture through test_gpu_parity._cmp_bounce: bit for
bit against the reference's own kernels, and with the CPU-oracle fallback under
_cmp_bounce's tolerance.  The conditions on the inputs (enough rays hit, enough
of them more than once on the coplanar soups) are asserted on the reference's
output, so a case cannot go vacuous.

Piece cuts.  run_intersect cuts every live run at the shallowest level with at
least g nodes (the last level if none has), g = q_level(n) =
min(4096, ceil(LPC_Q_TARGET / (ceil(n / 64) * live runs))), LPC_Q_TARGET = 65 536.
With n <= 5 000 rays and a handful of meshes g >= 277, more than any level of a
4 097-triangle run below its leaves holds: such scenes are always cut at the leaf
level, whatever the test does.  A cut at a middle level or at the run roots needs
many live runs, so the scenes that pin those cuts (and the queue guards, which
only a wave walking a whole run can reach) add one-triangle filler meshes far
from the rays: `live` below counts them.
"""
import os
import re
import types

import numpy as np
import pytest

import soup_util as su
from test_gpu_parity import _POLICIES, _cmp_bounce

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MRL = np.float32(1e3)
SEED = 3


def _define(name, path):
    with open(os.path.join(ROOT, "lightpycl_amd", "csrc", path)) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, f.read(), re.M)
    assert m, name
    return int(m.group(1))


def q_cut(n, live, tris):
    """(g, level, levels): q_level's g for n rays and `live` runs, and the level
    (0 = the run root) a run of `tris` hierarchy triangles is cut at."""
    npk = -(-n // 64)
    g = min(4096, max(1, -(-_define("LPC_Q_TARGET", "lpc_runtime.hip") // (npk * live))))
    counts = [-(-tris // 8)]
    while counts[-1] > 1:
        counts.append(-(-counts[-1] // 8))
    counts = counts[::-1]
    lv = 0
    while lv + 1 < len(counts) and counts[lv] < g:
        lv += 1
    return g, lv, len(counts)


def with_fillers(big, F, before=0, seed=0):
    """The soup `big` (one mesh) among F one-triangle filler meshes, `before` of
    them in front of it: 0.01-size triangles 1 000 away from everything."""
    rng = np.random.default_rng([91, F, before, seed])
    c = np.array([1000.0, 0.0, 0.0]) + rng.uniform(-5.0, 5.0, (F, 3))
    f = [su._rows(c), su._rows(c + 0.01 * rng.normal(size=(F, 3))), su._rows(c + 0.01 * rng.normal(size=(F, 3)))]
    v = [np.concatenate((x[:before], b, x[before:])) for x, b in zip(f, big[:3])]
    Mb = big[0].shape[0]
    mesh_id = np.concatenate((np.arange(before), np.full(Mb, before), np.arange(before + 1, F + 1))).astype(np.int32)
    # the big mesh refractive, the fillers terminators
    mat = su.materials(F + 1, mats=((2, 1.0, 0.0, 0.0),))
    for k, val in zip(range(4), (0, 1.5, 0.0, 0.02)):
        mat[k][before] = val
    return (v[0], v[1], v[2], mesh_id) + mat


def _bounce_both(engine, checker, arrs, o4, d4, pw, prev=None, mrl=MRL, meas=None):
    n = o4.shape[0]
    engine.upload_arrays(*arrs)
    S = _scene(arrs)
    z = np.zeros(n, np.int32) if meas is None else meas
    pm = np.full(n, -2, np.int32) if prev is None else prev
    g = engine.bounce(o4, d4, pw, z, pm, mrl, 1.0)
    o = checker[0](S, o4, d4, pw, z, pm, mrl, 1.0)
    return g, o


_scenes = {}


def _scene(arrs):
    """One reference scene object per soup (the reference runner keeps its
    device copy while it sees the same object)."""
    key = id(arrs[0])
    if key not in _scenes or _scenes[key][0] is not arrs[0]:
        _scenes[key] = (arrs[0], su.oracle_scene(arrs))
    return _scenes[key][1]


def _not_vacuous(ref, kind=None, ties=False, frac=0.25):
    cnt = ref["isects_count"].max(axis=1)
    hit = cnt > 0
    assert hit.sum() >= frac * hit.size, (int(hit.sum()), hit.size)
    if ties:
        assert (cnt > 1).sum() >= 0.80 * hit.sum(), (int((cnt > 1).sum()), int(hit.sum()))


# ---------------------------------------------------------------------------
# a. sizes: (kind, M, K, fillers, n, ray seed); the switches each triple sits at:
#    S- / S+ below / at kSortMin = 4096 rays (unsorted / coherence-sorted packets);
#    P the 128-ray sliver packet: one packet, a second packet of one ray, a ragged one;
#    B+ / B- the hand-over budget on (n < 16 M) / off (n >= 16 M);
#    cut: every plain triple has <= 3 live runs, so g >= 337 and the cut is the leaf
#    level ("flat": the run's only level); the filler triples reach the other cuts.
SIZES = [
    ("uniform", 1, 1, 0, 1, 1),         # flat; one ray that hits the one triangle; B+ (1 < 16)
    ("mixed", 1, 3, 0, 63, 0),          # flat or no hierarchy at all; B- (63 >= 16); P one half packet
    ("coplanar", 8, 1, 0, 64, 0),       # flat, a full leaf; B+ (64 < 128); one whole packet
    ("clustered", 8, 1, 0, 65, 0),      # flat; B+ (65 < 128); a second packet of one ray
    ("mixed", 8, 1, 0, 129, 0),         # flat; B- (129 >= 128); P a second 128-packet of one ray
    ("uniform", 9, 3, 0, 129, 0),       # flat runs of ~3; B+ (129 < 144)
    ("mixed", 9, 1, 0, 257, 0),         # 2 levels, leaf cut (2 nodes); B- (257 >= 144); P three packets
    ("coplanar", 9, 1, 0, 4096, 0),     # 2 levels, leaf cut; S+ exactly at kSortMin
    ("coplanar", 64, 1, 0, 257, 0),     # 2 levels (8 full leaves), leaf cut; B+ (257 < 1024)
    ("coplanar", 64, 1, 0, 1237, 0),    # the same run; B- (1237 >= 1024)
    ("mixed", 64, 3, 0, 64, 0),         # runs of ~21 with slivers; P half a packet
    ("clustered", 64, 3, 0, 4095, 0),   # S- one ray below kSortMin
    ("uniform", 65, 1, 0, 257, 0),      # 3 levels (9 leaves, 2, 1), leaf cut; B+ (257 < 1040)
    ("uniform", 65, 1, 0, 1237, 0),     # the same run; B- (1237 >= 1040)
    ("mixed", 65, 3, 0, 65, 0),         # P one packet and one lane of its second half
    ("clustered", 65, 1, 0, 4100, 0),   # S+; B-
    ("uniform", 513, 1, 0, 63, 0),      # 3-4 levels, leaf cut (g = 4096)
    ("mixed", 513, 3, 0, 129, 0),       # P; slivers and thin triangles in every run
    ("coplanar", 513, 1, 0, 4095, 0),   # S-; ties in every leaf
    ("coplanar", 513, 1, 0, 4096, 0),   # S+; the same soup, sorted
    ("clustered", 513, 3, 0, 1237, 0),  # a ragged last packet
    ("mixed", 513, 1, 0, 4100, 0),      # S+; P 33 packets, the last of 4 rays
    ("uniform", 4097, 1, 0, 64, 0),     # 5 levels, leaf cut (513 pieces); B+
    ("mixed", 4097, 3, 0, 257, 0),      # >= 100 slivers per run
    ("coplanar", 4097, 1, 0, 1237, 0),  # ~1 000 positions of ~4 coincident triangles
    ("clustered", 4097, 3, 0, 4095, 0),  # S-
    ("uniform", 4097, 3, 0, 4096, 0),   # S+
    ("mixed", 4097, 1, 0, 4100, 0),     # S+; the largest sliver population
    # The filler triples: 4 097 triangles in all, F of them one-triangle meshes, the rest one run.
    # cut at a middle level: 65 packets x 201 live runs -> g = 6; a run of 2 561..3 897 hierarchy
    # triangles has levels (1, 6..8, 41..61, 321..488): the 6..8-node level; S+; B+
    ("uniform", 4097, 1, 200, 4100, 0),
    # cut at the run roots: 65 x 1 101 >= 65 536 -> g = 1; the 1 101 pieces go to k_roots_s in two
    # batches; the wave walks 4 levels under the hand-over budget; S+; B+
    ("uniform", 4097, 1, 1100, 4100, 0),
    # cut at the run roots, unsorted: 20 packets x 3 501 live runs -> g = 1; ties; levels (1, 2, 10, 75)
    ("coplanar", 4097, 1, 3500, 1237, 0),
    # a middle level of a run with slivers: 64 x 401 -> g = 3; 1 025..3 697 hierarchy triangles have
    # levels (1, 3..8, ...): the 3..8-node level; S-
    ("mixed", 4097, 1, 400, 4095, 0),
]
_WANT_CUT = {200: "middle", 1100: "root", 3500: "root", 400: "middle"}
_HIER = {"uniform": (0.66, 1.0), "coplanar": (1.0, 1.0), "mixed": (0.28, 1.0)}   # bounds on the hierarchy's share


@pytest.mark.parametrize("kind,M,K,F,n,rseed", SIZES, ids=lambda v: str(v))
def test_soup_sizes_two_levels(engine, checker, kind, M, K, F, n, rseed):
    arrs = su.soup(kind, M - F, K, seed=SEED)
    if F:
        big = arrs
        arrs = with_fillers(big, F, before=F // 2)
        for share in _HIER[kind]:                               # (thin triangles and slivers leave the hierarchy)
            g, lv, levels = q_cut(n, F + 1, int(share * (M - F)))
            assert levels >= 3 and {"root": lv == 0, "middle": 0 < lv < levels - 1}[_WANT_CUT[F]], (g, lv, levels)
        o4, d4, pw = su.aimed_rays(big, n, seed=rseed)          # aimed at the big mesh only
    else:
        assert q_cut(n, K, M)[1] == q_cut(n, K, M)[2] - 1       # the leaf level
        o4, d4, pw = su.aimed_rays(arrs, n, seed=rseed)
    g, o = _bounce_both(engine, checker, arrs, o4, d4, pw)
    _not_vacuous(o, ties=(kind == "coplanar" and M >= 7 and K == 1))
    _cmp_bounce(g, o, checker[1])
    o2, d2, p2, m2 = su.kept_children(o)
    if o2.shape[0]:
        g2, r2 = _bounce_both(engine, checker, arrs, o2, d2, p2, prev=m2)
        _cmp_bounce(g2, r2, checker[1])


# ---------------------------------------------------------------------------
# b. the queue guards of the walk
COPIES, HITS = 200, 23
GUARD_FILL, GUARD_AT = 1100, 500        # filler meshes, and how many of them come first


def _guard_scene():
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    big = tuple(su._rows(np.repeat(tri[k:k + 1], COPIES, axis=0)) for k in range(3))
    return with_fillers(big, GUARD_FILL, before=GUARD_AT)


def _guard_rays(n, hit_lanes, seed):
    """n rays in packets of 64: lanes in `hit_lanes` go straight down through the
    coincident triangles, the others pass 10 above them along x (their lines
    miss every sphere of the run)."""
    rng = np.random.default_rng([17, n, seed])
    u, v = rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n)
    o = np.stack([u, v, 10.0 + rng.uniform(0.0, 1.0, n)], axis=1)
    hits = np.isin(np.arange(n) % 64, hit_lanes)
    d = np.where(hits[:, None], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0])
    return su._rows(o), su._rows(d), np.ones(n, np.float32), hits


@pytest.mark.parametrize("case", ["dense", "sparse", "tail"])
@pytest.mark.parametrize("budget", ["default", "0"])
def test_coincident_triangles_fill_the_walk_queues(checker, monkeypatch, case, budget):
    """200 coincident copies of one triangle (mesh 500 of 1 101; triangle indices
    500..699) walked from the run's root by one wave, n < kSortMin so the packets
    keep the input order.  Every hitting ray must report count 200 and triangle
    500, the lowest index among 200 equal t (slot_key's index half decides).

    The cut.  1 101 live runs: 63 packets x 1 101 = 69 363 >= LPC_Q_TARGET, so
    g = 1 and the run's piece is its root (levels 1, 4, 25 nodes).  With fewer
    runs the pieces would be single leaves and no queue would hold more than 8
    entries.  LPC_BUDGET 0 keeps the whole run in the one wave; under the default
    budget the wave hands over after 20 nodes, later than the first drains below.
    dense (i):  all 64 lanes hit, so each triangle is one dense entry
      (64 >= LPC_DRAIN_U = 32), 8 per leaf.  trav_packet drains before a leaf when
      nq > 64 - W = 56: after 8 leaves nq = 64 = len(qidx), exactly full, and the
      9th leaf drains mid-walk; 25 leaves do that three times.
    sparse (ii): 23 lanes hit and 41 aim away, so each triangle adds 23 pairs
      (23 < LPC_DRAIN_U), 184 per leaf.  The guard is np > LPC_PAIRS - W (LPC_DRAIN_U - 1)
      = 512 - 248 = 264: after two leaves np = 368 > 264 and the third leaf drains
      mid-walk (320 pairs tested, 48 kept); np never exceeds 264 + 184 = 448 <= 512.
    tail (iii): 4 033 rays, so the last packet holds one ray and 63 lanes that
      duplicate it: the duplicates walk and queue, only lane 0 may flush."""
    from lightpycl_amd.engine import Engine
    W, U, PAIRS = 8, _define("LPC_DRAIN_U", "lpc_kernels.hip"), _define("LPC_PAIRS", "lpc_kernels.hip")
    n = 63 * 64 + (1 if case == "tail" else 0)
    lanes = np.arange(64) if case != "sparse" else np.sort(np.random.default_rng(5).permutation(64)[:HITS])
    # the arithmetic above, from the constants as they are now
    assert q_cut(n, GUARD_FILL + 1, COPIES) == (1, 0, 3) and n < 4096
    assert 64 >= U and COPIES // W > (64 - W) // W + 1                  # dense: qidx fills, then drains mid-walk
    assert HITS < U and 2 * W * HITS > PAIRS - W * (U - 1) and COPIES // W >= 3   # sparse: the guard trips
    assert PAIRS - W * (U - 1) + W * HITS <= PAIRS
    if budget != "default":
        monkeypatch.setenv("LPC_BUDGET", budget)
    arrs = _guard_scene()
    o4, d4, pw, hits = _guard_rays(n, lanes, seed=1)
    e = Engine(0)
    try:
        g, o = _bounce_both(e, checker, arrs, o4, d4, pw)
    finally:
        e.close()
    assert np.all(o["isects_count"][hits, GUARD_AT] == COPIES) and np.all(o["isects_count"][~hits] == 0)
    assert np.all(o["isect_idx"][hits] == GUARD_AT) and np.all(o["isect_mid"][hits] == GUARD_AT)
    assert hits.sum() == (n if case != "sparse" else 63 * HITS)
    _cmp_bounce(g, o, checker[1])


# ---------------------------------------------------------------------------
# c. mesh-id sequences the upload accepts (K = 4): a run flushes into the slot of
# the next run's id - 1, the last into its own; later runs overwrite, dead runs
# are skipped.  Each entry is a block of 40 triangles.
SEQUENCES = ["0,0,2,2,1,1", "0,0,3,3", "1,1,2,2", "0,1,2,1"]


def _sequence_scene(seq):
    ids = [int(x) for x in seq.split(",")]
    arrs = su.soup("uniform", 40 * len(ids), 1, seed=SEED + len(ids) + ids[-1])
    mesh_id = np.repeat(np.array(ids, np.int32), 40)
    return arrs[:3] + (mesh_id,) + su.materials(4)


def _live_part(arrs):
    """The triangles of the runs whose results the reference keeps (a run whose
    slot a later run overwrites is dead): the rays are aimed at these."""
    lo, hi, slot = su.runs_of(arrs[3])
    live = np.zeros(arrs[3].size, bool)
    for r in range(lo.size):
        if r == np.flatnonzero(slot == slot[r])[-1]:
            live[lo[r]:hi[r]] = True
    return tuple(a[live] for a in arrs[:3])


@pytest.mark.parametrize("seq", SEQUENCES)
def test_mesh_id_sequences_bounce(engine, checker, seq):
    arrs = _sequence_scene(seq)
    lo, hi, slot = su.runs_of(arrs[3])
    assert slot.min() >= 0
    if seq in ("0,0,2,2,1,1", "0,1,2,1"):
        assert len(set(slot.tolist())) < slot.size             # a later run overwrites an earlier one
    o4, d4, pw = su.aimed_rays(_live_part(arrs), 1237, seed=1)
    g, o = _bounce_both(engine, checker, arrs, o4, d4, pw)
    _not_vacuous(o)
    _cmp_bounce(g, o, checker[1])


@pytest.mark.parametrize("seq", SEQUENCES)
def test_mesh_id_sequences_dropin_slots(engine, exact_ref, seq):
    """lpc_intersect's [ray][mesh] slot arrays against the reference kernel's."""
    torch = pytest.importorskip("torch")
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    arrs = _sequence_scene(seq)
    o4, d4, pw = su.aimed_rays(_live_part(arrs), 500, seed=2)
    n, K = 500, 4
    engine.upload_arrays(*arrs)
    ref = exact_ref.bounce(_scene(arrs), o4, d4, pw, np.zeros(n, np.int32), np.full(n, -2, np.int32), MRL, 1.0)
    _not_vacuous(ref)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
    tmin = torch.full((n, K), float(MRL), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n, K), dtype=torch.int32, device=dev)
    itmp = torch.zeros((n, K), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine._c(engine.L.lpc_intersect(engine.h, n, to.data_ptr(), td.data_ptr(), MRL, tmin.data_ptr(), cnt.data_ptr(),
                                     itmp.data_ptr()))
    np.testing.assert_array_equal(tmin.cpu().numpy(), ref["isect_min_ray_len"])
    np.testing.assert_array_equal(cnt.cpu().numpy(), ref["isects_count"])
    np.testing.assert_array_equal(itmp.cpu().numpy(), ref["isect_idx_tmp"])


# ---------------------------------------------------------------------------
# d. non-finite rays
@pytest.mark.parametrize("n", [300, 4100])
def test_non_finite_rays_among_ordinary_ones(engine, checker, n):
    """Four rays among ordinary ones on a mixed soup with slivers: NaN in an
    origin, a zero direction, an infinite and a NaN direction component; n = 300
    (unsorted packets) and n = 4 100 (the coherence sort).  What the code does:
      * host_dmax2 takes a NaN |D|^2 as "large" and an infinite one is large, so
        check_dcap rebuilds the records with Dcap = inf (no tiny-triangle drops)
        and the launch culls no sliver piece (a NaN dmax2 counts as +inf);
      * k_raykey clamps with fmaxf / fminf, which drop a NaN operand: such a ray
        gets a key and a place in the order like any other;
      * k_packet marks a packet with such a ray `all` (every sliver packet test
        passes); in the walk the ray's own filter value is NaN, which is not
        <= 0, so it is a candidate for nothing; a zero direction makes the unit
        direction NaN the same way.
    Expected: the four rays hit nothing (isect_mid -1, meas -1), as in the
    reference (DEN == 0, or a NaN t that fails t > eps); the other rays, their
    packet mates included, are bit-exact."""
    arrs = su.soup("mixed", 513, 3, seed=SEED)
    o4, d4, pw = su.aimed_rays(arrs, n, seed=6)
    bad = np.array([7, 64 + 13, 130, n - 2])
    o4[bad[0], 1] = np.nan
    d4[bad[1], :3] = 0.0
    d4[bad[2], 0] = np.inf
    d4[bad[3], 2] = np.nan
    g, o = _bounce_both(engine, checker, arrs, o4, d4, pw)
    for out in (g, o):
        assert np.all(out["isect_mid"][bad] == -1) and np.all(out["meas"][bad] == -1)
    good = np.setdiff1d(np.arange(n), bad)
    sub = lambda d: {k: v[good] for k, v in d.items() if isinstance(v, np.ndarray) and v.shape[:1] == (n,)}
    _not_vacuous(sub(o))
    _cmp_bounce(sub(g), sub(o), checker[1])
    _cmp_bounce(g, o, checker[1])          # and the four themselves (NaN compares equal to NaN)


# ---------------------------------------------------------------------------
# e. lengths
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_short_max_ray_len_and_long_directions(engine, checker, kind):
    """max_ray_len 20 with origins up to 100 away: hits beyond the length count
    (entering / leaving) but never become the nearest.  Then direction lengths
    0.05, 12 and 40: 40 exceeds the records' Dcap = 16 and forces their rebuild
    (check_dcap), after which the first population must still give its results."""
    arrs = su.soup(kind, 513, 1 if kind == "uniform" else 3, seed=SEED + 1)
    o4, d4, pw = su.aimed_rays(arrs, 1237, seed=8)
    short = np.float32(20.0)
    g, o = _bounce_both(engine, checker, arrs, o4, d4, pw, mrl=short)
    beyond = (o["isects_count"].max(axis=1) > 0) & (o["isect_mid"] < 0)
    assert beyond.sum() >= 50 and (o["isect_mid"] >= 0).sum() >= 50, (int(beyond.sum()), int((o["isect_mid"] >= 0).sum()))
    _cmp_bounce(g, o, checker[1])
    ol, dl, pl = su.aimed_rays(arrs, 1237, seed=9, lengths=(0.05, 12.0, 40.0))
    assert np.linalg.norm(dl[:, :3], axis=1).max() > 16.0
    g2, r2 = _bounce_both(engine, checker, arrs, ol, dl, pl)
    _not_vacuous(r2)
    _cmp_bounce(g2, r2, checker[1])
    g3 = engine.bounce(o4, d4, pw, np.zeros(1237, np.int32), np.full(1237, -2, np.int32), short, 1.0)
    _cmp_bounce(g3, o, checker[1])


# ---------------------------------------------------------------------------
# f. launch policies
_policy_ref = {}


@pytest.mark.parametrize("kind", ["mixed", "coplanar"])
@pytest.mark.parametrize("cfg", _POLICIES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_launch_policies_on_soups(checker, monkeypatch, cfg, kind):
    from lightpycl_amd.engine import Engine
    for k, v in cfg.items():
        monkeypatch.setenv(k, v)
    if kind not in _policy_ref:
        arrs = su.soup(kind, 4097, 1 if kind == "coplanar" else 3, seed=SEED)
        _policy_ref[kind] = [arrs, su.aimed_rays(arrs, 4100, seed=4), None]
    arrs, (o4, d4, pw), ref = _policy_ref[kind]
    e = Engine(0)
    try:
        e.upload_arrays(*arrs)
        z, pm = np.zeros(4100, np.int32), np.full(4100, -2, np.int32)
        g = e.bounce(o4, d4, pw, z, pm, MRL, 1.0)
    finally:
        e.close()
    if ref is None:
        ref = _policy_ref[kind][2] = checker[0](_scene(arrs), o4, d4, pw, z, pm, MRL, 1.0)
        _not_vacuous(ref, ties=kind == "coplanar")
    _cmp_bounce(g, ref, checker[1])


# ---------------------------------------------------------------------------
# g. whole traces
TRACE_SEED, TRACE_RAYS, TRACE_ITER = 2, 3000, 6


def _trace_scene():
    """Four soup meshes -- refractive, mirror, terminator, measure -- and rays
    aimed at them with unit directions."""
    parts = [su.soup(kind, M, 1, seed=TRACE_SEED + j) for j, (kind, M) in
             enumerate((("uniform", 600), ("mixed", 300), ("clustered", 200), ("uniform", 400)))]
    v = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    mesh_id = np.repeat(np.arange(4, dtype=np.int32), [p[0].shape[0] for p in parts])
    mats = ((0, 1.5, 0.0, 0.02), (1, 1.0, 0.9, 0.0), (2, 1.0, 0.0, 0.0), (3, 1.0, 0.0, 0.0))
    arrs = (v[0], v[1], v[2], mesh_id) + su.materials(4, mats=mats)
    o4, d4, pw = su.aimed_rays(arrs, TRACE_RAYS, seed=TRACE_SEED, sigmas=(5.0, 30.0), lengths=(1.0,))
    src = types.SimpleNamespace(rays_origin=o4, rays_dir=d4, rays_power=pw.reshape(-1, 1))
    return arrs, su.meshes_of(arrs), src


def test_soup_trace_results_mode(oracle_mod, exact_ref):
    """Results mode: every results tuple element for element against the
    reference host loop over the reference's kernels."""
    from lightpycl_amd.iterative_tracer import CL_Tracer
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    arrs, meshes, src = _trace_scene()
    ref, info = oracle_mod.trace_rays(src.rays_origin, src.rays_dir, src.rays_power, meshes, TRACE_ITER, 0.99, MRL, 1.0,
                                      bounce_fn=exact_ref.bounce)
    assert len(info["counts"]) >= 3, info["counts"]
    assert info["mesh_power"][3] > 0.0
    tr = CL_Tracer(device=0)
    res = tr.iterative_tracer(light_source=[src], meshes=meshes, trace_iterations=TRACE_ITER,
                              trace_until_dissipated=0.99, max_ray_len=MRL, ior_env=1.0)
    assert [len(r[3]) for r in res] == info["counts"]
    for it, (a, b) in enumerate(zip(res, ref)):
        np.testing.assert_array_equal(a[0][:, :3], b[0][:, :3], err_msg=f"origin it{it}")
        np.testing.assert_array_equal(a[1][:, :3], b[1][:, :3], err_msg=f"dest it{it}")
        np.testing.assert_array_equal(a[3], b[3], err_msg=f"meas it{it}")
        assert a[2].shape == b[2].shape
        np.testing.assert_array_equal(a[2], b[2], err_msg=f"pow it{it}")


def test_soup_trace_aggregate_mode(oracle_mod, exact_ref):
    """Aggregate mode: per-iteration counts, per-mesh power and the measured rays
    as a set, against the reference host loop over the reference's kernels."""
    from parity_util import assert_aggregate_equal, lib_aggregate, ref_aggregate
    from lightpycl_amd.engine import Engine
    if exact_ref is None:
        pytest.skip("oracle/_ref not built")
    arrs, meshes, src = _trace_scene()
    o4, d4, pw = src.rays_origin, src.rays_dir, src.rays_power.reshape(-1)
    thr = (1.0 - 0.99) * float(np.sum(pw, dtype=np.float64))
    e = Engine(0)
    try:
        e.upload_arrays(*arrs)
        e.set_rays(o4, d4, pw, MRL, 1.0)
        lib = lib_aggregate(e, TRACE_ITER, thr, reps=2)
    finally:
        e.close()
    ref = ref_aggregate(oracle_mod, exact_ref.bounce, meshes, o4, d4, pw, TRACE_ITER, 0.99, MRL, 1.0)
    assert len(ref[0]) >= 3 and ref[1][3] > 0.0
    assert_aggregate_equal(lib, ref, "soup trace")
