"""postproc<KU> (lpc_math.hpp) against the oracle's intersect_postproc on
enumerated slot tables, on the host.  tests/postproc_tables.py builds the rows:
seven t values around the nearest hit and max_ray_len, crossed with the count's
parity and refractive / other material in every slot.

  K = 1..4   every table of 28^K symbols under every prev in {-2, -1, 0..K-1}
  K in 5, 8, 9, 12, 13, 16, 17, 33, 65
             200 000 rows each from a fixed stream, one slot at the nearest hit

for max_ray_len 1000, 1 and 37.5.  The harness (tests/csrc/
postproc_tables_harness.cpp) runs postproc<0> and the KU the shading kernels
pick for K (4, 8, 12, 16; 0 above), slots from K up clean as the kernels load
them; orc_intersect_postproc (oracle/lpc_oracle.c) runs the same rows with
origin 0 and direction +x, so dest.x is t_min.  All six fields are equal on
every row.

So that the sweep cannot go hollow, each K's rows must show, in the oracle's own
output (postproc_tables.outcomes): a hit taken over by an entering slot; by an
exiting slot with n2 from the min-max rule (three slots at least: K >= 3); by
an exiting slot with no min-max slot; hit_mesh != n2 != -1; a tie in the first
loop (lowest index) and in the second (highest index); and every material type
as the hit mesh and both refractive types as a taken-over n2 (K >= 2: one slot
alone is never taken over).
"""
import numpy as np
import pytest

import postproc_tables as pt

NEED = ("entering_takeover", "exiting_alone", "n2_other", "tie_first", "tie_second")


@pytest.fixture(scope="module")
def run():
    return pt.harness()


class _Seen:
    def __init__(self):
        self.rows = 0
        self.count = {}
        self.hit_types = set()
        self.n2_types = set()

    def add(self, rows, ref):
        self.rows += rows.n
        oc = pt.outcomes(rows, ref)
        for k, v in oc.items():
            self.count[k] = self.count.get(k, 0) + int(v.sum())
        assert oc["tie_first_lowest"].all() and oc["tie_second_highest"].all()
        ar = np.arange(rows.n)
        h = ref[:, 0]
        self.hit_types |= set(np.unique(rows.mat[ar[h >= 0], h[h >= 0]]).tolist())
        tk = oc["entering_takeover"]
        self.n2_types |= set(np.unique(rows.mat[ar[tk], ref[tk, 3]]).tolist())

    def check(self, K, expect_rows):
        assert self.rows == expect_rows, (K, self.rows, expect_rows)
        if K == 1:
            assert self.hit_types == {0, 1, 2, 3, 4}
            return
        need = NEED + (("exiting_minmax",) if K >= 3 else ())
        for k in need:
            assert self.count[k] > 0, f"K={K}: no row with outcome {k}: {self.count}"
        assert self.hit_types == {0, 1, 2, 3, 4}, (K, self.hit_types)
        assert self.n2_types == {0, 4}, (K, self.n2_types)


def _compare(run, oracle_mod, rows, seen, what):
    ref = pt.oracle_postproc(oracle_mod, rows)
    g0, gk = run(rows)
    for got, name in ((g0, "postproc<0>"), (gk, f"postproc<{run.lib.postproc_tables_ku(rows.K)}>")):
        bad = np.flatnonzero(np.any(got != ref, axis=1))
        if bad.size:
            r = bad[0]
            raise AssertionError(
                f"{what}, {name}: {bad.size} of {rows.n} rows differ; first row {r}: prev={rows.prev[r]} "
                f"mat={rows.mat[r].tolist()} t={rows.t[r].tolist()} cnt={rows.cnt[r].tolist()} idx={rows.idx[r].tolist()}\n"
                f"  {pt.FIELDS}\n  library {got[r].tolist()}\n  oracle  {ref[r].tolist()}")
    seen.add(rows, ref)


@pytest.mark.parametrize("K", pt.EXHAUSTIVE_K)
def test_exhaustive_tables(run, oracle_mod, K):
    for mrl in pt.MAX_RAY_LENS:
        seen = _Seen()
        for prev in range(-2, K):
            _compare(run, oracle_mod, pt.exhaustive_rows(K, mrl, prev), seen, f"K={K} max_ray_len={mrl} prev={prev}")
        seen.check(K, pt.exhaustive_count(K))


@pytest.mark.parametrize("K", pt.SAMPLED_K)
def test_sampled_tables(run, oracle_mod, K):
    for mrl in pt.MAX_RAY_LENS:
        seen = _Seen()
        rows = pt.sampled_rows(K, mrl)
        assert np.all((rows.t == pt.alphabet(mrl)[0]).any(axis=1)), "a slot at the nearest hit in every row"
        _compare(run, oracle_mod, rows, seen, f"K={K} max_ray_len={mrl}")
        seen.check(K, pt.SAMPLED_ROWS)


def test_ku_follows_the_runtime():
    """The harness picks KU as with_ku (lpc_runtime.hip) does: the test reads the
    runtime's own thresholds out of its source."""
    import os
    import re
    src = open(os.path.join(pt.ROOT, "lightpycl_amd", "csrc", "lpc_runtime.hip")).read()
    body = src[src.index("static void with_ku(int K, F &&f)"):]
    body = body[:body.index("\n}\n")]
    pairs = [(int(a), int(b)) for a, b in re.findall(r"K <= (\d+)\) f\(std::integral_constant<int, (\d+)>", body)]
    assert pairs == [(4, 4), (8, 8), (12, 12), (16, 16)] and "integral_constant<int, 0>" in body
    L = pt.harness().lib
    for K in range(1, 70):
        want = next((ku for lim, ku in pairs if K <= lim), 0)
        assert L.postproc_tables_ku(K) == want
