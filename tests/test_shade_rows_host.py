"""shade() (lpc_math.hpp), built for the host, against the oracle's
reflect_refract_rays on the constructed rows of tests/shade_rows.py: every
material branch, the back-face flip, the critical angle ulp by ulp, the
dissipation threshold, the rescaling branches of normalize and length, meas_in
and the NaN-TIR path.  Both sides are host code with the same correctly rounded
square roots and the same C library, so every output is equal bit for bit; the
device's side of the same rows is tests/test_gpu_shade_tables.py."""
import numpy as np
import pytest

import postproc_tables as pt
import shade_rows as sr


@pytest.mark.parametrize("with_huge", [True, False], ids=["huge", "no-huge"])
def test_shade_rows_equal_the_oracle(oracle_mod, with_huge):
    sc = sr.scene(with_huge)
    R = sr.rows(sc)
    want = sr.oracle_shade(oracle_mod, sc, R)
    got = sr.host_shade(pt.harness().lib, sc, R)
    seen = sr.check_coverage(sc, R, want)
    assert seen["nan"] > 0
    for k in sr.OUT:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        bad = np.flatnonzero(np.any((a.view(np.int32) != b.view(np.int32)).reshape(R.n, -1), axis=1))
        assert bad.size == 0, (k, bad.size, R.group[bad[0]], int(bad[0]), a[bad[0]], b[bad[0]])
    # the NaN-TIR rows: dead children
    nan = sr.nan_rows(sc, R, want)
    assert not got["r_dir"][nan].any() and not got["t_dir"][nan].any() and not got["t_pow"][nan].any()
    assert np.all(got["r_meas"][nan] == -1) and np.all(got["t_meas"][nan] == -1)
