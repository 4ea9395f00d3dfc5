"""The layer-stack scene (tests/stack_util.py) does what its columns declare: the
oracle's bounce of the emitted rays resolves, in every column, the declared hit
mesh, n1, n2 and destination layer, and counts each mesh's layers.  A column the
reference does not realise is a failure here, so the GPU comparison of
tests/test_gpu_stack.py cannot run on a scene that lost its situations."""
import numpy as np
import pytest

import stack_util as su
from soup_util import oracle_scene


@pytest.mark.parametrize("meshes,K", [(su.FULL, None), (su.FULL, 17), (su.REDUCED, None)],
                         ids=["full", "full-K17", "reduced"])
def test_columns_show_their_situation(oracle_mod, meshes, K):
    sc = su.scene(meshes, K)
    assert len(sc.cols) == (len(su.COLUMNS) if meshes is su.FULL else 13)
    cols = su.cycle(sc, 3 * len(sc.cols))
    o, d, p = su.rays(cols)
    n = len(p)
    out = oracle_mod.bounce(oracle_scene(sc.arrs), o, d, p, np.zeros(n, np.int32), np.full(n, -2, np.int32),
                            su.MAX_RAY_LEN, su.IOR_ENV)
    su.check_declared(sc, cols, out)


def test_scene_holds_the_situations():
    """The declared table itself covers what the columns are for: a take-over by
    an entering and by an exiting slot, n2 from the min-max rule, ties, a type-4
    mesh in each role of the second loop, a non-refractive hit taken over."""
    by = {c.name: c for c in su.COLUMNS}
    assert len(by) == len(su.COLUMNS)
    moved = [c for c in su.COLUMNS if c.t_layer != 0]
    assert {c.hit for c in moved} >= {"A", "B", "MIR", "MEAS", "T4"}
    assert any(c.n2 == "T4" and c.t_layer == 1 for c in su.COLUMNS)          # type 4 takes a hit over
    assert any(c.n2 == "T4" and c.t_layer == 0 and c.hit != "T4" for c in su.COLUMNS)   # type 4 as the min-max slot
    ties = [c for c in su.COLUMNS if len({z for z, _ in c.layers}) < len(c.layers)]
    assert len(ties) >= 4
    for c in su.COLUMNS:                # NEAR inside EPSILON, every other gap at least 3e-5
        zs = sorted({z for z, _ in c.layers})
        gaps = np.diff(zs)
        assert np.all((np.abs(gaps - su.NEAR) < 1e-12) | (gaps >= 3e-5)), c.name
    assert su.NEAR < 1e-6 * float(su.MAX_RAY_LEN)
