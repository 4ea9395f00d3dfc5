"""Host-only condition of tests/test_gpu_iter_launches.py: its pole cases give
the sliver path something to decide.  By the CPU oracle some of their rays have
the nearest hit on a triangle with E1 x E2 = 0, which no hierarchy record holds."""
import numpy as np
import pytest

import iter_launch_util as ilu
from lightpycl_amd import scenes


@pytest.fixture(scope="module")
def scene():
    return scenes.synthetic(n=16, seed=7, iterations=6)


@pytest.mark.parametrize("n", ilu.POLE_SIZES)
def test_pole_rays_end_on_zero_cross_triangles(oracle_mod, scene, n):
    S = oracle_mod.Scene(scene.meshes)
    o4, d4, pw = ilu.pole_rays(S, n)
    assert len(np.unique(pw)) == n
    out = oracle_mod.bounce(S, o4, d4, pw, np.zeros(n, np.int32), np.full(n, -2, np.int32), scene.max_ray_len,
                            scene.ior_env)
    assert np.all(out["isect_mid"] == 0)            # every ray ends on the hemisphere
    count = ilu.nearest_on_zero_cross(S, out)
    print(f"pole rays {n}: nearest hit on a zero-cross triangle: {count}")
    assert count > 0
