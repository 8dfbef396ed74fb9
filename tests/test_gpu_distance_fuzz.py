"""Seeded random CSG programs (tests/fuzz_programs.py: one generator per record loop -- general, tree, chain) through
rm_distance_solid on 24^3 points, against the brute-force form of the restatement (tests/distance_ref.py): every point against
every point of the other class.  The occupancy is the oracle's; the volume, the counts and one features call compare with ==."""
import numpy as np
import pytest

import distance_ref as DR
import fuzz_programs as FP
import mass_ref as M
import scenes
from test_gpu_topology import box_lattice, use
from ray_marching_amd import renderer

pytestmark = pytest.mark.gpu

CASES = [(cls, seed) for cls, n in zip(FP.CLASSES, (7, 7, 6)) for seed in range(n)]       # 20 programs


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    yield r
    r.close()


@pytest.mark.parametrize("cls,seed", CASES)
def test_random_programs_against_brute_force(res, oracle, cls, seed):
    assert len(CASES) == 20
    c = FP.case(oracle, cls, seed)
    res.set_materials(c.table)
    try:
        use(res, c.cc, c.words, c.limits)
        origin, step, shape = box_lattice(24)
        level = (0.0, 0.03, -0.02)[seed % 3]
        inside = M.lattice_inside(c.cc, c.words, origin, step, shape, level, c.limits[1])
        want = DR.brute(inside)
        got = res.distance_solid_grid(origin, step, shape, level)
        print("%s seed %d: %s" % (cls, seed, got.counts))
        assert np.array_equal(got.d2(), want), FP.describe(c)
        assert got.counts == DR.counts(want), FP.describe(c)
        feats = got.features(2, 2)
        want_mask, want_counts = DR.features(inside, 2, 2, volume=want)
        assert np.array_equal(feats.mask(), want_mask) and feats.counts == want_counts, FP.describe(c)
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
