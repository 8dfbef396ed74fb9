"""Seeded random CSG programs (tests/fuzz_programs.py: one generator per record loop -- general, tree, chain) through
rm_islands_solid on 24^3 points with a random build direction, squared reach and plate, against the per-point form of the
restatement (tests/islands_ref.py): per layer a flood fill, per point a loop over the disc.  The occupancy is the oracle's; counts,
region table, labels, mask and profile compare with ==."""
import numpy as np
import pytest

import fuzz_programs as FP
import islands_ref as IR
import mass_ref as M
import scenes
import support_ref as SR
from test_gpu_topology import box_lattice, use
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

CASES = [(cls, seed) for cls, n in zip(FP.CLASSES, (7, 7, 6)) for seed in range(n)]       # 20 programs


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    yield r
    r.close()


@pytest.mark.parametrize("cls,seed", CASES)
def test_random_programs_against_the_definitions(res, oracle, cls, seed):
    assert len(CASES) == 20
    c = FP.case(oracle, cls, seed)
    res.set_materials(c.table)
    try:
        use(res, c.cc, c.words, c.limits)
        origin, step, shape = box_lattice(24)
        level = (0.0, 0.03, -0.02)[seed % 3]
        rng = np.random.default_rng(2000 * FP.CLASSES.index(cls) + seed + 500)
        up = SR.UPS[int(rng.integers(6))]
        r2 = int(rng.choice((0, 1, 2, 4, 5, 9, 18)))
        plate = (None, 0, int(rng.integers(24)))[int(rng.integers(3))]
        inside = M.lattice_inside(c.cc, c.words, origin, step, shape, level, c.limits[1])
        want = IR.per_point(inside, up, r2, plate)
        got = res.islands_solid_grid(origin, step, shape, level, up=up, r2=r2, plate=plate)
        print("%s seed %d up %s r2 %d plate %s: %s" % (cls, seed, up, r2, plate, got.counts))
        assert got.counts == want.counts, FP.describe(c)
        assert np.array_equal(got.rows().view(np.uint32).reshape(-1, _ffi.RM_ISL_ROW_WORDS), want.rows), FP.describe(c)
        assert np.array_equal(got.profile(), want.profile), FP.describe(c)
        assert np.array_equal(got.labels(), want.labels), FP.describe(c)
        assert np.array_equal(got.mask(), want.mask), FP.describe(c)
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
