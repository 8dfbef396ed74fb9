"""Seeded random CSG programs (tests/fuzz_programs.py: one generator per record loop -- general, tree, chain) and the Scale-by-0
program through rm_label_solid on 24^3 points: the nine counts, both row tables and the whole label volume == the numpy restatement
(tests/topology_ref.py) on the oracle's occupancy, in one merge pass; the brick statistics and the summed body rows ==
rm_mass_moments' on the same lattice and level.  The pass that fills proven-clear bricks from the probe's side sees arbitrary
programs here, not only the named scenes."""
import pytest

import fuzz_programs as FP
import scenes
from test_gpu_topology import box_lattice, check_solid, use
from ray_marching_amd import renderer

pytestmark = pytest.mark.gpu

CASES = [(cls, seed) for cls, n in zip(FP.CLASSES, (7, 7, 6)) for seed in range(n)]       # 20 programs


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    yield r
    r.close()


def check_case(res, c, level):
    res.set_materials(c.table)
    try:
        use(res, c.cc, c.words, c.limits)
        origin, step, shape = box_lattice(24)
        got = check_solid(res, c.cc, c.words, origin, step, shape, level, c.limits[1], what=FP.describe(c))
        assert got.stats["merge_passes"] == 1, FP.describe(c)
        return got
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)


@pytest.mark.parametrize("cls,seed", CASES)
def test_random_programs_against_the_restatement(res, oracle, cls, seed):
    assert len(CASES) == 20
    check_case(res, FP.case(oracle, cls, seed), (0.0, 0.03, -0.02)[seed % 3])


def test_scale_by_zero_next_to_healthy_operands(res, oracle):
    check_case(res, FP.nan_case(oracle), 0.0)
