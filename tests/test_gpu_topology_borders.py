"""rm_label_occupancy where the random occupancies of tests/test_gpu_topology.py may never go: every one of
the 26 neighbour offsets across every kind of brick border (face, edge, corner: 124 cases, for bodies and for voids), the same on
a lattice whose last bricks are one and two points thick, and the worst cases of single passes -- a path of 143 points that fills
one brick (the local pass's rounds), checkerboards (32 labels to a wave of the rows pass, 131 072 bodies), 29 791 cavities, and
cavities and bodies that cross many bricks.  Every result == the numpy restatement (tests/topology_ref.py) -- counts, both row
tables, the whole label volume -- in ONE merge pass, and == the literals of tests/topology_cases.py, which
tests/test_topology_cpu.py checks against the restatement without a GPU."""
import functools

import numpy as np
import pytest

import mass_ref as M
import scenes
import topology_cases as TC
import topology_ref as TR
from test_gpu_topology import BRICK_STATS, same, summary
from ray_marching_amd import renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def label(res, occ, what):
    """label_occupancy(occ) == the restatement, in one merge pass (same() asserts both)."""
    got = res.label_occupancy(occ)
    same(got, TR.topology(occ), what)
    assert got.stats["merge_passes"] == 1, what
    assert {k: got.stats[k] for k in BRICK_STATS} == dict.fromkeys(BRICK_STATS, 0)
    return got


# ---- every offset across every border ---------------------------------------------------------------------------------------------
def test_there_are_124_cases():
    assert len(TC.BORDER_CASES) == 124 and sum(len(TC.packed_pairs(d)) for d in TC.OFFSETS) == 124


@pytest.mark.parametrize("inside", [True, False], ids=["bodies", "voids"])
@pytest.mark.parametrize("d", TC.OFFSETS, ids=lambda d: "%+d%+d%+d" % d)
def test_a_pair_across_each_kind_of_border(res, d, inside):
    """The 2, 4 or 8 straddle subsets of offset d in one lattice: an inside pair is one body across a face and two bodies across
    an edge or a corner; a void pair in a full lattice is one cavity of exactly 2 points, and nothing is exterior."""
    pairs = TC.packed_pairs(d)
    occ = TC.occupancy_of(pairs, TC.PACKED_SHAPE, inside)
    got = label(res, occ, "offset %s %s" % (d, "bodies" if inside else "voids"))
    TC.check_expected(got.counts, got.cavity_moments, TC.expected_of_pairs(d, pairs, TC.PACKED_SHAPE, inside))
    if inside:
        assert got.bodies == len(pairs) * (1 if TC.faces_of(d) == 1 else 2) and got.cavities == 0
    else:
        assert got.cavities == len(pairs) and got.counts["exterior_points"] == 0
        for q in range(len(pairs)):
            assert int(got.cavity_moments[q][0]) == 2
        lab = got.labels()
        for a, b in pairs:                                                    # the two points of a pair carry one cavity's number
            assert lab[a[2], a[1], a[0]] == lab[b[2], b[1], b[0]] and lab[a[2], a[1], a[0]] & TR.CAVITY_BIT


@pytest.mark.parametrize("inside", [True, False], ids=["bodies", "voids"])
def test_pairs_across_thin_last_bricks(res, inside):
    """17 x 18 x 23 points: the last brick is one point thick in x and two in y.  A void at i = 16 lies on the border now: it is
    exterior, not a cavity."""
    for d in TC.OFFSETS:
        pairs = [TC.thin_pair(d)]
        occ = TC.occupancy_of(pairs, TC.THIN_SHAPE, inside)
        got = label(res, occ, "thin %s %s" % (d, "bodies" if inside else "voids"))
        want = TC.expected_of_pairs(d, pairs, TC.THIN_SHAPE, inside)
        TC.check_expected(got.counts, got.cavity_moments, want)
        if not inside:
            assert (got.cavities, got.counts["exterior_points"]) == ((0, 2) if d[0] != 0 else (1, 0)), d


# ---- worst cases of single passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", TC.ORIENTATIONS, ids=lambda m: "".join("-+"[not x] for x in m))
@pytest.mark.parametrize("way", sorted(TC.SNAKE_WAYS))
def test_snake(res, way, mirror):
    """One path of 143 points through one brick (the local pass needs its rounds), through eight, and as a cavity; mirrored in
    every axis, so that the smallest index sits at either end and the index order runs with and against the path."""
    got = label(res, TC.snake_case(way, mirror), "snake %s %s" % (way, mirror))
    assert summary(got) == TC.SNAKE_WAYS[way]
    if way == "complement":
        assert int(got.cavity_moments[0][0]) == 143 and got.counts["points"] == 24 ** 3 - 143
    else:
        assert got.counts["points"] == 143 and int(got.body_moments[0][0]) == 143


@pytest.mark.parametrize("parity", [0, 1])
def test_checkerboard_small(res, parity):
    """33 x 20 x 17: 5610 one-point bodies, 32 distinct labels in every full wave of the rows pass; the other colour is one
    exterior component held together by edge diagonals only."""
    got = label(res, TC.checkerboard(TC.SMALL, parity), "checkerboard parity %d" % parity)
    assert summary(got) == (5610, 0, 5610, 0) and got.counts["exterior_points"] == 5610
    assert all(int(r[0]) == 1 for r in got.body_moments)


@functools.lru_cache(maxsize=None)
def big_reference(name):
    occ = TC.checkerboard((64, 64, 64)) if name == "checkerboard" else TC.buried_voids(64)
    occ.setflags(write=False)
    return occ, TR.topology(occ)


def points_of(mask):
    """(i, j, k) of the True points in linear order."""
    k, j, i = np.nonzero(mask)
    return i, j, k


def rows_of_single_points(i, j, k):
    """mass_ref.box_moments of each one-point box, as an array."""
    rows = np.empty((len(i), 16), dtype=np.uint64)
    for e, col in enumerate((np.ones_like(i), i, j, k, i * i, j * j, k * k, i * j, j * k, k * i, i, j, k, i, j, k)):
        rows[:, e] = col
    for n in (0, len(i) // 2, len(i) - 1):
        p = (int(i[n]), int(j[n]), int(k[n]))
        assert [int(x) for x in rows[n]] == M.box_moments(p, tuple(x + 1 for x in p))
    return rows


def test_checkerboard_above_2_to_the_16_bodies(res):
    occ, want = big_reference("checkerboard")
    got = label(res, occ, "checkerboard 64^3")
    assert got.bodies == 131072 > 2 ** 16 and got.cavities == 0 and got.counts["exterior_points"] == 131072
    lab = got.labels()
    assert np.array_equal(lab[occ], np.arange(131072, dtype=np.uint32))      # its rank among the inside points in linear order
    assert np.array_equal(got.body_moments, rows_of_single_points(*points_of(occ)))


def test_29791_cavities(res):
    occ, want = big_reference("voids")
    got = label(res, occ, "buried voids 64^3")
    assert (got.bodies, got.cavities) == (1, 31 ** 3) and 31 ** 3 == 29791 and got.counts["exterior_points"] == 0
    lab = got.labels()
    assert np.array_equal(lab[~occ], TR.CAVITY_BIT | np.arange(29791, dtype=np.uint32))   # numbered in linear order
    assert np.array_equal(got.cavity_moments, rows_of_single_points(*points_of(~occ)))


@pytest.mark.parametrize("axis", sorted(TC.FRAMED))
def test_plane_cavities_that_cross_every_brick(res, axis):
    got = label(res, TC.framed_planes(axis), "framed planes along %s" % axis)
    assert summary(got) == TC.FRAMED[axis]
    nz, ny, nx = TC.SMALL
    size = {"k": (nx - 2) * (ny - 2), "j": (nx - 2) * (nz - 2), "i": (ny - 2) * (nz - 2)}[axis]
    assert all(int(r[0]) == size for r in got.cavity_moments)


def test_rods_through_five_bricks(res):
    got = label(res, TC.rods(), "rods")
    assert summary(got) == (90, 0, 90, 0) and all(int(r[0]) == 33 for r in got.body_moments)
