"""Surface measures on the GPU (rm_surface_solid, rm_surface_classes): the 840 counts against the numpy
restatement (tests/surface_ref.py) with ==, at the shapes and contents at which the kernel can go wrong -- the tile extents of
rml::SurfTileLds on every axis, axes of 1024 points, class boundaries on wave and tile borders, the wave-uniform path next to the
general one --; solids against the oracle's occupancy and rm_mass_moments' statistics; the labelling's edges and the support
analysis' runs and landings as independent witnesses on the device; isolation and errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuzz_programs as FP
import mass_ref as M
import scenes
import support_ref
import surface_ref as SR
from test_gpu_topology import box_lattice, scene_program, use
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = (0.01, 100.0, 256)
BRICK_STATS = ("bricks", "bricks_kept", "bricks_inside", "evaluations")


def tile_extents():
    """(x, y, z) points of a tile of the padded lattice, from rml::SurfTileLds' constants."""
    text = open(os.path.join(ROOT, "ray-marching_amd", "csrc", "rm_lds_layout.h")).read()
    m = re.search(r"kSurfTileX = (\d+)u, kSurfTileY = (\d+)u, kSurfTileZ = (\d+)u", text)
    assert m
    return tuple(int(x) for x in m.groups())


TILE = tile_extents()
SMALL = ((0, 5, 4), (6, 0, 3), (3, 4, 0))
# per axis: one below, at and one above the tile extent -- and the two sizes around which the PADDED lattice (n + 2 points) takes a second tile
TILE_SHAPES = [tuple(TILE[ax] + d if a == ax else SMALL[ax][a] for a in range(3)) for ax in range(3) for d in (-3, -2, -1, 0, 1)]
SHAPES = [(2, 2, 2), (3, 5, 7)] + TILE_SHAPES + [(65, 33, 17), (1024, 2, 2), (2, 1024, 2), (2, 2, 1024)]


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def same(got, data, what=""):
    want = SR.counts(data)
    assert got.counts.dtype == np.uint64 and got.counts.shape == (SR.COUNTS,)
    bad = np.flatnonzero(got.counts != want)
    assert len(bad) == 0, "%s: %d words differ, the first at %d: %d, expected %d" % (what, len(bad), bad[0], got.counts[bad[0]], want[bad[0]])
    assert np.array_equal(got.points, SR.points(want)) and np.array_equal(got.pairs, SR.pairs(want))
    assert int(got.points.sum()) == np.asarray(data).size and got.stats["scratch_bytes"] > 0
    return want


def contents(shape, rng):
    nx, ny, nz = shape
    s = (nz, ny, nx)
    yield "all zero", np.zeros(s, dtype=np.uint8)
    yield "all one", np.ones(s, dtype=np.uint8)
    corners = np.zeros(s, dtype=np.uint8)
    for k in (0, nz - 1):
        for j in (0, ny - 1):
            for i in (0, nx - 1):
                corners[k, j, i] = 1 + (i > 0) + 2 * (j > 0) + 4 * (k > 0) if (i, j, k) != (nx - 1, ny - 1, nz - 1) else 7
    yield "corners", corners
    yield "random bytes", rng.integers(0, 256, size=s, dtype=np.uint8)
    yield "random classes", rng.integers(0, 8, size=s, dtype=np.uint8)
    yield "sparse", (rng.random(s) < 0.1).astype(np.uint8) * 3


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_lattices(res, shape):
    rng = np.random.default_rng(shape[0] + 7 * shape[1] + 13 * shape[2])
    for what, data in contents(shape, rng):
        got = res.surface_classes(data)
        same(got, data, "%s %s" % (shape, what))
        assert got.shape == shape and all(got.stats[k] == 0 for k in BRICK_STATS)


def test_single_corner_points(res):
    nx, ny, nz = 5, 4, 3
    for k in (0, nz - 1):
        for j in (0, ny - 1):
            for i in (0, nx - 1):
                data = np.zeros((nz, ny, nx), dtype=np.uint8)
                data[k, j, i] = 1
                got = res.surface_classes(data)
                same(got, data, "corner %s" % ((i, j, k),))
                assert int(got.pairs.sum()) == 26 and np.all(got.pairs[1, 0] == 1) and np.all(got.pairs[0, 1] == 1)


def test_slabs_on_wave_and_tile_borders(res):
    """Class boundaries where a wave's row of owners and a tile of the padded lattice begin (its owners start at coordinate -1, so
    tile t begins at t * extent - 1), one point to either side, and in the lattice's first and last layer."""
    tx, ty, tz = TILE
    nx, ny, nz = 2 * tx + 2, 2 * ty + 3, 2 * tz + 3
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for dx in (-2, -1, 0):
        data = (1 + (i >= tx + dx) + 2 * (j >= ty + dx) + 4 * (k >= tz + dx)).astype(np.uint8) - 1
        same(res.surface_classes(data), data, "slabs at %d" % dx)
        for axis, n in ((i, nx), (j, ny), (k, nz)):
            for at in (0, n - 1):
                layer = np.where(axis == at, 6, data).astype(np.uint8)
                same(res.surface_classes(layer), layer, "slabs at %d with a layer" % dx)


def test_uniform_block_with_one_odd_point(res):
    """Most waves see one class in all lanes and all neighbours (one count from one lane), the waves around the odd point and at
    the block's faces do not: both paths in one call, and again with the odd point in every lane position of a row."""
    tx, ty, tz = TILE
    nx, ny, nz = 2 * tx + 5, ty + 9, tz + 6
    block = np.zeros((nz, ny, nx), dtype=np.uint8)
    block[1:-1, 2:-1, 3:-2] = 3
    same(res.surface_classes(block), block, "block")
    full = np.full((nz, ny, nx), 3, dtype=np.uint8)
    want = same(res.surface_classes(full), full, "full")
    assert int(SR.pairs(want)[3, 3, 0]) == (nx - 1) * ny * nz
    for x in (0, 1, tx - 2, tx - 1, tx, nx - 1):
        odd = block.copy()
        odd[nz // 2, ny // 2, x] = 5
        got = res.surface_classes(odd)
        same(got, odd, "odd point at x = %d" % x)
        assert int(got.points[5]) == 1


def test_device_classes_on_a_user_stream(res):
    import torch
    data = np.random.default_rng(3).integers(0, 256, size=(17, 33, 65), dtype=np.uint8)
    stream = torch.cuda.Stream(device=0)
    with torch.cuda.stream(stream):
        t = torch.from_numpy(data).to("cuda:0", non_blocking=True)          # (the copy is queued on the stream the call must wait for)
        got = res.surface_classes(t)
    same(got, data, "device, user stream")


# ---- solids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,seed", [("general", 1), ("tree", 2)])
def test_solids_of_random_programs(res, oracle, cls, seed):
    c = FP.case(oracle, cls, seed)
    res.set_materials(c.table)
    try:
        use(res, c.cc, c.words, c.limits)
        origin, step, shape = box_lattice((40, 33, 24))
        level = (0.0, 0.03)[seed % 2]
        inside = M.lattice_inside(c.cc, c.words, origin, step, shape, level, c.limits[1])
        got = res.surface_solid_grid(origin, step, shape, level)
        print("%s: %s %s" % (FP.describe(c), got, got.stats))
        same(got, inside.astype(np.uint8), FP.describe(c))
        mass = res.mass_moments(origin, step, shape, level)
        assert {k: got.stats[k] for k in BRICK_STATS} == {k: mass.stats[k] for k in BRICK_STATS}
        assert int(got.points[1]) == int(mass.moments[_ffi.RM_MOMENT_COUNT]) and int(got.points[2:].sum()) == 0
        m, ref = got.measures(1, 0), SR.measures(got.counts, step, [1], [0])
        assert m["facet_area"] == pytest.approx(ref["facet_area"], rel=1e-14)
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)


def test_sphere_area(res):
    """The unit sphere g1 on 64^3 points over [-2.5, 2.5]^3: R = 12.6 index units, between the radii 10.3 and 14.7 of DESIGN.md
    section 25's table, whose larger recorded error (1.08 %) bounds it."""
    cc, w = scene_program("g1")
    use(res, cc, w)
    got = res.surface_solid((-2.5,) * 3, (2.5,) * 3, 64)
    m = got.measures(1, 0)
    radius = float(np.asarray(w[1:5]).view(np.float32)[3])
    print("g1: radius %g, area %.6f, facet area %.6f, 4 pi R^2 %.6f" % (radius, m["area"], m["facet_area"], 4 * np.pi * radius ** 2))
    assert abs(m["area"] / (4.0 * np.pi * radius * radius) - 1.0) <= 0.0108


# ---- the other analyses as witnesses -------------------------------------------------------------------------------------------------
def scene_occupancy():
    cc, w = scene_program("g8")
    origin, step, shape = box_lattice((40, 36, 28))
    return M.lattice_inside(cc, w, origin, step, shape, 0.0, LIM[1]).astype(np.uint8)


def test_edges_of_the_labelling(res):
    occ = scene_occupancy()
    got = res.surface_classes(occ)
    assert int(got.pairs[1, 1, 0:3].sum()) == res.label_occupancy(occ).counts["edges"] > 0


@pytest.mark.parametrize("up", ["+z", "-z", "+x", "-y"])
def test_runs_and_landings_of_the_support_analysis(res, up):
    occ = scene_occupancy()
    sup = res.support_occupancy(occ, up=up, r2=1)
    P = res.surface_classes(sup.mask()).pairs
    axis, neg = divmod(support_ref.up_index(up), 2)
    pair = (lambda lo, hi: int(P[hi, lo, axis])) if neg else (lambda lo, hi: int(P[lo, hi, axis]))
    assert sum(pair(s, 2) for s in (3, 4)) == sup.counts["runs"] and sup.counts["runs"] > 0
    assert sum(pair(a, s) for a in (1, 2) for s in (3, 4)) == sup.counts["landings"]


# ---- isolation ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_the_retained_results(res):
    occ = scene_occupancy()
    topo = res.label_occupancy(occ)
    labels = topo.labels()
    first = res.surface_classes(occ)
    second = res.surface_classes(occ)
    assert np.array_equal(first.counts, second.counts)
    assert np.array_equal(topo.labels(), labels)                       # the labelling is still there, and still the same
    cc, w = scene_program("g8")
    use(res, cc, w)
    origin, step, shape = box_lattice((40, 36, 28))
    solid = res.surface_solid_grid(origin, step, shape, 0.0)
    assert np.array_equal(solid.counts, first.counts) and np.array_equal(topo.labels(), labels)


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch(res):
    cc, w = scene_program("g1")
    use(res, cc, w)
    L, h = res._L, res._h
    counts, stats = np.full(SR.COUNTS, 77, dtype=np.uint64), np.full(_ffi.RM_SURF_STATS, 77, dtype=np.uint64)
    cp, sp = counts.ctypes.data_as(C.POINTER(C.c_uint64)), stats.ctypes.data_as(C.POINTER(C.c_uint64))
    f3 = lambda *v: np.array(v, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))    # noqa: E731
    o, s = f3(-2.5, -2.5, -2.5), f3(0.1, 0.1, 0.1)
    data = np.ones((4, 4, 4), dtype=np.uint8)
    dp = C.c_void_p(data.ctypes.data)
    n, ns = SR.COUNTS, _ffi.RM_SURF_STATS
    cases = [
        (L.rm_surface_solid(h, o, s, 8, 8, 8, 0.0, None, n, sp, ns), _ffi.RM_ERR_NULL),
        (L.rm_surface_solid(h, o, s, 8, 8, 8, 0.0, cp, n, None, ns), _ffi.RM_ERR_NULL),
        (L.rm_surface_solid(None, o, s, 8, 8, 8, 0.0, cp, n, sp, ns), _ffi.RM_ERR_NULL),
        (L.rm_surface_solid(h, o, s, 8, 8, 8, 0.0, cp, n - 1, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, o, s, 8, 8, 8, 0.0, cp, n, sp, ns - 1), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, o, s, 8, 8, 8, float("nan"), cp, n, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, o, s, 8, 8, 8, float("inf"), cp, n, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, o, f3(0.1, 0.0, 0.1), 8, 8, 8, 0.0, cp, n, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, f3(0.0, float("nan"), 0.0), s, 8, 8, 8, 0.0, cp, n, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_solid(h, o, s, 1, 8, 8, 0.0, cp, n, sp, ns), _ffi.RM_ERR_RANGE),
        (L.rm_surface_solid(h, o, s, 8, 1025, 8, 0.0, cp, n, sp, ns), _ffi.RM_ERR_RANGE),
        (L.rm_surface_solid(h, o, s, 1024, 1024, 257, 0.0, cp, n, sp, ns), _ffi.RM_ERR_RANGE),
        (L.rm_surface_classes(h, 4, 4, 4, None, 0, None, cp, n, sp, ns), _ffi.RM_ERR_NULL),
        (L.rm_surface_classes(h, 4, 4, 4, dp, 0, None, None, n, sp, ns), _ffi.RM_ERR_NULL),
        (L.rm_surface_classes(h, 4, 4, 4, dp, 0, None, cp, n - 1, sp, ns), _ffi.RM_ERR_ARG),
        (L.rm_surface_classes(h, 4, 4, 4, dp, 0, None, cp, n, sp, ns - 1), _ffi.RM_ERR_ARG),
        (L.rm_surface_classes(h, 4, 1, 4, dp, 0, None, cp, n, sp, ns), _ffi.RM_ERR_RANGE),
        (L.rm_surface_classes(h, 4, 4, 1025, dp, 0, None, cp, n, sp, ns), _ffi.RM_ERR_RANGE),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    assert np.all(counts == 77) and np.all(stats == 77)
    # the messages are the labelling's, word for word, under this call's names
    assert L.rm_surface_classes(h, 4, 4, 4, dp, 0, None, cp, n - 1, sp, ns) == _ffi.RM_ERR_ARG
    mine = L.rm_last_error(h).decode()
    assert L.rm_label_occupancy(h, 4, 4, 4, dp, 0, None, cp, _ffi.RM_TOPO_COUNTS - 1, sp, ns + 1) == _ffi.RM_ERR_ARG
    theirs = L.rm_last_error(h).decode()
    assert mine == theirs.replace("rm_label_occupancy", "rm_surface_classes").replace("RM_TOPO_COUNTS", "RM_SURF_COUNTS").replace(
        "n_counts %d" % (_ffi.RM_TOPO_COUNTS - 1), "n_counts %d" % (n - 1))
    assert L.rm_surface_classes(h, 4, 4, 4, dp, 0, None, cp, n, sp, ns) == _ffi.RM_OK and int(counts[1]) == 64
