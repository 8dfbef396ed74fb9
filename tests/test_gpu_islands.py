"""Layer regions and islands on the GPU (rm_islands_solid, rm_islands_occupancy, rm_read_islands): the eight
counts, the region table, the label volume, the mask and the profile against the layer-wise form of the numpy restatement
(tests/islands_ref.py) with ==, on the small shapes against its per-point form too; the brick statistics against rm_mass_moments;
all six build directions at the shapes at which a labelling kernel can go wrong -- the word and the tile borders, long union
chains, every point a root, axes of 1024 points --; known geometry by closed forms; the labelling of rm_label_occupancy as an
independent witness on the device; one lattice above 2^24 points; errors and isolation."""
import ctypes as C
import functools

import numpy as np
import pytest

import islands_ref as IR
import mass_ref as M
import scenes
import support_ref as SR
from test_gpu_topology import box_lattice, program, scene_program, use
from ray_marching_amd import _ffi, csg, renderer

pytestmark = pytest.mark.gpu

LIM = (0.01, 100.0, 256)
BRICK_STATS = ("bricks", "bricks_kept", "bricks_inside", "evaluations")
DENSITIES = (0.02, 0.3, 0.5, 0.98)
R2S = (0, 1, 2, 4, 5, 255)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def plain(rows):
    """The structured region table as uint32 (REGIONS, 12)."""
    return rows.view(np.uint32).reshape(-1, _ffi.RM_ISL_ROW_WORDS)


def same(got, want, what=""):
    """Counts, rows, labels, mask and profile == the restatement's Result."""
    rows, labels, mask, profile = got.rows(), got.labels(), got.mask(), got.profile()
    assert rows.dtype == renderer.ISL_ROW_DTYPE and labels.dtype == np.uint32 and mask.dtype == np.uint8 and profile.dtype == np.uint32
    assert got.counts == want.counts, (what, got.counts, want.counts)
    assert np.array_equal(profile, want.profile), what
    assert np.array_equal(plain(rows), want.rows), what
    assert np.array_equal(labels, want.labels), what
    assert np.array_equal(mask, want.mask), what
    assert got.stats["scratch_bytes"] > 0
    return rows, labels, mask, profile


def middle(shape_xyz, up):
    return shape_xyz[SR.up_index(up) >> 1] // 2


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_inside(name, level):
    cc, w = scene_program(name)
    origin, step, shape = box_lattice(40)
    return M.lattice_inside(cc, w, origin, step, shape, level, LIM[1])


@pytest.mark.parametrize("up", ["+z", "-x"])
@pytest.mark.parametrize("level", [0.0, 0.1])
@pytest.mark.parametrize("name", ["g1", "g8", "g32", "ext_mix", "xform_mix"])
def test_named_scenes(res, name, level, up):
    cc, w = scene_program(name)
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    got = res.islands_solid_grid(origin, step, shape, level, up=up, r2=1)
    print("%s level %g up %s: %s %s" % (name, level, up, got.counts, got.stats))
    rows, *_ = same(got, IR.layerwise(scene_inside(name, level), up, 1), "%s level %g up %s" % (name, level, up))
    mass = res.mass_moments(origin, step, shape, level)
    assert {k: got.stats[k] for k in BRICK_STATS} == {k: mass.stats[k] for k in BRICK_STATS}
    assert got.counts["points"] == int(mass.moments[0]) > 0
    assert np.array_equal(got.roots(rows), IR.roots(plain(rows))) and len(got.islands(rows)) == got.counts["islands"]


# ---- random occupancies at the shapes where a kernel can go wrong -----------------------------------------------------------------
WORD_SHAPES = [tuple(n if a == ax else small[a] for a in range(3)) for n in (63, 64, 65, 129) for ax, small in
               ((0, (0, 5, 4)), (1, (6, 0, 3)), (2, (3, 4, 0)))]                  # (nx, ny, nz): the word / tile border along each axis
SHAPES = [(2, 2, 2), (9, 17, 10), (33, 20, 17)] + WORD_SHAPES + [(1024, 3, 2), (2, 1024, 3), (3, 2, 1024)]


def occupancy_arg(occ, device):
    if not device:
        return occ
    import torch
    return torch.from_numpy(occ.astype(np.uint8) * 255).to("cuda:0")           # any nonzero byte is inside


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_random_occupancies(res, shape):
    """Every direction with every r2; the density, the plate (automatic, 0, a middle layer) and the memory the occupancy comes
    from (host, a torch tensor) go round, so that each meets every direction and every r2."""
    nx, ny, nz = shape
    rng = np.random.default_rng(nx + 7 * ny + 13 * nz)
    occs = [rng.random((nz, ny, nx)) < d for d in DENSITIES]
    small = nx * ny * nz <= 9 * 17 * 10
    for iu, up in enumerate(SR.UPS):
        for ir, r2 in enumerate(R2S):
            occ = occs[(iu + ir) % 4]
            plate = (None, 0, middle(shape, up))[(iu // 2 + ir) % 3]
            device = bool((iu + ir // 2) % 2)
            what = "%s up %s r2 %d plate %s density %g %s" % (shape, up, r2, plate, DENSITIES[(iu + ir) % 4], "device" if device else "host")
            got = res.islands_occupancy(occupancy_arg(occ, device), up=up, r2=r2, plate=plate)
            same(got, IR.layerwise(occ, up, r2, plate), what)
            assert {k: got.stats[k] for k in BRICK_STATS} == dict.fromkeys(BRICK_STATS, 0)
            if small and r2 in (1, 5):
                same(got, IR.per_point(occ, up, r2, plate), what)              # the yardstick's other form, on this very input


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("device", [False, True])
def test_every_plate_and_density_with_every_direction(res, density, device):
    occ = np.random.default_rng(int(density * 100)).random((17, 20, 33)) < density
    for up in SR.UPS:
        for plate in (None, 0, middle((33, 20, 17), up)):
            for r2 in (1, 4):
                got = res.islands_occupancy(occupancy_arg(occ, device), up=up, r2=r2, plate=plate)
                same(got, IR.layerwise(occ, up, r2, plate), "33x20x17 at %g up %s plate %s r2 %d" % (density, up, plate, r2))


@pytest.mark.parametrize("up", SR.UPS)
def test_all_outside_and_all_inside(res, up):
    shape = (17, 20, 33)
    n_a = (33, 20, 17)[SR.up_index(up) >> 1]
    got = res.islands_occupancy(np.zeros(shape, dtype=np.uint8), up=up, r2=2)
    same(got, IR.layerwise(np.zeros(shape, dtype=np.uint8), up, 2), "all outside")
    assert got.counts == dict.fromkeys(IR.COUNT_NAMES, 0) and not got.mask().any() and not got.labels().any() and len(got.rows()) == 0
    full = np.ones(shape, dtype=np.uint8)
    got = res.islands_occupancy(full, up=up, r2=0, plate=3)
    rows, labels, mask, profile = same(got, IR.layerwise(full, up, 0, 3), "all inside")
    layer = 17 * 20 * 33 // n_a
    assert got.counts == {"points": 17 * 20 * 33, "plate": 3, "regions": n_a - 3, "base_regions": 1, "islands": 0, "island_points": 0,
                          "merges": 0, "max_layer_regions": 1}
    assert np.all(mask == 1) and np.all(rows["points"] == layer) and np.all(rows["supported"] == layer)
    assert np.array_equal(rows["below_min"], np.arange(n_a - 3)) and np.array_equal(rows["below_max"], rows["below_min"])


# ---- the shapes that break a labelling kernel -----------------------------------------------------------------------------------
def serpentine(n):
    """Full rows at every other row, joined at alternating ends: one region that crosses every tile border many times."""
    a = np.zeros((n, n), dtype=np.uint8)
    a[0::2, :] = 1
    for t, r in enumerate(range(1, n, 2)):
        a[r, n - 1 if t % 2 == 0 else 0] = 1
    return a, 1


def spiral(n):
    """A square spiral, one point wide with one point of clearance: one region."""
    a = np.zeros((n, n), dtype=np.uint8)
    lo, hi = 0, n - 1
    a[lo, lo:hi + 1] = 1
    while hi - lo >= 2:
        a[lo:hi + 1, hi] = 1                                                       # down the right side
        a[hi, lo:hi + 1] = 1                                                       # back along the bottom
        a[lo + 2:hi + 1, lo] = 1                                                   # up the left side, short of the turn before
        if hi - lo < 4:
            break
        a[lo + 2, lo:hi - 1] = 1                                                   # and along the next turn's top
        lo, hi = lo + 2, hi - 2
    return a, 1


def checker(n):
    j, i = np.indices((n, n))
    return ((i + j) % 2 == 0).astype(np.uint8), (n * n + 1) // 2


def rings(n):
    """Five concentric square rings: nested, not connected."""
    a = np.zeros((n, n), dtype=np.uint8)
    for t in range(5):
        m = 12 * t
        a[m, m:n - m] = a[n - 1 - m, m:n - m] = 1
        a[m:n - m, m] = a[m:n - m, n - 1 - m] = 1
    return a, 5


def staircase(n):
    """The diagonal: as many regions as points."""
    return np.eye(n, dtype=np.uint8), n


def comb(n):
    """Teeth at every other column from row 0 that meet only in row 63, the last row of a tile; the same again below it, meeting in
    the lattice's last row: two regions."""
    a = np.zeros((n, n), dtype=np.uint8)
    a[0:64, 0::2] = 1
    a[63, :] = 1
    a[65:n, 0::2] = 1
    a[n - 1, :] = 1
    return a, 2


def serpentine_columns(n):
    """The serpentine turned: full columns, so that it crosses the border between two tiles of rows at every other column."""
    a, regions = serpentine(n)
    return np.ascontiguousarray(a.T), regions


LAYER_SHAPES = {"serpentine": serpentine, "serpentine_columns": serpentine_columns, "spiral": spiral, "checkerboard": checker, "rings": rings, "staircase": staircase, "comb": comb}


@pytest.mark.parametrize("up", ["+z", "-y", "+x"])
@pytest.mark.parametrize("name", sorted(LAYER_SHAPES))
def test_layers_that_break_a_labelling_kernel(res, name, up):
    """A single layer of 130 x 130 points repeated over three heights, for each frame of the bit rows."""
    layer, regions = LAYER_SHAPES[name](130)
    occ = np.ascontiguousarray(np.moveaxis(np.repeat(layer[None], 3, axis=0), 0, 2 - (SR.up_index(up) >> 1)))
    want = IR.layerwise(occ, up, 1)
    got = res.islands_occupancy(occ, up=up, r2=1)
    print(name, up, got.counts)
    same(got, want, "%s up %s" % (name, up))
    assert got.counts["regions"] == 3 * regions and got.counts["max_layer_regions"] == regions
    assert got.counts["islands"] == 0 and got.counts["base_regions"] * 3 == got.counts["regions"]


# ---- known geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", [0, 1, 4])
def test_stalactites(res, r2):
    occ = IR.stalactites()
    got = res.islands_occupancy(occ, up="+z", r2=r2)
    rows, labels, mask, _ = same(got, IR.layerwise(occ, "+z", r2), "stalactites r2 %d" % r2)
    assert got.counts == {"points": 181, "plate": 0, "regions": 18, "base_regions": 1, "islands": 3, "island_points": 3, "merges": 1,
                          "max_layer_regions": 4}
    merges = np.flatnonzero(rows["below_min"] != rows["below_max"])
    assert len(merges) == 1 and rows[merges[0]]["layer"] == 8 and rows[merges[0]]["points"] == 14 * 10      # the slab
    assert sorted((i["layer"], i["points"]) for i in got.islands(rows)) == [(3, 1), (5, 1), (7, 1)]
    assert np.count_nonzero(mask == 2) == 3 and mask[3, 9, 13] == mask[5, 5, 6] == mask[7, 5, 10] == 2
    root = got.roots(rows)
    assert root[labels[8, 1, 1] - 1] == 1 and len(set(root)) == 4                # the slab grows from the leg; four roots in all
    down = res.islands_occupancy(occ, up="-z", r2=r2)
    same(down, IR.layerwise(occ, "-z", r2), "stalactites down")
    assert down.counts == {"points": 181, "plate": 1, "regions": 18, "base_regions": 1, "islands": 0, "island_points": 0, "merges": 0,
                           "max_layer_regions": 4}


def test_sphere(res):
    """A sphere of radius 1.5 on 24^3 points over [-2, 2]^3, up +z: from plate 0 its lowest layer (3) is an island of 4 points
    at every reach; the automatic plate lies under it."""
    cc, w = program(csg.Sphere((0.0, 0.0, 0.0), 1.5))
    use(res, cc, w)
    origin, step, shape = box_lattice(24, -2.0, 2.0)
    inside = M.lattice_inside(cc, w, origin, step, shape, 0.0, LIM[1])
    assert np.array_equal(inside != 0, IR.sphere24() != 0)
    for r2 in (0, 1, 2, 9):
        got = res.islands_solid_grid(origin, step, shape, 0.0, up="+z", r2=r2, plate=0)
        same(got, IR.layerwise(inside, "+z", r2, 0), "sphere r2 %d" % r2)
        assert got.counts == {"points": 2608, "plate": 0, "regions": 18, "base_regions": 0, "islands": 1, "island_points": 4, "merges": 0,
                              "max_layer_regions": 1}, (r2, got.counts)
        (island,) = got.islands()
        assert island["layer"] == 3 and island["points"] == 4 and np.allclose(island["centroid"][:2], 0.0, atol=1e-6)
    got = res.islands_solid_grid(origin, step, shape, 0.0, up="+z", r2=1)
    assert got.counts["plate"] == 3 and got.counts["islands"] == 0 and got.counts["base_regions"] == 1 and got.counts["regions"] == 18


def test_checkerboard_every_point_is_a_region(res):
    occ = IR.checkerboard()
    got = res.islands_occupancy(occ, up="+z", r2=0)
    same(got, IR.layerwise(occ, "+z", 0), "checkerboard r2 0")
    assert got.counts == {"points": 297, "plate": 0, "regions": 297, "base_regions": 50, "islands": 247, "island_points": 247, "merges": 0,
                          "max_layer_regions": 50}
    got = res.islands_occupancy(occ, up="+z", r2=1)
    same(got, IR.layerwise(occ, "+z", 1), "checkerboard r2 1")
    assert got.counts == {"points": 297, "plate": 0, "regions": 297, "base_regions": 50, "islands": 0, "island_points": 0, "merges": 247,
                          "max_layer_regions": 50}


@pytest.mark.parametrize("up", ["+z", "-y", "+x"])
def test_regions_are_the_bodies_of_every_other_layer(res, up):
    """An independent witness on the device: with every other layer cleared the face-connected bodies of rm_label_occupancy are
    the layers' regions."""
    import torch
    occ = (np.random.default_rng(17).random((40, 70, 67)) < 0.55).astype(np.uint8)
    axis = 2 - (SR.up_index(up) >> 1)
    index = [slice(None)] * 3
    index[axis] = slice(1, None, 2)
    occ[tuple(index)] = 0
    dev = torch.from_numpy(occ).to("cuda:0")
    got = res.islands_occupancy(dev, up=up, r2=0, plate=0)
    topo = res.label_occupancy(dev)
    print(up, got.counts, topo.bodies)
    assert got.counts["regions"] == topo.bodies > 100 and got.counts["points"] == topo.counts["points"]
    assert got.counts["islands"] == got.counts["regions"] - got.counts["base_regions"]      # every layer rests on an empty one


def test_island_mask_through_the_labelling(res):
    """(mask == 2) as a device tensor is an occupancy for rm_label_occupancy: the islands as bodies.  A chip two layers high is an island
    only in its lower layer."""
    import torch
    occ = IR.stalactites()
    occ[4:6, 2, 12] = 1                                                         # a chip in mid air, two layers high
    got = res.islands_occupancy(occ, up="+z", r2=0)
    rows, labels, mask, _ = same(got, IR.layerwise(occ, "+z", 0), "chip")
    assert got.counts["islands"] == 4 and got.counts["island_points"] == 4
    dev = torch.zeros(occ.shape, dtype=torch.uint8, device="cuda:0")
    res.read_islands_device(mask_ptr=dev.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    topo = res.label_occupancy((dev == 2).to(torch.uint8))
    assert topo.bodies == 4 and topo.counts["points"] == 4
    assert np.array_equal(got.mask(), mask) and np.array_equal(got.labels(), labels)      # the result outlives the labelling


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_words(res):
    cc, w = scene_program("g32")
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    for up in ("+y", "-x"):
        a = res.islands_solid_grid(origin, step, shape, up=up, r2=2)
        first = [x.tobytes() for x in (a.rows(), a.labels(), a.mask(), a.profile())]
        b = res.islands_solid_grid(origin, step, shape, up=up, r2=2)
        assert a.counts == b.counts and a.stats == b.stats
        assert first == [x.tobytes() for x in (b.rows(), b.labels(), b.mask(), b.profile())]


def test_device_and_host_read_outs_agree(res):
    import torch
    occ = np.random.default_rng(3).random((17, 20, 33)) < 0.4
    got = res.islands_occupancy(occ, up="-y", r2=2)
    rows, labels, mask, profile = got.rows(), got.labels(), got.mask(), got.profile()
    R = got.counts["regions"]
    assert profile.shape == (20, 4) and R > 10
    stream = torch.cuda.current_stream().cuda_stream
    for want in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
        r = torch.full((R + 2, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        lab = torch.full(occ.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        m = torch.full(occ.shape, 0x5A, dtype=torch.uint8, device="cuda:0")
        p = torch.full((20, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        res.read_islands_device(r.data_ptr() if want[0] else 0, R + 2, lab.data_ptr() if want[1] else 0, m.data_ptr() if want[2] else 0,
                                p.data_ptr() if want[3] else 0, stream=stream)
        torch.cuda.synchronize()
        rr = r.cpu().numpy().view(np.uint32)
        assert np.all(rr[R:] == 0x5A5A5A5A) and (np.array_equal(rr[:R], plain(rows)) if want[0] else np.all(rr == 0x5A5A5A5A))
        assert lab.cpu().numpy().view(np.uint32).tobytes() == (labels.tobytes() if want[1] else np.full(occ.shape, 0x5A5A5A5A, np.uint32).tobytes())
        assert m.cpu().numpy().tobytes() == (mask.tobytes() if want[2] else np.full(occ.shape, 0x5A, np.uint8).tobytes())
        assert p.cpu().numpy().view(np.uint32).tobytes() == (profile.tobytes() if want[3] else np.full((20, 4), 0x5A5A5A5A, np.uint32).tobytes())
    t = torch.zeros(128, dtype=torch.int32, device="cuda:0")
    L = res._L
    assert L.rm_read_islands(res._h, None, 0, None, None, C.c_void_p(t.data_ptr() + 2), 1, None) == _ffi.RM_ERR_ARG      # misaligned
    buf = np.full((R, 12), 0x5A5A5A5A, dtype=np.uint32)
    assert L.rm_read_islands(res._h, buf.ctypes.data, R - 1, None, None, None, 0, None) == _ffi.RM_ERR_RANGE and np.all(buf == 0x5A5A5A5A)
    assert L.rm_read_islands(res._h, None, 0, None, mask.ctypes.data, None, 0, None) == _ffi.RM_OK       # no rows wanted: any capacity
    assert L.rm_read_islands(res._h, buf.ctypes.data, R, None, None, None, 0, None) == _ffi.RM_OK and np.array_equal(buf, plain(rows))


def lattice(o=(-2.0, -2.0, -2.0), s=(0.25, 0.25, 0.25)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


SENTINEL = 0x5A5A5A5A5A5A5A5A
AUTO = _ffi.RM_SUPPORT_PLATE_AUTO


def test_errors_leave_the_outputs_untouched():
    L = _ffi.hip_lib()
    r = renderer.RayMarchingResources(0)                                      # a context of its own: no islands call yet
    try:
        r.resize_command_buffer(65536)
        cc, w = scene_program("g8")
        use(r, cc, w)
        NC, NS = _ffi.RM_ISL_COUNTS, _ffi.RM_ISL_STATS
        counts, stats = (C.c_uint64 * NC)(*[SENTINEL] * NC), (C.c_uint64 * NS)(*[SENTINEL] * NS)
        untouched = lambda: all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in stats)   # noqa: E731
        buf = np.full(17 ** 3, 0x5A, dtype=np.uint8)
        lab = np.full(17 ** 3, 0x5A5A5A5A, dtype=np.uint32)
        prof = np.full(17 * 4, 0x5A5A5A5A, dtype=np.uint32)
        rows = np.full(4096 * 12, 0x5A5A5A5A, dtype=np.uint32)
        read = lambda h=r._h, m=buf.ctypes.data, p=prof.ctypes.data: \
            L.rm_read_islands(h, rows.ctypes.data, 4096, lab.ctypes.data, m, p, 0, None)   # noqa: E731
        assert read() == _ffi.RM_ERR_ARG and read(h=None) == _ffi.RM_ERR_NULL                  # before any islands call
        o, s = lattice()
        solid = lambda h=r._h, o=o, s=s, n=(17, 17, 17), level=0.0, up=4, r2=1, plate=AUTO, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_islands_solid(h, o, s, n[0], n[1], n[2], level, up, r2, plate, counts, nc, stats, ns)   # noqa: E731
        assert solid(h=None) == _ffi.RM_ERR_NULL
        assert solid(counts=None) == _ffi.RM_ERR_NULL and solid(stats=None) == _ffi.RM_ERR_NULL
        assert solid(o=None) == _ffi.RM_ERR_NULL and solid(s=None) == _ffi.RM_ERR_NULL
        assert solid(nc=NC - 1) == _ffi.RM_ERR_ARG and solid(ns=NS - 1) == _ffi.RM_ERR_ARG
        for up in (6, 7, 0xFFFFFFFF):
            assert solid(up=up) == _ffi.RM_ERR_ARG, up
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2), (2, 65536, 2), (1024, 1024, 512)):
            assert solid(n=n) == _ffi.RM_ERR_RANGE, n
        for r2 in (256, 1 << 16, 0xFFFFFFFF):
            assert solid(r2=r2) == _ffi.RM_ERR_RANGE, r2
        for up, n, plate in ((4, (17, 17, 17), 17), (4, (17, 17, 17), 0xFFFFFFFE), (0, (5, 17, 17), 5), (3, (17, 6, 17), 6)):
            assert solid(up=up, n=n, plate=plate) == _ffi.RM_ERR_RANGE, (up, n, plate)
        for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
            assert solid(s=lattice(s=bad)[1]) == _ffi.RM_ERR_ARG, bad
        assert solid(o=lattice(o=(0.0, np.inf, 0.0))[0]) == _ffi.RM_ERR_ARG
        for level in (np.nan, np.inf):
            assert solid(level=level) == _ffi.RM_ERR_ARG
        occ = np.ones((4, 4, 4), dtype=np.uint8)
        occupancy = lambda h=r._h, n=(4, 4, 4), p=occ.ctypes.data, up=4, r2=1, plate=AUTO, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_islands_occupancy(h, n[0], n[1], n[2], p, 0, None, up, r2, plate, counts, nc, stats, ns)   # noqa: E731
        assert occupancy(h=None) == _ffi.RM_ERR_NULL and occupancy(p=None) == _ffi.RM_ERR_NULL
        assert occupancy(counts=None) == _ffi.RM_ERR_NULL and occupancy(stats=None) == _ffi.RM_ERR_NULL
        assert occupancy(nc=NC - 1) == _ffi.RM_ERR_ARG and occupancy(ns=NS - 1) == _ffi.RM_ERR_ARG
        assert occupancy(up=6) == _ffi.RM_ERR_ARG and occupancy(r2=256) == _ffi.RM_ERR_RANGE and occupancy(plate=4) == _ffi.RM_ERR_RANGE
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2)):
            assert occupancy(n=n) == _ffi.RM_ERR_RANGE, n
        # an invalid program: the status a query gives
        r.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
        assert solid() == _ffi.RM_ERR_STACK_UNDERFLOW
        assert untouched() and np.all(buf == 0x5A) and np.all(prof == 0x5A5A5A5A) and np.all(lab == 0x5A5A5A5A) and np.all(rows == 0x5A5A5A5A)
        assert read() == _ffi.RM_ERR_ARG                                                        # still no islands call
        for bad in ({"up": "+w"}, {"up": 6}, {"r2": -1}, {"plate": -1}):
            with pytest.raises(ValueError):
                r.islands_occupancy(occ, **bad)
        with pytest.raises(ValueError):
            r.islands_solid_grid((0, 0, 0), (0.1, 0.1, 0.1), (1, 4, 4))
        with pytest.raises(ValueError):
            r.islands_occupancy(np.zeros((4, 4, 4), dtype=np.float32))
        use(r, cc, w)
        assert solid(plate=16) == _ffi.RM_OK and all(x != SENTINEL for x in stats) and counts[_ffi.RM_ISL_PLATE] == 16
        assert read() == _ffi.RM_OK and set(np.unique(buf)) <= {0, 1} and prof[3 * 4] == np.count_nonzero(buf.reshape(17, 17, 17)[3])
        assert occupancy(plate=3) == _ffi.RM_OK and counts[_ffi.RM_ISL_POINTS] == 64 and counts[_ffi.RM_ISL_REGIONS] == 1
        assert counts[_ffi.RM_ISL_BASE_REGIONS] == 1 and counts[_ffi.RM_ISL_ISLANDS] == 0
        assert read(p=None) == _ffi.RM_OK and np.all(buf[:64] == 1) and list(rows[:4]) == [3, 48, 16, 16]
    finally:
        r.close()


def test_draws_meshes_slices_labels_distances_and_supports_are_left_alone(res, oracle):
    cc, w = scene_program("xform_mix")
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    first = res.draw(W, H)
    origin, step, shape = box_lattice(40)
    mesh = res.extract_mesh_grid_sparse(origin, step, shape)
    slices = res.slice_contours((-2.5,) * 3, (2.5,) * 3, 40, heights=[0.0, 0.4])
    topo = res.label_solid_grid(origin, step, shape)
    labels = topo.labels()
    dist = res.distance_solid_grid(origin, step, shape)
    d2 = dist.d2()
    feats = dist.features(4, 4)
    dmask = feats.mask()
    sup = res.support_solid_grid(origin, step, shape, up="+y", r2=1)
    smask, sprofile = sup.mask(), sup.profile()
    assert len(mesh.triangles) > 0 and len(slices.points) > 0 and topo.bodies == 3
    infos = sorted(k for k in dir(_ffi) if k.startswith("RM_INFO_") and isinstance(getattr(_ffi, k), int))
    before = {k: res.info(getattr(_ffi, k)) for k in infos}
    for up in ("+z", "-x"):
        got = res.islands_solid_grid(origin, step, shape, up=up, r2=1)
        assert got.counts["points"] == topo.counts["points"] == sup.counts["points"]
    assert res.islands_occupancy(np.ones((9, 9, 9), dtype=bool), up="+y").counts["regions"] == 9
    assert {k: res.info(getattr(_ffi, k)) for k in infos} == before
    assert res.draw(W, H).tobytes() == first.tobytes()
    v, t = np.empty((len(mesh.vertices), 3), dtype=np.float32), np.empty((len(mesh.triangles), 3), dtype=np.uint32)
    res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, None, None, 0, None))
    assert v.tobytes() == mesh.vertices.tobytes() and t.tobytes() == mesh.triangles.tobytes()
    p = np.empty((len(slices.points), 3), dtype=np.float32)
    res._check(res._L.rm_read_slices(res._h, p.ctypes.data, None, None, None, None, 0, None))
    assert p.tobytes() == np.asarray(slices.points).tobytes()
    assert topo.labels().tobytes() == labels.tobytes()
    rows = np.zeros((3, 16), dtype=np.uint64)
    res._check(res._L.rm_read_topology(res._h, rows.ctypes.data, None, None, 0, None))
    assert rows.tobytes() == topo.body_moments.tobytes()
    assert dist.d2().tobytes() == d2.tobytes() and feats.mask().tobytes() == dmask.tobytes()
    assert sup.mask().tobytes() == smask.tobytes() and sup.profile().tobytes() == sprofile.tobytes()


# ---- above 2^24 points ------------------------------------------------------------------------------------------------------------
BIG = (264, 256, 256)                                                        # nx, ny, nz


def test_above_2_to_the_24_points(res):
    """The buried stack of eleven plates [40, 200) x [40, 200) of the support tests, two points thick, at k = 150 + 10 t -- the last
    one lies past linear index 2^24.  Up +z every plate is two regions, one per layer; from the automatic plate (150) the lower
    layer of every plate but the first is an island at every r2, from plate 0 the first one too.  Up -x the plates stand on their
    edges: eleven strips per layer, each resting on the one below."""
    nx, ny, nz = BIG
    assert nx * ny * nz > 2 ** 24 and 250 * ny * nx > 2 ** 24
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    for t in range(11):
        occ[150 + 10 * t:152 + 10 * t, 40:200, 40:200] = 1
    A = 160 * 160
    got = res.islands_occupancy(occ, up="+z", r2=5)
    print(got.counts, got.stats)
    assert got.counts == {"points": 22 * A, "plate": 150, "regions": 22, "base_regions": 1, "islands": 10, "island_points": 10 * A,
                          "merges": 0, "max_layer_regions": 1}
    rows = got.rows()
    layers = np.array([150 + 10 * t + d for t in range(11) for d in (0, 1)])
    sums = 160 * (40 + 199) * 160 // 2
    assert np.array_equal(rows["layer"], layers) and np.array_equal(rows["first"], 40 + nx * (40 + ny * layers))
    assert np.all(rows["points"] == A) and np.all(rows["sum_a"] == sums) and np.all(rows["sum_b"] == sums)
    for name, value in (("min_a", 40), ("max_a", 199), ("min_b", 40), ("max_b", 199)):
        assert np.all(rows[name] == value)
    upper = np.arange(22) % 2 == 1
    assert np.array_equal(rows["below_min"], np.where(upper, np.arange(22), 0)) and np.array_equal(rows["below_max"], rows["below_min"])
    assert np.array_equal(rows["supported"], np.where(upper | (np.arange(22) == 0), A, 0))
    want = occ.copy()
    for t in range(1, 11):
        want[150 + 10 * t, 40:200, 40:200] = 2
    assert np.array_equal(got.mask(), want)
    labels = got.labels()
    assert labels.max() == 22 and labels[251, 199, 199] == 22 and labels[250, 40, 40] == 21 and np.count_nonzero(labels) == 22 * A
    profile = got.profile()
    assert profile.shape == (256, 4) and np.array_equal(profile[:, 0], occ.reshape(nz, -1).sum(axis=1))
    assert np.array_equal(profile[:, 1], (profile[:, 0] > 0).astype(np.uint32)) and profile[:, 2].sum() == 10 and profile[:, 3].sum() == 10 * A
    got = res.islands_occupancy(occ, up="+z", r2=0, plate=0)
    assert got.counts == {"points": 22 * A, "plate": 0, "regions": 22, "base_regions": 0, "islands": 11, "island_points": 11 * A,
                          "merges": 0, "max_layer_regions": 1}
    want[150, 40:200, 40:200] = 2
    assert np.array_equal(got.mask(), want)
    got = res.islands_occupancy(occ, up="-x", r2=0)
    assert got.counts == {"points": 22 * A, "plate": 263 - 199, "regions": 11 * 160, "base_regions": 11, "islands": 0, "island_points": 0,
                          "merges": 0, "max_layer_regions": 11}
    rows = got.rows()
    assert np.all(rows["points"] == 320) and np.all(rows["supported"] == 320) and np.array_equal(rows["layer"], 64 + np.arange(1760) // 11)
    assert np.array_equal(rows["below_min"], np.where(np.arange(1760) < 11, 0, np.arange(1760) - 10)) and np.array_equal(got.mask(), occ)
