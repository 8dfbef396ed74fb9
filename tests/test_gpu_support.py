"""Overhangs and supports on the GPU (rm_support_solid, rm_support_occupancy, rm_read_support): the whole
mask, the eight counts and the profile against the layer-wise form of the numpy restatement (tests/support_ref.py) with ==, on the
small shapes against its per-point form too; the brick statistics against rm_mass_moments on the same lattice; all six build
directions at the shapes at which a kernel can go wrong -- the word boundary of the bit rows and its carries, axes of 1024 points
--; known geometry by closed forms; one lattice above 2^24 points; errors and isolation."""
import ctypes as C
import functools

import numpy as np
import pytest

import mass_ref as M
import scenes
import support_ref as SR
import topology_ref as TR
from test_gpu_topology import box_lattice, program, scene_program, use
from ray_marching_amd import _ffi, csg, renderer

pytestmark = pytest.mark.gpu

F = np.float32
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


def same(got, want, what=""):
    """Mask, counts and profile == the restatement's (mask, counts, profile)."""
    want_mask, want_counts, want_profile = want
    mask, profile = got.mask(), got.profile()
    assert mask.dtype == np.uint8 and mask.shape == want_mask.shape and profile.dtype == np.uint32
    assert got.counts == want_counts, (what, got.counts, want_counts)
    assert np.array_equal(profile, want_profile), what
    assert np.array_equal(mask, want_mask), what
    assert got.stats["scratch_bytes"] > 0
    return mask


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
    got = res.support_solid_grid(origin, step, shape, level, up=up, r2=1)
    print("%s level %g up %s: %s %s" % (name, level, up, got.counts, got.stats))
    same(got, SR.layerwise(scene_inside(name, level), up, 1), "%s level %g up %s" % (name, level, up))
    mass = res.mass_moments(origin, step, shape, level)
    assert {k: got.stats[k] for k in BRICK_STATS} == {k: mass.stats[k] for k in BRICK_STATS}
    assert got.counts["points"] == int(mass.moments[0]) > 0
    assert got.volume() == got.support_points * float(np.prod(np.asarray(step, dtype=np.float64)))


# ---- random occupancies at the shapes where a kernel can go wrong -----------------------------------------------------------------
WORD_SHAPES = [tuple(n if a == ax else small[a] for a in range(3)) for n in (63, 64, 65, 129) for ax, small in
               ((0, (0, 5, 4)), (1, (6, 0, 3)), (2, (3, 4, 0)))]                  # (nx, ny, nz): the word boundary along each axis
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
            got = res.support_occupancy(occupancy_arg(occ, device), up=up, r2=r2, plate=plate)
            same(got, SR.layerwise(occ, up, r2, plate), what)
            assert {k: got.stats[k] for k in BRICK_STATS} == dict.fromkeys(BRICK_STATS, 0)
            if small and r2 in (1, 5):
                mask, counts, profile = SR.per_point(occ, up, r2, plate)        # the yardstick's other form, on this very input
                assert np.array_equal(got.mask(), mask) and got.counts == counts and np.array_equal(got.profile(), profile), what


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("device", [False, True])
def test_every_plate_and_density_with_every_direction(res, density, device):
    occ = np.random.default_rng(int(density * 100)).random((17, 20, 33)) < density
    for up in SR.UPS:
        for plate in (None, 0, middle((33, 20, 17), up)):
            for r2 in (1, 4):
                got = res.support_occupancy(occupancy_arg(occ, device), up=up, r2=r2, plate=plate)
                same(got, SR.layerwise(occ, up, r2, plate), "33x20x17 at %g up %s plate %s r2 %d" % (density, up, plate, r2))


@pytest.mark.parametrize("up", SR.UPS)
def test_all_outside_and_all_inside(res, up):
    shape = (17, 20, 33)
    n_a = (33, 20, 17)[SR.up_index(up) >> 1]
    got = res.support_occupancy(np.zeros(shape, dtype=np.uint8), up=up, r2=2)
    same(got, SR.layerwise(np.zeros(shape, dtype=np.uint8), up, 2), "all outside")
    assert got.counts == dict.fromkeys(SR.COUNT_NAMES, 0) and not got.mask().any() and not got.profile().any()
    full = np.ones(shape, dtype=np.uint8)
    got = res.support_occupancy(full, up=up, r2=0, plate=3)
    same(got, SR.layerwise(full, up, 0, 3), "all inside")
    layer = 17 * 20 * 33 // n_a
    assert got.counts == {"points": 17 * 20 * 33, "plate": 3, "base": layer, "overhang": 0, "support_on_plate": 0, "support_on_part": 0,
                          "runs": 0, "landings": 0}
    assert np.all(got.mask() == 1) and np.all(got.profile() == [layer, 0, 0, 0])


# ---- known geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", sorted(SR.TABLE_OVERHANG))
def test_table(res, r2):
    """A leg under a top that juts out on all sides: the top's lower layer overhangs but for the disc around the leg, and every
    support column stands on the plate, six points high."""
    occ = SR.table()
    got = res.support_occupancy(occ, up="+z", r2=r2)
    same(got, SR.layerwise(occ, "+z", r2), "table r2 %d" % r2)
    n = SR.TABLE_OVERHANG[r2]
    assert got.counts == {"points": 184, "plate": 0, "base": 4, "overhang": n, "support_on_plate": 6 * n, "support_on_part": 0, "runs": n,
                          "landings": 0}
    down = res.support_occupancy(occ, up="-z", r2=r2)
    assert down.counts == {"points": 184, "plate": 1, "base": 80, "overhang": 0, "support_on_plate": 0, "support_on_part": 0, "runs": 0,
                           "landings": 0}
    assert np.array_equal(down.mask(), occ)


def test_shelf_supports_land_on_the_part(res):
    """tests/support_ref.py shelf(): 9 x 7 shelf points less the 4 over the post overhang at r2 = 0; their columns stand on the base
    slab, five points each."""
    occ = SR.shelf()
    got = res.support_occupancy(occ, up="+z", r2=0)
    same(got, SR.layerwise(occ, "+z", 0), "shelf")
    n = 9 * 7 - 4
    assert got.counts == {"points": 16 * 12 * 2 + 4 * 5 + 63, "plate": 1, "base": 16 * 12, "overhang": n, "support_on_plate": 0,
                          "support_on_part": 5 * n, "runs": n, "landings": n}
    assert got.contact_area() == 2.0 * n and got.volume() == 5.0 * n


def test_sphere(res):
    """A sphere of radius 1.5 on 24^3 points over [-2, 2]^3, up +z: the lowest layer that holds a point is 3, and the cap below
    the equator overhangs less the wider the disc."""
    cc, w = program(csg.Sphere((0.0, 0.0, 0.0), 1.5))
    use(res, cc, w)
    origin, step, shape = box_lattice(24, -2.0, 2.0)
    inside = M.lattice_inside(cc, w, origin, step, shape, 0.0, LIM[1])
    for r2, n in ((0, 228), (1, 72), (2, 44), (9, 8)):
        got = res.support_solid_grid(origin, step, shape, 0.0, up="+z", r2=r2)
        same(got, SR.layerwise(inside, "+z", r2), "sphere r2 %d" % r2)
        assert got.counts["plate"] == 3 and got.counts["overhang"] == n, (r2, got.counts)
        assert got.counts["support_on_part"] == 0 and got.counts["landings"] == 0 and got.counts["runs"] == n


def test_overhang_regions_through_the_labelling(res):
    """(mask == 2) as a device tensor is an occupancy for rm_label_occupancy: the overhang regions as bodies."""
    import torch
    occ = np.zeros((12, 20, 20), dtype=np.uint8)
    occ[0:8, 9:11, 9:11] = 1                                                   # a post ...
    occ[8:10, 2:18, 2:18] = 1                                                  # ... under a plate: one ring of overhang
    occ[4, 2:5, 2:5] = 1                                                       # and two floating chips
    occ[5, 14:17, 15:18] = 1
    got = res.support_occupancy(occ, up="+z", r2=1)
    mask = same(got, SR.layerwise(occ, "+z", 1), "regions")
    dev = torch.zeros(occ.shape, dtype=torch.uint8, device="cuda:0")
    res.read_support_device(mask_ptr=dev.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    topo = res.label_occupancy((dev == 2).to(torch.uint8))
    want = TR.topology(mask == 2)["counts"]
    print("overhang regions %d, points %d" % (topo.bodies, topo.counts["points"]))
    assert topo.bodies == want["bodies"] == 3 and topo.counts["points"] == want["points"] == got.counts["overhang"]
    supports = res.label_occupancy((dev >= 3).to(torch.uint8))
    assert supports.bodies == TR.topology(mask >= 3)["counts"]["bodies"] and supports.counts["points"] == got.support_points
    assert np.array_equal(got.mask(), mask)                                    # the mask outlives the labelling


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_words(res):
    cc, w = scene_program("g32")
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    for up in ("+y", "-x"):
        a = res.support_solid_grid(origin, step, shape, up=up, r2=2)
        ma, pa = a.mask(), a.profile()
        b = res.support_solid_grid(origin, step, shape, up=up, r2=2)
        assert a.counts == b.counts and a.stats == b.stats
        assert ma.tobytes() == b.mask().tobytes() and pa.tobytes() == b.profile().tobytes()


def test_device_and_host_read_outs_agree(res):
    import torch
    occ = np.random.default_rng(3).random((17, 20, 33)) < 0.4
    got = res.support_occupancy(occ, up="-y", r2=2)
    mask, profile = got.mask(), got.profile()
    assert profile.shape == (20, 4)
    stream = torch.cuda.current_stream().cuda_stream
    for want_mask, want_profile in ((True, False), (False, True), (True, True)):
        m = torch.full(occ.shape, 0x5A, dtype=torch.uint8, device="cuda:0")
        p = torch.full((20, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        res.read_support_device(m.data_ptr() if want_mask else 0, p.data_ptr() if want_profile else 0, stream=stream)
        torch.cuda.synchronize()
        assert m.cpu().numpy().tobytes() == (mask.tobytes() if want_mask else np.full(occ.shape, 0x5A, np.uint8).tobytes())
        assert p.cpu().numpy().view(np.uint32).tobytes() == (profile.tobytes() if want_profile else np.full((20, 4), 0x5A5A5A5A, np.uint32).tobytes())
    t = torch.zeros(128, dtype=torch.int32, device="cuda:0")
    assert res._L.rm_read_support(res._h, None, C.c_void_p(t.data_ptr() + 2), 1, None) == _ffi.RM_ERR_ARG      # misaligned


def lattice(o=(-2.0, -2.0, -2.0), s=(0.25, 0.25, 0.25)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


SENTINEL = 0x5A5A5A5A5A5A5A5A
AUTO = _ffi.RM_SUPPORT_PLATE_AUTO


def test_errors_leave_the_outputs_untouched():
    L = _ffi.hip_lib()
    r = renderer.RayMarchingResources(0)                                      # a context of its own: no support call yet
    try:
        r.resize_command_buffer(65536)
        cc, w = scene_program("g8")
        use(r, cc, w)
        NC, NS = _ffi.RM_SUP_COUNTS, _ffi.RM_SUP_STATS
        counts, stats = (C.c_uint64 * NC)(*[SENTINEL] * NC), (C.c_uint64 * NS)(*[SENTINEL] * NS)
        untouched = lambda: all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in stats)   # noqa: E731
        buf = np.full(17 ** 3, 0x5A, dtype=np.uint8)
        prof = np.full(17 * 4, 0x5A5A5A5A, dtype=np.uint32)
        read = lambda h=r._h, m=buf.ctypes.data, p=prof.ctypes.data: L.rm_read_support(h, m, p, 0, None)   # noqa: E731
        assert read() == _ffi.RM_ERR_ARG and read(h=None) == _ffi.RM_ERR_NULL                  # before any support call
        o, s = lattice()
        solid = lambda h=r._h, o=o, s=s, n=(17, 17, 17), level=0.0, up=4, r2=1, plate=AUTO, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_support_solid(h, o, s, n[0], n[1], n[2], level, up, r2, plate, counts, nc, stats, ns)   # noqa: E731
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
            L.rm_support_occupancy(h, n[0], n[1], n[2], p, 0, None, up, r2, plate, counts, nc, stats, ns)   # noqa: E731
        assert occupancy(h=None) == _ffi.RM_ERR_NULL and occupancy(p=None) == _ffi.RM_ERR_NULL
        assert occupancy(counts=None) == _ffi.RM_ERR_NULL and occupancy(stats=None) == _ffi.RM_ERR_NULL
        assert occupancy(nc=NC - 1) == _ffi.RM_ERR_ARG and occupancy(ns=NS - 1) == _ffi.RM_ERR_ARG
        assert occupancy(up=6) == _ffi.RM_ERR_ARG and occupancy(r2=256) == _ffi.RM_ERR_RANGE and occupancy(plate=4) == _ffi.RM_ERR_RANGE
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2)):
            assert occupancy(n=n) == _ffi.RM_ERR_RANGE, n
        # an invalid program: the status a query gives
        r.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
        assert solid() == _ffi.RM_ERR_STACK_UNDERFLOW
        assert untouched() and np.all(buf == 0x5A) and np.all(prof == 0x5A5A5A5A)
        assert read() == _ffi.RM_ERR_ARG                                                        # still no support call
        for bad in ({"up": "+w"}, {"up": 6}, {"r2": -1}, {"plate": -1}):
            with pytest.raises(ValueError):
                r.support_occupancy(occ, **bad)
        with pytest.raises(ValueError):
            r.support_solid_grid((0, 0, 0), (0.1, 0.1, 0.1), (1, 4, 4))
        with pytest.raises(ValueError):
            r.support_occupancy(np.zeros((4, 4, 4), dtype=np.float32))
        use(r, cc, w)
        assert solid(plate=16) == _ffi.RM_OK and all(x != SENTINEL for x in stats) and counts[_ffi.RM_SUP_PLATE] == 16
        assert read() == _ffi.RM_OK and set(np.unique(buf)) <= {0, 1} and prof[3 * 4] == np.count_nonzero(buf.reshape(17, 17, 17)[3])
        assert occupancy(plate=3) == _ffi.RM_OK and counts[_ffi.RM_SUP_POINTS] == 64 and counts[_ffi.RM_SUP_BASE] == 16
        assert read(p=None) == _ffi.RM_OK and np.all(buf[:64] == 1)
    finally:
        r.close()


def test_draws_meshes_slices_labels_and_distances_are_left_alone(res, oracle):
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
    assert len(mesh.triangles) > 0 and len(slices.points) > 0 and topo.bodies == 3
    infos = sorted(k for k in dir(_ffi) if k.startswith("RM_INFO_") and isinstance(getattr(_ffi, k), int))
    before = {k: res.info(getattr(_ffi, k)) for k in infos}
    for up in ("+z", "-x"):
        got = res.support_solid_grid(origin, step, shape, up=up, r2=1)
        assert got.counts["points"] == topo.counts["points"]
    assert res.support_occupancy(np.ones((9, 9, 9), dtype=bool), up="+y").counts["base"] == 81
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


# ---- above 2^24 points ------------------------------------------------------------------------------------------------------------
BIG = (264, 256, 256)                                                        # nx, ny, nz


def test_above_2_to_the_24_points(res):
    """A buried stack of eleven plates [40, 200) x [40, 200), two points thick, at k = 150 + 10 t -- the last one lies past linear
    index 2^24.  Up +z, automatic plate (150): the lower layer of every plate but the first overhangs at every r2 (the layer below is
    empty), and its supports stand on the plate below, eight points high.  Plate 0: the first plate overhangs too, 150 points above
    the plate.  Up -x: the plates stand on their edges, and nothing overhangs."""
    nx, ny, nz = BIG
    assert nx * ny * nz > 2 ** 24 and 250 * ny * nx > 2 ** 24
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    for t in range(11):
        occ[150 + 10 * t:152 + 10 * t, 40:200, 40:200] = 1
    A = 160 * 160
    want = occ.copy()
    for t in range(1, 11):
        want[150 + 10 * t, 40:200, 40:200] = 2
        want[142 + 10 * t:150 + 10 * t, 40:200, 40:200] = 4
    got = res.support_occupancy(occ, up="+z", r2=5)
    print(got.counts, got.stats)
    assert got.counts == {"points": 22 * A, "plate": 150, "base": A, "overhang": 10 * A, "support_on_plate": 0, "support_on_part": 80 * A,
                          "runs": 10 * A, "landings": 10 * A}
    assert np.array_equal(got.mask(), want)
    profile = got.profile()
    assert profile.shape == (256, 4) and np.array_equal(profile[:, 0], occ.reshape(nz, -1).sum(axis=1))
    assert np.array_equal(profile[:, 1], (want == 2).reshape(nz, -1).sum(axis=1)) and not profile[:, 2].any()
    assert np.array_equal(profile[:, 3], (want == 4).reshape(nz, -1).sum(axis=1))
    want[150, 40:200, 40:200] = 2
    want[0:150, 40:200, 40:200] = 3
    got = res.support_occupancy(occ, up="+z", r2=0, plate=0)
    assert got.counts == {"points": 22 * A, "plate": 0, "base": 0, "overhang": 11 * A, "support_on_plate": 150 * A, "support_on_part": 80 * A,
                          "runs": 11 * A, "landings": 10 * A}
    assert np.array_equal(got.mask(), want)
    got = res.support_occupancy(occ, up="-x", r2=0)
    assert got.counts == {"points": 22 * A, "plate": 263 - 199, "base": 22 * 160, "overhang": 0, "support_on_plate": 0, "support_on_part": 0,
                          "runs": 0, "landings": 0}
    assert np.array_equal(got.mask(), occ)
    # ... and up +x from plate 0 their lower edges (i = 40) overhang, 40 points above the plate
    got = res.support_occupancy(occ, up="+x", r2=1, plate=0)
    assert got.counts["plate"] == 0 and got.counts["base"] == 0 and got.counts["overhang"] == 22 * 160
    assert got.counts["support_on_plate"] == 22 * 160 * 40 and got.counts["support_on_part"] == 0 and got.counts["landings"] == 0
