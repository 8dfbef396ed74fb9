"""The distance transform on the GPU (rm_distance_solid, rm_distance_occupancy, rm_distance_features, rm_read_distance; DESIGN.md
section 20): the whole distance volume, the five counts, the feature mask and its four counts against the numpy restatement
(tests/distance_ref.py) with ==; the brick statistics against rm_mass_moments on the same lattice; shapes at which a kernel can
go wrong, up to rows and columns of 1024 points; known geometry; one lattice above 2^24 points with closed-form answers; errors
and isolation."""
import ctypes as C
import functools

import numpy as np
import pytest

import distance_ref as DR
import mass_ref as M
import scenes
import topology_ref as TR
from test_gpu_topology import box_lattice, hollow_sphere, program, scene_program, use
from ray_marching_amd import _ffi, csg, renderer

pytestmark = pytest.mark.gpu

F = np.float32
LIM = (0.01, 100.0, 256)
BRICK_STATS = ("bricks", "bricks_kept", "bricks_inside", "evaluations")
BIT, NONE = DR.INSIDE_BIT, DR.NONE


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def same(got, want, what=""):
    """The distance volume and the five counts == the restatement's."""
    print("%s: counts %s; stats %s" % (what, got.counts, got.stats))
    vol = got.d2()
    assert vol.dtype == np.uint32 and vol.shape == want.shape
    assert np.array_equal(vol, want), what
    assert got.counts == DR.counts(want), what
    assert got.stats["scratch_bytes"] > 0
    return vol


def check_solid(res, cc, w, origin, step, shape, level=0.0, max_dist=LIM[1], what=""):
    """distance_solid_grid == the restatement; its brick statistics and inside points == rm_mass_moments'."""
    got = res.distance_solid_grid(origin, step, shape, level)
    same(got, DR.solid(cc, w, origin, step, shape, level, max_dist), "%s %s level %g" % (what, shape, level))
    mass = res.mass_moments(origin, step, shape, level)
    assert {k: got.stats[k] for k in BRICK_STATS} == {k: mass.stats[k] for k in BRICK_STATS}, what
    assert got.counts["points"] == int(mass.moments[0])
    return got


def check_features(dist, occ, r2_wall, r2_gap, what=""):
    feats = dist.features(r2_wall, r2_gap)
    want_mask, want_counts = DR.features(occ, r2_wall, r2_gap)
    print("%s r2 %s %s: %s" % (what, r2_wall, r2_gap, feats.counts))
    mask = feats.mask()
    assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask), (what, r2_wall, r2_gap)
    assert feats.counts == want_counts, (what, r2_wall, r2_gap)
    return mask


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.0, 0.1])
@pytest.mark.parametrize("name", ["g1", "g8", "g32", "g32_balanced", "ext_mix", "xform_mix"])
def test_named_scenes(res, name, level):
    cc, w = scene_program(name)
    use(res, cc, w)
    got = check_solid(res, cc, w, *box_lattice(40), level=level, what=name)
    assert got.counts["points"] > 0 and got.counts["max_inside"] >= 1


# ---- shapes where a kernel can go wrong -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 2), (9, 17, 10), (33, 20, 17)])
def test_partial_bricks_and_tiny_lattices(res, shape):
    cc, w = scene_program("g8")
    use(res, cc, w)
    check_solid(res, cc, w, *box_lattice(shape, -1.5, 1.5), what="g8")
    cc, w = hollow_sphere()
    use(res, cc, w)
    check_solid(res, cc, w, *box_lattice(shape, -1.9, 1.9), what="hollow sphere")


@pytest.mark.parametrize("shape", [(65, 3, 2), (3, 65, 2), (2, 3, 65)])
def test_rows_and_columns_past_a_wave(res, shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(nx + 2 * ny)
    for density in (0.1, 0.5, 0.97):
        occ = rng.random((nz, ny, nx)) < density
        dist = res.distance_occupancy(occ)
        same(dist, DR.separable(occ), "%s at %g" % (shape, density))
        check_features(dist, occ, 4, 4, "%s at %g" % (shape, density))


@pytest.mark.parametrize("shape", [(1024, 3, 2), (2, 1024, 3), (3, 2, 1024)])
def test_the_longest_axis(res, shape):
    """Rows and columns of 1024 points.  All inside: only the layer bounds the distance, and every window is as long as the axis
    allows.  Then one outside point at index 700 of the long axis."""
    nx, ny, nz = shape
    full = np.ones((nz, ny, nx), dtype=np.uint8)
    want = (DR.layer_bound(full.shape).astype(np.uint32) | np.uint32(BIT))            # the closed form
    got = res.distance_occupancy(full)
    same(got, want, "%s full" % (shape,))
    assert got.counts["max_inside"] == int((want & NONE).max()) and got.counts["max_outside"] == 0
    assert got.counts["argmax_outside"] == DR.NO_INDEX
    hole = [0, 1, 0]
    hole[(nz, ny, nx).index(1024)] = 700
    occ = full.copy()
    occ[tuple(hole)] = 0
    want = DR.separable(occ)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    closed = np.minimum(DR.layer_bound(occ.shape), (k - hole[0]) ** 2 + (j - hole[1]) ** 2 + (i - hole[2]) ** 2)
    assert np.array_equal((want & NONE)[occ != 0], closed[occ != 0]) and want[tuple(hole)] == 1
    dist = res.distance_occupancy(occ)
    same(dist, want, "%s with a hole" % (shape,))
    check_features(dist, occ, 1, 1, "%s with a hole" % (shape,))


# ---- random occupancies ---------------------------------------------------------------------------------------------------------
DENSITIES = (0.02, 0.3, 0.5, 0.98)
R2S = (0, 1, 2, 4, 9)


@functools.lru_cache(maxsize=None)
def random_occupancies(seed):
    rng = np.random.default_rng(seed)
    return {d: rng.random((17, 20, 33)) < d for d in DENSITIES}


@functools.lru_cache(maxsize=None)
def random_reference(seed, density):
    return DR.separable(random_occupancies(seed)[density])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("seed,density", [(s, d) for s in (5, 6) for d in DENSITIES])
def test_random_occupancies(res, seed, density, device):
    occ = random_occupancies(seed)[density]
    if device:
        import torch
        arg = torch.from_numpy(occ.astype(np.uint8) * 255).to("cuda:0")       # any nonzero byte is inside
    else:
        arg = occ
    got = res.distance_occupancy(arg)
    same(got, random_reference(seed, density), "random %g seed %d %s" % (density, seed, "device" if device else "host"))
    assert {k: got.stats[k] for k in BRICK_STATS} == dict.fromkeys(BRICK_STATS, 0)
    if seed == 5 and not device:
        assert np.array_equal(random_reference(seed, density), DR.brute(occ))  # the yardstick's two forms, on this very input


def test_all_outside_and_all_inside(res):
    shape = (17, 20, 33)
    got = res.distance_occupancy(np.zeros(shape, dtype=np.uint8))
    vol = same(got, np.full(shape, NONE, dtype=np.uint32), "all outside")
    assert vol.min() == NONE
    assert got.counts == {"points": 0, "max_inside": 0, "argmax_inside": DR.NO_INDEX, "max_outside": NONE, "argmax_outside": 0}
    feats = got.features(4, 4)
    assert feats.counts == {"core": 0, "thin": 0, "gap_core": 17 * 20 * 33, "narrow": 0} and not feats.mask().any()
    got = res.distance_occupancy(np.ones(shape, dtype=np.uint8))
    same(got, DR.layer_bound(shape).astype(np.uint32) | np.uint32(BIT), "all inside")
    assert got.counts["points"] == 17 * 20 * 33 and got.counts["max_inside"] == 9 ** 2
    assert (got.counts["max_outside"], got.counts["argmax_outside"]) == (0, DR.NO_INDEX)
    assert got.counts["argmax_inside"] == 8 + 33 * (8 + 20 * 8)


# ---- known geometry -------------------------------------------------------------------------------------------------------------
def test_inscribed_ball_of_a_sphere(res):
    """A sphere of radius 1.5 on 48^3 points: the nearest outside lattice point to the lattice point nearest the centre lies
    between 1.5 - sqrt(3) step / 2 ... and 1.5 + sqrt(3) step away (a cell's diagonal on either end), and no inside point is
    farther from the outside than the radius: sqrt(MAX_INSIDE) step is within sqrt(3) step of 1.5, the centre of the ball within
    one point of the sphere's."""
    cc, w = program(csg.Sphere((0.0, 0.0, 0.0), 1.5))
    use(res, cc, w)
    origin, step, shape = box_lattice(48)
    got = check_solid(res, cc, w, origin, step, shape, what="sphere")
    radius, centre = got.inscribed_radius()
    print("sphere: radius %.6f at %s, step %.6f" % (radius, centre, float(step[0])))
    assert abs(radius - 1.5) <= np.sqrt(3.0) * float(step[0])
    assert radius == float(step[0]) * np.sqrt(got.counts["max_inside"])
    assert all(abs(c - 23.5) <= 1.0 for c in centre)
    with pytest.raises(ValueError):
        got.inscribed_radius(step=(0.1, 0.1, 0.2))


def test_hollow_sphere_is_thickest_in_its_shell(res):
    cc, w = hollow_sphere()                                                    # radius 1.8, a hole of radius 1 around (0.1, 0, 0)
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    got = check_solid(res, cc, w, origin, step, shape, what="hollow sphere")
    vol = got.d2()
    _, (i, j, k) = got.inscribed_radius()
    assert vol[k, j, i] == (BIT | got.counts["max_inside"])
    p = np.array([origin[a] + F(c) * step[a] for a, c in enumerate((i, j, k))], dtype=np.float64)
    assert np.linalg.norm(p - (0.1, 0.0, 0.0)) > 1.0 and np.linalg.norm(p) < 1.8     # on the shell
    assert not vol[20, 20, 20] & BIT and (i, j, k) != (20, 20, 20)                      # the centre lies in the cavity


# ---- features ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,density", [(s, d) for s in (5, 6) for d in DENSITIES])
def test_features_of_random_occupancies(res, seed, density):
    occ = random_occupancies(seed)[density]
    dist = res.distance_occupancy(occ)
    for r2 in R2S:
        check_features(dist, occ, r2, r2, "random %g seed %d" % (density, seed))
    mask = check_features(dist, occ, 2, 9, "random")
    # a skipped half leaves its classes at 0 or 1, and the other half is what it was
    wall = check_features(dist, occ, 2, None, "random")
    gap = check_features(dist, occ, None, 9, "random")
    assert not (wall == 3).any() and not (gap == 2).any()
    assert np.array_equal(wall == 2, mask == 2) and np.array_equal(gap == 3, mask == 3)
    assert np.array_equal(check_features(dist, occ, None, None, "random"), occ.astype(np.uint8))


def fin_block():
    """40 x 24 x 24 points: a block [4, 20)^3 with a fin two points thick, [20, 36) x [11, 13) x [4, 20)."""
    occ = np.zeros((24, 24, 40), dtype=np.uint8)
    occ[4:20, 4:20, 4:20] = 1
    occ[4:20, 11:13, 20:36] = 1
    return occ


def test_a_fin_two_points_thick_is_thin(res):
    occ = fin_block()
    dist = res.distance_occupancy(occ)
    same(dist, DR.separable(occ), "fin")
    mask = check_features(dist, occ, 1, None, "fin")
    assert np.all(mask[4:20, 11:13, 21:36] == 2)          # the fin's points further than one from the block
    assert np.all(mask[5:19, 11:13, 20] == 1)             # ... and those a ball in the block reaches
    assert mask[12, 12, 12] == 1 and np.all(mask[6:18, 6:18, 6:18] == 1)
    feats = dist.features(0, None)
    assert feats.counts["thin"] == 0 and feats.counts["core"] == int(occ.sum()) and np.array_equal(feats.mask(), occ)
    # the thin points as an occupancy on the device: their regions are bodies
    import torch
    dev = torch.zeros(occ.shape, dtype=torch.uint8, device="cuda:0")
    dist.features(1, None)
    res.read_distance_device(mask_ptr=dev.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    thin = (dev == 2).to(torch.uint8)
    topo = res.label_occupancy(thin)
    want = TR.topology(mask == 2)["counts"]
    print("fin: thin regions %d, points %d" % (topo.bodies, topo.counts["points"]))
    assert topo.bodies == want["bodies"] and topo.counts["points"] == want["points"] == int((mask == 2).sum())
    assert topo.bodies >= 1
    # the distance volume and the mask outlive the labelling
    assert np.array_equal(dist.d2(), DR.separable(occ))


def test_a_slot_three_points_wide_is_narrow(res):
    """A box [4, 36) x [4, 20) x [4, 20) with a slot [18, 21) x all j x [10, 20), open at the top."""
    occ = np.zeros((24, 24, 40), dtype=np.uint8)
    occ[4:20, 4:20, 4:36] = 1
    occ[10:20, 4:20, 18:21] = 0
    dist = res.distance_occupancy(occ)
    same(dist, DR.separable(occ), "slot")
    mask = check_features(dist, occ, None, 4, "slot")
    assert np.all(mask[10:17, 12, 18:21] == 3)            # the slot's interior: no ball of radius 2 fits between the walls
    assert np.all(mask[21:, 12, :] == 0)                   # free space above the box
    mask = check_features(dist, occ, None, 1, "slot")
    assert np.all(mask[12:20, 12, 18:21] == 0)            # a ball of radius 1 does
    assert np.all(mask[occ != 0] == 1)


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_words(res):
    cc, w = scene_program("g32")
    use(res, cc, w)
    origin, step, shape = box_lattice(40)
    a = res.distance_solid_grid(origin, step, shape)
    va, fa = a.d2(), a.features(4, 4)
    ma = fa.mask()
    b = res.distance_solid_grid(origin, step, shape)
    fb = b.features(4, 4)
    assert a.counts == b.counts and a.stats == b.stats and fa.counts == fb.counts
    assert va.tobytes() == b.d2().tobytes() and ma.tobytes() == fb.mask().tobytes()


def test_device_and_host_read_outs_agree(res):
    import torch
    occ = random_occupancies(5)[0.5]
    dist = res.distance_occupancy(occ)
    feats = dist.features(2, 2)
    vol, mask = dist.d2(), feats.mask()
    stream = torch.cuda.current_stream().cuda_stream
    for want_d2, want_mask in ((True, False), (False, True), (True, True)):
        d = torch.full(occ.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        m = torch.full(occ.shape, 0x5A, dtype=torch.uint8, device="cuda:0")
        res.read_distance_device(d.data_ptr() if want_d2 else 0, m.data_ptr() if want_mask else 0, stream=stream)
        torch.cuda.synchronize()
        assert d.cpu().numpy().view(np.uint32).tobytes() == (vol.tobytes() if want_d2 else np.full(occ.shape, 0x5A5A5A5A, np.uint32).tobytes())
        assert m.cpu().numpy().tobytes() == (mask.tobytes() if want_mask else np.full(occ.shape, 0x5A, np.uint8).tobytes())
    t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    assert res._L.rm_read_distance(res._h, C.c_void_p(t.data_ptr() + 2), None, 1, None) == _ffi.RM_ERR_ARG      # misaligned


def lattice(o=(-2.0, -2.0, -2.0), s=(0.25, 0.25, 0.25)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


SENTINEL = 0x5A5A5A5A5A5A5A5A


def test_errors_leave_the_outputs_untouched():
    L = _ffi.hip_lib()
    r = renderer.RayMarchingResources(0)                                      # a context of its own: no distance volume yet
    try:
        r.resize_command_buffer(65536)
        cc, w = scene_program("g8")
        use(r, cc, w)
        NC, NS, NF = _ffi.RM_DIST_COUNTS, _ffi.RM_DIST_STATS, _ffi.RM_DIST_FEATURE_COUNTS
        counts, stats = (C.c_uint64 * NC)(*[SENTINEL] * NC), (C.c_uint64 * NS)(*[SENTINEL] * NS)
        fcounts = (C.c_uint64 * NF)(*[SENTINEL] * NF)
        untouched = lambda: all(x == SENTINEL for x in counts) and all(x == SENTINEL for x in stats) and \
            all(x == SENTINEL for x in fcounts)   # noqa: E731
        buf = np.full(17 ** 3, 0x5A5A5A5A, dtype=np.uint32)
        read = lambda h=r._h, d=buf.ctypes.data, m=None: L.rm_read_distance(h, d, m, 0, None)   # noqa: E731
        features = lambda h=r._h, rw=1, rg=1, c=fcounts, n=NF: L.rm_distance_features(h, rw, rg, c, n)   # noqa: E731
        assert read() == _ffi.RM_ERR_ARG and read(h=None) == _ffi.RM_ERR_NULL                  # before any distance call
        assert features() == _ffi.RM_ERR_ARG and features(h=None) == _ffi.RM_ERR_NULL
        o, s = lattice()
        solid = lambda h=r._h, o=o, s=s, n=(17, 17, 17), level=0.0, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_distance_solid(h, o, s, n[0], n[1], n[2], level, counts, nc, stats, ns)   # noqa: E731
        assert solid(h=None) == _ffi.RM_ERR_NULL
        assert solid(counts=None) == _ffi.RM_ERR_NULL and solid(stats=None) == _ffi.RM_ERR_NULL
        assert solid(o=None) == _ffi.RM_ERR_NULL and solid(s=None) == _ffi.RM_ERR_NULL
        assert solid(nc=NC - 1) == _ffi.RM_ERR_ARG and solid(ns=NS - 1) == _ffi.RM_ERR_ARG
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2), (2, 65536, 2), (1024, 1024, 512)):
            assert solid(n=n) == _ffi.RM_ERR_RANGE, n
        for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
            assert solid(s=lattice(s=bad)[1]) == _ffi.RM_ERR_ARG, bad
        assert solid(o=lattice(o=(0.0, np.inf, 0.0))[0]) == _ffi.RM_ERR_ARG
        for level in (np.nan, np.inf):
            assert solid(level=level) == _ffi.RM_ERR_ARG
        occ = np.ones((4, 4, 4), dtype=np.uint8)
        occupancy = lambda h=r._h, n=(4, 4, 4), p=occ.ctypes.data, counts=counts, nc=NC, stats=stats, ns=NS: \
            L.rm_distance_occupancy(h, n[0], n[1], n[2], p, 0, None, counts, nc, stats, ns)   # noqa: E731
        assert occupancy(h=None) == _ffi.RM_ERR_NULL and occupancy(p=None) == _ffi.RM_ERR_NULL
        assert occupancy(counts=None) == _ffi.RM_ERR_NULL and occupancy(stats=None) == _ffi.RM_ERR_NULL
        assert occupancy(nc=NC - 1) == _ffi.RM_ERR_ARG and occupancy(ns=NS - 1) == _ffi.RM_ERR_ARG
        for n in ((1, 4, 4), (4, 4, 1), (1025, 2, 2)):
            assert occupancy(n=n) == _ffi.RM_ERR_RANGE, n
        # an invalid program: the status a query gives
        r.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
        assert solid() == _ffi.RM_ERR_STACK_UNDERFLOW
        assert untouched() and np.all(buf == 0x5A5A5A5A)
        assert read() == _ffi.RM_ERR_ARG and features() == _ffi.RM_ERR_ARG                      # still no distance volume
        with pytest.raises(ValueError):
            r.distance_solid_grid((0, 0, 0), (0.1, 0.1, 0.1), (1, 4, 4))
        with pytest.raises(ValueError):
            r.distance_occupancy(np.zeros((4, 4, 4), dtype=np.float32))
        use(r, cc, w)
        assert solid() == _ffi.RM_OK and all(x != SENTINEL for x in counts) and all(x != SENTINEL for x in stats)
        # a volume, but no mask yet; the features' own checks
        mask = np.full(17 ** 3, 0x5A, dtype=np.uint8)
        assert read(m=mask.ctypes.data) == _ffi.RM_ERR_ARG and np.all(mask == 0x5A) and np.all(buf == 0x5A5A5A5A)
        assert features(c=None) == _ffi.RM_ERR_NULL and features(n=NF - 1) == _ffi.RM_ERR_ARG
        for bad in (1 << 22, 0xFFFFFFFE, 1 << 31):
            assert features(rw=bad) == _ffi.RM_ERR_RANGE and features(rg=bad) == _ffi.RM_ERR_RANGE
        assert all(x == SENTINEL for x in fcounts)
        assert read(m=mask.ctypes.data) == _ffi.RM_ERR_ARG
        assert features(rw=(1 << 22) - 1, rg=_ffi.RM_DIST_SKIP) == _ffi.RM_OK and fcounts[_ffi.RM_DIST_GAP_CORE] == 0
        assert fcounts[_ffi.RM_DIST_CORE] == 0 and fcounts[_ffi.RM_DIST_THIN] == counts[_ffi.RM_DIST_POINTS]   # no ball that large fits
        assert read(m=mask.ctypes.data) == _ffi.RM_OK and set(np.unique(mask)) <= {0, 2} and not np.all(buf == 0x5A5A5A5A)
        # a new volume has no mask again
        assert occupancy() == _ffi.RM_OK and counts[_ffi.RM_DIST_POINTS] == 64 and counts[_ffi.RM_DIST_MAX_INSIDE] == 4
        assert read(m=mask.ctypes.data) == _ffi.RM_ERR_ARG and read() == _ffi.RM_OK
        assert np.array_equal(buf[:64], (DR.layer_bound((4, 4, 4)).astype(np.uint32) | np.uint32(BIT)).ravel())
        with pytest.raises(ValueError):
            renderer.Distance(r, {}, {}, np.zeros(3, F), np.array([0.1, 0.1, 0.2], F), (4, 4, 4)).features(wall=0.4)
    finally:
        r.close()


def test_draws_meshes_slices_and_labels_are_left_alone(res, oracle):
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
    assert len(mesh.triangles) > 0 and len(slices.points) > 0 and topo.bodies == 3
    infos = sorted(k for k in dir(_ffi) if k.startswith("RM_INFO_") and isinstance(getattr(_ffi, k), int))
    before = {k: res.info(getattr(_ffi, k)) for k in infos}
    got = res.distance_solid_grid(origin, step, shape)
    assert got.counts["points"] == topo.counts["points"]
    assert got.features(4, 4).counts["core"] > 0
    assert res.distance_occupancy(np.ones((9, 9, 9), dtype=bool)).counts["max_inside"] == 25
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


# ---- above 2^24 points ------------------------------------------------------------------------------------------------------------
BIG = (264, 256, 256)                                                        # nx, ny, nz


def test_above_2_to_the_24_points(res):
    """A buried block [40, 200) x [40, 200) x [190, 250) -- its upper planes lie past linear index 2^24 -- and a comb of thirty
    plates two points thick, [4, 200) x [8 t + 2, 8 t + 4) x [10, 100), on a spine [2, 4) x [2, 236) x [10, 100).  Closed forms:
    inside a box the nearest outside point lies straight across the nearest face; between two plates six points apart the
    nearest inside point is the nearer plate's; straight above the block it is the block's top."""
    nx, ny, nz = BIG
    assert nx * ny * nz > 2 ** 24 and 249 * ny * nx > 2 ** 24
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    occ[190:250, 40:200, 40:200] = 1
    occ[10:100, 2:236, 2:4] = 1
    for t in range(30):
        occ[10:100, 8 * t + 2:8 * t + 4, 4:200] = 1
    got = res.distance_occupancy(occ)
    print(got.counts, got.stats)
    vol = got.d2()
    assert np.array_equal((vol & BIT) != 0, occ != 0)
    assert got.counts == DR.counts(vol)                                        # the maxima are the volume's, smallest index first
    j, i = np.meshgrid(np.arange(40, 200), np.arange(40, 200), indexing="ij")
    face = np.minimum(np.minimum(i - 39, 200 - i), np.minimum(j - 39, 200 - j))
    for k in (190, 200, 219, 220, 248, 249):
        want = np.minimum(face, min(k - 189, 250 - k)) ** 2
        assert np.array_equal(vol[k, 40:200, 40:200], want.astype(np.uint32) | np.uint32(BIT)), k
    assert got.counts["max_inside"] == 30 ** 2 and got.counts["argmax_inside"] == 69 + nx * (69 + ny * 219)
    for k, h in ((250, 1), (252, 3), (255, 6)):                                # straight above the block
        assert np.all(vol[k, 40:200, 40:200] == h * h), k
    comb = vol[50]                                                             # a plane through the comb, 40 points from its ends in k
    assert np.all(comb[:, 5:200][occ[50][:, 5:200] != 0] == (BIT | 1))      # the plates
    for t in range(29):                                                        # the gaps, away from the teeth's ends
        for dj, d in enumerate((1, 2, 3, 3, 2, 1)):
            assert np.all(comb[8 * t + 4 + dj, 10:190] == d * d), (t, dj)
    # thin walls: every plate is thinner than a ball of radius 2, the block is not; the gaps are narrower than one of radius 3
    feats = got.features(4, 9)
    mask = feats.mask()
    comb_points = int(occ[10:100].sum())
    assert feats.counts["thin"] >= comb_points and np.all(mask[50][occ[50] != 0] == 2)
    assert np.all(mask[195:245, 45:195, 45:195] == 1)
    assert np.all(mask[50, 12:228, 10:190][occ[50, 12:228, 10:190] == 0] == 3)
    assert feats.counts["thin"] == int((mask == 2).sum()) and feats.counts["narrow"] == int((mask == 3).sum())
