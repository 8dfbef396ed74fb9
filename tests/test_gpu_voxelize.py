"""Mesh voxelisation on the GPU (rm_voxelize_mesh, rm_read_voxels): the occupancy and all six counts == the
numpy restatement (tests/voxel_ref.py) for convex bodies, a box and an octahedron on lattice points (every tie), a torus, an open
mesh, awkward steps and origins, rejected triangles, long rows and word borders, meshes off the lattice, many crossings of one row,
a triangle larger than the lattice, a soup of sub-cell triangles; device inputs, run-to-run and order invariance; the round trip
extract_mesh -> voxelize_mesh; the hand-over of the device occupancy to the analyses; errors and retention."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as DR
import surface_ref as SR
import topology_ref as TR
import voxel_ref as VR
from test_gpu_topology import box_lattice, scene_program, use
from ray_marching_amd import _ffi, mesh, renderer

pytestmark = pytest.mark.gpu

UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
SHAPE = (20, 18, 16)
CENTRE, RADIUS = (9.5, 8.25, 7.75), 6.3
# The scenes whose mesh_ref mesh voxel_ref voxelises on the CPU with no open row and every differing point within the one-point shell
# of the solid's surface, on 40^3 points over [-2.5, 2.5]^3 (21, 18, 11 and 13 differing points): all four of the issue's candidates.
ROUND_TRIP_SCENES = ("g1", "g8", "g32", "ext_mix")


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)      # no program: a voxelisation needs none
    yield r
    r.close()


def check(res, v, t, origin, step, shape, what=""):
    """voxelize_mesh == the restatement: the occupancy and every count."""
    want, counts = VR.voxelize(v, t, origin, step, shape)
    got = res.voxelize_mesh(v, t, origin, step, shape)
    print("%s: counts %s; stats %s" % (what, got.counts, got.stats))
    assert got.counts == counts, what
    occ = got.occupancy()
    assert occ.dtype == np.uint8 and occ.shape == want.shape and np.array_equal(occ, want), what
    assert all(got.stats[k] == 0 for k in ("bricks", "bricks_kept", "bricks_inside", "evaluations")) and got.stats["scratch_bytes"] > 0
    return got


@pytest.mark.parametrize("level, inside", [(0, 646), (1, 914), (2, 1018)])
def test_icospheres(res, level, inside):
    v, t = VR.icosphere(level, RADIUS, CENTRE)
    got = check(res, v, t, *UNIT, SHAPE, "icosphere %d" % level)
    assert got.counts["inside"] == inside and got.counts["open_rows"] == 0 and got.counts["triangles"] == 20 * 4 ** level
    cls = VR.convex_classes(v, t, *UNIT, SHAPE)
    assert (cls == 0).sum() == 0 and (cls == 1).sum() == inside
    assert np.array_equal(got.occupancy(), (cls == 1).astype(np.uint8))


def test_box_on_lattice_points_is_the_half_open_block(res):
    v, t = VR.box((3, 2, 4), (12, 11, 9))
    got = check(res, v, t, *UNIT, SHAPE, "box")
    want = np.zeros(SHAPE[::-1], np.uint8)
    want[4:9, 3:12, 3:12] = 1
    assert np.array_equal(got.occupancy(), want) and got.counts["inside"] == 405 and got.counts["edge_on"] == 8


def test_octahedron_on_lattice_points(res):
    v, t = VR.octahedron()
    got = check(res, v, t, *UNIT, SHAPE, "octahedron")
    cls = VR.convex_classes(v, t, *UNIT, SHAPE)
    assert (cls == 0).sum() == 146 and (cls == 1).sum() == 231 and (cls == 0).sum() <= 0.03 * cls.size
    occ = got.occupancy()
    assert np.array_equal(occ[cls != 0], (cls[cls != 0] == 1).astype(np.uint8)) and got.counts["open_rows"] == 0


def test_torus_keeps_its_hole(res):
    v, t = VR.torus()
    got = check(res, v, t, *UNIT, (24, 24, 12), "torus")
    assert got.counts["open_rows"] == 0 and got.occupancy()[:, 10:14, 10:14].sum() == 0


def test_open_mesh_reports_open_rows(res):
    v, t = VR.icosphere(2, RADIUS, CENTRE)
    got = check(res, v, t[:-7], *UNIT, SHAPE, "open icosphere")
    assert got.counts["open_rows"] == 9


@pytest.mark.parametrize("origin, step", [((-0.73, 0.19, 1.07), (0.1, 1.0 / 3.0, 0.1)), ((1e-3, -7.7, 3.3), (1.0 / 3.0, 0.1, 1.0 / 3.0))])
def test_awkward_steps_and_origins_snap_as_numpy_does(res, origin, step):
    o, s = np.asarray(origin, np.float32), np.asarray(step, np.float32)
    v, t = VR.icosphere(2, RADIUS, CENTRE)
    vw = (o + v * s).astype(np.float32)
    check(res, vw, t, o, s, SHAPE, "icosphere, step %s" % (step,))
    rng = np.random.default_rng(3)                                  # 1500 small triangles: most vertices decide a row or a bit
    base = rng.random((1500, 1, 3)) * (np.array(SHAPE) - 1)
    tri = base + rng.random((1500, 3, 3)) * 2.5
    soup = (o + tri.reshape(-1, 3) * s).astype(np.float32)
    check(res, soup, None, o, s, SHAPE, "soup, step %s" % (step,))


def test_rejected_triangles_leave_the_rest_alone(res):
    v, t = VR.icosphere(1, RADIUS, CENTRE)
    clean = check(res, v, t, *UNIT, SHAPE, "clean")
    n = len(v)
    vv = np.concatenate([v, [[np.nan, 1, 1], [1, 1, 1], [2, 5, 1], [3000, 1, 1]]]).astype(np.float32)
    tt = np.concatenate([t[:40], [[n, n + 1, n + 2], [n + 1, n + 2, n + 3], [0, 1, n + 4]], t[40:]]).astype(np.uint32)
    got = check(res, vv, tt, *UNIT, SHAPE, "three rejected")
    assert got.counts["rejected"] == 3 and got.counts["triangles"] == len(t) + 3
    assert all(got.counts[k] == clean.counts[k] for k in ("edge_on", "crossings", "inside", "open_rows"))
    assert np.array_equal(got.occupancy(), VR.voxelize(v, t, *UNIT, SHAPE)[0])
    big = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)  # every index of a triangle out of range, and 0xFFFFFFFF
    got = check(res, big, np.array([[3, 4, 5], [0, 1, 0xFFFFFFFF]], np.uint32), *UNIT, SHAPE, "indices out of range")
    assert got.counts["rejected"] == 2 and got.counts["inside"] == 0


def test_long_rows_and_word_carries(res):
    v, t = VR.box((100.5, -1.0, -1.0), (900.25, 5.0, 5.0))
    got = check(res, v, t, *UNIT, (1024, 3, 2), "1024 x 3 x 2")
    assert got.counts["inside"] == 800 * 6
    v, t = VR.box((1023.5, -1.0, -1.0), (1030.0, 5.0, 5.0))           # both crossings clamp to bit 1024: the 33rd word
    got = check(res, v, t, *UNIT, (1024, 3, 2), "beyond +x")
    assert got.counts["inside"] == 0 and got.counts["open_rows"] == 0 and got.counts["crossings"] == 12
    v, t = VR.box((0.5, -1.0, 100.3), (1.5, 3.0, 900.7))
    got = check(res, v, t, *UNIT, (3, 2, 1024), "3 x 2 x 1024")
    assert got.counts["inside"] == 800 * 2


@pytest.mark.parametrize("nx", [31, 32, 33, 63, 64, 65])
def test_word_borders(res, nx):
    for lo, hi in ((0.5, nx - 1.5), (0.5, nx - 0.5), (nx - 1.5, nx + 3.0), (-2.0, nx + 3.0)):
        v, t = VR.box((lo, 0.5, 0.5), (hi, 4.5, 3.5))
        got = check(res, v, t, *UNIT, (nx, 6, 5), "nx %d, box %g..%g" % (nx, lo, hi))
        assert got.counts["open_rows"] == 0
        assert got.counts["inside"] == 12 * (min(int(np.floor(hi)), nx - 1) - max(int(np.ceil(lo)), 0) + 1)


@pytest.mark.parametrize("centre", [(100.0, 100.0, 100.0), (-50.0, 8.0, 8.0), (70.0, 8.0, 8.0)])
def test_mesh_off_the_lattice(res, centre):
    v, t = VR.icosphere(1, RADIUS, centre)
    got = check(res, v, t, *UNIT, SHAPE, "off the lattice %s" % (centre,))
    assert got.counts["inside"] == 0 and got.counts["open_rows"] == 0 and not got.occupancy().any()


def test_forty_crossings_of_one_row(res):
    plates = [VR.box((1.0 + 1.5 * k + 0.25, -1.0, -1.0), (1.0 + 1.5 * k + 0.75, 7.0, 7.0)) for k in range(20)]
    v = np.concatenate([p[0] for p in plates])
    t = np.concatenate([p[1] + 8 * k for k, p in enumerate(plates)]).astype(np.uint32)
    got = check(res, v, t, *UNIT, (40, 6, 5), "comb")
    assert got.counts["crossings"] == 40 * 30 and got.counts["open_rows"] == 0


def test_triangle_larger_than_the_lattice(res):
    for tri in ([[5.3, -100, -100], [5.3, 300, -100], [5.3, -100, 300]], [[0, -100, -100], [40, 300, -100], [-20, -100, 300]]):
        got = check(res, np.array(tri, np.float32), None, *UNIT, SHAPE, "large triangle")
        assert got.counts["crossings"] == 18 * 16 and got.counts["open_rows"] == 18 * 16 and got.stats["items"] == 5   # ceil(288 / 64)
    v, t = VR.box((-500.0, -400.0, -300.0), (600.0, 700.0, 800.0))
    got = check(res, v, t, *UNIT, SHAPE, "box round the lattice")
    assert got.counts["inside"] == 20 * 18 * 16 and got.stats["items"] == 4 * 5


def test_soup_of_sub_cell_triangles(res):
    rng = np.random.default_rng(27)
    base = rng.random((2000, 1, 3)) * (np.array(SHAPE) - 1)
    soup = (base + rng.random((2000, 3, 3)) * 0.95).reshape(-1, 3).astype(np.float32)   # boxes of 0, 1, 2 or 4 rows
    got = check(res, soup, None, *UNIT, SHAPE, "sub-cell soup")
    assert got.counts["triangles"] == 2000 and got.counts["crossings"] > 0 and got.stats["items"] == 0   # the setup lanes' own rows


def test_device_inputs_runs_and_orders_give_identical_words(res):
    import torch
    v, t = VR.torus()
    shape = (24, 24, 12)
    host = res.voxelize_mesh(v, t, *UNIT, shape)
    words = host.occupancy().tobytes()
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda()
    dev = res.voxelize_mesh(dv, dt, *UNIT, shape)
    assert dev.counts == host.counts and dev.occupancy().tobytes() == words
    with pytest.raises(ValueError):
        host.occupancy()                                           # replaced by the later call
    soup = res.voxelize_mesh(torch.from_numpy(VR.soup_of(v, t)).cuda(), None, *UNIT, shape)
    assert soup.counts == host.counts and soup.occupancy_device().cpu().numpy().tobytes() == words
    rng = np.random.default_rng(5)
    for k in range(3):
        tt = np.roll(t[rng.permutation(len(t))], k, axis=1)
        again = res.voxelize_mesh(v, tt if k < 2 else tt[:, ::-1].copy(), *UNIT, shape)
        assert again.counts == host.counts and again.occupancy().tobytes() == words
    m = res.voxelize_mesh(mesh.Mesh(v, t), origin=UNIT[0], step=UNIT[1], shape=shape)
    assert m.counts == host.counts and m.occupancy().tobytes() == words


def test_voxelize_mesh_box_leaves_the_margin_empty(res):
    v, t = VR.icosphere(1, 1.7, (0.3, -0.2, 0.1))
    vox = res.voxelize_mesh_box(v, t, 32, margin=3)
    occ = vox.occupancy()
    assert vox.shape[0] <= 32 and max(vox.shape) == 32 and vox.counts["open_rows"] == 0 and vox.counts["inside"] > 3000
    for axis in range(3):
        o = np.moveaxis(occ, axis, 0)
        assert not o[:3].any() and not o[-3:].any() and o[3:-3].any()
    assert np.array_equal(occ, VR.voxelize(v, t, vox.origin, vox.step, vox.shape)[0])


@pytest.mark.parametrize("name", ROUND_TRIP_SCENES)
def test_round_trip_through_the_mesh_exporter(name):
    import torch
    r = renderer.RayMarchingResources(0)
    try:
        r.resize_command_buffer(65536)
        use(r, *scene_program(name))
        origin, step, shape = box_lattice(40)
        m = r.extract_mesh_grid(origin, step, shape, normals=False, ids=False, device=True)
        assert isinstance(m.vertices, torch.Tensor) and 1000 < len(m.triangles) < 6000
        vox = r.voxelize_mesh(m, origin=origin, step=step, shape=shape)
        occ = vox.occupancy()
        solid = (r.sample_grid(origin, step, shape) < np.float32(0.0)).astype(np.uint8)
    finally:
        r.close()
    assert vox.counts["open_rows"] == 0 and vox.counts["rejected"] == 0 and vox.counts["triangles"] == len(m.triangles)
    differs = occ != solid
    near_surface = np.zeros(solid.shape, dtype=bool)               # a 6-neighbour of the other class in the solid's occupancy
    for axis in range(3):
        a, b = np.moveaxis(solid, axis, 0), np.moveaxis(near_surface, axis, 0)
        b[1:] |= a[1:] != a[:-1]
        b[:-1] |= a[:-1] != a[1:]
    print("%s: %d triangles, %d points differ from d < 0, %d inside" % (name, len(m.triangles), differs.sum(), occ.sum()))
    assert not (differs & ~near_surface).any()
    mm = m.numpy()
    want, counts = VR.voxelize(mm.vertices, mm.triangles, origin, step, shape)
    assert np.array_equal(occ, want) and vox.counts == counts


def test_hand_over_of_the_device_occupancy_to_the_analyses(res):
    import torch
    v, t = VR.torus()
    vox = res.voxelize_mesh(v, t, *UNIT, (24, 24, 12))
    occ = vox.occupancy_device()
    assert isinstance(occ, torch.Tensor) and occ.device.type == "cuda" and occ.dtype == torch.uint8 and tuple(occ.shape) == (12, 24, 24)
    host = vox.occupancy()
    topo = res.label_occupancy(occ)
    assert (topo.bodies, topo.cavities, topo.tunnels) == (1, 0, 1) and topo.counts == TR.topology(host != 0)["counts"]
    dist = res.distance_occupancy(occ)
    assert dist.counts == DR.counts(DR.separable(host)) and np.array_equal(dist.d2(), DR.separable(host))
    surf = res.surface_classes(occ)
    assert np.array_equal(np.asarray(surf.counts, dtype=np.uint64), SR.counts(host))
    assert np.array_equal(vox.occupancy(), host)                  # none of them replaced the voxel result


# ---- errors and retention --------------------------------------------------------------------------------------------------------
def raw_call(res, nv, xyz, nt, idx, origin, step, shape, counts, n_counts, stats, n_stats, is_device=0):
    f3 = lambda a: np.asarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None  # noqa: E731
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None  # noqa: E731
    return res._L.rm_voxelize_mesh(res._h, nv, p(xyz), nt, p(idx), is_device, None, f3(origin), f3(step), *shape, u64(counts), n_counts,
                                   u64(stats), n_stats)


def last_error(r):
    return (r._L.rm_last_error(r._h) or b"").decode()


def test_refusals_leave_outputs_and_the_previous_result_alone(res):
    v, t = VR.icosphere(0, RADIUS, CENTRE)
    kept = res.voxelize_mesh(v, t, *UNIT, SHAPE)
    words = kept.occupancy().tobytes()
    counts, stats = np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64)
    nv, nt, o, s = len(v), len(t), UNIT[0], UNIT[1]
    nan, inf = float("nan"), float("inf")
    cases = [
        ((nv, None, nt, t, o, s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_NULL),
        ((nv, v, nt, t, o, s, SHAPE, None, 6, stats, 6), _ffi.RM_ERR_NULL),
        ((nv, v, nt, t, o, s, SHAPE, counts, 6, None, 6), _ffi.RM_ERR_NULL),
        ((nv, v, nt, t, o, s, SHAPE, counts, 5, stats, 5), _ffi.RM_ERR_ARG),                # n_counts before n_stats ...
        ((nv, v, nt, t, o, s, SHAPE, counts, 6, stats, 5), _ffi.RM_ERR_ARG),
        ((nv, v, nt, t, None, s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_NULL),
        ((nv, v, nt, t, (0, nan, 0), s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),
        ((nv, v, nt, t, o, (1, 0, 1), SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),
        ((nv, v, nt, t, o, (1, inf, 1), SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),
        ((nv, v, nt, t, o, (1, -1, 1), (1025, 2, 2), counts, 6, stats, 6), _ffi.RM_ERR_ARG),  # ... the step before the lattice's range
        ((nv, v, nt, t, o, s, (1025, 2, 2), counts, 6, stats, 6), _ffi.RM_ERR_RANGE),
        ((nv, v, nt, t, o, s, (20, 1, 16), counts, 6, stats, 6), _ffi.RM_ERR_RANGE),
        ((nv, v, nt, t, o, s, (1024, 1024, 512), counts, 6, stats, 6), _ffi.RM_ERR_RANGE),
        ((nv, v, 0, t, o, s, (1025, 2, 2), counts, 6, stats, 6), _ffi.RM_ERR_RANGE),        # ... and the range before the mesh
        ((nv, v, 0, t, o, s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),
        ((0, v, nt, t, o, s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),
        ((nv, v, nt, None, o, s, SHAPE, counts, 6, stats, 6), _ffi.RM_ERR_ARG),             # a soup of 12 vertices is not 20 triangles
    ]
    for args, status in cases:
        assert raw_call(res, *args) == status, args
        assert "rm_voxelize_mesh" in last_error(res)
        assert np.all(counts == 0x5A5A5A5A5A5A5A5A) and np.all(stats == 0x5A5A5A5A5A5A5A5A)
        assert kept.occupancy().tobytes() == words
    assert res._L.rm_voxelize_mesh(None, nv, C.c_void_p(v.ctypes.data), nt, C.c_void_p(t.ctypes.data), 0, None, None, None, 20, 18, 16, None, 6, None, 6) == _ffi.RM_ERR_NULL
    import torch
    dv = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    assert res._L.rm_voxelize_mesh(res._h, 3, C.c_void_p(dv.data_ptr() + 2), 1, None, 1, None, np.zeros(3, np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                   np.ones(3, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 20, 18, 16, counts.ctypes.data_as(C.POINTER(C.c_uint64)), 6,
                                   stats.ctypes.data_as(C.POINTER(C.c_uint64)), 6) == _ffi.RM_ERR_ARG
    assert last_error(res) == "rm_voxelize_mesh: device xyz and indices need 4-byte alignment"
    assert np.all(counts == 0x5A5A5A5A5A5A5A5A) and kept.occupancy().tobytes() == words
    with pytest.raises(ValueError):
        res.voxelize_mesh(v.reshape(-1), t, *UNIT, SHAPE)
    with pytest.raises(ValueError):
        res.voxelize_mesh(v, t.astype(np.float32), *UNIT, SHAPE)
    with pytest.raises(ValueError):
        res.voxelize_mesh(v, t, *UNIT, (20, 1, 16))
    assert kept.occupancy().tobytes() == words


def test_read_refusals():
    fresh = renderer.RayMarchingResources(0)
    try:
        host = np.full(64, 0x5A, np.uint8)
        assert fresh._L.rm_read_voxels(fresh._h, host.ctypes.data, 0, None) == _ffi.RM_ERR_ARG
        assert last_error(fresh) == "rm_read_voxels: no mesh has been voxelised"
        assert np.all(host == 0x5A)
        assert fresh._L.rm_read_voxels(None, host.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
        # an empty command buffer, and an invalid one: a voxelisation needs no program
        v, t = VR.icosphere(0, RADIUS, CENTRE)
        assert fresh.voxelize_mesh(v, t, *UNIT, SHAPE).counts["inside"] == 646
        fresh.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([3, 0xDEAD, 0xBEEF, 7], np.uint32).tobytes())
        with pytest.raises(_ffi.RmError):
            fresh.validate()
        assert fresh.voxelize_mesh(v, t, *UNIT, SHAPE).counts["inside"] == 646
        assert fresh._L.rm_read_voxels(fresh._h, None, 0, None) == _ffi.RM_OK                   # nothing wanted
    finally:
        fresh.close()


def test_other_results_survive_a_voxel_call_and_it_survives_them():
    r = renderer.RayMarchingResources(0)
    try:
        use(r, *scene_program("g8"))
        origin, step, shape = box_lattice((17, 16, 15))
        image = r.draw(64, 48)
        m = r.extract_mesh_grid(origin, step, shape)
        topo = r.label_solid_grid(origin, step, shape)
        dist = r.distance_solid_grid(origin, step, shape)
        labels, d2 = topo.labels(), dist.d2()
        verts = np.empty_like(m.vertices)
        v, t = VR.icosphere(1, RADIUS, CENTRE)
        vox = r.voxelize_mesh(v, t, *UNIT, SHAPE)
        words = vox.occupancy().tobytes()
        assert np.array_equal(topo.labels(), labels) and np.array_equal(dist.d2(), d2)
        r._check(r._L.rm_read_mesh(r._h, verts.ctypes.data, None, None, None, 0, None))
        assert np.array_equal(verts, m.vertices)
        assert np.array_equal(r.draw(64, 48), image)
        r.extract_mesh_grid(origin, step, shape)
        r.label_solid_grid(origin, step, shape)
        r.distance_solid_grid(origin, step, shape).features(r2_wall=1)
        r.support_solid_grid(origin, step, shape)
        r.islands_solid_grid(origin, step, shape)
        r.surface_solid_grid(origin, step, shape)
        r.slice_contours_grid(1, (-2.0, -2.0), (0.25, 0.25), (17, 17), [0.0])
        assert vox.occupancy().tobytes() == words
    finally:
        r.close()
