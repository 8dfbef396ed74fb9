"""Lattice meshing on the GPU: rm_mesh_classes / rm_read_class_mesh against the contract's restatement
tests/class_mesh_ref.py -- counts, vertices (bit for bit), triangles and ids all equal --, on the smallest lattices at which the
kernels can go wrong; determinism, both kinds of input and of destination; the round trip mesh -> lattice -> mesh -> lattice on the
device; the isolation of the retained slot; and the refusals, message for message.

The mark kernel has no tile in y or z: a wave takes a WORD of 64 consecutive corners of an x row and a workgroup 16 consecutive
words in the order of the corner index, four to a wave.  So the shapes straddle the word (nx + 1 corners around 64 and 128), the
wave's and the workgroup's run of words (15, 16, 18, 20 words, by ny and by nz in turn), more than 256 rows for the reducer's
fold, and more than 1024 workgroups for the scan's serial part."""
import ctypes as C

import numpy as np
import pytest

import class_mesh_ref as CR
import lattice_cases as LC
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
SOLID = [1, 2, 3, 4, 5, 6, 7]
SETS = ((SOLID, [0]), ([0], SOLID), ([1, 2], [3, 7]))
PATTERNS = ("empty", "full", "random", "checkerboard", "corners", "hollow_brick")
SHAPES = [(2, 2, 2), (3, 5, 7),
          (62, 3, 2), (63, 2, 3), (64, 3, 2), (65, 2, 2), (127, 2, 3), (128, 3, 2),          # nx + 1 corners straddle one, two, three words
          (2, 2, 4), (2, 3, 3), (2, 2, 5), (2, 4, 3), (2, 4, 2), (2, 5, 2), (2, 3, 4),        # 15, 16, 18, 20 words; by nz and by ny
          (65, 33, 17),                                                                       # many workgroups, two words to a row
          (1024, 2, 2), (2, 1024, 2), (2, 2, 1024),                                           # the longest rows; 386 rows to fold
          (2, 128, 127)]                                                                      # 1032 workgroups: the scan's serial part


def pattern(shape, kind, seed):
    nx, ny, nz = shape
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 10, size=(nz, ny, nx), dtype=np.uint8)    # bytes above 7 clamp
    if kind == "checkerboard":
        return CR.checkerboard(shape)
    if kind == "corners":                                                                        # faces against the padding
        c = np.zeros((nz, ny, nx), dtype=np.uint8)
        for k in (0, -1):
            for j in (0, -1):
                for i in (0, -1):
                    c[k, j, i] = 1 + (i + 2 * j + 4 * k) % 7
        return c
    return LC.contents(shape, kind, seed)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    yield r
    r.close()


def words(m):
    """The three arrays of a ClassMesh as host uint32 words."""
    return [np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.uint32) for x in (m.vertices, m.triangles, m.ids)]


def assert_is_restatement(m, ref, what):
    assert m.counts == ref["counts"], (what, m.counts, ref["counts"])
    for got, name in zip(words(m), ("vertices", "triangles", "ids")):
        assert got.shape == ref[name].shape and np.array_equal(got, ref[name].view(np.uint32)), (what, name)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_mesh_is_the_restatement(res, shape):
    for n, kind in enumerate(PATTERNS):
        data = pattern(shape, kind, seed=100 + n)
        for A, B in SETS:
            m = res.mesh_classes(data, A, B, LC.ORIGIN, LC.STEP)
            assert_is_restatement(m, CR.mesh(data, A, B, LC.ORIGIN, LC.STEP), (shape, kind, A))
            assert m.normals is None and m.stats["retained_bytes"] >= 20 * m.counts["triangles"] and m.stats["bricks"] == 0
            if kind == "empty" and A == SOLID:
                assert m.counts["vertices"] == 0 and len(m.vertices) == 0 and len(m.triangles) == 0 and m.is_closed()
            if A == [0] and m.counts["faces"]:
                assert np.any(m.face_point == _ffi.RM_NO_ID)                                    # padding on the A side
            if len(m.triangles):
                assert np.array_equal(m.face_classes[:, 0] | m.face_classes[:, 1] << 8 | m.face << 16, m.ids[:, 0])


def test_default_b_is_the_complement(res):
    data = pattern((9, 8, 7), "random", 3)
    a, b = res.mesh_classes(data, [1, 2]), res.mesh_classes(data, [1, 2], [0, 3, 4, 5, 6, 7])
    assert all(np.array_equal(x, y) for x, y in zip(words(a), words(b))) and a.counts == b.counts
    assert a.counts["open_edges"] == 0 and a.is_closed()


def test_runs_inputs_and_destinations_agree(res):
    import torch
    data = pattern((65, 33, 17), "random", 5)
    first = res.mesh_classes(data, SOLID, None, LC.ORIGIN, LC.STEP)
    again = res.mesh_classes(data, SOLID, None, LC.ORIGIN, LC.STEP)
    on_device = torch.from_numpy(data).to("cuda:0")
    from_device = res.mesh_classes(on_device, SOLID, None, LC.ORIGIN, LC.STEP)
    to_device = res.mesh_classes(on_device, SOLID, None, LC.ORIGIN, LC.STEP, device=True)
    assert isinstance(to_device.vertices, torch.Tensor) and to_device.triangles.dtype == torch.int32
    torch.cuda.synchronize()
    for other in (again, from_device, to_device):
        assert other.counts == first.counts
        assert all(np.array_equal(x, y) for x, y in zip(words(first), words(other)))
    # device destinations through read_class_mesh_device, each output alone and all together
    V, T = first.counts["vertices"], first.counts["triangles"]
    v = torch.zeros((V, 3), dtype=torch.float32, device="cuda:0")
    t = torch.zeros((T, 3), dtype=torch.int32, device="cuda:0")
    i = torch.zeros((T, 2), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    res.read_class_mesh_device(v.data_ptr(), 0, 0, stream=stream)
    res.read_class_mesh_device(0, t.data_ptr(), i.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    for got, want in zip((v, t, i), words(first)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    with pytest.raises(_ffi.RmError) as e:
        res.read_class_mesh_device(v.data_ptr() + 2, 0, 0, stream=stream)
    assert e.value.status == _ffi.RM_ERR_ARG and "rm_read_class_mesh: device arrays need 4-byte alignment" in str(e.value)


@pytest.mark.parametrize("name", ["ball", "torus"])
def test_round_trip_on_the_device(res, name):
    import torch
    import voxel_ref as VR
    if name == "ball":
        v, t = VR.icosphere(3, 26.3, (31.6, 31.4, 31.5))
        shape, tunnels = (64, 64, 64), 0
    else:
        v, t = VR.torus(nu=64, nv=32, R=20.0, r=7.3, centre=(31.5, 31.5, 15.5))
        shape, tunnels = (64, 64, 32), 1
    origin, step = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125)
    world = (np.asarray(origin, F) + v.astype(F) * np.asarray(step, F)).astype(F)
    vox = res.voxelize_mesh(world, t, origin, step, shape)
    occ = vox.occupancy_device()
    m = res.mesh_classes(occ, [1], [0], origin, step, device=True)
    assert m.counts["open_edges"] == 0 and m.counts["faces"] > 0
    back = res.voxelize_mesh(m, None, origin, step, shape)
    occ2 = back.occupancy_device()
    assert back.counts["open_rows"] == 0 and back.counts["rejected"] == 0
    assert torch.equal(occ, occ2)
    topo = res.label_occupancy(occ2)
    assert (topo.bodies, topo.cavities, topo.tunnels) == (1, 0, tunnels)
    if m.counts["branch_edges"] == 0:
        assert m.counts["vertices"] - m.counts["edges"] + m.counts["faces"] == 2 - 2 * tunnels


# ---- isolation ------------------------------------------------------------------------------------------------------------------------
def test_other_results_survive_and_the_class_mesh_survives_them():
    from test_gpu_topology import box_lattice, scene_program, use
    import voxel_ref as VR
    r = renderer.RayMarchingResources(0)
    try:
        use(r, *scene_program("g8"))
        origin, step, shape = box_lattice((17, 16, 15))
        em = r.extract_mesh_grid(origin, step, shape)
        topo = r.label_solid_grid(origin, step, shape)
        dist = r.distance_solid_grid(origin, step, shape)
        sup = r.support_solid_grid(origin, step, shape)
        isl = r.islands_solid_grid(origin, step, shape)
        v, t = VR.icosphere(1, 6.3, (9.5, 8.25, 7.75))
        vox = r.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (20, 18, 16))
        before = [topo.labels(), dist.d2(), sup.mask(), isl.labels(), vox.occupancy()]
        data = pattern((17, 16, 15), "random", 7)
        m = r.mesh_classes(data, SOLID, None, origin, step)
        kept = [w.copy() for w in words(m)]
        after = [topo.labels(), dist.d2(), sup.mask(), isl.labels(), vox.occupancy()]
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        verts = np.empty_like(em.vertices)
        r._check(r._L.rm_read_mesh(r._h, verts.ctypes.data, None, None, None, 0, None))
        assert np.array_equal(verts.view(np.uint32), em.vertices.view(np.uint32))
        for call in (lambda: r.extract_mesh_grid(origin, step, shape), lambda: r.label_solid_grid(origin, step, shape),
                     lambda: r.distance_solid_grid(origin, step, shape).features(r2_wall=1), lambda: r.support_solid_grid(origin, step, shape),
                     lambda: r.islands_solid_grid(origin, step, shape), lambda: r.surface_classes(data),
                     lambda: r.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (20, 18, 16)), lambda: r.set_lattice(data, origin, step)):
            call()
            assert all(np.array_equal(x, y) for x, y in zip(words(m.read()), kept))
        # the serial: a later mesh_classes makes the earlier object stale
        later = r.mesh_classes(pattern((33, 9, 5), "full", 9), SOLID)
        with pytest.raises(ValueError) as e:
            m.read()
        assert "ClassMesh" in str(e.value) and "rm_mesh_classes" in str(e.value)
        assert later.read().counts["vertices"] == len(later.vertices)
    finally:
        r.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_mesh(res, nx, ny, nz, cls, origin, step, mask_a, mask_b, counts, n_counts, stats, n_stats):
    fp = lambda a: None if a is None else np.asarray(a, dtype=F).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    up = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    return res._L.rm_mesh_classes(res._h, nx, ny, nz, None if cls is None else C.c_void_p(cls.ctypes.data), 0, None, fp(origin), fp(step),
                                  mask_a, mask_b, up(counts), n_counts, up(stats), n_stats)


def last_error(r):
    return (r._L.rm_last_error(r._h) or b"").decode()


def test_refusals_in_order_leave_outputs_and_the_previous_mesh_alone(res):
    data = pattern((9, 8, 7), "random", 11)
    kept = res.mesh_classes(data, SOLID, None, LC.ORIGIN, LC.STEP)
    first = [w.copy() for w in words(kept)]
    counts, stats = np.full(16, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64)
    o, s, nan, inf = (0, 0, 0), (1, 1, 1), float("nan"), float("inf")
    fn = "rm_mesh_classes: "
    cases = [
        ((9, 8, 7, None, o, s, 2, 1, counts, 12, stats, 6), _ffi.RM_ERR_NULL, fn + "classes, out_counts or out_stats is NULL"),
        ((9, 8, 7, data, o, s, 2, 1, None, 12, stats, 6), _ffi.RM_ERR_NULL, fn + "classes, out_counts or out_stats is NULL"),
        ((9, 8, 7, data, o, s, 2, 1, counts, 12, None, 6), _ffi.RM_ERR_NULL, fn + "classes, out_counts or out_stats is NULL"),
        ((9, 8, 7, data, None, s, 2, 1, counts, 11, stats, 5), _ffi.RM_ERR_ARG, fn + "n_counts 11 < RM_CMESH_COUNTS"),       # n_counts first
        ((9, 8, 7, data, None, s, 2, 1, counts, 12, stats, 5), _ffi.RM_ERR_ARG, fn + "n_stats 5 < RM_CMESH_STATS"),
        ((1025, 2, 2, data, None, s, 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_NULL, fn + "origin or step is NULL"),
        ((1025, 2, 2, data, o, None, 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_NULL, fn + "origin or step is NULL"),
        ((1025, 2, 2, data, (0, nan, 0), s, 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "origin[1] = nan is not finite"),
        ((1025, 2, 2, data, o, (1, 0, 1), 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "step[1] = 0: a step must be finite and > 0"),
        ((1025, 2, 2, data, o, (1, 1, inf), 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "step[2] = inf: a step must be finite and > 0"),
        ((1025, 2, 2, data, o, s, 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_RANGE,                                              # the lattice before the masks
         fn + "lattice 1025x2x2: 2..1024 points per axis, at most 2^28 in all"),
        ((9, 1, 7, data, o, s, 2, 1, counts, 12, stats, 6), _ffi.RM_ERR_RANGE, fn + "lattice 9x1x7: 2..1024 points per axis, at most 2^28 in all"),
        ((1024, 1024, 512, data, o, s, 2, 1, counts, 12, stats, 6), _ffi.RM_ERR_RANGE,
         fn + "lattice 1024x1024x512: 2..1024 points per axis, at most 2^28 in all"),
        ((9, 8, 7, data, o, s, 3, 1, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "masks 0x3, 0x1: non-empty, disjoint, no bit above 7"),
        ((9, 8, 7, data, o, s, 0, 1, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "masks 0x0, 0x1: non-empty, disjoint, no bit above 7"),
        ((9, 8, 7, data, o, s, 2, 0, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "masks 0x2, 0x0: non-empty, disjoint, no bit above 7"),
        ((9, 8, 7, data, o, s, 2, 256, counts, 12, stats, 6), _ffi.RM_ERR_ARG, fn + "masks 0x2, 0x100: non-empty, disjoint, no bit above 7"),
    ]
    for args, status, message in cases:
        assert raw_mesh(res, *args) == status, args
        assert last_error(res) == message
        assert np.all(counts == 0x5A5A5A5A5A5A5A5A) and np.all(stats == 0x5A5A5A5A5A5A5A5A)
        assert all(np.array_equal(x, y) for x, y in zip(words(kept.read()), first))              # the previous mesh still reads
    assert res._L.rm_mesh_classes(None, 9, 8, 7, C.c_void_p(data.ctypes.data), 0, None, None, None, 2, 1, None, 12, None, 6) == _ffi.RM_ERR_NULL
    assert res._L.rm_read_class_mesh(None, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    res._check(res._L.rm_read_class_mesh(res._h, None, None, None, 0, None))                     # every output may be NULL
    with pytest.raises(ValueError):
        res.mesh_classes(data.astype(np.float32), SOLID)
    with pytest.raises(ValueError):
        res.mesh_classes(data, [1], [1])


def test_before_any_class_mesh_and_without_a_program():
    fresh = renderer.RayMarchingResources(0)
    try:
        out = np.full(8, -1.0, dtype=F)
        assert fresh._L.rm_read_class_mesh(fresh._h, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_ARG
        assert last_error(fresh) == "rm_read_class_mesh: no lattice has been meshed" and np.all(out == -1.0)
        fresh.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([3, 0xDEAD, 0xBEEF, 7], np.uint32).tobytes())   # an invalid program: none is needed
        data = np.zeros((2, 2, 2), dtype=np.uint8)
        data[0, 0, 0] = 1
        m = fresh.mesh_classes(data, SOLID)
        assert m.counts["vertices"] == 8 and m.counts["triangles"] == 12 and tuple(m.triangles[0]) == (0, 6, 2)
        assert tuple(m.vertices[0]) == (-0.5, -0.5, -0.5) and tuple(m.ids[0]) == (1, 0)
        empty = fresh.mesh_classes(np.zeros((2, 2, 2), dtype=np.uint8), SOLID)
        assert empty.counts["vertices"] == 0 and empty.read().vertices.shape == (0, 3) and empty.stats["retained_bytes"] == 0
    finally:
        fresh.close()
