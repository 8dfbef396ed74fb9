"""The lattice draw on the GPU (rm_set_lattice, rm_draw_lattice, rm_cast_lattice): the counts == numpy; every
word of a cast == the restatement (tests/lattice_draw_ref.py, which visits every cell: so equality on the sparse and
one-point-per-brick lattices and on the degenerate rays is the proof that the jumps over empty bricks are exact); a draw == the
restatement in all three output formats and == the sixteen camera_rays -> cast_lattice colours accumulated in numpy; row bands,
destinations, windows, the round trip from a voxelised mesh without a host copy; isolation and refusals."""
import ctypes as C

import numpy as np
import pytest

import lattice_cases as LC
import lattice_draw_ref as LR
from ray_marching_amd import _ffi, camera, renderer

pytestmark = pytest.mark.gpu

F = np.float32
# 7 / 8 / 9 and 15 / 16 / 17 points on each axis in turn, around the brick's edge of 8
EDGE_SHAPES = [tuple(v if b == a else (10, 9, 11)[b] for b in range(3)) for a in range(3) for v in (7, 8, 9, 15, 16, 17)]
COUNT_SHAPES = [(2, 2, 2), (3, 5, 7)] + EDGE_SHAPES + [(65, 33, 17), (1024, 2, 2), (2, 1024, 2), (2, 2, 1024)]
CAST_CASES = [((2, 2, 2), "full"), ((3, 5, 7), "random"), ((9, 8, 7), "corners"), ((17, 16, 15), "empty"), ((17, 16, 15), "full"),
              ((17, 16, 15), "sparse"), ((17, 16, 15), "one_per_brick"), ((15, 17, 16), "random"), ((65, 33, 17), "hollow_brick"),
              ((65, 33, 17), "sparse"), ((65, 33, 17), "one_per_brick"), ((1024, 2, 2), "sparse"), ((2, 1024, 2), "sparse"),
              ((2, 2, 1024), "random")]


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)      # no program: a lattice draw needs none
    r.set_materials(LC.PALETTE)
    yield r
    r.close()


def same(a, b):
    """Bit-identical, with any two NaNs equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def words(out):
    """cast_lattice's dict as the restatement's three arrays."""
    hit = np.concatenate([out["t"][:, None], out["position"], out["normal"], out["diffuse"][:, None]], axis=1).astype(F)
    ids = np.stack([out["kind"], out["index"], out["cls"], out["face"]], axis=1).astype(np.uint32)
    return {"hit": hit, "ids": ids, "rgb": out["rgb"]}


def assert_cast(res, cls, rays, window=None, what=""):
    got = words(res.cast_lattice(rays, window=window))
    want = LR.cast(cls, LC.ORIGIN, LC.STEP, rays, LC.PALETTE, window)
    for key in ("ids", "hit", "rgb"):
        bad = np.nonzero((got[key].view(np.uint32) != want[key].view(np.uint32)).any(axis=1))[0]
        assert same(got[key], want[key]), (what, key, len(bad), bad[:4], rays[bad[:4]], got[key][bad[:4]], want[key][bad[:4]])
    return want


def look(res, W, H, target, distance, angles=(35.0, -25.0)):
    """The orbit camera on the context -> the uniforms as the restatement takes them."""
    ctl = camera.OrbitCameraController.new([float(x) for x in target], float(distance))
    ctl.update(camera.Orbit([float(angles[0]), float(angles[1])]))
    u = renderer.prepare_uniforms((W, H), ctl.camera())
    res.set_uniforms(u)
    return {"viewport_extent": list(u.viewport_extent), "inv_proj": list(u.inv_proj), "inv_view": list(u.inv_view)}


def centre_of(shape):
    lo, hi = LC.box(shape)
    return 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))


@pytest.mark.parametrize("shape", COUNT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts(res, shape):
    nx, ny, nz = shape
    for kind in LC.CONTENTS:
        cls = LC.contents(shape, kind, seed=nx + 2 * ny + 3 * nz)
        lat = res.set_lattice(cls, LC.ORIGIN, LC.STEP)
        pad = np.zeros((-(-nz // 8) * 8, -(-ny // 8) * 8, -(-nx // 8) * 8), dtype=bool)
        pad[:nz, :ny, :nx] = cls != 0
        bricks = pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8, pad.shape[2] // 8, 8).any(axis=(1, 3, 5))
        assert lat.counts == {"points": int(np.count_nonzero(cls)), "bricks": int(bricks.sum())}, (shape, kind)
        assert all(lat.stats[k] == 0 for k in ("bricks", "bricks_kept", "bricks_inside", "evaluations", "scratch_bytes"))
        assert lat.stats["retained_bytes"] >= cls.size + cls.size // 8 and lat.shape == shape


@pytest.mark.parametrize("shape,kind", CAST_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_cast_is_the_restatement(res, shape, kind):
    cls = LC.contents(shape, kind, seed=17)
    res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    rays = np.concatenate([LC.random_rays(shape, 1500, seed=19), LC.degenerate_rays(shape)])
    assert len(rays) <= 4096
    want = assert_cast(res, cls, rays, None, (shape, kind))
    hits = int((want["ids"][:, 0] == LR.RM_HIT_SURFACE).sum())
    assert (hits == 0) == (kind == "empty") and hits < len(rays)
    if min(shape) > 2:
        assert_cast(res, cls, rays, LC.windows(shape)[3], (shape, kind, "window"))


def test_cast_windows_outputs_and_device_arrays(res):
    import torch
    shape = (17, 16, 15)
    cls = LC.contents(shape, "random", seed=23)
    res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    rays = np.concatenate([LC.random_rays(shape, 1000, seed=29), LC.degenerate_rays(shape)])
    for w in LC.windows(shape):
        assert_cast(res, cls, rays, w, w)
    # a window == the same call on a lattice zeroed outside it (rays without ties at the window's faces: random ones)
    generic = LC.random_rays(shape, 2000, seed=31)
    for w in LC.windows(shape):
        res.set_lattice(cls, LC.ORIGIN, LC.STEP)
        a = words(res.cast_lattice(generic, window=w))
        cut = np.zeros_like(cls)
        cut[w[2]:w[5], w[1]:w[4], w[0]:w[3]] = cls[w[2]:w[5], w[1]:w[4], w[0]:w[3]]
        res.set_lattice(cut, LC.ORIGIN, LC.STEP)
        b = words(res.cast_lattice(generic))
        assert all(same(a[k], b[k]) for k in a), w
    # torch tensors in and out, single outputs, n == 0
    res.set_lattice(torch.from_numpy(cls).to("cuda:0"), LC.ORIGIN, LC.STEP)
    want = LR.cast(cls, LC.ORIGIN, LC.STEP, rays, LC.PALETTE)
    dev = res.cast_lattice(torch.from_numpy(rays).to("cuda:0"))
    torch.cuda.synchronize()
    got = words({k: v.cpu().numpy() for k, v in dev.items()})
    assert same(got["hit"], want["hit"]) and same(got["ids"].astype(np.uint32), want["ids"]) and same(got["rgb"], want["rgb"])
    ids = np.empty((len(rays), 4), dtype=np.uint32)
    res._check(res._L.rm_cast_lattice(res._h, len(rays), rays.ctypes.data, None, None, ids.ctypes.data, None, 0, None))
    assert same(ids, want["ids"])
    assert res._L.rm_cast_lattice(res._h, 0, None, None, None, ids.ctypes.data, None, 0, None) == _ffi.RM_OK


def test_palette_follows_the_table_at_the_cast(res):
    shape = (9, 8, 7)
    cls = LC.contents(shape, "full", seed=37)
    res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    rays = LC.random_rays(shape, 500, seed=41)
    try:
        for table in ([[0.25, 0.5, 0.75]], LC.PALETTE[:3], [[i / 255.0, 1.0 - i / 255.0, 0.5] for i in range(256)]):
            res.set_materials(table)
            got = words(res.cast_lattice(rays))
            want = LR.cast(cls, LC.ORIGIN, LC.STEP, rays, table)
            assert same(got["rgb"], want["rgb"]) and same(got["ids"], want["ids"]), len(table)
    finally:
        res.set_materials(LC.PALETTE)


# shape, contents, frame, the cell the camera looks at (None: the box's centre) and its distance (in box diagonals; with a cell: in
# world units).  The third camera sits inside the lattice, the fourth inside the hollow brick of a solid block.
DRAW_CASES = [((17, 16, 15), "sparse", 64, 48, None, 1.6), ((17, 16, 15), "random", 33, 17, None, 1.2),
              ((17, 16, 15), "random", 33, 17, None, 0.15), ((65, 33, 17), "hollow_brick", 64, 48, (11.5, 11.5, 11.5), 0.3),
              ((65, 33, 17), "one_per_brick", 33, 17, None, 1.0), ((9, 8, 7), "empty", 33, 17, None, 1.5)]


@pytest.mark.parametrize("shape,kind,W,H,cell,far", DRAW_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "x".join(map(str, v)))
def test_draw_is_the_restatement_and_the_composition(res, shape, kind, W, H, cell, far):
    cls = LC.contents(shape, kind, seed=43)
    res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    target, diagonal = centre_of(shape)
    u = look(res, W, H, target, far * diagonal) if cell is None else look(res, W, H, LC.ORIGIN + np.asarray(cell, dtype=F) * LC.STEP, far)
    want = LR.draw(cls, LC.ORIGIN, LC.STEP, LC.PALETTE, u, W, H)
    try:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)
        got = res.draw_lattice(W, H)
        assert got.dtype == F and same(got, want)
        assert len(np.unique(got.reshape(-1, 4), axis=0)) > 30                                     # (a picture, not one colour)
        # the sixteen camera_rays -> cast_lattice colours, accumulated in numpy in sample order
        samples = [res.cast_lattice(res.camera_rays(W, H, sample=s))["rgb"] for s in range(16)]
        assert same(got, LR.resolve(samples).reshape(H, W, 4))
        # row bands concatenate to the frame
        bands = [res.draw_lattice(W, H, r0, n) for r0, n in ((0, 5), (5, 1), (6, H - 6))]
        assert same(np.concatenate(bands), got)
        for fmt, bgra in ((_ffi.RM_FORMAT_RGBA8_UNORM, False), (_ffi.RM_FORMAT_BGRA8_UNORM, True)):
            res.set_output_format(fmt)
            q = res.draw_lattice(W, H)
            assert q.dtype == np.uint8 and np.array_equal(q, LR.unorm8(want, bgra)), fmt
    finally:
        res.set_output_format(_ffi.RM_FORMAT_RGBA32F)


def test_draw_destinations_windows_and_streams(res):
    import torch
    shape, W, H = (17, 16, 15), 33, 17
    cls = LC.contents(shape, "random", seed=47)
    res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    target, diagonal = centre_of(shape)
    u = look(res, W, H, target, 1.3 * diagonal, angles=(-50.0, 20.0))
    host = res.draw_lattice(W, H)
    # host and device destinations give the same bytes, on the caller's stream and on the context's own
    side = torch.cuda.Stream(device="cuda:0")
    for stream in (side.cuda_stream, _ffi.RM_STREAM_OWN):
        out = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        res.draw_lattice_device(W, H, out.data_ptr(), stream=stream)
        if stream == _ffi.RM_STREAM_OWN:
            res.sync_context()
        else:
            side.synchronize()
        assert same(out.cpu().numpy(), host)
    band = torch.full((H + 2, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
    res.draw_lattice_device(W, H, band[1:].data_ptr(), row0=3, rows=4, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    b = band.cpu().numpy()
    assert same(b[1:5], host[3:7]) and np.all(b[0] == -1.0) and np.all(b[5:] == -1.0)              # its rows and nothing else
    # a window: the restatement, and the same draw of the lattice zeroed outside it (cut-away: the cells behind show)
    for w in LC.windows(shape)[:2]:
        cut = np.zeros_like(cls)
        cut[w[2]:w[5], w[1]:w[4], w[0]:w[3]] = cls[w[2]:w[5], w[1]:w[4], w[0]:w[3]]
        res.set_lattice(cls, LC.ORIGIN, LC.STEP)
        a = res.draw_lattice(W, H, window=w)
        assert same(a, LR.draw(cls, LC.ORIGIN, LC.STEP, LC.PALETTE, u, W, H, window=w)) and not same(a, host)
        res.set_lattice(cut, LC.ORIGIN, LC.STEP)
        assert same(res.draw_lattice(W, H), a), w


def test_round_trip_from_a_voxelised_mesh_without_a_host_copy(res):
    import voxel_ref as VR
    W, H = 64, 48
    v, t = VR.icosphere(1, 6.3, (9.5, 8.25, 7.75))
    origin, step, shape = (0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (20, 18, 16)
    vox = res.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), shape)
    occ = vox.occupancy_device()                                 # a torch tensor on the GPU
    lat = res.set_lattice(occ, origin, step)
    assert lat.counts["points"] == vox.counts["inside"] == 914
    u = look(res, W, H, (1.2, 1.0, 1.0), 4.0)
    got = res.draw_lattice(W, H)
    assert same(got, LR.draw(vox.occupancy(), np.asarray(origin, F), np.asarray(step, F), LC.PALETTE, u, W, H))
    assert np.any(got[..., 0] > got[..., 1] + 0.2)               # class 1: the palette's red shows


def raw_set(res, nx, ny, nz, cls, origin, step, counts, n_counts, stats, n_stats):
    fp = lambda a: None if a is None else np.asarray(a, dtype=F).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    up = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    return res._L.rm_set_lattice(res._h, nx, ny, nz, None if cls is None else C.c_void_p(cls.ctypes.data), 0, None, fp(origin), fp(step), up(counts),
                                 n_counts, up(stats), n_stats)


def last_error(r):
    return (r._L.rm_last_error(r._h) or b"").decode()


def test_refusals_leave_outputs_and_the_previous_lattice_alone(res):
    shape, W, H = (9, 8, 7), 33, 17
    cls = LC.contents(shape, "random", seed=53)
    kept = res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    target, diagonal = centre_of(shape)
    look(res, W, H, target, 1.4 * diagonal)
    image = res.draw_lattice(W, H)
    counts, stats = np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64)
    o, s, nan, inf = (0, 0, 0), (1, 1, 1), float("nan"), float("inf")
    cases = [                                                    # the front end's order of checks
        ((9, 8, 7, None, o, s, counts, 2, stats, 6), _ffi.RM_ERR_NULL),
        ((9, 8, 7, cls, o, s, None, 2, stats, 6), _ffi.RM_ERR_NULL),
        ((9, 8, 7, cls, o, s, counts, 2, None, 6), _ffi.RM_ERR_NULL),
        ((9, 8, 7, cls, o, s, counts, 1, stats, 5), _ffi.RM_ERR_ARG),                              # n_counts before n_stats ...
        ((9, 8, 7, cls, o, s, counts, 2, stats, 5), _ffi.RM_ERR_ARG),
        ((9, 8, 7, cls, None, s, counts, 2, stats, 6), _ffi.RM_ERR_NULL),
        ((9, 8, 7, cls, (0, nan, 0), s, counts, 2, stats, 6), _ffi.RM_ERR_ARG),
        ((9, 8, 7, cls, o, (1, 0, 1), counts, 2, stats, 6), _ffi.RM_ERR_ARG),
        ((9, 8, 7, cls, o, (1, inf, 1), counts, 2, stats, 6), _ffi.RM_ERR_ARG),
        ((1025, 2, 2, cls, o, (1, -1, 1), counts, 2, stats, 6), _ffi.RM_ERR_ARG),                  # ... the step before the range
        ((1025, 2, 2, cls, o, s, counts, 2, stats, 6), _ffi.RM_ERR_RANGE),
        ((9, 1, 7, cls, o, s, counts, 2, stats, 6), _ffi.RM_ERR_RANGE),
        ((1024, 1024, 512, cls, o, s, counts, 2, stats, 6), _ffi.RM_ERR_RANGE),
    ]
    for args, status in cases:
        assert raw_set(res, *args) == status, args
        assert "rm_set_lattice" in last_error(res)
        assert np.all(counts == 0x5A5A5A5A5A5A5A5A) and np.all(stats == 0x5A5A5A5A5A5A5A5A)
        assert kept.current() and same(res.draw_lattice(W, H), image)                              # the previous lattice still draws
    assert res._L.rm_set_lattice(None, 9, 8, 7, C.c_void_p(cls.ctypes.data), 0, None, None, None, None, 2, None, 6) == _ffi.RM_ERR_NULL
    # draws and casts: NULL, the frame, the window
    out = np.full((H, W, 4), -1.0, dtype=F)
    draw = lambda W_, H_, r0, n, w, o_: res._L.rm_draw_lattice(res._h, W_, H_, r0, n, w, o_, 0, None)  # noqa: E731
    win = lambda *v: np.asarray(v, dtype=np.uint32).ctypes.data_as(C.c_void_p)  # noqa: E731
    assert draw(W, H, 0, H, None, None) == _ffi.RM_ERR_NULL
    assert res._L.rm_draw_lattice(None, W, H, 0, H, None, out.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
    for band in ((0, H + 1), (H, 1), (3, 0)):
        assert draw(W, H, *band, None, out.ctypes.data) == _ffi.RM_ERR_RANGE
    assert draw(0, H, 0, H, None, out.ctypes.data) == _ffi.RM_ERR_RANGE
    for w in ((0, 0, 0, 10, 8, 7), (3, 0, 0, 3, 8, 7), (0, 5, 0, 9, 4, 7), (0, 0, 7, 9, 8, 8)):
        assert draw(W, H, 0, H, win(*w), out.ctypes.data) == _ffi.RM_ERR_ARG and "window" in last_error(res)
        rays = LC.random_rays(shape, 4)
        hit = np.full((4, 8), -1.0, dtype=F)
        assert res._L.rm_cast_lattice(res._h, 4, rays.ctypes.data, win(*w), hit.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_ARG
        assert np.all(hit == -1.0)
    assert np.all(out == -1.0)
    rays = LC.random_rays(shape, 4)
    assert res._L.rm_cast_lattice(res._h, 4, rays.ctypes.data, None, None, None, None, 0, None) == _ffi.RM_ERR_NULL
    assert res._L.rm_cast_lattice(res._h, 4, None, None, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_NULL
    import torch
    d = torch.zeros(256, dtype=torch.float32, device="cuda:0")
    assert res._L.rm_cast_lattice(res._h, 4, C.c_void_p(d.data_ptr()), None, C.c_void_p(d.data_ptr() + 4), None, None, 1, None) == _ffi.RM_ERR_ARG
    with pytest.raises(ValueError):
        res.set_lattice(cls.astype(np.float32), LC.ORIGIN, LC.STEP)
    with pytest.raises(ValueError):
        res.set_lattice(cls[:1], LC.ORIGIN, LC.STEP)
    with pytest.raises(ValueError):
        res.draw_lattice(W, H, window=(0, 0, 0, 9, 8))
    assert kept.current() and same(res.draw_lattice(W, H), image)
    later = res.set_lattice(cls, LC.ORIGIN, LC.STEP)
    assert later.current() and not kept.current()


def test_before_any_lattice_and_without_a_program():
    fresh = renderer.RayMarchingResources(0)
    try:
        out = np.full((8, 8, 4), -1.0, dtype=F)
        rays = LC.random_rays((9, 8, 7), 4)
        assert fresh._L.rm_draw_lattice(fresh._h, 8, 8, 0, 8, None, out.ctypes.data, 0, None) == _ffi.RM_ERR_ARG
        assert last_error(fresh) == "rm_draw_lattice: no lattice has been set (rm_set_lattice)"
        assert fresh._L.rm_cast_lattice(fresh._h, 4, rays.ctypes.data, None, out.ctypes.data, None, None, 0, None) == _ffi.RM_ERR_ARG
        assert last_error(fresh) == "rm_cast_lattice: no lattice has been set (rm_set_lattice)"
        assert np.all(out == -1.0)
        assert fresh._L.rm_draw_lattice(fresh._h, 8, 9, 0, 10, None, out.ctypes.data, 0, None) == _ffi.RM_ERR_RANGE  # the frame first
        # an invalid command buffer: a lattice draw needs no program; the default table has one entry
        fresh.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([3, 0xDEAD, 0xBEEF, 7], np.uint32).tobytes())
        with pytest.raises(_ffi.RmError):
            fresh.validate()
        cls = LC.contents((9, 8, 7), "random", seed=59)
        fresh.set_lattice(cls, LC.ORIGIN, LC.STEP)
        got = words(fresh.cast_lattice(rays))
        want = LR.cast(cls, LC.ORIGIN, LC.STEP, rays, [[0.4, 0.7, 0.1]])
        assert all(same(got[k], want[k]) for k in got)
    finally:
        fresh.close()


def test_other_results_and_the_draw_state_survive_and_the_lattice_survives_them():
    from test_gpu_topology import box_lattice, scene_program, use
    import voxel_ref as VR
    r = renderer.RayMarchingResources(0)
    try:
        use(r, *scene_program("g8"))
        origin, step, shape = box_lattice((17, 16, 15))
        look(r, 64, 48, (0.0, 0.0, 0.0), 5.0)
        image = r.draw(64, 48)
        m = r.extract_mesh_grid(origin, step, shape)
        topo = r.label_solid_grid(origin, step, shape)
        dist = r.distance_solid_grid(origin, step, shape)
        v, t = VR.icosphere(1, 6.3, (9.5, 8.25, 7.75))
        vox = r.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (20, 18, 16))
        labels, d2, occ = topo.labels(), dist.d2(), vox.occupancy()
        verts = np.empty_like(m.vertices)
        cls = LC.contents((17, 16, 15), "random", seed=61)
        lat = r.set_lattice(cls, origin, step)
        picture = r.draw_lattice(64, 48)
        rays = LC.random_rays((17, 16, 15), 64, origin=np.asarray(origin, F), step=np.asarray(step, F))
        cast = r.cast_lattice(rays)
        assert np.array_equal(topo.labels(), labels) and np.array_equal(dist.d2(), d2) and np.array_equal(vox.occupancy(), occ)
        r._check(r._L.rm_read_mesh(r._h, verts.ctypes.data, None, None, None, 0, None))
        assert np.array_equal(verts, m.vertices)
        assert np.array_equal(r.draw(64, 48), image)                                               # the draw state
        r.extract_mesh_grid(origin, step, shape)
        r.label_solid_grid(origin, step, shape)
        r.distance_solid_grid(origin, step, shape).features(r2_wall=1)
        r.support_solid_grid(origin, step, shape)
        r.islands_solid_grid(origin, step, shape)
        r.surface_solid_grid(origin, step, shape)
        r.voxelize_mesh(v, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (20, 18, 16))
        r.slice_contours_grid(1, (-2.0, -2.0), (0.25, 0.25), (17, 17), [0.0])
        r.cast_rays(rays)
        assert lat.current() and same(r.draw_lattice(64, 48), picture)
        again = r.cast_lattice(rays)
        assert all(same(again[k], cast[k]) for k in cast)
    finally:
        r.close()
