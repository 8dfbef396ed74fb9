"""Slicing on the GPU (rm_slice_contours / rm_read_slices) against the numpy restatement of the contract
(tests/slice_ref.py), bit for bit: every mesh scene on every axis, odd lattices, unsorted and duplicated heights, levels,
case coverage, open contours, chains longer than 4096 points over more than one batch, consistency with the mesh, the
per-point attributes, orientation, lattice planes far from the origin with steps down to the coordinates' ulp, errors, device
reads, and isolation from the draws and the mesh."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import scenes
import slice_ref as R
import test_mesh_bound_cpu as B
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
MESH_SCENES = ("g1", "g8", "g32", "g32_balanced", "g8x", "g32s", "ext_mix", "xform_mix", "mat_mix")
LIM = (0.01, 100.0, 256)


@pytest.fixture(scope="module")
def res():
    r = renderer.RayMarchingResources(0)
    r.resize_command_buffer(65536)
    r.set_materials(scenes.MATERIAL_TABLE)
    yield r
    r.close()


def same(a, b):
    """Bit-identical, with any two NaNs equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype.kind == "f":
        both_nan = np.isnan(a) & np.isnan(b)
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))
    return bool(np.array_equal(a, b))


def program(oracle, name):
    if name == "empty":
        return 0, np.zeros(0, dtype=np.uint32)
    return oracle.serialize(*ALL_SCENES[name]())


def oracle_layers(cc, w, axis, origin_uv, step_uv, shape_uv, heights, max_dist=LIM[1]):
    out = []
    for h in heights:
        p = R.layer_points(axis, origin_uv, step_uv, shape_uv, h)
        with np.errstate(all="ignore"):
            d = onp.map_scene(cc, w, F(max_dist), p[:, 0], p[:, 1], p[:, 2])
        out.append(np.asarray(d, dtype=F).reshape(shape_uv[1], shape_uv[0]))
    return out


def sampled_layer(res, axis, origin_uv, step_uv, shape_uv, height):
    """A layer's distances through rm_sample_grid (bit-identical to the oracle: test_gpu_mesh.py), as (nv, nu)."""
    u, v = R.in_plane_axes(axis)
    o, s, n = [0.0] * 3, [1.0] * 3, [1] * 3
    o[u], o[v], o[axis] = origin_uv[0], origin_uv[1], height
    s[u], s[v] = step_uv[0], step_uv[1]
    n[u], n[v] = shape_uv
    d = res.sample_grid(o, s, n)                        # [z, y, x]
    plane = np.take(d, 0, axis=2 - axis)                # the other two in (higher, lower) axis order
    return np.ascontiguousarray(plane if v > u else plane.T)


def check_slices(res, axis, origin, step, shape, heights, level, layers):
    pts, con, lf = R.slice_contours(layers, axis, origin, step, heights, level)
    s = res.slice_contours_grid(axis, origin, step, shape, heights, level=level)
    assert same(s.points, pts)
    assert same(s.contours, con)
    assert same(s.layer_first, lf)
    assert s.normals is None and s.leaf is None and s.axis == axis
    return s


# ---- scenes and lattices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", MESH_SCENES)
def test_slices_vs_restatement(res, oracle, name, axis):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    n_points = 0
    # odd lattices; heights unsorted and with a duplicate
    origin, step, shape, heights = (-2.0, -1.9), (F(0.1), F(0.105)), (41, 37), [0.1, -0.4, 0.1, 0.75]
    layers = oracle_layers(cc, w, axis, origin, step, shape, heights)
    for level in (0.0, 0.05):
        s = check_slices(res, axis, origin, step, shape, heights, level, layers)
        n_points += len(s.points)
    a, b = slice(int(s.layer_first[0]), int(s.layer_first[1])), slice(int(s.layer_first[2]), int(s.layer_first[3]))
    assert same(s.contours[a][:, [1, 3]], s.contours[b][:, [1, 3]])          # the duplicated height: the same layer again
    origin, step, shape, heights = (-2.5, -2.4), (F(5.0) / F(129), F(0.073)), (130, 67), [0.2, -0.3]
    layers = oracle_layers(cc, w, axis, origin, step, shape, heights)
    s = check_slices(res, axis, origin, step, shape, heights, 0.0, layers)
    n_points += len(s.points)
    assert n_points > 100, n_points
    # through slice_contours (lo, hi, resolution): the same lattice
    lo, hi = np.zeros(3, F), np.zeros(3, F)
    u, v = R.in_plane_axes(axis)
    lo[u], lo[v], lo[axis] = -2.5, -2.0, -1.0
    hi[u], hi[v], hi[axis] = 2.5, 2.0, 1.0
    s2 = res.slice_contours(lo, hi, (33, 29), layer_height=0.45, axis="xyz"[axis])
    su, sv = F(5.0) / F(32), F(4.0) / F(28)
    hs = [F(-1.0) + (F(k) + F(0.5)) * F(0.45) for k in range(5)]
    hs = [h for h in hs if h < F(1.0)]
    assert same(s2.heights, np.asarray(hs, F)) and len(hs) == 4
    pts, con, lf = R.slice_contours(oracle_layers(cc, w, axis, (-2.5, -2.0), (su, sv), (33, 29), hs), axis, (-2.5, -2.0), (su, sv), hs)
    assert same(s2.points, pts) and same(s2.contours, con) and same(s2.layer_first, lf)


def test_empty_program_gives_no_contours(res):
    res.set_limits(LIM)
    res.set_program(0, np.zeros(0, dtype=np.uint32))
    s = res.slice_contours_grid(1, (-1.0, -1.0), (0.1, 0.1), (21, 23), [0.0, 0.5, -0.5], normals=True, ids=True)
    assert s.points.shape == (0, 3) and s.contours.shape == (0, 4) and s.normals.shape == (0, 3) and s.leaf.shape == (0,)
    assert same(s.layer_first, np.zeros(4, np.uint32))
    # ... but a level above max_dist makes every point inside: still no crossing
    s = res.slice_contours_grid(1, (-1.0, -1.0), (0.1, 0.1), (21, 23), [0.0], level=1000.0)
    assert len(s.points) == 0 and same(s.layer_first, np.zeros(2, np.uint32))


# ---- far from the origin, and steps near the coordinates' ulp --------------------------------------------------------------------
def far_cases():
    return dict(list(B.far_lattices().items()) + [("72 step 2^-15 (near ulp)", B.near_ulp_lattice())])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("label", list(far_cases()))
def test_far_lattice_planes(res, label, axis):
    """Planes of the far lattices of tests/test_mesh_bound_cpu.py: coordinates of magnitude 800, steps of 200 ulps down to half an
    ulp, where neighbouring lattice points share a coordinate (a cell of zero width: its two sides carry the same distances, so
    no contour crosses between them and the interpolation never divides by the width)."""
    cc, w = B.far_program()
    origin3, step3, shape3 = far_cases()[label]
    u, v = R.in_plane_axes(axis)
    origin, step, shape = (origin3[u], origin3[v]), (step3[u], step3[v]), (shape3[u], shape3[v])
    along = R.axis_coords(origin3[axis], step3[axis], shape3[axis])
    n = shape3[axis]
    heights = [along[n // 2], along[n // 5], along[n // 2 + 1], along[n - 3]]
    if "ulp" in label:
        cu = R.axis_coords(origin3[0], step3[0], shape3[0])
        assert len(np.unique(cu)) < 0.6 * len(cu)                              # coincident lattice coordinates along x
    res.set_limits(LIM)
    res.set_program(cc, w)
    layers = oracle_layers(cc, w, axis, origin, step, shape, heights)
    n_points = 0
    for level in (0.0, 0.03):
        s = check_slices(res, axis, origin, step, shape, heights, level, layers)
        n_points += len(s.points)
    assert n_points > 0, "no plane meets the surface: the lattice misses it"


# ---- case coverage ---------------------------------------------------------------------------------------------------------
def sphere_soup():
    """The 1200-sphere program of test_gpu_mesh.py test_case_coverage."""
    rng = np.random.default_rng(600)
    n = 40
    step = F(2.0) / F(n - 1)
    words, cc = [], 0
    for s in range(1200):
        c = rng.uniform(-1.0, 1.0, 3).astype(F)
        r = F(rng.uniform(0.4, 1.5) * step)
        words += [0] + [int(x) for x in np.asarray(list(c) + [r], dtype=F).view(np.uint32)]
        cc += 1
        if s > 0:
            words.append(101 if rng.random() < 0.5 else 100)
            cc += 1
    return cc, np.asarray(words, dtype=np.uint32), n, step


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_case_coverage(res, axis):
    cc, w, n, step = sphere_soup()
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, shape = (-1.0, -1.0), (n, n)
    heights = F(-1.0) + np.arange(n, dtype=np.float64).astype(F) * step
    layers = oracle_layers(cc, w, axis, origin, (step, step), shape, heights)
    cases = np.concatenate([R.layer_cases(d).ravel() for d in layers])
    assert np.bincount(cases, minlength=16).min() >= 1            # all 16 cases occur
    s = check_slices(res, axis, origin, (step, step), shape, heights, 0.0, layers)
    closed = int(np.count_nonzero(s.contours[:, 3]))
    print("axis %d: cases at least %d times, %d closed, %d open" % (axis, np.bincount(cases, minlength=16).min(), closed,
                                                                    len(s.contours) - closed))
    assert closed > 100 and len(s.contours) - closed > 10


# ---- open contours ---------------------------------------------------------------------------------------------------------
def test_open_contours(res, oracle):
    cc, w = program(oracle, "g32")
    res.set_limits(LIM)
    res.set_program(cc, w)
    step = F(3.0) / F(127)
    origin, shape, heights = (-1.0, -1.0), (128, 128), [0.1]
    layers = oracle_layers(cc, w, 1, origin, (step, step), shape, heights)
    s = check_slices(res, 1, origin, (step, step), shape, heights, 0.0, layers)
    closed = s.contours[:, 3]
    assert np.any(closed == 0) and np.any(closed == 1)
    # an open contour starts and ends on the lattice's border
    cu = R.axis_coords(-1.0, step, 128)
    for first, count, _, c in s.contours.tolist():
        if not c:
            for p in (s.points[first], s.points[first + count - 1]):
                assert p[2] in (cu[0], cu[-1]) or p[0] in (cu[0], cu[-1])          # axis 1: u = z, v = x


# ---- long chains and batches -------------------------------------------------------------------------------------------------
def test_long_chains_over_batches(res, oracle):
    cc, w = program(oracle, "g1")
    res.set_limits(LIM)
    res.set_program(cc, w)
    n, n_layers = 2049, 40
    step = F(3.0) / F(n - 1)
    origin, shape = (-1.5, -1.5), (n, n)
    assert n * n * n_layers > 1 << 27                               # more than one batch of layers
    heights = (F(-0.9) + np.arange(n_layers, dtype=np.float64).astype(F) * F(1.8 / (n_layers - 1))).astype(F)
    s = res.slice_contours_grid(1, origin, (step, step), shape, heights)
    s2 = res.slice_contours_grid(1, origin, (step, step), shape, heights)          # two runs: identical arrays
    assert same(s2.points, s.points) and same(s2.contours, s.contours) and same(s2.layer_first, s.layer_first)
    pts, cons, lf = [], [], [0]
    for k in range(n_layers):
        d = sampled_layer(res, 1, origin, (step, step), shape, heights[k])
        p, c, _ = R.slice_contours([d], 1, origin, (step, step), [heights[k]])
        # the single call over all layers is the per-layer calls concatenated, indices shifted
        one = res.slice_contours_grid(1, origin, (step, step), shape, [heights[k]])
        assert same(one.points, p) and same(one.contours, c) and same(one.layer_first, np.asarray([0, len(c)], np.uint32))
        c = c.copy()
        c[:, 0] += sum(len(x) for x in pts)
        c[:, 2] = k
        pts.append(p)
        cons.append(c)
        lf.append(lf[-1] + len(c))
    pts, cons = np.concatenate(pts), np.concatenate(cons)
    assert int(cons[:, 1].max()) > 4096, int(cons[:, 1].max())       # ranking needs more than 12 rounds
    assert same(s.points, pts) and same(s.contours, cons) and same(s.layer_first, np.asarray(lf, np.uint32))


# ---- consistency with the mesh -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", ["g32", "xform_mix"])
def test_layers_are_the_mesh_vertices_of_their_lattice_planes(res, oracle, name, axis):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = (-2.5, -2.3, -2.4), (F(0.11), F(0.1), F(0.105)), (45, 47, 46)
    m = res.extract_mesh_grid(origin, step, shape, normals=False, ids=False)
    dist = res.sample_grid(origin, step, shape)
    # the lattice point and the axis of every mesh vertex, in the mesh's vertex order
    inside = dist < F(0.0)
    nx, ny, nz = shape
    cross = np.zeros((nz, ny, nx, 3), dtype=bool)
    cross[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    cross[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    cross[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    p, a = np.nonzero(cross.reshape(-1, 3))
    assert len(p) == len(m.vertices)
    ijk = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], axis=1)
    u, v = R.in_plane_axes(axis)
    heights = MR.axis_coords(origin, step, shape)[axis]
    s = res.slice_contours_grid(axis, (origin[u], origin[v]), (step[u], step[v]), (shape[u], shape[v]), heights)
    assert len(s.points) > 1000

    def rows(x):
        x = np.ascontiguousarray(x, dtype=F)
        return x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))]
    layer_of_point = np.repeat(s.contours[:, 2], s.contours[:, 1])
    for k in range(shape[axis]):
        mine = s.points[layer_of_point == k]
        theirs = m.vertices[(ijk[:, axis] == k) & (a != axis)]
        assert same(rows(mine), rows(theirs)), (name, axis, k)


# ---- attributes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g8", "xform_mix", "mat_mix"])
def test_attributes_are_those_of_the_point_query(res, oracle, name):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    args = (1, (-2.5, -2.5), (F(0.05), F(0.05)), (101, 101), [-0.3, 0.2, 0.6])
    s = res.slice_contours_grid(*args, normals=True, ids=True)
    assert len(s.points) > 200
    q = res.query_points(s.points, normals=True)
    assert same(s.normals, q["normal"]) and same(s.leaf, q["leaf"]) and same(s.material, q["material"])
    a = res.slice_contours_grid(*args, normals=True)
    b = res.slice_contours_grid(*args, ids=True)
    assert a.leaf is None and b.normals is None
    assert same(a.normals, s.normals) and same(b.leaf, s.leaf) and same(b.material, s.material) and same(b.points, s.points)


# ---- orientation -----------------------------------------------------------------------------------------------------------
def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_outer_boundary_counter_clockwise_and_hole_clockwise(res, axis):
    cc, w = words_of((0, [0, 0, 0, 1.0]), (0, [0, 0, 0, 0.5]), (101, []))          # a sphere minus a smaller concentric one
    res.set_limits(LIM)
    res.set_program(cc, w)
    s = res.slice_contours((-1.5,) * 3, (1.5,) * 3, 129, heights=[0.1], axis=axis)
    assert len(s.contours) == 2 and np.all(s.contours[:, 3] == 1)
    areas = sorted(R.shoelace(uv) for uv, closed in s.layer(0))
    assert areas[0] < 0 < areas[1]
    assert abs(areas[1] / (np.pi * 0.99) - 1.0) < 0.01 and abs(-areas[0] / (np.pi * 0.24) - 1.0) < 0.02
    assert abs(s.area(0) / (np.pi * 0.75) - 1.0) < 0.01
    # the outer loop starts at the lowest vertex id, so it comes first
    assert R.shoelace(s.contour(0)[0]) > 0


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_errors(res, oracle):
    import torch
    L = _ffi.hip_lib()
    cc, w = program(oracle, "g8")
    res.set_limits(LIM)
    res.set_program(cc, w)
    f2 = lambda *x: (C.c_float * len(x))(*x)  # noqa: E731
    o, s, h = f2(-2.0, -2.0), f2(0.1, 0.1), f2(0.0, 0.5)
    counts = (C.c_uint64 * 2)()

    def call(axis=1, o=o, s=s, nu=41, nv=41, h=h, nl=2, level=0.0, flags=0, counts=counts, n_counts=2):
        return L.rm_slice_contours(res._h, axis, o, s, nu, nv, h, nl, level, flags, counts, n_counts)
    assert call() == _ffi.RM_OK and counts[0] > 0 and counts[1] > 0
    # NULL pointers
    for kw in (dict(o=None), dict(s=None), dict(h=None), dict(counts=None)):
        assert call(**kw) == _ffi.RM_ERR_NULL, kw
    # dimension limits
    for kw in (dict(nu=1), dict(nv=1), dict(nu=65537, nv=2), dict(nu=8193, nv=8192), dict(nl=0), dict(nl=65537)):
        assert call(**kw) == _ffi.RM_ERR_RANGE, kw
    # arguments
    for kw in (dict(axis=3), dict(n_counts=1), dict(flags=4), dict(level=np.nan), dict(level=np.inf), dict(s=f2(0.1, 0.0)),
               dict(s=f2(-0.1, 0.1)), dict(s=f2(np.inf, 0.1)), dict(s=f2(0.1, np.nan)), dict(o=f2(np.inf, 0.0)), dict(o=f2(0.0, np.nan)),
               dict(h=f2(0.0, np.nan)), dict(h=f2(-np.inf, 0.0))):
        assert call(**kw) == _ffi.RM_ERR_ARG, kw
    # these are refused before anything changes: the earlier result can still be read
    assert L.rm_read_slices(res._h, None, None, None, None, None, 0, None) == _ffi.RM_OK
    # misaligned device arrays, attributes that were not computed
    both = _ffi.RM_MESH_NORMALS | _ffi.RM_MESH_IDS
    assert call(flags=both) == _ffi.RM_OK
    P, Cn = int(counts[0]), int(counts[1])
    buf = torch.empty(P * 3 + 4, dtype=torch.float32, device="cuda:0")
    ids = torch.empty(max(P * 2, Cn * 4) + 8, dtype=torch.int32, device="cuda:0")
    assert L.rm_read_slices(res._h, buf.data_ptr() + 2, None, None, None, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, None, ids.data_ptr() + 8, None, None, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, None, None, ids.data_ptr() + 2, None, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, None, None, None, buf.data_ptr() + 1, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, None, None, None, None, ids.data_ptr() + 4, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, None, None, ids.data_ptr() + 4, None, None, 1, None) == _ffi.RM_OK
    assert L.rm_read_slices(res._h, None, None, None, None, ids.data_ptr(), 1, None) == _ffi.RM_OK
    assert call(flags=_ffi.RM_MESH_NORMALS) == _ffi.RM_OK
    assert L.rm_read_slices(res._h, None, None, None, None, ids.data_ptr(), 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_slices(res._h, buf.data_ptr(), None, None, buf.data_ptr(), None, 1, None) == _ffi.RM_OK
    assert call() == _ffi.RM_OK
    assert L.rm_read_slices(res._h, None, None, None, buf.data_ptr(), None, 1, None) == _ffi.RM_ERR_ARG
    torch.cuda.synchronize()
    # reading before any slice call
    fresh = renderer.RayMarchingResources(0)
    try:
        v = np.empty(12, dtype=np.float32)
        assert L.rm_read_slices(fresh._h, v.ctypes.data, None, None, None, None, 0, None) == _ffi.RM_ERR_ARG
    finally:
        fresh.close()
    # max_iter beyond 65536
    res.set_limits((0.01, 100.0, 65537))
    assert call() == _ffi.RM_ERR_RANGE
    res.set_limits(LIM)
    # an invalid program: the status a draw gives
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    with pytest.raises(_ffi.RmError) as draw_error:
        res.draw(16, 16)
    assert draw_error.value.status == _ffi.RM_ERR_STACK_UNDERFLOW
    assert call() == draw_error.value.status
    # ... which, like the limits, is refused before the previous result is touched
    assert L.rm_read_slices(res._h, None, None, None, None, None, 0, None) == _ffi.RM_OK


# ---- device reads ------------------------------------------------------------------------------------------------------------
def test_device_reads(res, oracle):
    import torch
    cc, w = program(oracle, "mat_mix")
    res.set_limits(LIM)
    res.set_program(cc, w)
    args = (2, (-2.5, -2.5), (F(0.04), F(0.04)), (126, 126), [0.3, -0.2])
    host = res.slice_contours_grid(*args, normals=True, ids=True)
    dev = res.slice_contours_grid(*args, normals=True, ids=True, device=True)
    torch.cuda.synchronize()
    assert dev.points.device.type == "cuda" and dev.contours.dtype == torch.int32
    d = dev.numpy()
    assert same(d.points, host.points) and same(d.contours, host.contours) and same(d.layer_first, host.layer_first)
    assert same(d.normals, host.normals) and same(d.leaf, host.leaf) and same(d.material, host.material)
    assert len(d.layer(1)) == len(host.layer(1)) and d.area(0) == host.area(0)
    # a read on another stream is ordered before the next slice call
    pts = torch.empty((len(host.points), 3), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res.read_slices_device(points_ptr=pts.data_ptr(), stream=st.cuda_stream)
        other = res.slice_contours_grid(0, (-2.0, -2.0), (0.1, 0.1), (41, 41), [0.0])
    st.synchronize()
    assert same(pts.cpu().numpy(), host.points)
    assert len(other.points) > 0


# ---- isolation -----------------------------------------------------------------------------------------------------------
def test_slicing_leaves_draws_and_the_mesh_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 2)
    res.set_option(_ffi.RM_OPT_TIMING, 1)
    first = res.draw(W, H)
    keys = (_ffi.RM_INFO_SPECIALIZED, _ffi.RM_INFO_JIT_STATE, _ffi.RM_INFO_INTERPRETER_LOOP, _ffi.RM_INFO_PRUNED)
    before = [res.info(k) for k in keys]
    ms = res.info(_ffi.RM_INFO_KERNEL_MS)
    assert ms > 0
    m = res.extract_mesh_grid((-3.0,) * 3, (F(6.0) / F(39),) * 3, (40, 40, 40))
    s = res.slice_contours((-3.0,) * 3, (3.0,) * 3, 257, layer_height=0.25, axis=1, normals=True, ids=True)
    assert len(s.contours) > 10
    assert [res.info(k) for k in keys] == before
    assert res.info(_ffi.RM_INFO_KERNEL_MS) == ms      # the slice call was not timed: nothing new to average
    assert res.draw(W, H).tobytes() == first.tobytes()
    res.set_option(_ffi.RM_OPT_TIMING, 0)
    res.set_option(_ffi.RM_OPT_SPECIALIZE, 1)
    # the mesh extracted before the slice call reads back unchanged
    V, T = len(m.vertices), len(m.triangles)
    v = np.empty((V, 3), dtype=np.float32)
    t = np.empty((T, 3), dtype=np.uint32)
    nrm = np.empty((V, 3), dtype=np.float32)
    ids = np.empty((V, 2), dtype=np.uint32)
    res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, nrm.ctypes.data, ids.ctypes.data, 0, None))
    assert same(v, m.vertices) and same(t, m.triangles) and same(nrm, m.normals) and same(ids[:, 0], m.leaf)
    # ... and a mesh extraction does not touch the slices
    res.extract_mesh_grid((-3.0,) * 3, (F(6.0) / F(31),) * 3, (32, 32, 32))
    pts = np.empty((len(s.points), 3), dtype=np.float32)
    con = np.empty((len(s.contours), 4), dtype=np.uint32)
    res._check(res._L.rm_read_slices(res._h, pts.ctypes.data, con.ctypes.data, None, None, None, 0, None))
    assert same(pts, s.points) and same(con, s.contours)
