"""Mesh export on the GPU (rm_sample_grid / rm_extract_mesh / rm_read_mesh) against the oracle and the numpy restatement
of the contract (tests/mesh_ref.py), bit for bit: lattice distances for every scene, vertices and triangles on the chain,
tree and general record loops, case coverage, a lattice of many scan blocks, the per-vertex attributes, topology, lattices
far from the origin with steps down to the coordinates' ulp (and the distances there against a binary64 evaluation), errors,
and isolation from the draws."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as R
import scene_f64
import scenes
import sparse_ref
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


def oracle_taps_normal(cc, words, max_dist, p):
    eps = F(0.0001)
    f = [onp.map_scene(cc, words, max_dist, p[:, 0] + F(kx) * eps, p[:, 1] + F(ky) * eps, p[:, 2] + F(kz) * eps)
         for kx, ky, kz in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1))]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx = ((f[0] + -f[1]) + -f[2]) + f[3]
        ny = ((-f[0] + -f[1]) + f[2]) + f[3]
        nz = ((-f[0] + f[1]) + -f[2]) + f[3]
        nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
        return np.stack([nx / nl, ny / nl, nz / nl], axis=1)


def oracle_grid(cc, w, origin, step, shape, max_dist=LIM[1]):
    p = R.lattice_points(origin, step, shape)
    with np.errstate(all="ignore"):
        d = onp.map_scene(cc, w, F(max_dist), p[:, 0], p[:, 1], p[:, 2])
    return np.asarray(d, dtype=F).reshape(shape[2], shape[1], shape[0])


def program(oracle, name):
    if name == "empty":
        return 0, np.zeros(0, dtype=np.uint32)
    return oracle.serialize(*ALL_SCENES[name]())


def cube(n, lo=-3.0, hi=3.0):
    return (lo,) * 3, (F(hi - lo) / F(n - 1),) * 3, (n, n, n)


# ---- lattice distances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_SCENES) + ["empty"])
def test_sample_grid_vs_oracle(res, oracle, name):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    shape = (41, 37, 29)
    for origin, step in (((-3.0, -2.5, -2.0), (0.15, 0.14, 0.15)), ((-1.0, -1.0, -1.0), (F(2) / F(40), 0.0625, 0.07)),
                         ((0.3, -7.0, 1e-3), (0.01, 0.4, 0.123))):
        d = res.sample_grid(origin, step, shape)
        assert d.shape == (29, 37, 41)
        assert same(d, oracle_grid(cc, w, origin, step, shape)), (name, origin, step)
    if cc == 0:
        assert np.all(d == F(LIM[1]))


def test_sample_grid_device_and_max_dist(res, oracle):
    import torch
    cc, w = program(oracle, "xform_mix")
    origin, step, shape = (-2.0, -2.0, -2.0), (0.1, 0.1, 0.1), (41, 37, 29)
    for lim in ((0.01, 2.5, 64), LIM):
        res.set_limits(lim)
        res.set_program(cc, w)
        ref = oracle_grid(cc, w, origin, step, shape, lim[1])
        out = torch.empty(41 * 37 * 29, dtype=torch.float32, device="cuda:0")
        assert res.sample_grid(origin, step, shape, out=out) is out
        torch.cuda.synchronize()
        assert same(out.cpu().numpy().reshape(29, 37, 41), ref), lim
        assert same(res.sample_grid(origin, step, shape), ref), lim
    with pytest.raises(ValueError):
        res.sample_grid(origin, step, shape, out=torch.empty(10, dtype=torch.float32, device="cuda:0"))


# ---- extraction against the restatement ------------------------------------------------------------------------------------
def check_mesh(res, cc, w, origin, step, shape, level=0.0, dist=None):
    if dist is None:
        dist = oracle_grid(cc, w, origin, step, shape)
    v, t = R.extract(dist, origin, step, level)
    m = res.extract_mesh_grid(origin, step, shape, level=level, normals=False, ids=False)
    assert same(m.vertices, v)
    assert same(m.triangles, t)
    return m, v, t


@pytest.mark.parametrize("name", MESH_SCENES)
def test_extract_mesh_vs_restatement(res, oracle, name):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = cube(64)
    dist = oracle_grid(cc, w, origin, step, shape)
    m, v, t = check_mesh(res, cc, w, origin, step, shape, dist=dist)
    assert len(t) > 1000, len(t)
    # through extract_mesh (lo, hi, resolution): the same lattice
    m2 = res.extract_mesh((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0), 64, normals=False, ids=False)
    assert same(m2.vertices, v) and same(m2.triangles, t)
    check_mesh(res, cc, w, origin, step, shape, level=0.05, dist=dist)


# ---- far from the origin, and steps near the coordinates' ulp --------------------------------------------------------------------
def far_cases():
    return dict(list(B.far_lattices().items()) + [("72 step 2^-15 (near ulp)", B.near_ulp_lattice())])


@pytest.mark.parametrize("label", list(far_cases()))
def test_far_from_the_origin_and_fine_steps(res, label):
    """Coordinates of magnitude 800 with steps of 200 ulps down to half an ulp (lattice points that share a coordinate):
    rm_sample_grid is the oracle bit for bit, every distance is within rm_program_bound's E of the binary64 value (DESIGN.md
    section 15 "The evaluation error", on the kernel's own evaluation), and the mesh is the restatement's."""
    cc, w = B.far_program()
    origin, step, shape = far_cases()[label]
    res.set_limits(LIM)
    res.set_program(cc, w)
    dist = oracle_grid(cc, w, origin, step, shape)
    d = res.sample_grid(origin, step, shape)
    assert same(d, dist), label
    L, E = B.program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
    p = R.lattice_points(origin, step, shape)
    assert np.abs(p).max() <= sparse_ref.lattice_P(origin, step, shape)
    err = np.abs(d.ravel().astype(np.float64) - scene_f64.map_scene(cc, w, LIM[1], p))
    print("%s: largest |gpu - f64| %.3g, E %.3g, ratio %.4f" % (label, float(err.max()), E, float(err.max() / E)))
    assert np.all(np.isfinite(err)) and np.all(err <= E), (label, float(err.max()), E)
    assert len(R.extract(dist, origin, step, 0.0)[1]) > 0, "the restatement finds no surface: the lattice misses it"
    for level in (0.0, 0.03):
        check_mesh(res, cc, w, origin, step, shape, level=level, dist=dist)


@pytest.mark.parametrize("name", ["g32", "g32_balanced", "xform_mix"])
def test_extract_mesh_on_odd_lattices(res, oracle, name):
    # nx not a multiple of a thread's 8 points: runs of points wrap into the next row and the next k-plane mid-thread
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    for origin, step, shape in (((-3.0, -2.5, -2.0), (0.15, 0.14, 0.15), (41, 37, 29)),
                                ((-2.5, -0.35, -2.5), (0.3, 0.3, 0.3), (17, 3, 19)),
                                ((-2.5, -2.5, -2.5), (0.08, 1.25, 0.09), (63, 5, 57)),
                                cube(63)):
        m, v, t = check_mesh(res, cc, w, origin, step, shape)
        assert len(t) > 0, (name, shape)


def test_case_coverage(res):
    rng = np.random.default_rng(600)
    n, origin = 40, (-1.0, -1.0, -1.0)
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
    w = np.asarray(words, dtype=np.uint32)
    res.set_limits(LIM)
    res.set_program(cc, w)
    shape = (n, n, n)
    dist = oracle_grid(cc, w, origin, (step,) * 3, shape)
    check_mesh(res, cc, w, origin, (step,) * 3, shape, dist=dist)
    inside = dist < 0
    case = np.zeros((n - 1,) * 3, dtype=np.int64)
    for c in range(8):
        ox, oy, oz = R.corner_pos(c)
        case |= inside[oz:oz + n - 1, oy:oy + n - 1, ox:ox + n - 1].astype(np.int64) << c
    assert len(np.unique(case)) >= 150, len(np.unique(case))


def test_many_scan_blocks(res, oracle):
    cc, w = program(oracle, "g32")
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = (-2.5,) * 3, (F(5.0) / F(255),) * 3, (256, 256, 256)
    dist = res.sample_grid(origin, step, shape)
    m, v, t = check_mesh(res, cc, w, origin, step, shape, dist=dist)
    assert len(t) > 100000
    m2 = res.extract_mesh_grid(origin, step, shape, normals=False, ids=False)   # two runs: identical arrays
    assert same(m2.vertices, m.vertices) and same(m2.triangles, m.triangles)


@pytest.mark.parametrize("name", ["g8", "g32", "xform_mix", "mat_mix"])
def test_attributes_are_those_of_the_point_query(res, oracle, name):
    cc, w = program(oracle, name)
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = cube(48)
    m = res.extract_mesh_grid(origin, step, shape)
    q = res.query_points(m.vertices, normals=True)
    assert same(m.normals, q["normal"]) and same(m.leaf, q["leaf"]) and same(m.material, q["material"])
    sub = m.vertices[::5]
    assert same(m.normals[::5], oracle_taps_normal(cc, w, F(LIM[1]), sub))
    # each attribute alone, and the device path
    import torch
    a = res.extract_mesh_grid(origin, step, shape, normals=True, ids=False)
    b = res.extract_mesh_grid(origin, step, shape, normals=False, ids=True)
    assert a.leaf is None and b.normals is None
    assert same(a.normals, m.normals) and same(b.material, m.material) and same(b.leaf, m.leaf)
    d = res.extract_mesh_grid(origin, step, shape, device=True)
    torch.cuda.synchronize()
    assert d.vertices.device.type == "cuda"
    dn = d.numpy()
    assert same(dn.vertices, m.vertices) and same(dn.triangles, m.triangles) and same(dn.normals, m.normals)
    assert same(dn.leaf.view(np.uint32), m.leaf) and same(dn.material.view(np.uint32), m.material)


# ---- topology on programs built here ---------------------------------------------------------------------------------------
def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


def test_sphere_topology(res):
    cc, w = words_of((0, [0, 0, 0, 1.0]))
    res.set_limits(LIM)
    res.set_program(cc, w)
    m = res.extract_mesh((-1.5,) * 3, (1.5,) * 3, 97, normals=False, ids=False)
    assert R.is_closed_manifold(m.triangles) and R.euler_characteristic(m.triangles) == 2
    assert m.is_closed()
    vol = R.signed_volume(m.vertices, m.triangles)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi) - 1.0) < 0.005


def test_box_minus_cylinder_topology(res):
    cc, w = words_of((1, [0, 0, 0, 1.0, 0.6, 0.8]), (10, [0, 0, 0, 0.35, 1.0]), (101, []))
    res.set_limits(LIM)
    res.set_program(cc, w)
    m = res.extract_mesh((-1.4,) * 3, (1.4,) * 3, 81, normals=False, ids=False)
    assert R.directed_edges_balance(m.triangles)
    assert R.euler_characteristic(m.triangles) == 0


# ---- errors -------------------------------------------------------------------------------------------------------------
def lattice(o=(0.0, 0.0, 0.0), s=(0.1, 0.1, 0.1)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


def test_errors(res, oracle):
    import torch
    L = _ffi.hip_lib()
    cc, w = program(oracle, "g8")
    res.set_limits(LIM)
    res.set_program(cc, w)
    o, s = lattice()
    counts = (C.c_uint64 * 2)()
    out = torch.empty(64 * 64 + 1, dtype=torch.float32, device="cuda:0")
    # dimension limits
    for nx, ny, nz in ((1, 4, 4), (4, 4, 1), (65537, 2, 2), (1024, 1024, 257)):
        assert L.rm_extract_mesh(res._h, o, s, nx, ny, nz, 0.0, 0, counts) == _ffi.RM_ERR_RANGE, (nx, ny, nz)
    for nx, ny, nz in ((0, 4, 4), (65537, 1, 1), (65536, 65536, 1)):
        assert L.rm_sample_grid(res._h, o, s, nx, ny, nz, out.data_ptr(), 1, None) == _ffi.RM_ERR_RANGE, (nx, ny, nz)
    # steps, non-finite inputs
    for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
        o2, s2 = lattice(s=bad)
        assert L.rm_extract_mesh(res._h, o2, s2, 4, 4, 4, 0.0, 0, counts) == _ffi.RM_ERR_ARG, bad
        assert L.rm_sample_grid(res._h, o2, s2, 4, 4, 4, out.data_ptr(), 1, None) == _ffi.RM_ERR_ARG, bad
    o2, s2 = lattice(o=(0.0, np.inf, 0.0))
    assert L.rm_extract_mesh(res._h, o2, s2, 4, 4, 4, 0.0, 0, counts) == _ffi.RM_ERR_ARG
    assert L.rm_sample_grid(res._h, o2, s2, 4, 4, 4, out.data_ptr(), 1, None) == _ffi.RM_ERR_ARG
    for level in (np.nan, np.inf):
        assert L.rm_extract_mesh(res._h, o, s, 4, 4, 4, level, 0, counts) == _ffi.RM_ERR_ARG
    assert L.rm_extract_mesh(res._h, o, s, 4, 4, 4, 0.0, 4, counts) == _ffi.RM_ERR_ARG      # unknown flag
    # misaligned device arrays
    assert L.rm_sample_grid(res._h, o, s, 8, 8, 8, out.data_ptr() + 2, 1, None) == _ffi.RM_ERR_ARG
    o3, s3 = lattice((-2.0, -2.0, -2.0), (0.25, 0.25, 0.25))
    both = _ffi.RM_MESH_NORMALS | _ffi.RM_MESH_IDS
    assert L.rm_extract_mesh(res._h, o3, s3, 17, 17, 17, 0.0, both, counts) == _ffi.RM_OK
    V = int(counts[0])
    assert V > 0
    buf = torch.empty(V * 3 + 4, dtype=torch.float32, device="cuda:0")
    ids = torch.empty(V * 2 + 2, dtype=torch.int32, device="cuda:0")
    assert L.rm_read_mesh(res._h, buf.data_ptr() + 2, None, None, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_mesh(res._h, buf.data_ptr(), None, buf.data_ptr() + 1, None, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_mesh(res._h, None, None, None, ids.data_ptr() + 4, 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_mesh(res._h, None, None, None, ids.data_ptr(), 1, None) == _ffi.RM_OK
    # attributes the extraction did not compute
    assert L.rm_extract_mesh(res._h, o3, s3, 17, 17, 17, 0.0, _ffi.RM_MESH_NORMALS, counts) == _ffi.RM_OK
    assert L.rm_read_mesh(res._h, None, None, None, ids.data_ptr(), 1, None) == _ffi.RM_ERR_ARG
    assert L.rm_read_mesh(res._h, buf.data_ptr(), None, buf.data_ptr(), None, 1, None) == _ffi.RM_OK
    assert L.rm_extract_mesh(res._h, o3, s3, 17, 17, 17, 0.0, 0, counts) == _ffi.RM_OK
    assert L.rm_read_mesh(res._h, None, None, buf.data_ptr(), None, 1, None) == _ffi.RM_ERR_ARG
    torch.cuda.synchronize()
    # reading before any extraction
    fresh = renderer.RayMarchingResources(0)
    try:
        v = np.empty(12, dtype=np.float32)
        assert L.rm_read_mesh(fresh._h, v.ctypes.data, None, None, None, 0, None) == _ffi.RM_ERR_ARG
    finally:
        fresh.close()
    # an invalid program: the status a draw gives
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    with pytest.raises(_ffi.RmError) as draw_error:
        res.draw(16, 16)
    assert draw_error.value.status == _ffi.RM_ERR_STACK_UNDERFLOW
    assert L.rm_extract_mesh(res._h, o3, s3, 17, 17, 17, 0.0, 0, counts) == draw_error.value.status
    assert L.rm_sample_grid(res._h, o3, s3, 4, 4, 4, out.data_ptr(), 1, None) == draw_error.value.status


# ---- isolation -----------------------------------------------------------------------------------------------------------
def test_extraction_leaves_draws_and_meshes_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    first = res.draw(W, H)
    origin, step, shape = cube(40)
    m = res.extract_mesh_grid(origin, step, shape)
    assert res.draw(W, H).tobytes() == first.tobytes()
    # a later program change does not touch the extracted mesh
    cc2, w2 = program(oracle, "g8")
    res.set_program(cc2, w2)
    V, T = len(m.vertices), len(m.triangles)
    v = np.empty((V, 3), dtype=np.float32)
    t = np.empty((T, 3), dtype=np.uint32)
    nrm = np.empty((V, 3), dtype=np.float32)
    ids = np.empty((V, 2), dtype=np.uint32)
    res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, nrm.ctypes.data, ids.ctypes.data, 0, None))
    assert same(v, m.vertices) and same(t, m.triangles) and same(nrm, m.normals) and same(ids[:, 1], m.material)
    # ... and a device read on another stream is ordered before the next extraction
    import torch
    dv = torch.empty((V, 3), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        res.read_mesh_device(vertices_ptr=dv.data_ptr(), stream=s.cuda_stream)
        m2 = res.extract_mesh_grid(origin, step, shape, normals=False, ids=False)
    s.synchronize()
    assert same(dv.cpu().numpy(), m.vertices)
    assert len(m2.vertices) > 0
