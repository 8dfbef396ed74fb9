"""Sparse mesh extraction on the GPU (rm_extract_mesh_sparse): its arrays against the numpy restatement
of the mesh contract (tests/mesh_ref.py on the oracle's lattice) and against the dense extraction, bit for bit; odd shapes;
programs without a usable bound; random programs; a lattice beyond the dense limit; that culling really culls; which bricks
are kept, against the numpy model of the skipping rule (tests/sparse_ref.py), exactly; lattices far from the origin with steps
down to the coordinates' ulp; errors and isolation."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as R
import scenes
import sparse_ref
import test_gpu_fuzz
import test_mesh_bound_cpu as B
from oracle import rm_oracle_np as onp
from ray_marching_amd import _ffi, renderer

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = dict(list(scenes.SCENES.items()) + list(scenes.EXT_SCENES.items()) + list(scenes.MAT_SCENES.items()))
MESH_SCENES = ("g1", "g8", "g32", "g32_balanced", "g8x", "g32s", "ext_mix", "xform_mix", "mat_mix")
LIM = (0.01, 100.0, 256)
BRICK = 8


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


def same_mesh(a, b):
    return (same(a.vertices, b.vertices) and same(a.triangles, b.triangles) and same(a.normals, b.normals)
            and same(a.leaf, b.leaf) and same(a.material, b.material))


def oracle_grid(cc, w, origin, step, shape, max_dist=LIM[1]):
    p = R.lattice_points(origin, step, shape)
    with np.errstate(all="ignore"):
        d = onp.map_scene(cc, w, F(max_dist), p[:, 0], p[:, 1], p[:, 2])
    return np.asarray(d, dtype=F).reshape(shape[2], shape[1], shape[0])


def cube(n, lo=-3.0, hi=3.0):
    return (lo,) * 3, (F(hi - lo) / F(n - 1),) * 3, (n, n, n)


def words_of(*cmds):
    out = []
    for op, params in cmds:
        out += [op] + [int(x) for x in np.asarray(params, dtype=F).view(np.uint32)]
    return len(cmds), np.asarray(out, dtype=np.uint32)


def check_stats(m, shape):
    s = m.stats
    assert s["vertices"] == len(m.vertices) and s["triangles"] == len(m.triangles)
    assert s["bricks"] == int(np.prod([(n + BRICK - 1) // BRICK for n in shape]))
    assert s["bricks_kept"] <= s["bricks"]
    assert s["bricks"] <= s["evaluations"] <= s["bricks"] + s["bricks_kept"] * (BRICK + 1) ** 3
    return s


def check_vs_restatement(res, cc, w, origin, step, shape, level=0.0, dist=None):
    if dist is None:
        dist = oracle_grid(cc, w, origin, step, shape)
    v, t = R.extract(dist, origin, step, level)
    m = res.extract_mesh_grid_sparse(origin, step, shape, level=level, normals=False, ids=False)
    print("sparse %s level %g: %s" % (shape, level, m.stats))
    assert same(m.vertices, v), "vertices differ from the restatement"
    assert same(m.triangles, t), "triangles differ from the restatement"
    check_stats(m, shape)
    return m


# ---- equality with the restatement and with the dense extraction --------------------------------------------------------------
@pytest.mark.parametrize("name", MESH_SCENES)
def test_sparse_equals_restatement_and_dense(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = cube(96)
    dist = oracle_grid(cc, w, origin, step, shape)
    for level in (0.0, 0.05):
        m = check_vs_restatement(res, cc, w, origin, step, shape, level, dist)
        assert len(m.triangles) > 1000
        assert m.stats["bricks_kept"] < m.stats["bricks"], "culling was not active"
        dense = res.extract_mesh_grid(origin, step, shape, level=level)
        sparse = res.extract_mesh_grid_sparse(origin, step, shape, level=level)
        assert same_mesh(sparse, dense), (name, level)
    # through extract_mesh_sparse (lo, hi, resolution): the same lattice
    m2 = res.extract_mesh_sparse((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0), 96, level=0.05)
    assert same_mesh(m2, dense)


@pytest.mark.parametrize("name", ["g32", "xform_mix"])
def test_odd_shapes(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    for origin, step, shape in (((-0.2, 0.1, -0.3), (0.6, 0.5, 0.7), (2, 2, 2)),
                                ((-1.0, -2.1, -0.2), (0.9, 0.55, 0.7), (3, 9, 2)),
                                ((-3.0, -0.35, -2.0), (0.1, 0.12, 0.031), (61, 7, 130)),
                                ((-3.0, -2.5, -2.0), (0.15, 0.14, 0.15), (4 * BRICK + 1, 5 * BRICK + 1, 3 * BRICK + 1)),
                                ((0.3, -7.0, 1e-3), (0.01, 0.4, 0.123), (41, 37, 29))):
        check_vs_restatement(res, cc, w, origin, step, shape)
        assert same_mesh(res.extract_mesh_grid_sparse(origin, step, shape), res.extract_mesh_grid(origin, step, shape)), shape


@pytest.mark.parametrize("name", ["g32", "mat_mix"])
def test_equals_dense_at_size(res, oracle, name):
    cc, w = oracle.serialize(*ALL_SCENES[name]())
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = cube(320)
    dense = res.extract_mesh_grid(origin, step, shape)
    sparse = res.extract_mesh_grid_sparse(origin, step, shape)
    print("320^3 %s: %s" % (name, sparse.stats))
    assert len(dense.triangles) > 100000
    assert same_mesh(sparse, dense)
    assert check_stats(sparse, shape)["bricks_kept"] < sparse.stats["bricks"] // 4


# ---- programs without a usable bound ----------------------------------------------------------------------------------------
def unbounded_programs():
    sphere, box = (0, [0.2, 0.1, -0.1, 0.9]), (1, [-0.4, 0.0, 0.3, 0.5, 0.6, 0.4])
    h = 0.5
    return {
        "scale 0": words_of(sphere, (204, [0.0]), box, (205, []), (100, [])),
        "negative scale": words_of(sphere, (204, [-0.7]), box, (205, []), (100, [])),
        "non-unit quaternion": words_of(sphere, (202, [1.3, 0.2, -0.4, h]), box, (203, []), (100, [])),
        "steep plane": words_of(sphere, (2, [30.0, 40.0, 0.0, 5.0]), (102, [])),
        "empty": (0, np.zeros(0, dtype=np.uint32)),
    }


@pytest.mark.parametrize("label", sorted(unbounded_programs()))
def test_programs_without_a_usable_bound(res, label):
    cc, w = unbounded_programs()[label]
    res.set_limits(LIM)
    res.set_program(cc, w)
    origin, step, shape = cube(56, -2.0, 2.0)
    m = check_vs_restatement(res, cc, w, origin, step, shape)
    L = renderer.program_lipschitz(cc, w)
    print(label, "L =", L)
    if np.isinf(L):
        assert m.stats["bricks_kept"] == m.stats["bricks"]
    if label == "empty":
        assert len(m.vertices) == 0 and len(m.triangles) == 0
    assert same_mesh(res.extract_mesh_grid_sparse(origin, step, shape), res.extract_mesh_grid(origin, step, shape))


# ---- random programs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_fuzz_against_the_restatement(res, oracle, seed):
    rng = np.random.default_rng(7000 + seed)
    t = scenes._Tab()
    root = test_gpu_fuzz.random_tree(rng, t, int(rng.integers(1, 5)), allow_plane=bool(rng.random() < 0.4), tags=True)
    cc, w = oracle.serialize(t.nodes, root)
    if oracle.validate(cc, w)[0] != 0:
        pytest.fail("seed %d does not give a valid program: pick another" % seed)
    res.set_limits(LIM)
    res.set_program(cc, w)
    res.set_materials(rng.uniform(0.0, 1.0, (8, 3)).astype(np.float32))     # the tags name indices up to 7
    try:
        origin, step, shape = cube(72)
        level = float(rng.choice([0.0, 0.03, -0.02]))
        check_vs_restatement(res, cc, w, origin, step, shape, level)
        assert same_mesh(res.extract_mesh_grid_sparse(origin, step, shape, level=level),
                         res.extract_mesh_grid(origin, step, shape, level=level))
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)


# ---- which bricks are kept -------------------------------------------------------------------------------------------------------
def fuzz_program(oracle, seed):
    """The program of test_fuzz_against_the_restatement's seed."""
    rng = np.random.default_rng(7000 + seed)
    t = scenes._Tab()
    root = test_gpu_fuzz.random_tree(rng, t, int(rng.integers(1, 5)), allow_plane=bool(rng.random() < 0.4), tags=True)
    return oracle.serialize(t.nodes, root)


def kept_cases():
    far = [("far " + label, 0.0) for label in B.far_lattices()]
    return far + [(name, level) for name in ("g32", "xform_mix") for level in (0.0, 0.05)] + [("fuzz 7", 0.0), ("fuzz 10", 0.03)]


@pytest.mark.parametrize("what, level", kept_cases())
def test_kept_bricks_equal_the_model(res, oracle, what, level):
    """BRICKS_KEPT and EVALUATIONS are those of tests/sparse_ref.py, exactly: the probe's distance is the oracle's bit for bit, the
    lattice coordinates are single binary32 operations, and the radius, the margin and the two comparisons are IEEE binary64
    operations (correctly rounded sqrt, no contraction) in one fixed order on both sides, so there is nothing to tolerate.  Fails
    when the probe ignores 2 E, drops `2 E <= L r / 2`, sizes a border tile's radius like a full tile's, or when P is formed
    differently (E scales with P)."""
    if what.startswith("far "):
        cc, w = B.far_program()
        origin, step, shape = B.far_lattices()[what[4:]]
    else:
        cc, w = fuzz_program(oracle, int(what[5:])) if what.startswith("fuzz ") else oracle.serialize(*ALL_SCENES[what]())
        origin, step, shape = cube(72)
    res.set_limits(LIM)
    res.set_program(cc, w)
    res.set_materials(np.full((8, 3), 0.5, dtype=np.float32))                 # the fuzz programs' tags name indices up to 7
    try:
        m = res.extract_mesh_grid_sparse(origin, step, shape, level=level, normals=False, ids=False)
    finally:
        res.set_materials(scenes.MATERIAL_TABLE)
    L, E = B.program_bound(cc, w, sparse_ref.lattice_P(origin, step, shape))
    assert np.isfinite(L) and np.isfinite(E)
    keep, evaluations = sparse_ref.brick_model(cc, w, origin, step, shape, level, L, E, max_dist=LIM[1])
    s = check_stats(m, shape)
    print("%s level %g: L = %.9g, E = %.3g; kept %d of %d bricks (model %d), %d evaluations (model %d)"
          % (what, level, L, E, s["bricks_kept"], s["bricks"], int(np.count_nonzero(keep)), s["evaluations"], evaluations))
    assert s["bricks"] == keep.size
    assert s["bricks_kept"] == int(np.count_nonzero(keep))
    assert s["evaluations"] == evaluations


# ---- far from the origin, and steps near the coordinates' ulp --------------------------------------------------------------------
def far_cases():
    return dict(list(B.far_lattices().items()) + [("72 step 2^-15 (near ulp)", B.near_ulp_lattice())])


@pytest.mark.parametrize("label", list(far_cases()))
def test_far_from_the_origin_and_fine_steps(res, label):
    """Coordinates of magnitude 800 with steps of 200 ulps down to half an ulp (lattice points that share a coordinate): the sparse
    mesh is the restatement's on the oracle's lattice, and the dense mesh is the sparse one, attributes included."""
    cc, w = B.far_program()
    origin, step, shape = far_cases()[label]
    res.set_limits(LIM)
    res.set_program(cc, w)
    dist = oracle_grid(cc, w, origin, step, shape)
    if "ulp" in label:
        xs = R.axis_coords(origin, step, shape)[0]
        assert len(np.unique(xs)) < 0.6 * len(xs)                              # coincident lattice coordinates
    assert len(R.extract(dist, origin, step, 0.0)[1]) > 0, "the restatement finds no surface: the lattice misses it"
    for level in (0.0, 0.03):
        m = check_vs_restatement(res, cc, w, origin, step, shape, level, dist)
        dense = res.extract_mesh_grid(origin, step, shape, level=level)
        sparse = res.extract_mesh_grid_sparse(origin, step, shape, level=level)
        assert same(sparse.vertices, m.vertices) and same(sparse.triangles, m.triangles)
        assert same_mesh(sparse, dense), (label, level)
        if "2^-8" in label or "ulp" in label:                                  # 2 E > L r / 2: nothing may be skipped
            assert sparse.stats["bricks_kept"] == sparse.stats["bricks"]


# ---- beyond the dense limit ---------------------------------------------------------------------------------------------------
def euler_characteristic(tris):
    t = np.asarray(tris, dtype=np.int64)
    n = int(t.max()) + 1
    lo, hi = np.minimum(t, np.roll(t, -1, axis=1)), np.maximum(t, np.roll(t, -1, axis=1))
    return len(np.unique(t)) - len(np.unique((lo * n + hi).ravel())) + len(t)


def triangle_keys(vertices, triangles):
    """Each triangle as the 36 bytes of its corners' positions."""
    p = np.ascontiguousarray(np.asarray(vertices, dtype=F)[np.asarray(triangles, dtype=np.int64)]).view(np.uint32).reshape(len(triangles), 9)
    return {row.tobytes() for row in p}


def test_beyond_the_dense_limit(res, oracle):
    cc, w = oracle.serialize(*scenes.g32())
    res.set_limits(LIM)
    res.set_program(cc, w)
    n, origin, step = 1281, (-2.5,) * 3, (F(2.0) ** -8,) * 3
    counts = (C.c_uint64 * 2)()
    o, s = (C.c_float * 3)(*origin), (C.c_float * 3)(*step)
    assert res._L.rm_extract_mesh(res._h, o, s, n, n, n, 0.0, 0, counts) == _ffi.RM_ERR_RANGE      # the dense call refuses it
    m = res.extract_mesh_grid_sparse(origin, step, (n, n, n), normals=False, ids=False)
    print("1281^3 g32:", m.stats)
    check_stats(m, (n, n, n))
    assert len(m.triangles) > 2000000
    assert m.is_closed()
    dense = res.extract_mesh((-2.5,) * 3, (2.5,) * 3, 512, normals=False, ids=False)
    assert euler_characteristic(m.triangles) == euler_characteristic(dense.triangles)
    again = res.extract_mesh_grid_sparse(origin, step, (n, n, n), normals=False, ids=False)
    assert same(again.vertices, m.vertices) and same(again.triangles, m.triangles)
    assert again.stats == m.stats
    # sub-lattices whose origins are lattice points (all positions exact): the restatement there is the big mesh there
    rng = np.random.default_rng(1281)
    sub, st = 41, float(step[0])
    for _ in range(8):
        v = m.vertices[int(rng.integers(0, len(m.vertices)))]
        first = np.clip(np.floor((v.astype(np.float64) + 2.5) / st).astype(np.int64) - int(rng.integers(8, 32)), 0, n - sub)
        so = tuple(F(-2.5 + int(i) * st) for i in first)
        hi = [float(so[a]) + (sub - 1) * st for a in range(3)]
        sv, stri = R.extract(oracle_grid(cc, w, so, step, (sub,) * 3), so, step)
        assert len(stri) > 0
        inside = np.all((m.vertices >= np.asarray(so, dtype=F)) & (m.vertices <= np.asarray(hi, dtype=F)), axis=1)
        deep = np.all((m.vertices > np.asarray(so, dtype=F) + F(st)) & (m.vertices < np.asarray(hi, dtype=F) - F(st)), axis=1)
        tri = np.asarray(m.triangles, dtype=np.int64)
        big_in = triangle_keys(m.vertices, tri[inside[tri].all(axis=1)])
        big_deep = triangle_keys(m.vertices, tri[deep[tri].all(axis=1)])
        small = triangle_keys(sv, stri)
        assert small <= big_in, "a triangle of the sub-lattice's restatement is missing from the big mesh"
        assert big_deep <= small, "a triangle of the big mesh is not in the sub-lattice's restatement"
        assert len(big_deep) > 0


# ---- culling is real ------------------------------------------------------------------------------------------------------------
def test_culling_on_a_unit_sphere(res):
    cc, w = words_of((0, [0.0, 0.0, 0.0, 1.0]))
    res.set_limits(LIM)
    res.set_program(cc, w)
    m = res.extract_mesh_grid_sparse((-2.0,) * 3, (F(4.0) / F(255.0),) * 3, (256,) * 3, normals=False, ids=False)
    print("sphere 256^3:", m.stats)
    assert m.stats["evaluations"] <= 0.20 * 256 ** 3
    assert m.is_closed() and R.euler_characteristic(m.triangles) == 2
    m = res.extract_mesh_grid_sparse((-2.0,) * 3, (F(4.0) / F(511.0),) * 3, (512,) * 3, normals=False, ids=False)
    print("sphere 512^3:", m.stats)
    assert m.stats["scratch_bytes"] <= (9 * 512 ** 3) / 4
    assert m.is_closed()


# ---- errors and isolation -------------------------------------------------------------------------------------------------------
def lattice(o=(0.0, 0.0, 0.0), s=(0.1, 0.1, 0.1)):
    return (C.c_float * 3)(*o), (C.c_float * 3)(*s)


def test_errors(res, oracle):
    L = _ffi.hip_lib()
    cc, w = oracle.serialize(*scenes.g8())
    res.set_limits(LIM)
    res.set_program(cc, w)
    o, s = lattice()
    N = _ffi.RM_MESH_STATS
    stats = (C.c_uint64 * N)()
    assert L.rm_extract_mesh_sparse(None, o, s, 4, 4, 4, 0.0, 0, stats, N) == _ffi.RM_ERR_NULL
    assert L.rm_extract_mesh_sparse(res._h, o, s, 4, 4, 4, 0.0, 0, None, N) == _ffi.RM_ERR_NULL
    assert L.rm_extract_mesh_sparse(res._h, o, s, 4, 4, 4, 0.0, 0, stats, N - 1) == _ffi.RM_ERR_ARG
    assert L.rm_extract_mesh_sparse(res._h, None, s, 4, 4, 4, 0.0, 0, stats, N) == _ffi.RM_ERR_NULL
    for nx, ny, nz in ((1, 4, 4), (4, 4, 1), (65537, 2, 2)):
        assert L.rm_extract_mesh_sparse(res._h, o, s, nx, ny, nz, 0.0, 0, stats, N) == _ffi.RM_ERR_RANGE, (nx, ny, nz)
    for bad in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.inf, 0.1, 0.1), (np.nan, 0.1, 0.1)):
        o2, s2 = lattice(s=bad)
        assert L.rm_extract_mesh_sparse(res._h, o2, s2, 4, 4, 4, 0.0, 0, stats, N) == _ffi.RM_ERR_ARG, bad
    o2, s2 = lattice(o=(0.0, np.inf, 0.0))
    assert L.rm_extract_mesh_sparse(res._h, o2, s2, 4, 4, 4, 0.0, 0, stats, N) == _ffi.RM_ERR_ARG
    for level in (np.nan, np.inf):
        assert L.rm_extract_mesh_sparse(res._h, o, s, 4, 4, 4, level, 0, stats, N) == _ffi.RM_ERR_ARG
    assert L.rm_extract_mesh_sparse(res._h, o, s, 4, 4, 4, 0.0, 4, stats, N) == _ffi.RM_ERR_ARG      # unknown flag
    o3, s3 = lattice((-2.0, -2.0, -2.0), (0.25, 0.25, 0.25))
    assert L.rm_extract_mesh_sparse(res._h, o3, s3, 17, 17, 17, 0.0, _ffi.RM_MESH_NORMALS, stats, N) == _ffi.RM_OK
    V = int(stats[_ffi.RM_MESH_STAT_VERTICES])
    assert V > 0
    ids = np.empty((V, 2), dtype=np.uint32)
    nrm = np.empty((V, 3), dtype=np.float32)
    assert L.rm_read_mesh(res._h, None, None, None, ids.ctypes.data, 0, None) == _ffi.RM_ERR_ARG   # not computed
    assert L.rm_read_mesh(res._h, None, None, nrm.ctypes.data, None, 0, None) == _ffi.RM_OK
    # an invalid program: the status a draw gives
    res.write_buffer(_ffi.RM_BUF_COMMANDS, 0, np.array([1, 100], np.uint32).tobytes())   # Union on an empty stack
    assert L.rm_extract_mesh_sparse(res._h, o3, s3, 17, 17, 17, 0.0, 0, stats, N) == _ffi.RM_ERR_STACK_UNDERFLOW


def test_sparse_and_dense_share_the_context_mesh_and_leave_draws_alone(res, oracle):
    cc, w = oracle.serialize(*scenes.xform_mix())
    W, H = 64, 48
    res.set_limits((0.01, 100.0, 128))
    res.set_program(cc, w)
    u, *_ = oracle.orbit_uniforms((float(W), float(H)), events=scenes.STILL_CAMERA_EVENTS)
    res.set_uniforms(_ffi.Uniforms.from_buffer_copy(bytes(u)))
    first = res.draw(W, H)
    origin, step, shape = cube(40)
    coarse = cube(24)

    def read(V, T):
        v, t = np.empty((V, 3), dtype=np.float32), np.empty((T, 3), dtype=np.uint32)
        res._check(res._L.rm_read_mesh(res._h, v.ctypes.data, t.ctypes.data, None, None, 0, None))
        return v, t

    dense = res.extract_mesh_grid(*coarse)
    sparse = res.extract_mesh_grid_sparse(origin, step, shape)
    assert res.draw(W, H).tobytes() == first.tobytes()
    v, t = read(len(sparse.vertices), len(sparse.triangles))          # rm_read_mesh: the last extraction, the sparse one
    assert same(v, sparse.vertices) and same(t, sparse.triangles)
    dense2 = res.extract_mesh_grid(*coarse)
    v, t = read(len(dense2.vertices), len(dense2.triangles))          # ... and now the dense one
    assert same(v, dense.vertices) and same(t, dense.triangles)
    # a later program change does not touch the extracted mesh
    sparse = res.extract_mesh_grid_sparse(origin, step, shape)
    res.set_program(*oracle.serialize(*scenes.g8()))
    v, t = read(len(sparse.vertices), len(sparse.triangles))
    assert same(v, sparse.vertices) and same(t, sparse.triangles)
    res.set_program(cc, w)
    assert res.draw(W, H).tobytes() == first.tobytes()
    # the device path
    import torch
    d = res.extract_mesh_grid_sparse(origin, step, shape, device=True)
    torch.cuda.synchronize()
    assert d.vertices.device.type == "cuda" and d.stats == sparse.stats
    dn = d.numpy()
    assert same(dn.vertices, sparse.vertices) and same(dn.triangles, sparse.triangles) and same(dn.normals, sparse.normals)
    assert same(dn.leaf.view(np.uint32), sparse.leaf) and same(dn.material.view(np.uint32), sparse.material)
