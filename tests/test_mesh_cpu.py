"""Mesh export without a GPU: the library's case table against the numpy restatement (tests/mesh_ref.py), the restatement's
topology on analytic fields, the OBJ / PLY / STL writers, the Python argument checks, and the C, Rust and Python faces of
the new ABI (tests/test_gpu_mesh.py runs the kernels)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import mesh_ref as R
from ray_marching_amd import _ffi, renderer
from ray_marching_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MESH_FUNCTIONS = ("rm_sample_grid", "rm_extract_mesh", "rm_read_mesh", "rm_mesh_case_table")


def lib_table():
    out = np.zeros(4096, dtype=np.uint32)
    assert _ffi.hip_lib().rm_mesh_case_table(out.ctypes.data, 4096) == _ffi.RM_OK
    return out.reshape(256, 16)


def test_case_table_matches_the_restated_rule():
    lib, ref = lib_table(), R.table()
    for case in range(256):
        assert np.array_equal(lib[case], ref[case]), (case, lib[case], ref[case])
    assert lib[0, 0] == 0 and lib[255, 0] == 0
    assert lib[:, 0].max() == 5
    assert list(lib[1, :4]) == [1, 0, 4, 8]
    assert np.all(lib[1, 4:] == R.NO_EDGE)
    # the complement of a case is the same surface, wound the other way
    for case in range(1, 255):
        a = sorted(tuple(sorted(t)) for t in lib[case, 1:1 + 3 * lib[case, 0]].reshape(-1, 3).tolist())
        b = sorted(tuple(sorted(t)) for t in lib[255 - case, 1:1 + 3 * lib[255 - case, 0]].reshape(-1, 3).tolist())
        assert set(x for t in a for x in t) == set(x for t in b for x in t), case


def test_case_table_arguments():
    L = _ffi.hip_lib()
    small = np.zeros(4095, dtype=np.uint32)
    assert L.rm_mesh_case_table(small.ctypes.data, 4095) == _ffi.RM_ERR_ARG
    assert L.rm_mesh_case_table(None, 4096) == _ffi.RM_ERR_NULL


def test_case_one_points_toward_larger_distance():
    # corner 0 inside, every other corner outside: the normal of (0, 4, 8) points away from corner 0
    d = np.ones((2, 2, 2), dtype=F)
    d[0, 0, 0] = -1.0
    v, t = R.extract(d, (0, 0, 0), (1, 1, 1))
    assert len(t) == 1
    a, b, c = v[t[0].astype(np.int64)].astype(np.float64)
    assert np.all(np.cross(b - a, c - a) > 0)


def field(origin, step, n, fn):
    p = R.lattice_points(origin, step, (n, n, n)).astype(np.float64)
    return fn(p[:, 0], p[:, 1], p[:, 2]).astype(F).reshape(n, n, n)


def test_sphere_is_a_closed_two_manifold():
    n = 49
    origin, step = (-1.5,) * 3, (F(3.0) / F(n - 1),) * 3
    v, t = R.extract(field(origin, step, n, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - 1.0), origin, step)
    assert R.is_closed_manifold(t) and R.euler_characteristic(t) == 2
    vol = R.signed_volume(v, t)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi) - 1.0) < 0.01
    # 16 cells per diameter already give 1 %
    n = 19
    origin, step = (-1.125,) * 3, (F(0.125),) * 3
    v, t = R.extract(field(origin, step, n, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - 1.0), origin, step)
    assert R.is_closed_manifold(t) and abs(R.signed_volume(v, t) / (4.0 / 3.0 * np.pi) - 1.0) < 0.01


def box_minus_cylinder(x, y, z):
    q = np.abs(np.stack([x, y, z])) - np.array([1.0, 0.6, 0.8])[:, None]
    box = np.linalg.norm(np.maximum(q, 0.0), axis=0) + np.minimum(q.max(axis=0), 0.0)
    cyl = np.sqrt(x * x + y * y) - 0.35          # along z, through the box
    return np.maximum(box, -cyl)


def test_box_minus_cylinder_is_a_torus():
    n = 57
    origin, step = (-1.4,) * 3, (F(2.8) / F(n - 1),) * 3
    v, t = R.extract(field(origin, step, n, box_minus_cylinder), origin, step)
    assert R.directed_edges_balance(t)
    assert R.euler_characteristic(t) == 0


def test_two_spheres_have_two_components():
    n = 45
    origin, step = (-2.2, -1.2, -1.2), (F(0.1),) * 3

    def two(x, y, z):
        return np.minimum(np.sqrt((x + 1) ** 2 + y * y + z * z) - 0.8, np.sqrt((x - 1) ** 2 + y * y + z * z) - 0.8)
    v, t = R.extract(field(origin, step, n, two), origin, step)
    assert R.is_closed_manifold(t) and R.euler_characteristic(t) == 4


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_with_an_outside_border_is_closed_and_oriented(seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (14, 15, 16)).astype(F)
    d[[0, -1], :, :] = 1.0
    d[:, [0, -1], :] = 1.0
    d[:, :, [0, -1]] = 1.0
    v, t = R.extract(d, (0, 0, 0), (1, 1, 1))
    assert len(t) > 100
    assert R.directed_edges_balance(t)
    assert np.all(t < len(v))
    assert len(np.unique(t)) == len(v)           # every vertex is used


def test_extraction_order_and_levels():
    rng = np.random.default_rng(7)
    d = rng.uniform(-1, 1, (5, 6, 7)).astype(F)
    v0, t0 = R.extract(d, (0.5, -1, 2), (0.25, 0.5, 1.0), level=0.0)
    v1, t1 = R.extract(d - F(0.25), (0.5, -1, 2), (0.25, 0.5, 1.0), level=-0.25)
    assert np.array_equal(t0, t1)
    # vertices lie on their lattice edges: two coordinates on the lattice, the third between two lattice values
    xs, ys, zs = R.axis_coords((0.5, -1, 2), (0.25, 0.5, 1.0), (7, 6, 5))
    on = np.isin(v0[:, 0], xs).astype(int) + np.isin(v0[:, 1], ys).astype(int) + np.isin(v0[:, 2], zs).astype(int)
    assert np.all(on >= 2)


# ---- files ---------------------------------------------------------------------------------------------------------------
def small_mesh():
    n = 13
    origin, step = (-1.2,) * 3, (F(0.2),) * 3
    d = field(origin, step, n, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - 1.0)
    v, t = R.extract(d, origin, step)
    rng = np.random.default_rng(0)
    nrm = v / np.linalg.norm(v, axis=1, keepdims=True).astype(F)
    mat = rng.integers(0, 6, len(v)).astype(np.uint32)
    return M.Mesh(v, t, nrm.astype(F), np.zeros(len(v), dtype=np.uint32), mat)


def test_obj_round_trip(tmp_path):
    m = small_mesh()
    p = str(tmp_path / "m.obj")
    M.write_obj(m, p)
    vs, vn, fs = [], [], []
    for line in open(p):
        w = line.split()
        if w and w[0] == "v":
            vs.append([float(x) for x in w[1:]])
        elif w and w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w and w[0] == "f":
            fs.append([int(x.split("/")[0]) - 1 for x in w[1:]])
    assert np.array_equal(np.asarray(vs, dtype=F), m.vertices)        # %.9g round-trips binary32
    assert np.array_equal(np.asarray(vn, dtype=F), m.normals)
    assert np.array_equal(np.asarray(fs), m.triangles.astype(np.int64))


def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().splitlines()
    assert head[1] == "format binary_little_endian 1.0"
    nv = int(next(x for x in head if x.startswith("element vertex")).split()[2])
    nf = int(next(x for x in head if x.startswith("element face")).split()[2])
    types = {"float": "<f4", "uchar": "u1"}
    props = [(x.split()[2], types[x.split()[1]]) for x in head if x.startswith("property ") and "list" not in x]
    v = np.frombuffer(data, dtype=props, count=nv, offset=end)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<u4", (3,))], count=nf, offset=end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(data)
    return v, f


def test_ply_round_trip_with_material_colours(tmp_path):
    m = small_mesh()
    p = str(tmp_path / "m.ply")
    M.write_ply(m, p, M.MATERIALS)
    v, f = read_ply(p)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], axis=1), m.vertices)
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], axis=1), m.normals)
    table = np.rint(np.asarray(M.MATERIALS) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], axis=1), table[m.material])
    assert np.all(f["n"] == 3) and np.array_equal(f["v"], m.triangles)
    # without a table: no colour properties
    M.write_ply(m, p)
    v, _ = read_ply(p)
    assert "red" not in v.dtype.names


def test_stl_round_trip_and_facet_normals(tmp_path):
    m = small_mesh()
    p = str(tmp_path / "m.stl")
    M.write_stl(m, p)
    data = open(p, "rb").read()
    (nt,) = struct.unpack_from("<I", data, 80)
    assert nt == len(m.triangles) and len(data) == 84 + 50 * nt
    rec = np.frombuffer(data, dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")], offset=84)
    assert np.array_equal(rec["v"], m.vertices[m.triangles.astype(np.int64)])
    # unit normals that point outward (away from the sphere's centre) and agree with the cross product of the edges
    n = rec["n"].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    centre = rec["v"].astype(np.float64).mean(axis=1)
    assert np.all((n * centre).sum(axis=1) > 0)
    e = np.cross(rec["v"][:, 1] - rec["v"][:, 0], rec["v"][:, 2] - rec["v"][:, 0]).astype(np.float64)
    assert np.allclose(n, e / np.linalg.norm(e, axis=1, keepdims=True), atol=1e-5)


def test_cli_colours_are_the_material_scenes_table():
    import scenes
    assert M.MATERIALS == scenes.MATERIAL_TABLE
    assert M.MATERIALS[0] == (0.4, 0.7, 0.1)          # the draws' colour of untagged surfaces (wgsl:105)


def test_mesh_is_closed():
    m = small_mesh()
    assert m.is_closed()
    assert not M.Mesh(m.vertices, m.triangles[1:]).is_closed()


def test_write_picks_the_format_by_extension(tmp_path):
    m = small_mesh()
    with pytest.raises(ValueError):
        M.write(m, str(tmp_path / "m.xyz"))
    M.write(m, str(tmp_path / "m.STL"))
    assert os.path.getsize(str(tmp_path / "m.STL")) == 84 + 50 * len(m.triangles)


# ---- Python argument checks (raised before any device call) ----------------------------------------------------------------
class _NoDevice(renderer.RayMarchingResources):
    def __init__(self):       # the argument checks only: no context
        self._L, self._h, self.device = _ffi.hip_lib(), None, 0


@pytest.mark.parametrize("lo, hi, res", [((-1, -1, -1), (1, 1, 1), 1), ((-1, -1, -1), (1, 1, 1), (8, 8, 1)),
                                         ((1, -1, -1), (1, 1, 1), 8), ((0, 0, 0), (-1, 1, 1), 8),
                                         ((-1, -1, -1), (1, 1, np.inf), 8), ((-1, -1, -1), (1, 1, 1), 2.5),
                                         ((-1, -1), (1, 1), 8)])
def test_extract_mesh_rejects_bad_boxes(lo, hi, res):
    with pytest.raises(ValueError):
        _NoDevice().extract_mesh(lo, hi, res)


@pytest.mark.parametrize("origin, step, shape", [((0, 0), (1, 1, 1), (4, 4, 4)), ((0, 0, 0), (1, 0, 1), (4, 4, 4)),
                                                 ((0, 0, 0), (1, -1, 1), (4, 4, 4)), ((0, np.nan, 0), (1, 1, 1), (4, 4, 4)),
                                                 ((0, 0, 0), (1, 1, 1), (4, 4)), ((0, 0, 0), (1, 1, 1), (4, 0, 4))])
def test_sample_grid_rejects_bad_lattices(origin, step, shape):
    with pytest.raises(ValueError):
        _NoDevice().sample_grid(origin, step, shape)


class _Recorder:
    """Stands in for the library: records the 3 floats behind each lattice pointer, then fails the call."""

    def __init__(self):
        self.calls = []

    def _record(self, o, s, dims):
        self.calls.append(([o[k] for k in range(3)], [s[k] for k in range(3)], dims))
        return _ffi.RM_ERR_ARG

    def rm_extract_mesh(self, h, o, s, nx, ny, nz, level, flags, counts):
        return self._record(o, s, (nx, ny, nz))

    def rm_sample_grid(self, h, o, s, nx, ny, nz, out, is_device, stream):
        return self._record(o, s, (nx, ny, nz))


def test_scalar_and_broadcast_lattices_reach_the_library_as_three_values():
    r = _NoDevice()
    rec = r._L = _Recorder()
    with pytest.raises(_ffi.RmError):
        r.extract_mesh(-2.5, 2.5, 64)
    assert rec.calls[-1] == ([-2.5] * 3, [float(F(5.0) / F(63.0))] * 3, (64, 64, 64))
    with pytest.raises(_ffi.RmError):
        r.extract_mesh((-1.0, -2.0, -3.0), 2.0, (9, 17, 33))
    assert rec.calls[-1] == ([-1.0, -2.0, -3.0], [float(F(3.0) / F(8.0)), float(F(4.0) / F(16.0)), float(F(5.0) / F(32.0))],
                             (9, 17, 33))
    # stride-0 and strided views handed in directly
    view = np.broadcast_to(F(1.5), (3,))
    strided = np.arange(6, dtype=F)[::2] + F(0.25)
    with pytest.raises(_ffi.RmError):
        r.extract_mesh_grid(view, strided, (8, 8, 8))
    assert rec.calls[-1] == ([1.5] * 3, [0.25, 2.25, 4.25], (8, 8, 8))
    with pytest.raises(_ffi.RmError):
        r.sample_grid(strided, view, (5, 6, 7))
    assert rec.calls[-1] == ([0.25, 2.25, 4.25], [1.5] * 3, (5, 6, 7))


def test_extract_mesh_grid_needs_two_points_per_axis():
    with pytest.raises(ValueError):
        _NoDevice().extract_mesh_grid((0, 0, 0), (1, 1, 1), (4, 1, 4))


# ---- the C, Rust and Python faces ------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rm_abi.h")).read(), flags=re.S)


def rust_text():
    return open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()


def test_mesh_symbols_constants_and_null_context():
    text, rust, L = header_text(), rust_text(), _ffi.hip_lib()
    for name in MESH_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    body = re.search(r"enum\s+rm_mesh\s*\{(.*?)\}", text, re.S).group(1)
    consts = {n: int(v) for n, v in re.findall(r"(RM_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)}
    assert consts == {"RM_MESH_NORMALS": 1, "RM_MESH_IDS": 2}
    for name, value in consts.items():
        assert getattr(_ffi, name) == value
        assert re.search(r"pub const %s: c_int = %d;" % (name, value), rust), name
    assert re.search(r"#define RM_ABI_VERSION 2\b", text)
    o = (C.c_float * 3)(0, 0, 0)
    s = (C.c_float * 3)(1, 1, 1)
    out = np.zeros(64, dtype=np.float32)
    counts = (C.c_uint64 * 2)()
    assert L.rm_sample_grid(None, o, s, 4, 4, 4, out.ctypes.data, 0, None) == _ffi.RM_ERR_NULL
    assert L.rm_extract_mesh(None, o, s, 4, 4, 4, 0.0, 0, counts) == _ffi.RM_ERR_NULL
    assert L.rm_read_mesh(None, out.ctypes.data, None, None, None, 0, None) == _ffi.RM_ERR_NULL


def test_rust_wrappers_check_their_slices():
    rust = rust_text()
    for fn in ("sample_grid", "extract_mesh", "read_mesh"):
        assert re.search(r"pub fn %s\(&self" % fn, rust), fn
    assert re.search(r"pub fn extract_mesh\(.*?\) -> Result<\(u64, u64\), RmError>", rust, re.S)
    # read_mesh checks its slices against the counts of the context's own mesh, not against counts the caller passes
    assert re.search(r"pub fn read_mesh\(&self, out_vertices: Option<&mut \[f32\]>", rust)
    body = rust[rust.index("pub fn read_mesh("):]
    body = body[:body.index("\n    }\n")]
    assert "self.mesh.get()" in body
    call = body.index("rm_read_mesh(")
    for arg in ("out_vertices", "out_triangles", "out_normals", "out_ids"):
        assert re.search(r"assert!\(%s\.as_ref\(\)" % arg, body[:call]), arg
    ext = rust[rust.index("pub fn extract_mesh("):]
    ext = ext[:ext.index("\n    }\n")]
    assert ext.index("self.mesh.set(None)") < ext.index("rm_extract_mesh(") < ext.index("self.mesh.set(Some(")
    body = rust[rust.index("pub fn sample_grid("):]
    assert "assert!(out_dist.len() >= n" in body[:body.index("\n    }\n")]
